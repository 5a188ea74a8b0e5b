// The extern "C" kernel launchers of the library and the structs that cross the host / device boundary.
// Internal header.  This is the ONLY declaration of every launcher: the file that defines one includes it (a definition that
// disagrees with its declaration does not compile: "conflicting types"), and so do the host files that call them.  C linkage
// carries no types to the linker, so a second, hand-copied prototype anywhere would go unchecked: there is none.
#pragma once
#include "apse_common.h"

struct UndistortParams;   // preproc_pixel.h
struct LabTables;
struct YuvSource;

// Slot length of the NMS keep lists (keep_idx [B][ncat][APSE_NMS_SLOT]): boxes per category, <= 1000 by construction
#define APSE_NMS_SLOT 1024

// ---------------------------------------------------------------- RPN top-k tournament (select_nms.hip)
struct RpnLevel {
    const float* head;     // [B][H*W][head_ld] : channels 0..2 objectness, 3..14 deltas (a*4+coord)
    int H, W, stride;
    int n;                 // H*W*3
    int k;                 // min(pre_topk, n)
    float base[3][4];      // cell anchors (x0,y0,x1,y1)
};
struct RpnLevels {
    RpnLevel lv[5];
    int head_ld;
    int pre_topk;          // 1000
};
struct TopkJob {
    int kind;              // 0: raw logits chunk, 1: merge of lists
    int level;
    int begin, count;      // kind 0: element range within the level
    int nsrc;
    int src[4];            // kind 1: source list slots
    int src_count[4];
    int dst;               // destination list slot
    int dst_count;         // min(pre_topk, total)
};
// C4 (Res5ROIHeads) RPN on res4: the head rows and the 15 cell anchors (select_nms.hip c4_rpn_select; built by plan.hip)
struct C4Rpn {
    const float* head;     // [B][H*W][ld]: channels 0..14 objectness (anchor a), 15 + 4 a + j deltas
    int H, W, ld, stride;
    int n, k;              // H*W*15, min(pre_topk, n)
    float base[15][4];     // cell anchors, a = 3 * size + ratio
};
// ---------------------------------------------------------------- ROIAlign over the pyramid (roi.hip)
struct FpnMaps {
    const void* p[4];      // p2..p5, each [B][H][W][256], f32 or 16-bit (st)
    int H[4], W[4];
    float scale[4];        // 1/4 .. 1/32
    int st;                // storage type of the maps: 0 f32, 1 bf16, 2 f16
};
// ---------------------------------------------------------------- mask paste (mask_tail.hip)
struct PasteParams {
    const float* boxes;      // packed [n][4], resized-image coordinates
    const int* cls;          // packed [n]
    const int* total;        // device count of packed detections
    const float* logits;     // [n][M][M][ldc] mask head output (NHWC), class channel = cls[n]
    int M, ldc;
    float sx, sy;            // output/resized scale factors (f32 of the Python doubles)
    int out_h, out_w;
    int words_per_row;       // ceil(out_w / 64)
    float thresh;
    float* boxes_out;        // [n][4] scaled + clipped boxes
    int* valid;              // [n] nonempty after scaling
    int* rect;               // [n][4] x0, y0, x1, y1 paste window
    uint64_t* bits;          // [n][out_h][words_per_row]
    unsigned long long* sums;   // [n][3] mass, sum(x+1), sum(y+1): zero when the launch starts (pack_detections clears them)
};
// ---------------------------------------------------------------- training augmentation (augment.hip)
// One image's parameters as the kernels read them: the f32 weights and the f64 complements, rounded on the host exactly once
struct AugmentImage {
    double one_minus_ws, one_minus_wc;   // 1.0 - saturation, 1.0 - contrast (f64)
    double vec[3];                       // lighting: EIGVEC . (lw * EIGVAL), added to channel 0, 1, 2
    float wb, ws, wc;                    // f32 of the brightness, saturation and contrast weights
    int flip;
};
struct AugmentBatch {
    AugmentImage im[64];                 // APSE_AUGMENT_MAX_BATCH; a kernel argument (3.5 KiB)
};
// ---------------------------------------------------------------- RPN-head training (rpn_train.hip)
// The anchors of the five levels in (level, y, x, a) order as a kernel argument: level l holds elements off[l] .. off[l + 1] - 1,
// element e of it is pixel e / 3, anchor e % 3, at (x stride, y stride) + base[l][a] -- the boxes rpn_decode computes
struct RpnAnchorGrid {
    int H[5], W[5], stride[5];
    int off[6];
    float base[5][3][4];   // cell anchors (x0,y0,x1,y1) per level: apse_cell_anchors3
};
struct RpnGatherMaps {
    const float* p[5];     // p2..p6 of ONE image, each [H][W][256] f32
};
// DefaultAnchorGenerator.generate_cell_anchors for one size and the ratios (0.5, 1, 2): Python doubles -> f32 (plan.hip; the one
// definition behind the inference plan and the training anchors)
void apse_cell_anchors3(int size, float (*base)[4]);

extern "C" {
// ---- elementwise.hip
int apse_k_round16(const float* x, uint16_t* y, size_t n, int dtype, hipStream_t s);
int apse_k_pil_resize(const uint8_t* src, uint8_t* tmp, void* out, int out_st, uint8_t* resized_u8, const int* hb, const int* hc,
                      int hk, const int* vb, const int* vc, int vk, int B, int H, int W, int OH, int OW, int PH, int PW,
                      const float* mean, const UndistortParams* cam, const LabTables* lut, const void* cam_map, const int* hcT, int tmp_pitch,
                      const YuvSource* yuv, hipStream_t s);
int apse_k_chw_norm(const float* img, void* out, int out_st, int B, int OH, int OW, int PH, int PW, const float* mean, hipStream_t s);
int apse_k_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, int st, hipStream_t s);
int apse_k_subsample2(const void* x, void* y, int B, int H, int W, int C, int st, hipStream_t s);
int apse_k_nhwc_to_nchw(const void* x, float* y, int B, int HW, int C, int st, hipStream_t s);
// ---- preproc.hip
int apse_k_undistort_build_map_compact(const UndistortParams* p, void* map, int* overflow_dev, hipStream_t s);
int apse_k_undistort_gamma(const UndistortParams* p, const uint8_t* src, uint8_t* dst, const LabTables* lab, int B, hipStream_t s);
int apse_k_yuv_to_bgr(const YuvSource* p, const uint8_t* src, uint8_t* dst, int B, hipStream_t s);
// ---- stem_pool16.hip, bottleneck16.hip
int apse_k_stem_pool16(const void* x, const uint16_t* w16, const float* bias, void* y, int B, int IH, int IW, int prec,
                       hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
int apse_k_bottleneck64_fused16(const void* x, const void* res, void* y, const uint16_t* w1, const float* b1,
                                const uint16_t* w2, const float* b2, const uint16_t* w3, const float* b3, int B, int H,
                                int W, int K1, int prec, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
// ---- select_nms.hip
int apse_k_rpn_topk_stage(const RpnLevels* L_dev, const TopkJob* jobs_dev, int njobs, uint64_t* lists, int nslots, int B,
                          uint32_t* zero_word, hipStream_t s);
int apse_k_rpn_decode(const RpnLevels* L_dev, int pre_topk, const uint64_t* lists, int nslots, const int* final_slot_dev,
                      float img_h, float img_w, float scale_clamp, float* boxes, float* scores, int* valid, uint32_t* maxc,
                      int level_mask, int B, hipStream_t s);
size_t apse_nms_scratch_bytes(int slots);
int apse_k_nms_percat(const float* boxes, const float* scores, const int* valid, int n_total, int cat_div, int cat_mod,
                      const uint32_t* maxc, float thr, int* keep_idx, int* keep_cnt, int ncat, void* scratch, int cat_mask,
                      int B, int presorted, hipStream_t s);
int apse_k_rank_final(const float* boxes, const float* scores, int n_total, const int* keep_idx, const int* keep_cnt,
                      int ncat, int K, float* out_boxes, float* out_scores, int* out_entry, int* out_count,
                      uint32_t* zero_word, int B, hipStream_t s);
int apse_k_box_candidates(const float* pred, int ld, int K, const float* props, const int* prop_cnt, int P, float img_h,
                          float img_w, float thresh, const float* wts, float scale_clamp, float* cboxes, float* cscores,
                          int* cvalid, uint32_t* maxc, float* probs_out, int B, hipStream_t s);
int apse_k_box_candidates_wide(const float* pred, int ld, int K, const float* props, const int* prop_cnt, int P, float img_h,
                               float img_w, float thresh, const float* wts, float scale_clamp, float* cboxes, float* cscores,
                               int* cvalid, uint32_t* maxc, float* probs_out, int* clist, int* ccnt, int B, hipStream_t s);
int apse_k_rank_wide(const float* boxes, const float* scores, int n_total, const int* keep_idx, const int* keep_cnt, int ncat,
                     int K, float* out_boxes, float* out_scores, int* out_entry, int* out_count, int B, hipStream_t s);
int apse_k_nms_lists(const float* boxes, const float* scores, int n_total, const int* clist, int* ccnt, int list_stride,
                     const uint32_t* maxc, float thr, int* keep_idx, int* keep_cnt, int ncat, void* scratch, int B, hipStream_t s);
size_t apse_c4_nms_scratch_bytes(int B);
int apse_k_c4_rpn(const C4Rpn* R, int pre, int post, float img_h, float img_w, float scale_clamp, float thr, float* dec_boxes,
                  float* dec_scores, int* dec_valid, void* scratch, float* props, float* prop_scores, int* prop_entry,
                  int* prop_count, int B, hipStream_t s);
size_t apse_rpn_train_scratch_bytes(int B);
int apse_k_rpn_train_select(const RpnLevels* L, int post, float img_h, float img_w, float scale_clamp, float thr, int level_mask,
                            uint64_t* keys, float* dec_boxes, float* dec_scores, int* dec_valid, void* scratch, float* props,
                            float* prop_scores, int* prop_entry, int* prop_count, int B, hipStream_t s);
int apse_k_pack_detections(const float* det_boxes, const float* det_scores, const int* det_entry, const int* det_cnt, int B,
                           int Kd, int ncls, float* pk_boxes, float* pk_scores, int* pk_cls, int* pk_img, int* pk_roi,
                           int* pk_total, int* pk_offset, unsigned long long* zero_sums, hipStream_t s);
// ---- roi.hip
int apse_k_roi_align(const FpnMaps* F, const float* rois, const int* roi_img, const int* cnt, const int* total, int per_img,
                     int n_max, int R, void* out, int out_st, hipStream_t s);
int apse_k_roi_pool(const void* feat, int st, int H, int W, const float* rois, const int* roi_img, const int* total, int n_max,
                    int R, float scale, float* out, int img0, int nchw, hipStream_t s);
int apse_k_roi_align_c4(const float* fmap, int H, int W, int C, float scale, const float* rois, const int* roi_img, const int* cnt,
                        const int* total, int per_img, int n_max, int R, float* out, hipStream_t s);
int apse_k_roi_pool_c4(const float* feat, int H, int W, int C, const float* rois, const int* roi_img, const int* total, int n_max,
                       int R, float scale, float* out, hipStream_t s);
int apse_k_mean_cells(const float* x, int n, int cells, int C, float* y, hipStream_t s);
int apse_k_mask_resize(const uint8_t* masks, int n, int H, int W, int OH, int OW, float* out, hipStream_t s);
int apse_k_roi_align_masked(const void* feat, int st, int H, int W, int img0, const float* rois, const float* mask, int n, int R,
                            int SR, float scale, float* out, hipStream_t s);
// roi_align(aligned=False, sampling_ratio=SR) of feat * m_r, m_r the bilinear resize (frame_h x frame_w -> H x W) of row r's bit
// mask: windows[r], or (windows == nullptr) plane r of `planes` inside rects[r], empty when valid[r] == 0.  Bit for bit
// apse_k_mask_resize + apse_k_roi_align_masked.  R <= 32, SR in {1, 2, 4}; nchw: out [row][256][R][R], else [row][R][R][256].
struct apse_mots_window;
int apse_k_roi_align_windows(const void* feat, int st, int H, int W, const float* rois, const int* roi_img, int img0, const int* total,
                             int n_max, const apse_mots_window* windows, const uint64_t* planes, const int* rects, const int* valid,
                             int plane_wpr, int frame_h, int frame_w, int R, int SR, float scale, float* out, int nchw, hipStream_t s);
int apse_k_l2_normalize(const float* x, float* y, int D, const int* total, int n_max, hipStream_t s);
bool apse_assoc_fc_ok(int K, int N);
int apse_k_assoc_fc(const float* x, const float* w, const float* bias, float* ws, const int* total, int n_max, int K, int N, float* raw,
                    float* y, hipStream_t s);
int apse_k_sqdist(const float* a, const float* b, int O, int N, int D, float* out, hipStream_t s);
// ---- mask_tail.hip
int apse_k_closest_single(const uint64_t* bits, int out_h, int out_w, int words_per_row, float px, float py,
                          unsigned long long* best_out, hipStream_t s);
int apse_k_mask_paste(const PasteParams* p, int n_max, unsigned long long* keys, int kd, hipStream_t s);
int apse_k_closest_points(const uint64_t* bits, const int* rect, const int* valid, const unsigned long long* sums, const int* img,
                          const int* offset, const int* total, int n_max, int kd, int out_h, int out_w, int words_per_row,
                          int* cent, int* mass, unsigned long long* keys, int hint, hipStream_t s);
int apse_k_copy_mask_windows(const uint64_t* bits, uint64_t* out, int n, const long long* src, const long long* dst, const int* nw,
                             const int* rows, int words_per_row, hipStream_t s);
int apse_k_bits_to_dense(const uint64_t* bits, const int* rect4, int out_h, int out_w, int words_per_row, uint8_t* dense,
                         hipStream_t s);
int apse_k_dense_to_bits(const uint8_t* dense, int out_h, int out_w, int words_per_row, uint64_t* bits,
                         unsigned long long* sums, hipStream_t s);
// ---- mask_train.hip
int apse_k_mask_roi_index(int* idx, int n, hipStream_t s);
// ---- coco_eval.hip (the polygon rule lives there; apse_coco_mask_targets of mask_train.hip checks the limits and calls this)
int apse_k_mask_targets(const double* xy, const int* part_vert_off, int n_parts, const int* obj_part_off, int n_obj, int n_verts,
                        const float* rois, const int* matched, int n, uint8_t* targets, int* info, hipStream_t s);
// ---- bitmask_targets.hip
struct apse_mots_window;
int apse_k_remap_windows(const apse_mots_window* src, int n, const int* xmap, const int* ymap, int h, int w,
                         const apse_mots_window* dst, hipStream_t s);
int apse_k_bitmask_targets(const apse_mots_window* windows, int n_obj, int h, int w, const float* rois, const int* matched, int n,
                           int mask_size, uint8_t* out, hipStream_t s);
// ---- augment.hip
int apse_k_augment(const uint8_t* src, int B, int H, int W, const AugmentBatch* P_host, uint8_t* out_u8, float* out_chw,
                   unsigned long long* sums, hipStream_t s);
// ---- rpn_train.hip
int apse_k_rpn_gather(const RpnAnchorGrid* grid, const RpnGatherMaps* maps, const int* anchor_idx, int S, float* x, int* slots,
                      float* anchor_boxes, int* levels, hipStream_t s);
int apse_k_pack_oihw(const float* w, int Cout, int Cin, int KH, int KW, int cin_p, int KWCp, int row0, float* out, hipStream_t s);
int apse_k_winograd_filters(const float* oihw, int Cout, int Cin, float* u, hipStream_t s);
}
