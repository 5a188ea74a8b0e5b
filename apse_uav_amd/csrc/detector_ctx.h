// The detector context and the launch plan's step types: shared by the host files of the library.
//   plan.hip      weight packing, add_conv / add_bottleneck, build_plan (FPN) and build_plan_c4: fills the context at apse_finalize_weights
//   detector.hip  run_plan and the context's C ABI (include/apse_hip.h)
//   ops.hip       the stateless operators of the C ABI (tests and tools; no context)
// Internal header.  Kernel launchers and the structs the kernels read: apse_kernels.h.
#pragma once
#include "apse_kernels.h"
#include "../../include/apse_hip.h"
#include "preproc_pixel.h"

#include <map>
#include <string>
#include <vector>

#define APSE_NARROW_CLASSES 6     // up to this many classes: box_candidates / rank_merge (one thread per ROI, ncat <= 8)
#define APSE_EV_HALF 1024    // HIP events per half of the profiling pool (one pair per timed launch)

struct HostW { std::vector<float> v; std::vector<int64_t> shape; };
struct Tens { float* p = nullptr; int H = 0, W = 0, C = 0; int st = 0; };   // per-item NHWC dims; st: 0 f32, 1 bf16, 2 f16 storage

struct ConvStep {
    ConvParams p;          // B/M filled at launch
    int b_mult = 1;        // items per image (1, post_topk, dets_per_image)
    int fixed_items = 0;   // > 0: the launch always covers this many items (a tensor laid out for max_batch: merged RPN head)
    int cfg = 0;
    double flops_per_item = 0;   // algorithmic 2*MACs per item (one image / one roi / one detection)
    int count_kind = 0;    // 0 none, 1 prop_cnt[0] (batch 1 only), 2 packed total
    void* pool_y = nullptr;   // != nullptr: the stem of the 16-bit modes, run as stem_s2d_pool16 (conv + ReLU + 3x3/2 max-pool) into this map
    std::string name;
};
enum StepKind { S_CONV, S_MAXPOOL, S_SUBSAMPLE, S_BNECK };
// S_BNECK: a whole 64-channel bottleneck as one launch (bottleneck16.hip); c = its conv1 (name, flops of all three), c2 / c3 the others
struct Step { StepKind kind; ConvStep c; const float* x; float* y; int H, W, C; int st = 0; ConvParams p2, p3; };

struct apse_ctx {
    apse_config cfg;
    std::string err;
    bool f32_winograd = true;    // APSE_F32_WINOGRAD=0 (read once, at apse_create): the named f32 3x3 layers (plan.hip: winograd_layer, winograd_trunk_layer) keep the direct kernel
    std::map<std::string, HostW> hw;
    bool finalized = false;
    int PH = 0, PW = 0;
    std::vector<void*> allocs;
    std::map<std::string, Tens> t;
    std::vector<Step> backbone, rpnhead, boxhead, maskhead, embedfc;
    float* ws = nullptr; size_t ws_floats = 0; int* tile_cnt = nullptr;
    // resize tables
    int *hb = nullptr, *hc = nullptr, *vb = nullptr, *vc = nullptr; int hk = 0, vk = 0; uint8_t* rs_tmp = nullptr;
    int rs_pitch = 0;
    int* hcT = nullptr;                                  // horizontal taps tap-major [8][image_w], zero past a pixel's count (hk <= 8)
    // rpn
    RpnLevels rl_host; RpnLevels* rl_dev = nullptr;
    std::vector<std::vector<TopkJob>> stages; std::vector<TopkJob*> stage_dev; int nslots = 0; uint64_t* lists = nullptr;
    int final_slot_host[5]; int* final_slot_dev = nullptr;
    float *dec_boxes = nullptr, *dec_scores = nullptr; int* dec_valid = nullptr; uint32_t* maxc = nullptr;   // maxc[2*B]: rpn, box
    int *keep_idx = nullptr, *keep_cnt = nullptr; void* nms_scratch = nullptr;
    float *props = nullptr, *prop_scores = nullptr; int *prop_entry = nullptr;
    // box head
    FpnMaps fm;
    float *cand_boxes = nullptr, *cand_scores = nullptr, *probs = nullptr; int* cand_valid = nullptr;
    int pred_ld = 32;                                    // row length of the fused predictor output: round_up(5 K + 1, 32)
    bool wide = false;                                   // num_classes > APSE_NARROW_CLASSES: the wide box-inference kernels
    int *cls_list = nullptr, *cls_cnt = nullptr;         // wide: class-major candidate lists [B][K][P] and counts [B][K]
    float *det_boxes = nullptr, *det_scores = nullptr; int *det_entry = nullptr, *det_cnt = nullptr;
    // results block (device) and layout
    apse_results_layout lay; uint8_t* res = nullptr;
    // mask tail
    uint64_t* bits2[2] = {nullptr, nullptr}; int bits_cur = 0, bits_read = 0;   // mask bit planes, alternating per forward (see apse_mask_tail)
    unsigned long long* sums = nullptr; int wpr = 0; bool sums_dirty = false;
    bool crop_features = false;     // apse_set_crop_features: apse_embed cuts the RoI features from p2 * mask (roi_align_windows)
    bool masks_fresh = false;       // apse_mask_tail has run on the current detection list (set bits_cur holds its masks)
    float* emb_raw = nullptr;
    float* ws_assoc = nullptr;      // [K / 128][max detections][embed_dim]: K slices of the association FC (apse_k_assoc_fc), or nullptr
    float* rf_mask = nullptr; size_t rf_mask_floats = 0;      // apse_roi_features: masks at p2 resolution (grown on demand)
    int* mrf_idx = nullptr; size_t mrf_cap = 0;               // apse_mask_roi_features: image index per RoI + live count (grown on demand)
    bool box_maxc_clean = false;
    UndistortParams cam; bool cam_on = false; LabTables* cam_lut = nullptr; void* cam_map = nullptr; bool cam_map_ok = false;     // apse_set_camera: fused undistort + gamma in apse_preprocess_frames
    uint8_t* yuv_bgr = nullptr;      // apse_preprocess_frames_yuv with a camera set: the converted BGR frames [max_batch][frame_h][frame_w][3] (first use)
    int hint_total = 8;      // detections seen in the previous forward: sizes the GRID of the packed-list GEMMs, nothing else
    hipEvent_t read_ev = nullptr; void* read_pending = nullptr;      // apse_read_results_begin / _end
    // apse_set_detections: two pinned staging blocks, each guarded by the event behind its H2D copies, so the call only enqueues
    // (a sequence driver puts the next given-boxes forward behind apse_read_results_begin like any other forward)
    uint8_t* given_host[2] = {nullptr, nullptr}; hipEvent_t given_ev[2] = {nullptr, nullptr}; int given_k = 0;
    // per-kernel profiling with HIP events on the caller's stream (bench.py roofline)
    bool prof_on = false; std::vector<hipEvent_t> ev_pool; int ev_used = 0;
    struct Pending { int cfg; double flops_per_item; int count_kind; int b_mult; int batch; int e0, e1; };
    std::vector<Pending> pending; double prof[APSE_NCFG][3] = {{0}};
    // the event pool has two halves: apse_read_results_begin hands the half (and the pending list) of the forward it reads to _end
    // and switches recording to the other half, so a forward enqueued between the two halves of a read keeps its own events
    int ev_base = 0, cal_read = -1; std::vector<Pending> pending_read;
    // The tail lane: a second stream of the context.  Of a forward that runs ahead (enqueued while a results
    // copy is pending: lane_armed) the proposal selection, box head, mask tail, embedding and results copy are enqueued on it; the
    // caller's stream keeps resize, trunk, FPN and the RPN convolutions, so the next frame's stem..res5 run beside this frame's
    // latency-bound tail.  Every other forward is on the caller's stream alone.  Off altogether: APSE_TAIL_LANE=0 (read once, at
    // apse_create), apse_config.tail_lane < 0, C4, and while profiling (prof_on) -- then every launch is on the caller's stream.
    //   fork_ev    recorded on the caller's stream behind work the lane's next launch must follow (the RPN convolutions)
    //   follow_ev  the same behind an entry that read or wrote lane-owned buffers on the caller's stream (apse_debug_tensor ...)
    //   tail_ev    recorded on the lane behind the last launch of every lane entry: the first FPN step of the next apse_backbone
    //              and every joining entry wait for it
    //   bits_ev[k] behind the mask tail that wrote bit-plane set k (apse_copy_mask_window(s) wait for their set only)
    bool lane_on = true;
    bool lane_armed = false;         // set per forward by apse_backbone: it was enqueued while a results copy was pending
    bool fwd_since_read = false;     // a forward was enqueued since the last apse_read_results_begin (the caller is running ahead)
    hipStream_t lane = nullptr;
    hipEvent_t fork_ev = nullptr, follow_ev = nullptr, tail_ev = nullptr, bits_ev[2] = {nullptr, nullptr};
    bool caller_dirty = false;       // the caller's stream holds library work that fork_ev does not cover yet
    bool fork_pending = false, follow_pending = false;      // recorded, and the lane has not been made to wait for it yet
    bool tail_live = false, bits_live[2] = {false, false};  // the event has been recorded at least once
    float* ws_lane = nullptr;        // split-K workspace of the head plans when they run on the lane (c->ws stays the trunk's)
    int fpn_step = -1;               // index in `backbone` of the first FPN step (the first lateral): where the trunk joins the lane
    long long lane_stats[4] = {0, 0, 0, 0};      // apse_lane_stats
    bool fwd_counted = false;        // this forward (since the last apse_backbone) is already in lane_stats[0]
    // stateless-op scratch
    uint64_t* op_bits = nullptr; unsigned long long* op_sums = nullptr; size_t op_bits_words = 0;
    // C4 (cfg.arch 1, Res5ROIHeads): the RPN on res4, the res5 stage on the box ROIs (c4_res5box, then the 7x7 mean and the
    // predictor in `boxhead`) and again on the detections (the front of `maskhead`)
    bool c4 = false;
    C4Rpn c4r; void* c4_nms = nullptr;
    std::vector<Step> c4_res5box;
};

// Sets the context's error message (apse_create's when c is null: apse_last_error(NULL)) and returns `code`.  detector.hip
int fail(apse_ctx* c, int code, const std::string& msg);
#define HIPCHK(c, call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return fail(c, APSE_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <typename T>
static T* dalloc(apse_ctx* c, size_t n, bool zero = true) {
    void* p = nullptr;
    if (hipMalloc(&p, n * sizeof(T) > 0 ? n * sizeof(T) : 16) != hipSuccess) return nullptr;
    if (zero) hipMemset(p, 0, n * sizeof(T));
    c->allocs.push_back(p);
    return reinterpret_cast<T*>(p);
}
template <typename T>
static T* dupload(apse_ctx* c, const std::vector<T>& v) {
    T* p = dalloc<T>(c, v.size(), false);
    if (p && !v.empty()) hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return p;
}

// ---- host helpers that the stateless operators share with the context
static inline int pow2_at_least(int v) { int p = 4; while (p < v) p <<= 1; return p; }
// plan.hip
void pack_oihw(const float* w, int Cout, int Cin, int KH, int KW, int cin_p, const float* scale, float* out, int KWCp);
std::vector<float> winograd_filters(const float* oihw, int Cout, int Cin, int cin_p);
// The FPN RPN selection plan: the five levels (head rows, cell anchors, k), the top-k tournament (4096-key sort jobs, then
// merges of up to four lists per job until one list per level is left), the number of 1024-key list slots and each level's
// final slot.  The context (build_plan) and the stateless apse_rpn_select both run the plan this function makes.
struct RpnSelectPlan {
    RpnLevels levels;
    std::vector<std::vector<TopkJob>> stages;
    int nslots;
    int final_slot[5];
};
void rpn_select_plan(const float* const head[5], const int H[5], const int W[5], int head_ld, int pre_topk, RpnSelectPlan* out);
// The five levels alone (head rows, cell anchors, n, k = min(pre_topk, n)): all the training-time selection needs
void rpn_levels_desc(const float* const head[5], const int H[5], const int W[5], int head_ld, int pre_topk, RpnLevels* out);
// The C4 RPN descriptor: head rows, the 15 cell anchors (sizes outer, ratios inner), n and k
void c4_rpn_desc(const float* head, int H, int W, int ld, int pre_topk, C4Rpn* R);
int build_plan(apse_ctx* c);        // FPN (cfg.arch 0)
int build_plan_c4(apse_ctx* c);     // C4 (cfg.arch 1)
// detector.hip (apse_set_camera)
int fill_camera(UndistortParams& p, int H, int W, const double* m, const double* dist, int ndist, int do_undistort, int do_gamma);
