/* apse_hip.h -- C ABI of libapse_hip.so: the MI355X (gfx950) implementation of the per-frame
 * hot path of vision-agh/apse_uav's dcnn/ subsystem.
 *
 * The reference has no FFI layer: its boundary is the Python surface
 *   dcnn/engines/track_predictor.py:31-52  TrackPredictor.__call__   (resize + TrackRCNN.inference)
 *   dcnn/networks/track_rcnn.py:16-58      TrackRCNN.inference       (preprocess, backbone+FPN, RPN, ROI heads, postprocess)
 *   dcnn/engines/rcnn_tracker.py:156-221   get_features_rois, association head, distance matrix
 *   dcnn/utils/mask_utils.py:6-38          get_mask_centroid, compute_closest_point
 *   dcnn/utils/mask_utils.py:41-77         compute_masks_iou, translate_and_crop_mask (the 'mask_iou' association metric)
 * Each entry point below names the reference code it replaces.  apse_uav_amd/_lib.py is the ctypes
 * binding; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 (APSE_OK) or a negative APSE_E_* code; apse_last_error()
 * gives the text.  Pointers named *_dev are device pointers owned by the caller; `stream` is a
 * hipStream_t passed as void*.  Calls enqueue work and return; only apse_read_results (or its _end half) waits.
 * A context is bound to one device and is not thread-safe (one per process rank).
 */
#ifndef APSE_HIP_H
#define APSE_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define APSE_OK 0
#define APSE_E_INVALID (-1)
#define APSE_E_HIP (-2)
#define APSE_E_NOMEM (-3)
#define APSE_E_STATE (-4)
#define APSE_E_MISSING (-5)

typedef struct apse_ctx apse_ctx;

/* Hyper-parameters that define results (dcnn/configs/Base-RCNN-FPN.yaml,
 * dcnn/scripts/tests/visualize_uav.py:30-48, dcnn/engines/rcnn_tracker.py:33).
 *
 * Limits (apse_create refuses a config outside them with APSE_E_INVALID; every kernel launches for a config inside them):
 *   1 <= frame_w <= APSE_MAX_FRAME_W (49152), any width (no alignment): the horizontal resize pass stages one source row in LDS,
 *       W*3 bytes + 15 bytes of slack for rows that are not dword-aligned + 32 zero tap slots, next to the fused form's Lab
 *       tables (14.7 KB); that has to fit the 160 KiB of one workgroup.  apse_resize_normalize has the same bound.
 *   1 <= frame_h <= APSE_MAX_FRAME_H (32768): with the width bound, frame_h * frame_w < 2^31 - 64, so the 32-bit pixel keys of
 *       the mask tail (y * frame_w + x, plus a 64-pixel word) and the host decode of them cannot overflow.  (Batches of more than
 *       2^31 bytes of frames still run; they take the undistort path without the compact remap table.)
 *   max_batch <= 64, dets_per_image <= 100, max_batch * dets_per_image <= 1024 (the packed detection list of the mask and
 *       association heads);
 *   1 <= num_classes <= APSE_MAX_CLASSES (80, COCO): up to 6 classes the box head runs the narrow kernels (one thread per ROI, a
 *       32-wide fused predictor row), from 7 on the wide ones (one wave per ROI, a round_up(5 * num_classes + 1, 32)-wide row,
 *       class-major candidate lists, one sort of at most num_classes * dets_per_image <= 8192 kept keys per image);
 *   rpn_post_topk * min(num_classes, ceil(1 / score_thresh) - 1) < 40000: fewer than 1 / score_thresh classes of a ROI can score
 *       above score_thresh, so this bounds the box candidates of an image below the count at which detectron2 0.1.2's
 *       batched_nms switches to a method without the category offset (COCO's 1000 x 19 = 19000 passes; 0.01 at 80 classes does not);
 *   rpn_pre_topk, rpn_post_topk <= 1000; embed_dim <= 256; compute_dtype 1 / 2 needs storage16 = 1.
 * C4 (arch = 1, detectron2 Base-RCNN-C4 / Res5ROIHeads) instead:
 *   rpn_pre_topk <= APSE_C4_MAX_PRE_TOPK (6000, detectron2's C4 PRE_NMS_TOPK_TEST; one single-level list per image);
 *   compute_dtype 0 (exact f32 only);
 *   max_batch <= APSE_C4_MAX_BATCH (2): the res5 stage runs on every box ROI, and its pooled input alone is
 *       rpn_post_topk x 14 x 14 x 1024 f32 = 0.8 GB per frame (about 2.5 GB of activations per frame in all); two frames
 *       keep every activation tensor below 2^31 bytes, the byte range the implicit-GEMM kernels address;
 *   the image is not padded (size_divisibility 0), blocks[3] = the roi_heads.res5 block count, and assoc_scale is the
 *       res4 width over the frame width. */
#define APSE_MAX_CLASSES 80
#define APSE_C4_MAX_PRE_TOPK 6000
#define APSE_C4_MAX_BATCH 2
#define APSE_MAX_FRAME_W 49152
#define APSE_MAX_FRAME_H 32768
typedef struct apse_config {
    int struct_size;              /* sizeof(apse_config), ABI check */
    int device;
    int max_batch;                /* frames per forward (reference: 1), 1..64 */
    int frame_h, frame_w;         /* original frame, e.g. 2160 x 3840 or 375 x 1242; any size within the limits above */
    int image_h, image_w;         /* after ResizeShortestEdge, e.g. 750 x 1333 */
    int blocks[4];                /* bottlenecks per stage, R-101 = 3,4,23,3 (C4: blocks[3] = roi_heads.res5 blocks) */
    int num_classes;              /* 4 (1..APSE_MAX_CLASSES = 80) */
    float score_thresh;           /* 0.5 */
    float box_nms;                /* 0.5 */
    float rpn_nms;                /* 0.7 */
    float mask_thresh;            /* 0.5 */
    int rpn_pre_topk;             /* 1000 (<= 1000) */
    int rpn_post_topk;            /* 1000 (<= 1000) */
    int dets_per_image;           /* 100  (<= 100) */
    float pixel_mean[3];          /* BGR means */
    int assoc_roi;                /* 10 */
    int embed_dim;                /* 128 */
    float assoc_scale;            /* roi_pool spatial scale = p2 width / frame width (rcnn_tracker.py:165); C4: res4 width */
    int compute_dtype;            /* 0 = exact f32 MFMA everywhere (reference numerics); 1 = bf16, 2 = f16 matrix cores with
                                     f32 accumulate for the trunk / head GEMMs (decision layers stay f32) */
    int storage16;                /* with compute_dtype 1/2: must be 1 = activations live in HBM in the 16-bit operand type (half
                                     the traffic, no conversion on the way to the matrix cores).  The f32-storage variant of
                                     the 16-bit modes was removed in round 4 (apse_create refuses it); ignored for f32 */
    int arch;                     /* 0 = FPN + StandardROIHeads (Base-RCNN-FPN); 1 = C4 + Res5ROIHeads (Base-RCNN-C4): stem and
                                     res2..res4 (keys backbone.stem.*, backbone.res{2,3,4}.N.*), the RPN on res4 with 15 anchors,
                                     roi_heads.res5 on 14 x 14 ROIAlign crops of res4, 14 x 14 masks, association on res4.  A
                                     caller passing the struct_size of the layout without this field gets 0 */
    int tail_lane;                /* 0 = default: the proposal selection, heads and results copy of a forward that runs ahead of a
                                     read go to a second stream of the context (the tail lane, see "per-frame stages" below);
                                     < 0 = off: every launch on the caller's stream.  The environment variable APSE_TAIL_LANE=0 (read at apse_create) switches it
                                     off for every context; C4 (arch 1) never has one.  A caller passing the struct_size of a layout
                                     without this field gets 0 */
} apse_config;

/* Byte offsets of the per-forward results block (one D2H copy, apse_read_results). n = max_batch*dets_per_image. */
typedef struct apse_results_layout {
    size_t bytes;
    int n_max, dets_per_image, embed_dim, max_batch;
    size_t total;        /* int                 number of packed detections                           */
    size_t offset;       /* int  [max_batch+1]  first packed index of each image                      */
    size_t prop_count;   /* int  [max_batch]    RPN proposals kept per image                          */
    size_t img;          /* int  [n]            image of each detection                               */
    size_t cls;          /* int  [n]            predicted class                                       */
    size_t roi;          /* int  [n]            proposal index the detection came from (-1 given box) */
    size_t score;        /* f32  [n]                                                                  */
    size_t box_resized;  /* f32  [n][4]         box in resized-image pixels                           */
    size_t box;          /* f32  [n][4]         box in frame pixels (scaled + clipped)                */
    size_t valid;        /* int  [n]            box non-empty after scaling (detector_postprocess)    */
    size_t rect;         /* int  [n][4]         paste window x0,y0,x1,y1                              */
    size_t mass;         /* int  [n]            mask pixel count                                      */
    size_t centroid;     /* int  [n][2]         1-based floor centroid, -1 if empty                   */
    size_t closest;      /* int  [n][dets_per_image][2]  closest mask pixel of det i to the centroid of
                                                 the j-th detection of the same image, -1 if none     */
    size_t embedding;    /* f32  [n][embed_dim] L2-normalised association embedding                   */
} apse_results_layout;

/* ---- lifetime ---- */
int apse_create(const apse_config* cfg, apse_ctx** out);
void apse_destroy(apse_ctx* ctx);
const char* apse_last_error(apse_ctx* ctx);          /* ctx may be NULL: last creation error */
const char* apse_version(void);

/* ---- weights: replaces DetectionCheckpointer.load / load_state_dict (track_predictor.py:20-21,
 * rcnn_tracker.py:55-57).  Names are detectron2 state_dict keys, plus "association.fc.weight|bias".
 * Host f32 arrays in PyTorch layout.  apse_finalize_weights folds FrozenBN into the convolutions,
 * re-lays the filters out for the implicit-GEMM kernels, uploads them and builds the launch plan. */
int apse_set_weight(apse_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
int apse_finalize_weights(apse_ctx* ctx);

/* Pillow resampling tables for frame->image (host int32; computed by the caller exactly as Pillow's
 * precompute_coeffs/normalize_coeffs_8bpc do): bounds [out][2] = (first, count), coef [out][ksize]. */
int apse_set_resize_tables(apse_ctx* ctx, const int* hbounds, const int* hcoef, int hksize, const int* vbounds,
                           const int* vcoef, int vksize);

/* Optional: preprocess_img of dcnn/scripts/tests/visualize_uav.py:56-71 (cv2.undistort with data/cam_params.json + gamma on the
 * Lab L channel) fused into apse_preprocess_frames -- the raw frame is undistorted / gamma-corrected while the horizontal
 * resize pass stages its rows, so no pre-processed 4K frame is ever written to HBM.  m: 3x3 camera matrix (row-major, host
 * f64), dist: up to 14 coefficients (k1 k2 p1 p2 k3 k4 k5 k6 s1..s4, tilt terms must be 0), lut: 256-entry L table (host).
 * do_undistort = do_gamma = 0 switches it off.  Synchronous (small host -> device copy). */
int apse_set_camera(apse_ctx* ctx, const double* m9, const double* dist, int ndist, const uint8_t* lut256_host, int do_undistort,
                    int do_gamma);

/* ---- per-frame stages ----
 * All enqueue and return.  apse_preprocess_*, apse_backbone and the convolutions of apse_rpn(_levels) go to `stream`.  The rest
 * of a forward -- proposal selection, apse_box_head / apse_set_detections, apse_mask_tail, apse_embed -- and the copy of
 * apse_read_results(_begin) go to `stream` too, unless the forward RUNS AHEAD: when apse_backbone is called between
 * apse_read_results_begin and _end (the software-pipelined loop), that forward's rest goes to the context's TAIL LANE, a
 * non-blocking stream of its own that follows `stream` by an event behind the RPN convolutions.  The next forward's stem..res5 on `stream` therefore run beside this forward's tail; its first
 * FPN step waits for the tail (the FPN overwrites the maps the heads read), so at most one forward runs ahead.  Results are
 * the same bits.  What a caller must know:
 *   - synchronising `stream` does NOT wait for the heads of a forward that ran ahead: results are complete when apse_read_results(_end) returns,
 *     and every other entry that touches the context (apse_copy_mask_window(s), apse_export_feature, apse_debug_tensor,
 *     apse_roi_features, apse_mask_roi_features, apse_box_roi_features, apse_proposals, apse_profile, apse_set_camera) first makes `stream` (or the host) wait for the lane;
 *   - use one `stream` per context for the calls of one forward.
 * The lane is off -- every launch on `stream`, in the order of the calls -- with apse_config.tail_lane < 0, APSE_TAIL_LANE=0,
 * under C4 and while apse_profile is enabled. */
/* ResizeShortestEdge.apply_image (PIL bilinear) + preprocess_image: u8 BGR frames [B][frame_h][frame_w][3]
 * -> internal normalised, /32-padded network input (track_predictor.py:48-49, track_rcnn.py:35). */
int apse_preprocess_frames(apse_ctx* ctx, const uint8_t* frames_dev, int batch, void* stream);
/* The same from YUV 4:2:0 frames, as video decoders hand them out: `batch` contiguous frames of the context's frame_h x frame_w
 * in `format` (APSE_FMT_*) with row pitch `pitch` bytes, converted with `matrix` (APSE_YUV_*).  The conversion runs inside the
 * horizontal resize pass while it stages a source row (luma row y, chroma row y >> 1 -> the row's BGR bytes in LDS), so the
 * network input holds the bytes apse_preprocess_frames builds from apse_yuv_to_bgr's output, and no BGR frame is written.
 * With a camera set (apse_set_camera) the frames are first converted into BGR frames owned by the context (allocated at the
 * first such call), then pre-processed as BGR: "convert, then preprocess_img".  Same contract as apse_preprocess_frames
 * otherwise (stream, tail lane, arch 1).  APSE_E_INVALID: a layout outside the rules at APSE_FMT_*, an unknown matrix, a batch
 * of 2 GiB or more. */
int apse_preprocess_frames_yuv(apse_ctx* ctx, const uint8_t* frames_dev, int batch, int pitch, int format, int matrix, void* stream);
/* Same from already-resized f32 CHW images [B][3][image_h][image_w] (the reference's model input). */
int apse_preprocess_images(apse_ctx* ctx, const float* images_dev, int batch, void* stream);
/* ResNet-101 + FPN (track_rcnn.py:42); C4: stem + res2..res4. */
int apse_backbone(apse_ctx* ctx, int batch, void* stream);
/* RPN head + proposal selection (track_rcnn.py:46). */
int apse_rpn(apse_ctx* ctx, int batch, void* stream);
/* Same with proposals taken only from the FPN levels in `level_mask` (bit 0 = p2 .. bit 4 = p6); mask 16 is
 * SelectiveRPN.gen_partial_proposals (dcnn/networks/selective_rpn.py:14-86: last level only). */
int apse_rpn_levels(apse_ctx* ctx, int batch, int level_mask, void* stream);
/* Box branch + FastRCNNOutputs.inference (track_rcnn.py:51) -> packed detection list. */
int apse_box_head(apse_ctx* ctx, int batch, void* stream);
/* roi_heads.forward_with_given_boxes (track_rcnn.py:52-54): host arrays, boxes in resized-image pixels,
 * counts[batch] detections per image, concatenated.  Replaces apse_rpn + apse_box_head.  Enqueues only: the arrays are
 * copied into pinned staging owned by the context before the call returns and may be freed by the caller at once. */
int apse_set_detections(apse_ctx* ctx, const float* boxes_host, const int* classes_host, const float* scores_host,
                        const int* counts_host, int batch, void* stream);
/* Mask branch + detector_postprocess/paste + centroids + closest-point table
 * (track_rcnn.py:51,57; mask_utils.py:6-38).  Idempotent on one detection list: a repeated call (a timing loop) gives the
 * same masses / centroids, not doubled ones. */
int apse_mask_tail(apse_ctx* ctx, int batch, void* stream);
/* roi_pool(p2) + AssociationHead (rcnn_tracker.py:156-189, association_head.py:16-27); with apse_set_crop_features on, the
 * mask-cropped roi_align instead of roi_pool (after apse_mask_tail of the same detection list). */
int apse_embed(apse_ctx* ctx, int batch, void* stream);
/* RoiFeaturesGenerator.get_rois_features (dcnn/engines/roi_features_generator.py:68-117; FPN only), to be called after
 * apse_backbone: RoI features of image `image` of the batch on p2 for the association-head training batches.
 * rois_dev: [n][4] x1,y1,x2,y2 in ORIGINAL-frame pixels.  masks_dev == NULL: torchvision roi_pool (:113);
 * else [n][frame_h][frame_w] u8 (non-zero = inside): p2 * bilinear-resized mask, then roi_align(aligned=False,
 * sampling_ratio=4) (:95-111).  out_dev: f32 [n][256][roi_size][roi_size]. */
int apse_roi_features(apse_ctx* ctx, int image, const float* rois_dev, const uint8_t* masks_dev, int n, int roi_size,
                      float* out_dev, void* stream);
/* apse_roi_features with the masks as bit windows: windows_dev is apse_mots_window[n] on the device (the struct under "MOTS
 * evaluation" below; frame pixels, a bit counts only inside its rect, NULL bits or an empty rect = the empty mask, the row stride
 * may exceed what the rect needs), e.g. what apse_mots_rle_to_bits filled.  One kernel evaluates the bilinear resize of each
 * 0 / 1 mask to p2's size from the bits and takes roi_align(aligned=False, sampling_ratio=4) of p2 * mask: no dense mask, no
 * scratch, and out_dev is bit for bit what apse_roi_features writes for the same masks given densely.  Same checks, same lane
 * join; windows_dev must not be NULL when n > 0. */
struct apse_mots_window;
int apse_roi_features_windows(apse_ctx* ctx, int image, const float* rois_dev, const struct apse_mots_window* windows_dev, int n,
                              int roi_size, float* out_dev, void* stream);
/* Crop features (rcnn_tracker.py:166-180, get_features_rois(crop_features=True)): context state, default 0.  With it on,
 * apse_embed replaces roi_pool by roi_align(aligned=False, sampling_ratio=4) of p2 * mask at the detections' boxes (same
 * assoc_scale, same assoc_roi), each detection's mask being the bit plane and rect that apse_mask_tail wrote for the same detection
 * list, resized bilinearly to p2's padded size inside the kernel; a detection whose `valid` is 0 reads the empty mask.  The FC, the
 * normalise and the results layout are unchanged.  apse_embed then returns APSE_E_STATE when no apse_mask_tail has run since the
 * detections were set (apse_box_head / apse_set_detections).  APSE_E_INVALID with on != 0 under C4 (arch 1): the branch reads p2
 * with 256 channels. */
int apse_set_crop_features(apse_ctx* ctx, int on);
/* backbone + rpn + box_head + mask_tail + embed. */
int apse_forward(apse_ctx* ctx, int batch, void* stream);

/* ---- results ---- */
int apse_results_describe(apse_ctx* ctx, apse_results_layout* out);
/* Copies the results block to host memory (layout->bytes) and waits for the copy (the implicit device sync of the reference loop:
 * rcnn_tracker.py:132 `.cpu()`, mask_utils.py:19,23,38 `.item()`).  = _begin + _end. */
int apse_read_results(apse_ctx* ctx, void* host_dst, size_t bytes, void* stream);
/* The same in two halves: _begin enqueues the copy (and an event behind it) and returns; _end waits for that copy only -- work the
 * caller enqueued on the stream in between is not waited for.  That may be the NEXT frame's apse_preprocess_frames AND its whole
 * forward: nothing in it depends on this frame, stream order keeps this copy in front of everything the forward overwrites, and the
 * mask bit planes alternate between two sets per forward, so apse_copy_mask_window after _end still reads THIS frame's masks.
 * host_dst must stay valid and unread until _end returns.  The closest-point table is decoded on the host inside _end (the device
 * leaves (distance, pixel index) keys in that field). */
int apse_read_results_begin(apse_ctx* ctx, void* host_dst, size_t bytes, void* stream);
int apse_read_results_end(apse_ctx* ctx, void* host_dst);
/* Tail lane counters since apse_create: out4[0] forwards whose tail was enqueued on the lane, [1] times another entry had to
 * wait for unfinished lane work, [2] first-FPN-step waits whose event was not yet complete when the trunk was enqueued,
 * [3] times the lane was emptied by a host wait (apse_profile, apse_set_camera, and apse_read_results_end when no forward was
 * enqueued behind the read: the lane's stream is then destroyed until a forward runs ahead again). */
int apse_lane_stats(apse_ctx* ctx, long long* out4);
/* Copies detection i's mask window (rows rect.y0..y1, 64-bit words (x0>>6)..((x1+63)>>6)) to dst_dev: the masks of the forward whose
 * results were last read (apse_read_results / _begin), or of the last forward when no read has been started since. */
int apse_copy_mask_window(apse_ctx* ctx, int det, int x0, int y0, int x1, int y1, uint64_t* dst_dev, void* stream);
/* The same for n detections in ONE launch (n <= 100): window k = detection dets[k], rect rects[k] = x0,y0,x1,y1, written as
 * (y1 - y0) rows of ((x1 + 63) >> 6) - (x0 >> 6) words at dst_dev + dst_word_offsets[k].  Host arrays, read before the call returns. */
int apse_copy_mask_windows(apse_ctx* ctx, int n, const int* dets_host, const int* rects_host, uint64_t* dst_dev,
                           const long long* dst_word_offsets_host, void* stream);
/* Named internal tensor -> caller buffer as NCHW f32 (p2..p6, res2..res5, stem; C4: res2..res4, stem): the feature dict
 * TrackRCNN.inference returns (track_rcnn.py:57-58).  dims (B,C,H,W) via apse_feature_shape. */
int apse_feature_shape(apse_ctx* ctx, const char* name, int* chw3);
int apse_export_feature(apse_ctx* ctx, const char* name, float* dst_nchw_dev, int batch, void* stream);
/* Debug/parity taps: copy a named intermediate (device, raw layout) to dst_dev; returns element count in *count. */
int apse_debug_tensor(apse_ctx* ctx, const char* name, void* dst_dev, size_t max_bytes, size_t* bytes, void* stream);
/* Algorithmic FLOPs of one forward for `batch` images with the given proposal/detection totals. */
double apse_flops(apse_ctx* ctx, int batch, double proposals, double detections);

/* Per-kernel timing with HIP events on the caller's stream (one pair per convolution launch, collected at
 * apse_read_results).  out42 = [14 kernel shapes][3] = {sum ms, sum algorithmic FLOPs, launches}; shapes
 * 0..3 = 128x128, 64x64, 128x32, 128x64 implicit-GEMM tiles, 4..7 their 32-deep / 8-wave variants, 8 = 256x128,
 * 9 / 10 = the memory-streaming 1x1 kernels, A strip resident / streamed, 11 = the LDS-DMA
 * 256x128 kernel of the 16-bit modes, 12 = the fused stem + max-pool kernel of the 16-bit modes, 13 = the <= 16-channel
 * head kernel (a split-K launch includes its reduce pass).  With the two-half read a forward enqueued between
 * apse_read_results_begin and _end keeps its own event pairs: _end accounts exactly the forward whose results it returns. */
int apse_profile(apse_ctx* ctx, int enable);
int apse_profile_read(apse_ctx* ctx, double* out42, int reset);

/* ---- stage-level operators (stateless; used by the parity tests and by host-side helpers) ---- */
typedef struct apse_conv_desc {
    int B, H, W, Cin;       /* NHWC input, Cin a power of two >= 4 */
    int Cout, KH, KW, stride, pad;
    int relu;
    int res_mode;           /* 0 none, 1 same-shape residual, 2 nearest-2x upsampled residual */
    int cfg;                /* -1 auto, else tile shape 0..8: 128x128, 64x64, 128x32, 128x64 (64-deep steps for the small
                               ones), 4/5 = 64x64 / 128x32 with 32-deep steps, 6/7 = 64x64 with 8 waves in two k groups, 8 = 256x128
                               (16-bit operands stored 16-bit only; otherwise 128x128) */
    int splitk;             /* 0 auto */
    int prec;               /* 0 f32 MFMA; 1 bf16 / 2 f16 MFMA with f32 accumulate: x must be STORED in that type (x_st == prec),
                               filter rows whole 64-element steps, no fuse_reduce -- anything else is refused */
    int fuse_reduce;        /* split-K: 1 = last-arriving block reduces in the launch, 0 = separate reduce kernel */
    int x_st, res_st, y_st; /* storage type of x / residual / y: 0 f32, 1 bf16, 2 f16 (16-bit tensors need C % 8 == 0;
                               with prec 1/2 a 16-bit x must be stored in the operand type) */
} apse_conv_desc;
size_t apse_conv_packed_elems(const apse_conv_desc* d);
/* OIHW host filter (+ optional per-channel scale) -> packed host filter for apse_conv2d. */
int apse_conv_pack_weight(const apse_conv_desc* d, const float* w_oihw, int cin_real, const float* scale, float* packed);
int apse_conv2d(const apse_conv_desc* d, const float* x_dev, const float* w_packed_dev, const float* bias_dev,
                const float* res_dev, float* y_dev, float* ws_dev, size_t ws_bytes, void* stream);
/* apse_conv2d in the forms the plan gives the ROI heads (a test / tool helper; the descriptor is apse_conv2d's, and with
 * count_dev = NULL, hint_items = y_ld = deconv = 0 so is the launch).  x / res / y are read in the descriptor's storage types.
 * count_dev: device int, the number of live items; rows from min(*count_dev, d->B) * OH * OW on are neither computed nor written
 * (d->B is the capacity in items; the split-K slabs are sized for it).  hint_items > 0: the expected count, which sizes the grid
 * of a counted launch only (rows min(hint_items * OH * OW, M)); no result depends on it.  y_ld > 0: the stride of an output row
 * in elements, >= Cout; columns from roundup(Cout, 4) on are never written, columns Cout .. roundup(Cout, 4) - 1 of a live row
 * are either left alone or written with the epilogue of an all-zero filter row (the padded bias, ReLU applied).  deconv != 0: a
 * 1x1 / stride 1 / pad 0 layer without residual and with Cout a multiple of 16 whose output is scattered as the 2x2 stride-2
 * transposed convolution to [B][2H][2W][Cout / 4] (filter rows (dy * 2 + dx) * Cout / 4 + co, bias of Cout / 4 entries padded
 * like any other).  APSE_E_INVALID, with nothing launched: y_ld < Cout, y_ld with deconv, a 16-bit y with y_ld (or Cout / 4 of a
 * deconvolution) not a multiple of 8, fuse_reduce or an explicit cfg 9 / 11 with a count, a residual with Cout % 4 != 0, and
 * whatever apse_conv2d refuses.  cfg = -1 with a count never takes the stream or LDS-DMA kernels (they are not count-limited). */
int apse_conv2d_ex(const apse_conv_desc* d, const void* x_dev, const float* w_packed_dev, const float* bias_dev, const void* res_dev,
                   void* y_dev, float* ws_dev, size_t ws_bytes, const int* count_dev, int hint_items, int y_ld, int deconv,
                   void* stream);
/* How many launches of this process took the pointwise address form of the tiled kernel (1x1 / pad 0 layers unless the
 * environment has APSE_IGEMM_ADDR=0; csrc/conv_igemm.hip).  A test / tool helper: it shows which kernel a layer ran. */
unsigned apse_conv_pointwise_launches(void);
/* One layer through the fused f32 Winograd F(2x2,3x3) kernel the f32 plan uses for its p2 / p3 3x3 layers (a test / tool helper,
 * like apse_conv2d, which keeps the direct kernels).  apse_winograd_pack_filter: OIHW host filter [Cout][Cin][3][3], Cin a power of
 * two >= 8 -> U = G g G^T, 16 * Cout * Cin floats on the host, the bytes a context uploads.  apse_winograd_conv2d: f32 NHWC in /
 * out, 3x3 / stride 1 / pad 1, Cout a multiple of 64, no residual, every storage type 0; anything else is APSE_E_INVALID. */
int apse_winograd_pack_filter(const float* w_oihw, int Cout, int Cin, float* packed);
int apse_winograd_conv2d(const apse_conv_desc* d, const float* x_dev, const float* wu_dev, const float* bias_dev, float* y_dev,
                         void* stream);
/* The same kernel with the Cin split and the block geometry the f32 plan of a large frame gives its trunk 3x3 layers.  d->splitk
 * (>= 1, at most Cin / 8) shares of whole 8-channel slices go to slabs ws_dev[splitk][B H W][Cout] (needed for splitk > 1 only) and
 * are summed in split order, then bias, then ReLU, by the split-K reduce kernel.  geometry: 0 = blocks of 16 x 4 Winograd tiles
 * (apse_winograd_conv2d's), 1 = 8 x 8.  A workspace too small, a split above Cin / 8, an unknown geometry and whatever
 * apse_winograd_conv2d refuses are APSE_E_INVALID, with y and ws untouched. */
int apse_winograd_conv2d_split(const apse_conv_desc* d, const float* x_dev, const float* wu_dev, const float* bias_dev, float* y_dev,
                               float* ws_dev, size_t ws_bytes, int geometry, void* stream);
int apse_maxpool3x3s2(const float* x_dev, float* y_dev, int B, int H, int W, int C, void* stream);
/* Same on a storage type (0 f32, 1 bf16, 2 f16): the form the 16-bit modes run after the stem. */
int apse_maxpool3x3s2_typed(const void* x_dev, void* y_dev, int B, int H, int W, int C, int storage, void* stream);
/* ROIAlignV2 over 4 levels (NHWC, C = 256); rois [n][4], batch index roi/per_img, all rois live. */
int apse_roi_align(const float* const* feats_dev, const int* hs, const int* ws, const float* rois_dev, int n, int per_img,
                   int out_size, float* out_dev, void* stream);
/* Same with the maps and the output in a storage type (0 f32, 1 bf16, 2 f16): the form the 16-bit modes run (two map cells
   per load instruction); arithmetic is f32 either way. */
int apse_roi_align_typed(const void* const* feats_dev, const int* hs, const int* ws, const float* rois_dev, int n, int per_img,
                         int out_size, int storage, void* out_dev, void* stream);
int apse_roi_pool(const float* feat_dev, int H, int W, const float* rois_dev, const int* roi_img_dev, int n, int out_size,
                  float scale, float* out_dev, void* stream);
/* Generic per-category NMS + ranking on [n] boxes (category = cat_dev[i] given as entry % cat_mod or / cat_div). */
int apse_nms_rank(const float* boxes_dev, const float* scores_dev, const int* valid_dev, int n, int cat_div, int cat_mod,
                  int ncat, float thr, int topk, float* out_boxes_dev, float* out_scores_dev, int* out_index_dev,
                  int* out_count_dev, void* stream);
/* The decision kernels on injected inputs.  Each entry runs the launchers of apse_rpn_levels / apse_box_head, in their order
 * and with their arguments, on scratch of its own, and synchronises `stream` before it returns.  All pointers but heads_dev,
 * H and W are device pointers.
 *
 * apse_rpn_select: the FPN RPN selection (top-k tournament, decode, per-level NMS, rank merge).  heads_dev: five device
 * pointers (a host array), level l [B][H[l]*W[l]][head_ld] f32 with the objectness of anchor a at channel a and its deltas
 * at 3 + 4 a; head_ld >= 15, 1 <= pre_topk <= 1000, level_mask as in apse_rpn_levels.  keys_dev (may be NULL): the final
 * sorted list of every level, [B][5][pre_topk] u64, entries past min(pre_topk, 3 H W) all ones; a key is
 * (~m << 32) | anchor with m = score bits ^ 0x80000000 for a score >= 0 and ~(score bits) below, so that ascending keys are
 * score descending, anchor ascending.  dec_boxes_dev [B][5*pre_topk][4], dec_scores_dev, dec_valid_dev [B][5*pre_topk]
 * (a zero score is +0 whatever the logit's sign); props_dev [B][post_topk][4], prop_scores_dev, prop_entry_dev
 * [B][post_topk] (entry = level * pre_topk + rank; zeros and -1 past the count), prop_count_dev [B]. */
int apse_rpn_select(const float* const* heads_dev, const int* H, const int* W, int head_ld, int B, int image_h, int image_w,
                    int pre_topk, int post_topk, float nms_thr, int level_mask, unsigned long long* keys_dev, float* dec_boxes_dev,
                    float* dec_scores_dev, int* dec_valid_dev, float* props_dev, float* prop_scores_dev, int* prop_entry_dev,
                    int* prop_count_dev, void* stream);
/* Box inference: candidates (softmax, decode with weights 10, 10, 5, 5, clip, score filter), per-class NMS, top
 * dets_per_image, pack.  wide = 0: the one-thread-per-ROI kernels (K <= 7); wide != 0: the wave-per-ROI kernels, list-fed NMS
 * and the rank sort (1 <= K <= 127, K * dets_per_image <= 8192).  pred_dev [B*P][ld]: K + 1 logits (background last), then
 * 4 K deltas; ld >= 5 K + 1; P <= 1024; props_dev [B*P][4], prop_cnt_dev [B].  Out: probs_dev [B*P][K+1]; cand_boxes_dev
 * [B*P*K][4], cand_scores_dev, cand_valid_dev [B*P*K] (entry = roi * K + class); det_boxes_dev [B][dets][4], det_scores_dev,
 * det_entry_dev [B][dets], det_cnt_dev [B]; pk_boxes_dev [B*dets][4], pk_scores_dev, pk_cls_dev, pk_img_dev, pk_roi_dev
 * [B*dets] (the first pk_total entries are written), pk_total_dev [1], pk_offset_dev [B+1]. */
int apse_box_inference(const float* pred_dev, int ld, int K, const float* props_dev, const int* prop_cnt_dev, int P, int B,
                       int image_h, int image_w, float score_thresh, float nms_thr, int dets_per_image, int wide,
                       float* probs_dev, float* cand_boxes_dev, float* cand_scores_dev, int* cand_valid_dev, float* det_boxes_dev,
                       float* det_scores_dev, int* det_entry_dev, int* det_cnt_dev, float* pk_boxes_dev, float* pk_scores_dev,
                       int* pk_cls_dev, int* pk_img_dev, int* pk_roi_dev, int* pk_total_dev, int* pk_offset_dev, void* stream);
/* The C4 proposal path (radix select, decode, long NMS, early-exit scan) on a head [B][H*W][80]: objectness of anchor a at
 * channel a, deltas at 15 + 4 a.  1 <= pre <= 6000, 1 <= post <= 1000.  dec_boxes_dev [B][pre][4], dec_scores_dev,
 * dec_valid_dev [B][pre]; props_dev [B][post][4], prop_scores_dev, prop_entry_dev [B][post] (entry = rank in the decoded
 * list), prop_count_dev [B]. */
int apse_c4_rpn_select(const float* head_dev, int H, int W, int B, int image_h, int image_w, int pre, int post, float nms_thr,
                       float* dec_boxes_dev, float* dec_scores_dev, int* dec_valid_dev, float* props_dev, float* prop_scores_dev,
                       int* prop_entry_dev, int* prop_count_dev, void* stream);
/* mask_utils on a dense bool frame (uint8 0/1): centroid (1-based floor) and closest point to (px, py). */
int apse_mask_centroid_dense(const uint8_t* mask_dev, int H, int W, int* out_xy_mass_host3, void* stream);
int apse_mask_closest_dense(const uint8_t* mask_dev, int H, int W, float px, float py, int* out_xy_host2, void* stream);
/* F.normalize(p=2) rows and the squared-distance matrix of rcnn_tracker.py:192-221. */
int apse_l2_normalize(const float* x_dev, float* y_dev, int n, int D, void* stream);
int apse_sqdist(const float* a_dev, const float* b_dev, int O, int N, int D, float* out_dev, void* stream);
/* PIL resize + normalise as a stand-alone op (tables as in apse_set_resize_tables, device pointers).  Frames of any size with
 * 1 <= H <= APSE_MAX_FRAME_H and 1 <= W <= APSE_MAX_FRAME_W (APSE_E_INVALID otherwise). */
/* preprocess_img (visualize_uav.py:56-71): cv2.undistort + Lab-L gamma on u8 BGR frames [B][H][W][3].
 * mtx3x3 row-major, dist up to 14 coefficients (k1 k2 p1 p2 k3 k4 k5 k6 s1..s4 tx ty; tilt must be 0),
 * lut256_host = the 256-entry L-channel table (HOST memory since round 3: the Lab step is integer arithmetic on tables derived
 * from it on the host, see apse_lab_tables_host).  Either stage can be disabled. */
int apse_undistort_gamma(const uint8_t* src_dev, uint8_t* dst_dev, int B, int H, int W, const double* mtx3x3_host,
                         const double* dist_host, int ndist, const uint8_t* lut256_host, int do_undistort, int do_gamma,
                         void* stream);
/* Host only (no GPU touched): the integer tables of the Lab step (cvtColor RGB2LAB / LAB2RGB of visualize_uav.py:63-69 in the
 * manner of OpenCV's 8-bit path; layout = struct LabTables of csrc/preproc_pixel.h) for a 256-entry L table, written to `out`.
 * Returns the size of the block in bytes (call with out = NULL to query it).  tests/test_host_logic.py compares every entry
 * with the oracle's numpy-built tables. */
size_t apse_lab_tables_host(const uint8_t* lut256_host, void* out, size_t cap);
int apse_resize_normalize(const uint8_t* frames_dev, uint8_t* tmp_dev, float* out_nhwc4_dev, uint8_t* resized_u8_dev,
                          const int* hb_dev, const int* hc_dev, int hk, const int* vb_dev, const int* vc_dev, int vk, int B,
                          int H, int W, int OH, int OW, int PH, int PW, const float* mean3_host, void* stream);

/* ---- YUV 4:2:0 frames.  With CH = (H + 1) / 2 and CW = (W + 1) / 2:
 *   APSE_FMT_NV12  H luma rows of `pitch` bytes, then CH rows of `pitch` bytes holding CW interleaved (U, V) pairs.  Any
 *                  pitch >= max(W, 2 CW) (decoder surfaces are padded), odd W and H allowed; a frame is (H + CH) * pitch bytes.
 *   APSE_FMT_I420  packed: H x W luma, a CH x CW U plane, a CH x CW V plane.  W and H even, pitch == W.
 * A batch is contiguous frames of one geometry, at any byte alignment.  Conversion (csrc/preproc_pixel.h; tests/yuv_ref.py is
 * the numpy restatement): pixel (x, y) takes Y at (x, y) and the chroma sample (x >> 1, y >> 1) -- nearest siting, as
 * OpenCV's COLOR_YUV2BGR_NV12; u = U - 128, v = V - 128, yy = max(0, Y - yoff) * CY,
 *   R = sat8((yy + CVR v + 2^19) >> 20), G = sat8((yy + CVG v + CUG u + 2^19) >> 20), B = sat8((yy + CUB u + 2^19) >> 20)
 * in int32 with a flooring shift.  (yoff, CY, CVR, CVG, CUG, CUB) per matrix: apse_yuv_matrix_host.  APSE_YUV_CV601 holds
 * OpenCV's ITUR_BT_601 constants; the others are rint(2^20 x) of the BT.601 / BT.709 expressions, limited (16..235) or full
 * range.  4K H.264 from a DJI camera is APSE_YUV_BT709. */
#define APSE_FMT_NV12 0
#define APSE_FMT_I420 1
#define APSE_YUV_CV601 0
#define APSE_YUV_BT601 1
#define APSE_YUV_BT709 2
#define APSE_YUV_BT601_FULL 3
#define APSE_YUV_BT709_FULL 4
/* B frames -> u8 BGR [B][H][W][3].  Reads nothing outside the B frames; src and dst at any byte alignment.  Frame sizes as
 * apse_resize_normalize; APSE_E_INVALID (text in apse_last_error(NULL)) for a size, layout or matrix outside the rules. */
int apse_yuv_to_bgr(const uint8_t* src_dev, uint8_t* dst_dev, int B, int H, int W, int pitch, int format, int matrix, void* stream);
/* Host only: the six integers (yoff, CY, CVR, CVG, CUG, CUB) of a matrix. */
int apse_yuv_matrix_host(int matrix, int* out6);
/* apse_resize_normalize from YUV frames: the conversion fused into the row staging, as in apse_preprocess_frames_yuv. */
int apse_resize_normalize_yuv(const uint8_t* frames_dev, int pitch, int format, int matrix, uint8_t* tmp_dev, float* out_nhwc4_dev,
                              uint8_t* resized_u8_dev, const int* hb_dev, const int* hc_dev, int hk, const int* vb_dev,
                              const int* vc_dev, int vk, int B, int H, int W, int OH, int OW, int PH, int PW,
                              const float* mean3_host, void* stream);

/* ---- host-only: native replay of the sequential association from per-frame records (rank 0 of a sharded run).
 * Same rules as RcnnTracker.associate_detections_to_objects / ObjectInstances / generate_log_oneline
 * (rcnn_tracker.py:122-147, object_instances.py:48-162, visualize_uav.py:117-141); no GPU is touched. */
typedef struct apse_replay apse_replay;
apse_replay* apse_replay_create(int host_id, int embed_dim, float dist_thresh, int max_unseen_frames);
void apse_replay_destroy(apse_replay* r);
int apse_replay_step(apse_replay* r, int frame_idx, int n, const float* emb_host, const int* centroid_host,
                     const int* closest_host, char* line_out, int line_cap, int* det_ids_out);
/* nrec records laid end to end in the wire format of the sharded gather (apse_uav_amd/sharding.py::pack_record: count-prefixed,
 * `total_floats` in all; a frame with n detections is 1 + 13 n + 2 n^2 + n * embed_dim floats): one call for a whole run;
 * lines separated by '\n'; returns bytes written. */
long long apse_replay_packed(apse_replay* r, const float* records_host, long long total_floats, int nrec, int dets_per_image,
                             int first_frame, char* lines_out, long long cap);
int apse_replay_max_id(const apse_replay* r);
int apse_replay_next_id(const apse_replay* r);


/* ---- host-only: staging copy of the ingest path.  memcpy(dst, src, bytes) split over a small persistent pool of threads
 * (the caller's thread takes one part): a pageable frame from cv2.VideoCapture.read (visualize_uav.py:188-191) into the pinned
 * buffer its H2D starts from.  threads <= 1 or < 1 MB: plain memcpy.  Calls are serialised. */
int apse_host_copy(void* dst, const void* src, size_t bytes, int threads);

/* ---- track renderer (csrc/render.hip): the picture of utils/track_visualizer.py (TrackVisualizer.draw_instance_predictions,
 * visualize_uav.py:74-82), drawn on the u8 frames [B][H][W][3] by the integer rules of DESIGN.md "Track rendering".  Stateless:
 * no context.  One item = one instance, passed in draw order (the host sorts by box area); at most APSE_RENDER_MAX_ITEMS per call
 * and 100 per image. */
#define APSE_RENDER_MAX_ITEMS 1024
#define APSE_RENDER_MAX_BREAKS 64
#define APSE_RENDER_MAX_LINES 4
typedef struct apse_render_item {
    int image;                    /* frame of the batch the item is drawn on */
    int rect[4];                  /* mask window x0, y0, x1, y1 (frame pixels, half-open) */
    int words_per_row;            /* 64-bit words per window row; word 0 holds pixels (x0 >> 6) << 6 .. +63, bit i = pixel +i */
    const uint64_t* bits;         /* device, (y1 - y0) rows of words_per_row words (WindowMask.bits); NULL: no mask */
    float box[4];                 /* x0, y0, x1, y1 */
    uint8_t rgb[4];               /* colour R, G, B (4th byte unused); placed in B, G, R byte order when bgr != 0 */
    int label_off, label_len;     /* label bytes in labels_dev; '\n' separates lines, lines after the 4th are not drawn */
} apse_render_item;
/* Workspace bytes of a call with n items on H x W frames. */
size_t apse_render_workspace_bytes(int H, int W, int n);
/* Draws n items onto frames_dev and writes the picture to out_dev (out_dev == frames_dev: in place, only the tiles an item reaches
 * are read and written; otherwise the frames are copied first).  items_dev [n] and labels_dev [label_bytes] are device memory;
 * scale_breaks_host [nbreaks <= APSE_RENDER_MAX_BREAKS] (host) holds the least label height at which the glyph scale reaches
 * 2, 3, ... (utils/track_visualizer.py render_scale_breaks).  ws_dev [ws_bytes >= apse_render_workspace_bytes(H, W, n)] is scratch.
 * Enqueues on `stream` only: no allocation, no synchronisation (capturable into a graph). */
int apse_render_instances(const uint8_t* frames_dev, uint8_t* out_dev, int B, int H, int W, int bgr,
                          const apse_render_item* items_dev, int n, const uint8_t* labels_dev, size_t label_bytes,
                          const float* scale_breaks_host, int nbreaks, void* ws_dev, size_t ws_bytes, void* stream);
/* Dense bool/u8 mask [H][W] (nonzero = set) -> words [H][(W + 63) >> 6] in the apse_render_item bit layout (x0 = 0). */
int apse_render_pack_mask(const uint8_t* mask_dev, int H, int W, uint64_t* words_dev, void* stream);
/* Host only: the renderer's 5x7 font, 95 glyphs (bytes 32..126) x 7 rows, bit 4 = leftmost column.  Returns the size in bytes
 * (665); writes it to `out` when cap is large enough. */
size_t apse_render_font_host(uint8_t* out, size_t cap);

/* ---- MOTS evaluation (csrc/mots.hip): the mask arithmetic of mots_tools/mots_eval (pycocotools area / iou / merge over the
 * KITTI MOTS id maps and RLE files) on bit windows, and the id map of utils/mots_evaluation.py (crop_overlapping_masks +
 * result_image_from_objects) straight from the tracker's masks.  Stateless: no context, enqueues on `stream` only, no allocation,
 * no synchronisation.  Every count is an exact integer (integer atomics only), so results are bit-reproducible.
 * A window is the WindowMask layout: rect x0, y0, x1, y1 (frame pixels, half-open), (y1 - y0) rows of words_per_row 64-bit words,
 * word 0 holds pixels (x0 >> 6) << 6 .. +63, bit i = pixel + i.  Bits outside the rect are ignored on input and 0 on output, so
 * two windows of one frame are aligned on absolute 64-pixel columns.
 * Limits (APSE_E_INVALID outside them): frames 1 <= H <= APSE_MAX_FRAME_H, 1 <= W <= APSE_MAX_FRAME_W; id maps u16; at most
 * APSE_MOTS_MAX_OBJECTS values per split and objects per render or RLE call; at most APSE_MOTS_MAX_PAIRS pairs per overlaps or
 * shift_overlaps call and APSE_MOTS_MAX_UNION union members per overlaps call.  KITTI MOTS frames hold tens of objects. */
#define APSE_MOTS_MAX_OBJECTS 1024
#define APSE_MOTS_MAX_PAIRS 65536
#define APSE_MOTS_MAX_UNION 1024
typedef struct apse_mots_window {
    int rect[4];                  /* x0, y0, x1, y1; x0 >= x1 or y0 >= y1: empty */
    int words_per_row;            /* (((x1 + 63) >> 6) - (x0 >> 6)) for the windows this file writes */
    int area;                     /* set pixels (written by apse_mots_split_idmap; informational elsewhere) */
    uint64_t* bits;               /* device, (y1 - y0) * words_per_row words */
} apse_mots_window;
typedef struct apse_mots_object {
    int rect[4];                  /* mask window, as apse_mots_window */
    int words_per_row;
    float score;                  /* owner rule: highest score, ties to the highest index */
    const uint64_t* bits;         /* device; NULL: no pixels */
} apse_mots_object;
/* Workspace bytes of apse_mots_split_idmap. */
size_t apse_mots_split_workspace_bytes(void);
/* u16 id map [H][W] (device) -> its distinct non-zero values in ascending order (np.unique order) in values[k], each with its
 * bounding-box window in windows[k] (rect, words_per_row, area, bits = pool + a packed offset) for k < min(n, max_values).
 * info[0] = n, info[1] = pool words the windows need, info[2] = 1 when the bits were written (n <= max_values and info[1] <=
 * pool_words), 0 otherwise: the caller reads info after the stream and retries with more room.  1 <= max_values <=
 * APSE_MOTS_MAX_OBJECTS.  ws [ws_bytes >= apse_mots_split_workspace_bytes()] is scratch. */
int apse_mots_split_idmap(const uint16_t* idmap, int H, int W, int max_values, uint64_t* pool, size_t pool_words, int* values,
                          apse_mots_window* windows, int* info, void* ws, size_t ws_bytes, void* stream);
/* COCO RLE -> window bits.  Object k's runs are ends[ends_off[k] .. ends_off[k + 1]), the running sums of its counts (column-major
 * over an h x w image, first run = zeros); windows[k] (device: rect, words_per_row, bits) is its window, which must contain every
 * set pixel (the host takes the bounding box from the runs).  Every word of each window is written. */
int apse_mots_rle_to_bits(const int* ends, const int* ends_off, int n, int h, int w, const apse_mots_window* windows,
                          void* stream);
/* out[p] = {|a & b|, |a|, |b|} for pairs[p] = {a, b} over windows[0 .. n_windows).  b = -1: b is the union of the windows
 * union_idx[0 .. n_union) (an empty list is the empty region), and out[p][2] = -1. */
int apse_mots_overlaps(const apse_mots_window* windows, int n_windows, const int* pairs, int npairs, const int* union_idx,
                       int n_union, int* out, void* stream);
/* out[p] = {|T(a) & b|, |T(a)|, |b|} for quads[p] = {a, b, dx, dy} over windows[0 .. n_windows): T(a) has pixel (x, y) set iff a
 * has (x - dx, y - dy) set and 0 <= x < W, 0 <= y < H (translate, zero fill, crop to the frame).  The overlap of
 * dcnn/utils/mask_utils.py:41-77 compute_masks_iou (translate_and_crop_mask, then intersection and union); utils/mask_utils.py
 * divides.  Any dx, dy is legal (a shift of a whole frame or more gives |T(a)| = 0); an index outside the list is the empty
 * mask.  0 <= npairs <= APSE_MOTS_MAX_PAIRS; npairs == 0 is a no-op. */
int apse_mots_shift_overlaps(const apse_mots_window* windows, int n_windows, const int* quads, int npairs, int H, int W,
                             int* out, void* stream);
/* Tracked objects -> u16 id map [H][W] (device): every pixel belongs to the object of highest score among those whose mask holds
 * it (ties: highest index) and takes values_host[owner] (0: a class MOTS does not score), 0 where no mask is set.  Equal to
 * result_image_from_objects(crop_overlapping_masks(objects)).  objects: device [n]; values_host: host [n], 0..65535. */
int apse_mots_render_idmap(const apse_mots_object* objects, const int* values_host, int n, int H, int W, uint16_t* idmap,
                           void* stream);

/* ---- Result writers (csrc/rle_encode.hip): the masks of one frame -> the cropped windows of crop_overlapping_masks, COCO RLE run
 * ends and pycocotools' compressed counts string, without a dense frame.  Stateless, integer only: enqueues on `stream`, no
 * allocation, no synchronisation.  Every output position is a count followed by a scan (no atomics hand out positions), so two
 * runs are bit-identical.  Windows and objects are the layouts above; here words_per_row may exceed
 * ((x1 + 63) >> 6) - (x0 >> 6) (a row stride), and bits outside the rect's columns are ignored.
 * Each entry takes its structs twice: on the device for the kernels and as a host copy (`*_host`, the same values; the bits
 * pointers are only compared with NULL), from which the limits are checked before anything is launched.  APSE_E_INVALID, with no
 * launch: a NULL pointer, n outside 0 .. APSE_MOTS_MAX_OBJECTS, a frame outside 1 <= h <= APSE_MAX_FRAME_H, 1 <= w <=
 * APSE_MAX_FRAME_W, a non-empty rect that leaves the frame, words_per_row too small for the rect, a workspace smaller than its
 * query.  n == 0 is a no-op.  A device struct that breaks these limits although its host copy keeps them is treated as empty.
 * Capacity protocol (as apse_mots_split_idmap): info[0] = the elements needed, info[1] = 1 when they were written; when the
 * need exceeds `cap` nothing is written to the data array, info[1] = 0, and the caller retries with more room.  The offsets
 * array is written either way.  info[0] saturates at INT_MAX. */
#define APSE_MOTS_RLE_SEG_ROWS 64 /* rows one lane walks: a window column is counted in segments of this many rows */
/* crop_overlapping_masks on the words: a pixel stays with object k iff k is the (score, index)-lexicographic maximum among the
 * objects whose mask holds it (the owner rule of apse_mots_render_idmap; equal to the reference's pair loop).  Object k's
 * cropped window (same rect, same words_per_row, every word of it written, 0 outside the rect's columns) goes to pool + pool_off[k]
 * (device int64 [n], in words); stats[k] (device int64 [n][4]) = {set pixels before, set pixels after, sum of (x + 1), sum of
 * (y + 1)} over the cropped mask, from which the host takes the 1-based floor centroid.  An object with NULL bits or an empty
 * rect has no pixels: it writes no words (the caller reserves none for it), its pool_off is not used beyond the range check, and
 * its stats are 0.  An object whose window does not fit pool_words from its offset writes nothing and gets stats -1.  The
 * regions [pool_off[k], pool_off[k] + rows * words_per_row) of the objects that have bits must not overlap. */
int apse_mots_crop_overlaps(const apse_mots_object* objects, const apse_mots_object* objects_host, int n, int H, int W,
                            uint64_t* pool, size_t pool_words, const long long* pool_off, long long* stats, void* stream);
/* Workspace bytes of apse_mots_bits_to_rle for these windows (host copy); 0 for arguments it would refuse. */
size_t apse_mots_rle_workspace_bytes(const apse_mots_window* windows_host, int n, int h, int w);
/* Window bits -> run ends over an h x w image in column-major order: with v(p), p = x * h + y, the window's bit inside its rect
 * and 0 elsewhere, object k's ends are every p in [1, h * w) with v(p) != v(p - 1), ascending, then h * w, preceded by 0 when
 * v(0) = 1: the running sums of pycocotools' counts, the input format of apse_mots_rle_to_bits.  An empty or NULL-bits window
 * gives the single end h * w.  ends [cap], ends_off [n + 1], info [2] are device int arrays. */
int apse_mots_bits_to_rle(const apse_mots_window* windows, const apse_mots_window* windows_host, int n, int h, int w, int* ends,
                          int cap, int* ends_off, int* info, void* ws, size_t ws_bytes, void* stream);
/* Workspace bytes of apse_mots_rle_pack for up to max_ends run ends. */
size_t apse_mots_rle_pack_workspace_bytes(int max_ends);
/* Run ends -> the bytes of pycocotools' compressed counts string (rleToString): count c_i = end_i - end_(i-1), value c_i -
 * c_(i-2) from the fourth count on, 5-bit groups low first with bit 0x20 as continuation, each byte + 48 (1 to 7 bytes per
 * value).  Object k's string is chars[chars_off[k] .. chars_off[k + 1]).  max_ends is the capacity the ends were written with:
 * ends_off[n] > max_ends (the ends were not written) gives info = {-1, 0} and chars_off all 0. */
int apse_mots_rle_pack(const int* ends, const int* ends_off, int n, int max_ends, char* chars, int cap, int* chars_off,
                       int* info, void* ws, size_t ws_bytes, void* stream);

/* ---- COCO evaluation (csrc/coco_eval.hip): the per-pair and per-group arithmetic of pycocotools 2.0 COCOeval for iouType
 * 'bbox' and 'segm' (utils/coco_eval.py keeps the bookkeeping on the host).  Stateless: no context, enqueues on `stream` only, no
 * allocation, no synchronisation.  Every floating-point value is f64 as pycocotools computes it; no float atomics, every reduction
 * is an exact max or an integer sum, so two runs are bit-identical.  Errors: APSE_E_INVALID outside the limits below, with the
 * text in apse_last_error(NULL).
 * Groups: detections and ground truths of one (image, category) pair, as CSR offsets over flat arrays: group k holds detections
 * dt_off[k] .. dt_off[k + 1] and ground truths gt_off[k] .. gt_off[k + 1] (device int [n_groups + 1]); its IoU block [D][G]
 * starts at iou[iou_off[k]] (device int64 [n_groups]).
 * Limits: at most APSE_COCO_MAX_GROUPS groups, APSE_COCO_MAX_GT ground truths and APSE_COCO_MAX_DET detections per group
 * (max_gt / max_dt: the caller's largest group), APSE_COCO_MAX_T IoU thresholds, APSE_COCO_MAX_R recall thresholds,
 * APSE_COCO_MAX_A area ranges, APSE_COCO_MAX_M maxDets values, APSE_COCO_MAX_CATS categories, APSE_COCO_MAX_KEYS detections
 * in one (category, maxDet) list.  COCO val2017 with default Params needs 400k groups, tens of ground truths per group, 100
 * detections per group, T = 10, R = 101, A = 4, M = 3, K = 80 and at most 500k detections per category. */
#define APSE_COCO_MAX_GROUPS (1 << 24)
#define APSE_COCO_MAX_GT 4096
#define APSE_COCO_MAX_DET 4096
#define APSE_COCO_MAX_T 64
#define APSE_COCO_MAX_R 1024
#define APSE_COCO_MAX_A 16
#define APSE_COCO_MAX_M 16
#define APSE_COCO_MAX_CATS 1024
#define APSE_COCO_MAX_KEYS (1 << 24)
#define APSE_COCO_MAX_POLY_OBJECTS (1 << 20)
#define APSE_COCO_MAX_POLY_PARTS (1 << 22)
#define APSE_COCO_MAX_POLY_VERTS (1 << 26)
/* maskApi bbIou: iou[iou_off[k] + d * G + g] for every group k, from XYWH boxes dt_box [n_dt][4] and gt_box [n_gt][4] (f64) and
 * gt_crowd [n_gt] (int, nonzero: crowd).  w = fmin(D0+D2, G0+G2) - fmax(D0, G0) (0 when <= 0), the same for h, i = w*h,
 * u = crowd ? D2*D3 : (D2*D3 + G2*G3) - i, IoU = i / u.  A group without detections or without ground truths writes nothing. */
int apse_coco_box_iou(const int* dt_off, const int* gt_off, const long long* iou_off, int n_groups, int max_dt, int max_gt,
                      const double* dt_box, const double* gt_box, const int* gt_crowd, double* iou, void* stream);
/* COCO polygons -> window bits, equal pixel for pixel to pycocotools rleFrPoly of every part followed by merge (union).  Object
 * i (an h x w image: obj_hw [n_obj][2] = {h, w}, device, and the same values in obj_hw_host) owns parts obj_part_off[i] ..
 * obj_part_off[i + 1]; part p owns vertices part_vert_off[p] .. part_vert_off[p + 1] of xy [n_verts][2] (f64, x then y), closed
 * back to its first vertex.  Vertex coordinates must be finite with |5 v + .5| < 2^31.  edge_off [n_verts + 1] (device) is the
 * exclusive scan of every edge's y-boundary point count: with lo / hi the smaller / larger scaled x (int)(5 x + .5) of the
 * edge's two vertices, the number of columns c in [0, w - 1] with lo <= 5c + 2 and 5c + 3 <= hi (utils/coco.py poly_layout).
 * An edge whose count the device finds different sets info[0] = 1 and writes nothing.  toggles [edge_off[n_verts]] (device int)
 * is scratch.  windows[i] (device: rect, words_per_row, bits) must hold every set pixel; every word of it is written. */
int apse_coco_poly_to_bits(const double* xy, const int* part_vert_off, int n_parts, const int* obj_part_off, int n_obj,
                           const int* obj_hw, const int* obj_hw_host, const int* edge_off, int n_verts, int* toggles,
                           const apse_mots_window* windows, int* info, void* stream);
/* evaluateImg for every (group, area range a, IoU threshold t) at once.  Each group's detections are already in stable score
 * order and cut to maxDets[-1]; dt_area / dt_id (int64) per detection, gt_area / gt_crowd / gt_id per ground truth (ground truths
 * in file order), iou as apse_coco_box_iou writes it.  area_rng_host [A][2] and iou_thrs_host [T] are Params' f64 arrays (host).
 * A ground truth is ignored in range a when crowd or area < lo or area > hi.  Greedy matching, detections in order: the
 * threshold is min(t, 1 - 1e-10); a ground truth already matched (its match > 0) and not crowd is skipped; the pick is the
 * not-ignored ground truth of highest IoU >= threshold (ties to the later one), else the ignored one by the same rule.
 * Outputs (device): dt_match [A][T][n_dt] = the matched ground truth's id (0: none), dt_ignore [A][T][n_dt] = the matched ground
 * truth's ignore flag, or 1 when unmatched (match == 0) with an area outside the range; gt_match [A][T][n_gt] = the matching
 * detection's id (0: none), ground truths in file order; gt_ignore [A][n_gt] in file order. */
int apse_coco_match(const int* dt_off, const int* gt_off, const long long* iou_off, int n_groups, int max_dt, int max_gt,
                    const double* iou, const double* dt_area, const long long* dt_id, int n_dt, const double* gt_area,
                    const int* gt_crowd, const long long* gt_id, int n_gt, const double* area_rng_host, int A,
                    const double* iou_thrs_host, int T, long long* dt_match, unsigned char* dt_ignore, long long* gt_match,
                    unsigned char* gt_ignore, void* stream);
/* Workspace bytes of apse_coco_accumulate for n_keys detections over all (category, maxDet) lists (0 outside the limits). */
size_t apse_coco_accumulate_workspace_bytes(long long n_keys);
/* The sort of apse_coco_accumulate on its own: list s = seg_idx[seg_off[s] .. seg_off[s + 1]) (indices into score, device
 * f64) -> sorted_idx[seg_off[s] ..] (device int [n_keys]) in the order of np.argsort(-score[list], kind='mergesort'): descending,
 * -0 and +0 equal, NaN last, ties in list order.  At most APSE_COCO_MAX_CATS * APSE_COCO_MAX_M lists of at most max_seg <=
 * APSE_COCO_MAX_KEYS keys; ws [ws_bytes >= apse_coco_accumulate_workspace_bytes(n_keys)] is scratch. */
int apse_coco_sort_lists(const double* score, const int* seg_off, int n_seg, const int* seg_idx, long long n_keys, int max_seg,
                         int* sorted_idx, void* ws, size_t ws_bytes, void* stream);
/* COCOeval.accumulate.  The list of (maxDet index m, category k) is segment m * K + k: seg_idx[seg_off[s] .. seg_off[s + 1])
 * holds the detection indices (into dt_score and the match outputs) of each image's first maxDets[m] detections of category k,
 * concatenated in image order; max_seg is the longest list.  Each list is sorted stably by descending score (the order of
 * np.argsort(-scores, kind='mergesort')).  npig (k, a) counts gt_ignore[a][g] == 0 over cat_gt_off[k] .. cat_gt_off[k + 1].
 * tp = match != 0 and not ignored, fp = match == 0 and not ignored, rc = tp / npig, pr = tp / ((fp + tp) + 2^-52) and its suffix
 * maximum; for each recall threshold rec_thrs[r] (device f64 [R]) the first i with rc[i] >= rec_thrs[r] gives precision and
 * scores, 0 past the end.  Writes precision [T][R][K][A][M], scores [T][R][K][A][M] and recall [T][K][A][M] (device f64); a
 * (k, a) with npig == 0 is -1 throughout. */
int apse_coco_accumulate(const double* dt_score, const long long* dt_match, const unsigned char* dt_ignore, int n_dt,
                         const unsigned char* gt_ignore, int n_gt, const int* cat_gt_off, const int* seg_off,
                         const int* seg_idx, long long n_keys, int max_seg, const double* rec_thrs, int T, int R, int K, int A,
                         int M, double* precision, double* recall, double* scores, void* ws, size_t ws_bytes, void* stream);

/* ---- Association-head training (csrc/assoc_train.hip): the f32 steps of dcnn/scripts/train/train_association_head.py --
 * AssociationHead's fc + F.normalize (dcnn/networks/association_head.py:16-31) forward and backward, batch_hard_triplet_loss and
 * batch_all_triplet_loss (dcnn/online_triplet_loss/losses.py:7-197) with their dE, and torch.optim.SGD's step.  Stateless,
 * enqueue on `stream` only, no allocation; the caller passes the workspace.  Deterministic: no float atomics, fixed reduction
 * orders, ties of max / min to the lowest index -- two runs of a step give bit-identical losses, gradients and weights.
 * Errors: APSE_E_INVALID outside the limits below, with the text in apse_last_error(NULL).
 * Limits: 1 <= n <= APSE_ASSOC_MAX_N rows (embeddings), 1 <= D <= APSE_ASSOC_MAX_D, 1 <= K <= APSE_ASSOC_MAX_K (256 x 32 x 32,
 * the roi_size bound of apse_roi_features).  The triplet entry points also accept n = 0 and then enqueue nothing (the loss of an
 * empty batch is the caller's: NaN for batch-hard's mean, 0 for batch-all). */
#define APSE_ASSOC_MAX_N 2048
#define APSE_ASSOC_MAX_D 256
#define APSE_ASSOC_MAX_K (256 * 32 * 32)
/* Workspace bytes of apse_assoc_fc_forward / _backward (0 outside the limits). */
size_t apse_assoc_fc_workspace_bytes(int n, int K, int D);
/* x [n][K] (the NCHW RoIs flattened in (C, H, W) order), w [D][K] (fc.weight), b [D] -> e [n][D] = Z / max(|Z|, 1e-12) with
 * Z = x w^T + b, and inv_norm [n] = 1 / max(|Z|, 1e-12) for the backward pass. */
int apse_assoc_fc_forward(const float* x, const float* w, const float* b, int n, int K, int D, float* e, float* inv_norm,
                          float* ws, size_t ws_bytes, void* stream);
/* dE [n][D] -> dZ = (dE - e (e . dE)) inv_norm (F.normalize above its eps), dw [D][K] = dZ^T x, db [D] = sum_i dZ.  Overwrites
 * dw and db (no dx: the RoIs do not require grad). */
int apse_assoc_fc_backward(const float* x, const float* e, const float* inv_norm, const float* de, int n, int K, int D, float* dw,
                           float* db, float* ws, size_t ws_bytes, void* stream);
/* Workspace bytes of the triplet entry points (0 outside the limits).  The forward call leaves the distances and the per-row
 * coefficients there; the backward call of the same loss reads them. */
size_t apse_triplet_workspace_bytes(int n);
/* labels [n] (compared as values), e [n][D] -> loss [1] = batch_hard_triplet_loss(labels, e, margin, squared). */
int apse_triplet_hard_forward(const double* labels, const float* e, int n, int D, float margin, int squared, float* loss,
                              void* ws, size_t ws_bytes, void* stream);
/* -> loss_frac [2] = (loss, fraction_positive_triplets) of batch_all_triplet_loss. */
int apse_triplet_all_forward(const double* labels, const float* e, int n, int D, float margin, int squared, float* loss_frac,
                             void* ws, size_t ws_bytes, void* stream);
/* de [n][D] = grad_loss[0] (device scalar; NULL: 1) x d loss / d e, from the workspace of the forward call. */
int apse_triplet_hard_backward(const float* e, int n, int D, int squared, const void* ws, const float* grad_loss, float* de,
                               void* stream);
int apse_triplet_all_backward(const float* e, int n, int D, int squared, const void* ws, const float* grad_loss, float* de,
                              void* stream);
/* One torch.optim.SGD step on n elements of p with grad g and momentum buffer buf (unused when momentum == 0): first_step != 0
 * sets buf = d_p, as torch does when the buffer does not exist yet.  nesterov needs momentum > 0 and dampening == 0. */
int apse_sgd_step(float* p, const float* g, float* buf, long long n, float lr, float momentum, float dampening,
                  float weight_decay, int nesterov, int first_step, void* stream);

/* ---- Mask-head training (csrc/mask_train.hip): the f32 steps of dcnn/scripts/train/finetune_segmentation.py for
 * MaskRCNNConvUpsampleHead (FPN models: ROIAlign 14 -> 4 x (conv3x3 256 + ReLU) -> deconv 2x2 stride 2 + ReLU -> 1x1 predictor with
 * K class channels) and mask_rcnn_loss.  NHWC f32 activations; the master weights stay in the checkpoint's layouts on the device.
 * Stateless, enqueue on `stream` only, no allocation; the caller passes the workspace (apse_mask_train_workspace_bytes covers every
 * entry below).  Deterministic: no float atomics, every sum has an order fixed by the shapes.  Errors: APSE_E_INVALID outside the
 * limits, with the text in apse_last_error(NULL).  Limits: 1 <= n <= APSE_MASK_TRAIN_MAX_N RoIs per call (the loss entries also
 * take n = 0 and then enqueue nothing), 1 <= K <= APSE_MAX_CLASSES. */
#define APSE_MASK_TRAIN_MAX_N 1024
/* ROIAlignV2 14x14 (aligned, sampling ratio 0) of `n` boxes over p2..p5 of image `image`, detectron2's level assignment: the
 * launch apse_mask_tail runs on its detection list, so the values equal the `mask_pooled` tensor of apse_set_detections +
 * apse_mask_tail for the same boxes.  To be called after apse_backbone (FPN only).  rois_dev [n][4] x1,y1,x2,y2 in RESIZED-image
 * pixels; out_dev f32 [n][14][14][256].  0 <= n <= 2^20 (not bound by the detection list). */
int apse_mask_roi_features(apse_ctx* ctx, int image, const float* rois_dev, int n, float* out_dev, void* stream);
/* Workspace bytes for n RoIs and K classes (0 outside the limits). */
size_t apse_mask_train_workspace_bytes(int n, int K);
/* Elements of a packed filter (= apse_conv_packed_elems of the same shape). */
size_t apse_mask_pack_elems(int Cout, int Cin, int KH, int KW);
/* Device-side filter packing into the rows apse_conv2d reads.  kind 0: w = OIHW [Cout][Cin][KH][KW] -> the bytes
 * apse_conv_pack_weight writes.  kind 1: w = OIHW [Cin][Cout][3][3] of a FORWARD 3x3 layer -> the filter of its data gradient
 * (taps flipped, channels transposed; Cout here = the forward layer's Cin).  kind 2: w = ConvTranspose2d [Cin][Cout / 4][2][2] ->
 * the 1x1 filter with rows (dy * 2 + dx) * Cout / 4 + co that the deconvolution runs as.  bias_packed (optional): bias (or zeros
 * when bias == NULL) padded to a multiple of 128 entries. */
int apse_mask_pack_weight(const float* w_dev, const float* bias_dev, int kind, int Cout, int Cin, int KH, int KW, float* packed_dev,
                          float* bias_packed_dev, void* stream);
/* y = conv(x) (+ bias, ReLU) on the inference kernel (conv_igemm_f32), tile shape and K split chosen as a max_batch = 1 context
 * chooses them for its mask head: the result does not depend on n and equals that context's bits.  x [n][H][W][Cin]; deconv != 0:
 * a 1x1 layer with Cout = 4 x channels whose output is scattered to [n][2H][2W][Cout / 4]. */
int apse_mask_conv_forward(const float* x_dev, const float* w_packed_dev, const float* bias_packed_dev, int n, int H, int W, int Cin,
                           int Cout, int KH, int KW, int stride, int pad, int relu, int deconv, float* y_dev, float* ws,
                           size_t ws_bytes, void* stream);
/* The 256 -> 256 3x3 layers (stride 1, pad 1) on [n][14][14][256]: y = conv(x) (+ bias, ReLU) from a kind 0 pack (forward of
 * mask_fcnN) or a kind 1 pack (its data gradient), on the exact-f32 MFMA with the reduction summed as 36 chains of 64 (the
 * inference kernel runs one long chain per K split; the forward error of training feeds the ReLU masks of the gradients). */
int apse_mask_conv3x3(const float* x_dev, const float* w_packed_dev, const float* bias_packed_dev, int n, int relu, float* y_dev,
                      void* stream);
/* g = y > 0 ? dy : 0 over `elems` floats (a multiple of 4; g may alias dy). */
int apse_mask_relu_grad(const float* y_dev, const float* dy_dev, long long elems, float* g_dev, void* stream);
/* db [256] = column sums of g [rows][256]: rows in ascending order inside at most 512 slices, slices in ascending order. */
int apse_mask_bias_grad(const float* g_dev, long long rows, float* db_dev, float* ws, size_t ws_bytes, void* stream);
/* Weight gradient as an implicit GEMM on the exact-f32 MFMA, split over the RoI pixels, partial tiles added in chunk order.
 * kind 0 (3x3, stride 1, pad 1): a = dY [n][14][14][256], b = X [n][14][14][256] -> dw [256][256][3][3] (OIHW).
 * kind 1 (deconvolution 2x2, stride 2): a = X [n][14][14][256], b = dY [n][28][28][256] -> dw [256][256][2][2] ([Cin][Cout][2][2]). */
int apse_mask_wgrad(const float* a_dev, const float* b_dev, int n, int kind, float* dw_dev, float* ws, size_t ws_bytes, void* stream);
/* mask_rcnn_loss: logits [n][28][28][K], classes [n] (ignored when K == 1), targets [n][28][28] bytes (non-zero = inside) ->
 * out4 = {loss_mask, accuracy, false_positive, false_negative}. */
int apse_mask_loss_forward(const float* logits_dev, int K, const int* classes_dev, const uint8_t* targets_dev, int n, float* out4_dev,
                           void* ws, size_t ws_bytes, void* stream);
/* d [n][28][28] = grad_loss[0] (device scalar; NULL: 1) x (sigmoid(x) - t) / (n x 784) on the ground-truth class channel (the other
 * channels' gradient is 0 and is not stored). */
int apse_mask_loss_backward(const float* logits_dev, int K, const int* classes_dev, const uint8_t* targets_dev, int n,
                            const float* grad_loss_dev, float* d_dev, void* stream);
/* Predictor backward from d: g5 [n][28][28][256] = a5 > 0 ? d x w_pred[class] : 0 (the gradient at the deconvolution's
 * pre-activation), dw [K][256] and db [K] (classes without a RoI: exactly 0).  a5 = the deconvolution's output. */
int apse_mask_predictor_backward(const float* d_dev, const float* a5_dev, const int* classes_dev, const float* w_pred_dev, int n, int K,
                                 float* g5_dev, float* dw_dev, float* db_dev, float* ws, size_t ws_bytes, void* stream);
/* The mask targets of sampled proposals: detectron2's PolygonMasks.crop_and_resize(boxes, 28) of mask_rcnn_loss on the device,
 * byte for byte what utils/COCO_utils.py mask_targets gives for the same boxes and polygons.  The polygons of ONE image, uploaded
 * once: object i owns parts obj_part_off[i] .. obj_part_off[i + 1] (int [n_obj + 1]); part p owns vertices part_vert_off[p] ..
 * part_vert_off[p + 1] (int [n_parts + 1]) of xy [n_verts][2] (f64, x then y, resized-image pixels), closed back to its first
 * vertex.  Row r: the box rois_dev[r] (f32 x1,y1,x2,y2) goes to f64 exactly; the vertices of object matched_dev[r] become
 * ((x - x1) * (28 / max(x2 - x1, 0.1)), (y - y1) * (28 / max(y2 - y1, 0.1))) in f64 without contraction; every part is then
 * rasterised by the rule of apse_coco_poly_to_bits (pycocotools rleFrPoly at h = w = 28) and the parts are ORed.
 * targets_dev u8 [n][28][28] (row y, column x): 1 inside, 0 elsewhere; every byte of the n rows is written and nothing past them.
 * An object without parts, or matched_dev[r] outside 0 .. n_obj - 1, gives an all-zero row.  A row with a scaled coordinate that
 * is not finite or above 2^31 / 5 - 1 in magnitude sets info_dev[0] = 1 (the caller zeroes it first) and its bytes are not
 * meaningful.  One launch, one block per row; no scratch, no allocation, no float atomics; integer XOR / OR only, so two calls
 * give the same bytes.  0 <= n <= APSE_MASK_TRAIN_MAX_N (n = 0 enqueues nothing), mask_size == 28 and the object / part / vertex
 * counts within the APSE_COCO_MAX_POLY_* limits, else APSE_E_INVALID before any launch. */
int apse_coco_mask_targets(const double* xy_dev, const int* part_vert_off_dev, int n_parts, const int* obj_part_off_dev, int n_obj,
                      int n_verts, const float* rois_dev, const int* matched_dev, int n, int mask_size, uint8_t* targets_dev,
                      int* info_dev, void* stream);
/* ---- Bitmask targets (csrc/bitmask_targets.hip): the same targets from bitmask ground truth (RLE, dense masks, result windows),
 * detectron2's INPUT.MASK_FORMAT = "bitmask".  DESIGN.md "Bitmask ground truth".  Windows are the layout of "MOTS evaluation".
 * Stateless, one launch each on `stream`, no scratch, no allocation, no atomics: two calls give the same bytes.
 *
 * Nearest-neighbour resize and / or flip of bit windows.  src [n] (device) are windows in a frame of H x W; xmap [w] and ymap [h]
 * (device int) give the source column of image column x and the source row of image row y.  dst [n] (device, with the same
 * values in dst_host) are windows in the image of h x w whose rect and words_per_row the caller has set and whose bits
 * (device) this writes: destination pixel (x, y) of dst[k]'s rect is set iff source pixel (xmap[x], ymap[y]) of src[k] is set.
 * Every word of each destination window is written; bits outside the rect are 0.  A map entry that points outside the source
 * window reads 0.  The caller derives each destination rect from the source rect and the maps (monotone maps cover one range
 * of columns and of rows); an empty destination rect, or NULL bits, writes nothing.  APSE_E_INVALID, with no launch: a frame
 * or image outside the frame limits, n outside 0 .. APSE_MOTS_MAX_OBJECTS, a NULL pointer, a non-empty dst_host rect that leaves
 * the image or whose words_per_row is too small.  n == 0 is a no-op. */
int apse_mots_remap_windows(const apse_mots_window* src, int n, int H, int W, const int* xmap, const int* ymap, int h, int w,
                            const apse_mots_window* dst, const apse_mots_window* dst_host, void* stream);
/* BitMasks.crop_and_resize(boxes, mask_size): row r of out u8 [n][mask_size][mask_size] is detectron2's ROIAlign((mask_size,
 * mask_size), 1.0, 0, aligned=True) of the 0 / 1 mask of windows[matched[r]] (device [n_obj], image coordinates, image h x w)
 * under rois[r] (device f32 x1,y1,x2,y2), 1 where the average is >= 0.5f.  ROIAlign_cpu.cpp in f32, every operation rounded on
 * its own: start = x1 - 0.5f, roi = end - start (not clamped to 1), bin = roi / mask_size, grid = (int)ceilf(bin), count =
 * max(gh * gw, 1); sample (iy, ix) of cell (ph, pw) at start + p * bin + (i + 0.5f) * bin / grid; outside (-1, size) a sample
 * adds 0, at or below 0 it is 0; low = (int)v, at low >= size - 1 both cells are size - 1 and the fraction 0; weights hy*hx,
 * hy*lx, ly*hx, ly*lx; w1*v1 + w2*v2 + w3*v3 + w4*v4 per sample, added into one accumulator with iy outer and ix inner, then
 * divided by count.  A zero row: matched[r] outside 0 .. n_obj - 1, an empty window or NULL bits, a box with a non-positive or
 * NaN extent (grid <= 0), and a box of more than 8192 * mask_size pixels along an axis (a limit of this entry).  Every byte
 * of the n rows is written and nothing past them.  APSE_E_INVALID, with no launch: an image outside the frame limits, n_obj
 * outside 0 .. APSE_MOTS_MAX_OBJECTS, n outside 0 .. APSE_MASK_TRAIN_MAX_N, mask_size outside 1 .. APSE_BITMASK_MAX_SIZE, a NULL
 * pointer.  n == 0 is a no-op. */
#define APSE_BITMASK_MAX_SIZE 64
int apse_bitmask_targets(const apse_mots_window* windows, int n_obj, int h, int w, const float* rois, const int* matched, int n,
                         int mask_size, uint8_t* out, void* stream);

/* ---- Box-head training (csrc/box_train.hip): the f32 steps of fine-tuning roi_heads.box_head.fc1 / fc2 and
 * roi_heads.box_predictor.cls_score / bbox_pred of a frozen FPN detector (dcnn/scripts/train/finetune_uav.py): proposal labelling,
 * the FC layers forward and backward, FastRCNNOutputs.losses of detectron2 0.1.2 (loss_cls, loss_box_reg).  DESIGN.md "Box-head
 * training" has the rules.  Apart from the two entries that read a context, every entry is stateless, enqueues on `stream` only
 * and allocates nothing; the caller passes the workspace (apse_box_train_workspace_bytes covers every entry below).
 * Deterministic: no float atomics, every sum has an order fixed by the shapes, max / argmax ties go to the lowest index.  Errors:
 * APSE_E_INVALID outside the limits, checked before anything is launched, with the text in apse_last_error(NULL).  Limits:
 * 1 <= n <= APSE_BOX_TRAIN_MAX_N sampled RoIs per call (the loss entries also take n = 0 and then enqueue nothing),
 * 1 <= K <= APSE_MAX_CLASSES foreground classes, at most 4096 ground truths per image. */
#define APSE_BOX_TRAIN_MAX_N 1024
/* ROIAlignV2 7x7 (aligned, sampling ratio 0) of `n` boxes over p2..p5 of image `image`, detectron2's level assignment: the launch
 * apse_box_head runs on its proposals, so for the context's own proposals the values equal the `box_pooled` tensor bit for bit.
 * To be called after apse_backbone (FPN only).  rois_dev [n][4] x1,y1,x2,y2 in RESIZED-image pixels; out_dev f32 [n][7][7][256].
 * 0 <= n <= 2^20. */
int apse_box_roi_features(apse_ctx* ctx, int image, const float* rois_dev, int n, float* out_dev, void* stream);
/* The proposals of the last apse_rpn run for image `image`: boxes_dev f32 [rpn_post_topk][4] in resized-image pixels (rows past
 * the count are not meaningful) and count_dev (one int), both device side.  Joins the tail lane first. */
int apse_proposals(apse_ctx* ctx, int image, float* boxes_dev, int* count_dev, void* stream);
/* Workspace bytes for n RoIs and K classes (0 outside the limits). */
size_t apse_box_train_workspace_bytes(int n, int K);
/* pairwise_iou + Matcher([iou_thresh], [0, 1], allow_low_quality_matches = False) + the class assignment of
 * ROIHeads._sample_proposals.  IoU = inter > 0 ? inter / (area_gt + area_proposal - inter) : 0 in f32.  Per proposal: the ground
 * truth of highest IoU (lowest index on ties) -> matched_idx, matched_iou; labels = that ground truth's class when
 * IoU >= iou_thresh, else K (background).  G = 0: every label K, index 0, IoU 0.  0 <= N <= 2^20, 0 <= G <= 4096. */
int apse_box_match(const float* proposals_dev, int N, const float* gt_boxes_dev, const int* gt_classes_dev, int G, int K,
                   float iou_thresh, int* matched_idx_dev, float* matched_iou_dev, int* labels_dev, void* stream);
/* out [n][12544] = x [n][7][7][256] with every row reordered from (h, w, c) to fc1's (c, h, w): done once per step, so that the
 * GEMM entries below read and write roi_heads.box_head.fc1.weight in the checkpoint's own layout.  Not in place. */
int apse_box_permute_features(const float* x_dev, int n, float* out_dev, void* stream);
/* The FC layers on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32), 128 x 128 output tiles that own their outputs over the whole
 * reduction (the gradients need no split), the reduction summed in chains of 64; rows and columns outside the shapes are masked at the loads.
 * x [n][K], w [O][K] (the checkpoint tensor), dy / y [n][O]; 1 <= O <= 1024, 1 <= K <= 16384.
 *   forward: y = x w^T + bias (bias may be NULL) (+ ReLU); a layer with K >= 4096 (fc1) runs as 8 chunks of the reduction whose
 *            sums (8 n O floats of workspace) a second kernel adds in chunk order -- the rule reads K only, so a row of y does
 *            not depend on n
 *   dgrad:   dx [n][K] = dy w, added to the dx already there when accumulate != 0
 *   wgrad:   dw [O][K] = sum over the rows m = 0 .. n - 1 of dy[m][o] x[m][k] */
int apse_box_fc_forward(const float* x_dev, const float* w_dev, const float* bias_dev, int n, int O, int K, int relu, float* y_dev,
                        float* ws, size_t ws_bytes, void* stream);
int apse_box_fc_dgrad(const float* dy_dev, const float* w_dev, int n, int O, int K, int accumulate, float* dx_dev, void* stream);
int apse_box_fc_wgrad(const float* dy_dev, const float* x_dev, int n, int O, int K, float* dw_dev, void* stream);
/* db [O] = column sums of dy [n][O]: rows in ascending order inside slices of 64 rows, slices in ascending order, summed in
 * f64 and rounded once. */
int apse_box_bias_grad(const float* dy_dev, int n, int O, float* db_dev, void* ws, size_t ws_bytes, void* stream);
/* FastRCNNOutputs.losses: logits [n][K + 1], deltas [n][4 K], labels [n] (K = background), the sampled boxes and their matched
 * ground-truth boxes [n][4]; weights4 (HOST, read before the call returns) = the Box2BoxTransform weights, (10, 10, 5, 5).
 * loss_cls = mean cross-entropy over the n rows; loss_box_reg = smooth_l1 (beta < 1e-5: L1) on the four columns of the label's
 * class of the foreground rows, summed and divided by n.
 * out8 = {loss_cls, loss_box_reg, cls_accuracy, fg_cls_accuracy, false_negative, num_fg, num_bg, 0}. */
int apse_box_loss_forward(const float* logits_dev, const float* deltas_dev, const int* labels_dev, const float* prop_boxes_dev,
                          const float* gt_boxes_dev, int n, int K, const float* weights4, float smooth_l1_beta, float* out8_dev,
                          void* ws, size_t ws_bytes, void* stream);
/* dlogits [n][K + 1] = (softmax - onehot) / n x grad_cls[0]; ddeltas [n][4 K] = d smooth_l1 / n x grad_box[0] on the four columns
 * of the foreground rows and exactly 0 elsewhere.  grad_cls / grad_box: device scalars (NULL: 1). */
int apse_box_loss_backward(const float* logits_dev, const float* deltas_dev, const int* labels_dev, const float* prop_boxes_dev,
                           const float* gt_boxes_dev, int n, int K, const float* weights4, float smooth_l1_beta,
                           const float* grad_cls_dev, const float* grad_box_dev, float* dlogits_dev, float* ddeltas_dev,
                           void* stream);

/* ---- RPN-head training (csrc/rpn_train.hip): the f32 steps of fine-tuning proposal_generator.rpn_head.conv / objectness_logits /
 * anchor_deltas of a frozen FPN detector: anchor labelling (RPNOutputs._get_ground_truth of detectron2 0.1.2 without the random
 * draw), the gather of the 3 x 3 x 256 input patches of the sampled anchors, and RPNOutputs.losses (loss_rpn_cls, loss_rpn_loc) with
 * its gradient.  The losses read the head only at the sampled anchors, so on the gathered rows X [S][2304] the head is three FC
 * layers, run on the box trainer's GEMM entries above (conv: O = 256, K = 2304, ReLU; objectness_logits: O = 3; anchor_deltas:
 * O = 12; S <= APSE_BOX_TRAIN_MAX_N per step) with the checkpoint's tensors as they are.  DESIGN.md "RPN-head training" has the
 * rules.  Apart from the gather, which reads a context, every entry is stateless, enqueues on `stream` only and allocates nothing;
 * the caller passes the workspace.  Deterministic: no float atomics, every sum has an order fixed by the shapes, ties go to the
 * lowest index.  Device arrays need only the alignment of their element type (boxes are read and written element by element).
 * Errors: APSE_E_INVALID outside the limits, checked before anything is launched, with the text in
 * apse_last_error(NULL) (the gather: in the context's).
 * Anchors: sizes 32 .. 512 on strides 4 .. 64, ratios (0.5, 1, 2), offset 0, global index in (level, y, x, a) order; the cell
 * anchors are the f32 roundings of Python doubles, computed by the function the inference plan uses, and the kernels generate the
 * boxes from the index as the inference decode does.  A = 3 sum(H W) over the five levels. */
/* Workspace bytes that cover the labelling of A anchors against G ground truths and the loss of S rows (0 outside the limits). */
size_t apse_rpn_train_workspace_bytes(int A, int G, int S);
/* level_h5 / level_w5 (HOST, read before the call returns): the sizes of p2 .. p6.  gt_boxes_dev [G][4] in resized-image pixels.
 * Per anchor: IoU = inter > 0 ? inter / (area_gt + area_anchor - inter) : 0 in f32 against every ground truth; matched_idx = the
 * ground truth of highest IoU (lowest index on ties), matched_iou = that IoU; labels (int32) = 1 at IoU >= iou_hi, 0 below
 * iou_lo, -1 between.  Then Matcher.set_low_quality_matches_, literally: every anchor whose IoU to some ground truth EQUALS that
 * ground truth's maximum over all anchors gets label 1 (a ground truth whose maximum is 0 included: then every anchor that does
 * not overlap it); matched_idx stays the anchor's own argmax.  The maximum is taken in two passes: per block of 1024 anchors into
 * the workspace, then over the blocks in block order.  Anchors outside the image are kept.  G = 0: every label 0, index 0,
 * IoU 0 (no workspace needed).  Limits: 0 <= G <= 4096, levels of at least 1 x 1, A <= 2^22. */
int apse_rpn_anchor_labels(const int* level_h5, const int* level_w5, const float* gt_boxes_dev, int G, float iou_lo, float iou_hi,
                           int* labels_dev, int* matched_idx_dev, float* matched_iou_dev, void* ws, size_t ws_bytes, void* stream);
/* For S anchors (global indices, anchor_idx_dev [S]) of image `image` of the last apse_backbone run: x_dev [S][2304] = the 3 x 3
 * neighbourhood of the anchor's position on its own level (p2 .. p6) in (c, kh, kw) order -- the input order of
 * proposal_generator.rpn_head.conv.weight [256][256][3][3] read as [256][2304] -- with zeros outside the map; per row the anchor
 * slot a = index % 3 (slots_dev), the anchor box (anchor_boxes_dev [S][4]) and the level 0 .. 4 (levels_dev).  Two rows may name
 * the same anchor or position.  An index outside 0 .. A - 1 gives a zero row, slot 0, a zero box and level -1.  Joins the tail lane
 * first.  FPN contexts that store f32 maps only.  0 <= S <= 2^20. */
int apse_rpn_patches(apse_ctx* ctx, int image, const int* anchor_idx_dev, int S, float* x_dev, int* slots_dev,
                     float* anchor_boxes_dev, int* levels_dev, void* stream);
/* RPNOutputs.losses on the sampled rows: logits [S][3], deltas [S][12], per row the slot a (0 .. 2), the label (1 positive,
 * 0 negative, negative values: the row is ignored), the anchor box and the matched ground-truth box [S][4].  Only column a of the
 * logits and columns 4 a .. 4 a + 3 of the deltas take part.  loss_rpn_cls = sum of binary cross-entropy with logits x 1 / norm;
 * loss_rpn_loc = sum over the positive rows of smooth_l1 (beta < 1e-5: L1) against Box2BoxTransform(1, 1, 1, 1).get_deltas(anchor,
 * gt) x 1 / norm; norm = batch_size_per_image x images.  The sums run in f64 through a fixed tree and are rounded once.
 * out8 = {loss_rpn_cls, loss_rpn_loc, num_pos, num_neg, share of positive rows with logit > 0, share of negative rows with
 * logit < 0, 0, 0}.  S = 0 enqueues nothing.  0 <= S <= 2^20, norm >= 1. */
int apse_rpn_loss_forward(const float* logits_dev, const float* deltas_dev, const int* slots_dev, const int* labels_dev,
                          const float* anchor_boxes_dev, const float* gt_boxes_dev, int S, int norm, float smooth_l1_beta,
                          float* out8_dev, void* ws, size_t ws_bytes, void* stream);
/* dlogits [S][3] = (sigmoid - label) / norm x grad_cls[0] on column a; ddeltas [S][12] = d smooth_l1 / norm x grad_loc[0] on
 * columns 4 a .. 4 a + 3 of the positive rows; exactly 0 elsewhere.  grad_cls / grad_loc: device scalars (NULL: 1). */
int apse_rpn_loss_backward(const float* logits_dev, const float* deltas_dev, const int* slots_dev, const int* labels_dev,
                           const float* anchor_boxes_dev, const float* gt_boxes_dev, int S, int norm, float smooth_l1_beta,
                           const float* grad_cls_dev, const float* grad_loc_dev, float* dlogits_dev, float* ddeltas_dev,
                           void* stream);

/* ---- Training-time proposals (csrc/select_nms.hip "training-time FPN selection", csrc/rpn_train.hip): what joint training of
 * the RPN head and the box head needs from a live context.  detectron2 0.1.2 runs the same find_top_rpn_proposals in training
 * and in test; only PRE_NMS_TOPK / POST_NMS_TOPK differ (2000 per level / 1000 in Base-RCNN-FPN.yaml), so the rules are those of
 * apse_rpn_select: per-level top-k (score descending, anchor ascending, the two zeros one score), decode with weights
 * (1, 1, 1, 1), clip, nonempty flag, batched_nms per level on boxes shifted by category x (max_coord + 1) with the categories
 * numbered over the levels present and `iou > thr` suppressing, merge by (score descending, entry ascending), first post_topk.
 * The reach is longer: 1 <= pre_topk <= APSE_RPN_TRAIN_MAX_PRE_TOPK per level, 1 <= post_topk <= APSE_RPN_TRAIN_MAX_POST_TOPK.
 * Inference keeps its own kernels and limits.  Every entry checks its limits before anything is launched: APSE_E_INVALID with
 * the text in apse_last_error (of the context where there is one, of NULL otherwise), nothing launched, outputs untouched. */
#define APSE_RPN_TRAIN_MAX_PRE_TOPK 2048
#define APSE_RPN_TRAIN_MAX_POST_TOPK 2048
/* The selection on injected inputs: the arguments and output layouts of apse_rpn_select (keys_dev [B][5][pre_topk], may be
 * NULL; dec_* [B][5*pre_topk]; props and friends [B][post_topk]; entry = level * pre_topk + rank; zeros and -1 past the count).
 * 1 <= B <= 64.  Allocates its own scratch and synchronises `stream` before it returns. */
int apse_rpn_select_train(const float* const* heads_dev, const int* H, const int* W, int head_ld, int B, int image_h, int image_w,
                          int pre_topk, int post_topk, float nms_thr, int level_mask, unsigned long long* keys_dev,
                          float* dec_boxes_dev, float* dec_scores_dev, int* dec_valid_dev, float* props_dev, float* prop_scores_dev,
                          int* prop_entry_dev, int* prop_count_dev, void* stream);
/* Bytes of workspace apse_rpn_train_proposals needs (0 outside the limits). */
size_t apse_rpn_train_proposals_workspace_bytes(int batch, int pre_topk);
/* The proposals a training step sees: runs the context's RPN convolutions on the maps of the last apse_backbone, then the
 * training selection (all five levels, the context's rpn_nms) on its rpn_head2 .. rpn_head6 tensors.  boxes_dev
 * [batch][post_topk][4] and scores_dev [batch][post_topk], best first, zeros past count_dev [batch].  Outputs and scratch are the
 * caller's: the context's own proposals, proposal counts and results block are not touched, so a later inference forward is
 * unchanged.  Everything is enqueued on `stream` after joining the tail lane; nothing is allocated, nothing synchronised.
 * workspace_dev: 16-byte aligned.  FPN contexts with compute_dtype 0 only. */
int apse_rpn_train_proposals(apse_ctx* ctx, int batch, int pre_topk, int post_topk, float* boxes_dev, float* scores_dev,
                             int* count_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Replaces the RPN head of a live context: the six tensors of proposal_generator.rpn_head in checkpoint layout, DEVICE pointers
 * (conv_w [256][256][3][3], conv_b [256], obj_w [3][256][1][1], obj_b [3], delta_w [12][256][1][1], delta_b [12]).  Kernels on
 * `stream` re-pack them as the plan packed them (the tiled layout of every level's 3 x 3 step and of the fused 1 x 1 head; the
 * Winograd filters U = G g G^T in float64, rounded once, where a level's step holds them) straight into the buffers the steps
 * own: no allocation, no host copy, no synchronisation, the plan is left alone.  Joins the tail lane first; RPN launches
 * enqueued on `stream` before the call read the old weights, those after it the new ones.  Afterwards the context's
 * rpn_head{l} maps and proposals equal, bit for bit, those of a context created from a state with these six tensors.
 * FPN contexts with compute_dtype 0 only. */
int apse_set_rpn_head(apse_ctx* ctx, const float* conv_w_dev, const float* conv_b_dev, const float* obj_w_dev,
                      const float* obj_b_dev, const float* delta_w_dev, const float* delta_b_dev, void* stream);

/* ---- Training augmentation (csrc/augment.hip): the transforms the reference's DatasetMapper applies after ResizeShortestEdge
 * (dcnn/utils/UAV_utils.py:311-449) -- RandomFlip, RandomBrightness, RandomSaturation, RandomContrast, RandomLighting of
 * detectron2 0.1.2 / fvcore, in that order, on resized u8 BGR images.  The rules, with the type of every operation (numpy 1.18
 * value-based casting), are DESIGN.md "Training augmentation"; each blend ends in clip(x, 0, 255) and a truncating conversion to
 * u8 that the next blend reads.  Stateless: no context, enqueues on `stream` only, no allocation, no synchronisation.  The only
 * cross-thread sum is an integer sum, so results are bit-reproducible.
 * brightness / saturation / contrast: the blend weights (1.0 = off); lighting_vec = EIGVEC . (lw * EIGVAL), f64, added to
 * channels 0, 1, 2 unscaled as detectron2 does (0 = off).  With every step off the output is the input, mirrored when flip.
 * src [B][H][W][3] u8; out_u8 [B][H][W][3] and / or out_chw [B][3][H][W] f32 (the layout apse_preprocess_images reads, the same
 * integers as out_u8); either may be NULL, not both; out_u8 must not overlap src (src is read twice).  sums_dev [B] receives the
 * exact sum S of the 3 H W values of each image after the saturation step (cleared on the stream first; the contrast step's mean
 * is S / (3 H W), derived on the device).  params: host memory, B entries, read before the call returns.
 * Limits (APSE_E_INVALID outside them, text in apse_last_error(NULL), nothing launched): 1 <= H <= APSE_MAX_FRAME_H,
 * 1 <= W <= APSE_MAX_FRAME_W, 1 <= B <= APSE_AUGMENT_MAX_BATCH (the per-image parameters travel as one kernel argument);
 * src, params and sums not NULL. */
#define APSE_AUGMENT_MAX_BATCH 64
typedef struct { int flip; double brightness, saturation, contrast; double lighting_vec[3]; } apse_augment_params;
int apse_augment_u8(const uint8_t* src_dev, int B, int H, int W, const apse_augment_params* params_host,
                    uint8_t* out_u8_dev, float* out_chw_dev, unsigned long long* sums_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
