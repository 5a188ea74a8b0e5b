// The stateless operators of the C ABI (include/apse_hip.h): single kernels and small chains behind plain pointers, for the
// tests and tools.  None of them touches a context; of the host code they share the weight packing (plan.hip) and fill_camera.
#include "detector_ctx.h"

#include <math.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

namespace {
struct DevBuf {                      // device scratch of one call
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    bool alloc(size_t bytes, bool zero = false) {
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { p = nullptr; return false; }
        if (zero) hipMemset(p, 0, bytes ? bytes : 16);
        return true;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};
}  // namespace

extern "C" {

size_t apse_conv_packed_elems(const apse_conv_desc* d) {
    const int cin_p = pow2_at_least(d->Cin);
    return (size_t)apse_roundup(d->Cout, 128) * d->KH * apse_roundup(d->KW * cin_p, 32);
}

int apse_conv_pack_weight(const apse_conv_desc* d, const float* w, int cin_real, const float* scale, float* packed) {
    if (!d || !w || !packed) return APSE_E_INVALID;
    const int cin_p = pow2_at_least(d->Cin);
    const int KWCp = apse_roundup(d->KW * cin_p, 32);
    memset(packed, 0, apse_conv_packed_elems(d) * sizeof(float));
    pack_oihw(w, d->Cout, cin_real, d->KH, d->KW, cin_p, scale, packed, KWCp);
    return APSE_OK;
}

// apse_conv2d and apse_conv2d_ex: one layer on the direct kernels.  The arguments behind ws_bytes are apse_conv2d_ex's (the forms
// run_plan gives the ROI heads); apse_conv2d passes none of them and launches what it always did.
static int conv2d_stateless(const apse_conv_desc* d, const void* x, const float* w, const float* bias, const void* res, void* y,
                            float* ws, size_t ws_bytes, const int* count_dev, int hint_items, int y_ld, int deconv, void* stream) {
    if (!d || !x || !w || !y) return APSE_E_INVALID;
    const int cin_p = pow2_at_least(d->Cin);
    if (cin_p != d->Cin) return APSE_E_INVALID;
    if (hint_items < 0 || y_ld < 0 || (y_ld > 0 && (y_ld < d->Cout || deconv))) return APSE_E_INVALID;
    if (deconv && (d->KH != 1 || d->KW != 1 || d->stride != 1 || d->pad != 0 || (d->Cout & 15) || d->res_mode != 0)) return APSE_E_INVALID;
    if (count_dev && (d->fuse_reduce || d->cfg == APSE_CFG_STREAM || d->cfg == APSE_CFG_GLDS)) return APSE_E_INVALID;
    if (d->res_mode != 0 && (d->Cout & 3) != 0) return APSE_E_INVALID;      // residual rows are read as float4
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.x = reinterpret_cast<const float*>(x); p.w = w; p.bias = bias; p.res = reinterpret_cast<const float*>(res);
    p.y = reinterpret_cast<float*>(y); p.ws = ws;
    p.B = d->B; p.H = d->H; p.W = d->W; p.cin_log2 = apse_ilog2(cin_p);
    p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad;
    p.KWCp = apse_roundup(d->KW * cin_p, 32);
    p.OH = (d->H + 2 * d->pad - d->KH) / d->stride + 1;
    p.OW = (d->W + 2 * d->pad - d->KW) / d->stride + 1;
    p.Cout = d->Cout; p.relu = d->relu; p.res_mode = d->res_mode;
    p.M = p.B * p.OH * p.OW; p.m_per_item = p.OH * p.OW;
    p.y_ld = d->Cout; p.steps_total = p.KH * (p.KWCp / 32);
    if (y_ld > 0) p.y_ld = y_ld;
    if (deconv) { p.out_mode = 1; p.cdec = d->Cout / 4; p.y_ld = d->Cout / 4; }
    if (count_dev) p.m_count = count_dev;
    if (hint_items > 0) p.m_hint = (long long)hint_items * p.m_per_item < p.M ? hint_items * p.m_per_item : p.M;
    p.prec = (d->prec == 1 || d->prec == 2) ? d->prec : 0;
    p.x_st = d->x_st; p.res_st = d->res_st; p.y_st = d->y_st;
    if (p.x_st < 0 || p.x_st > 2 || p.res_st < 0 || p.res_st > 2 || p.y_st < 0 || p.y_st > 2) return APSE_E_INVALID;
    if ((y_ld > 0 || deconv) && p.y_st && (p.y_ld & 7)) return APSE_E_INVALID;      // 16-bit rows are whole 16-byte groups
    if (p.prec && p.x_st && p.x_st != p.prec) return APSE_E_INVALID;       // 16-bit x must already be the operand type
    if (p.x_st && cin_p < 8) return APSE_E_INVALID;
    int sk = 1;
    int cfg = apse_conv_pick_cfg(p.M, p.Cout, p.steps_total, &sk);
    if (d->cfg >= 0) { cfg = d->cfg; sk = 1; p.no_stream = (d->cfg != APSE_CFG_STREAM && d->cfg != APSE_CFG_GLDS && d->cfg != APSE_CFG_SKINNY); }
    if (d->splitk > 0) sk = d->splitk;
    if (sk > p.steps_total) sk = p.steps_total;
    p.splitk = sk;
    if (sk > 1 && (size_t)sk * p.M * p.Cout * sizeof(float) > ws_bytes) return APSE_E_INVALID;
    if (sk > 1 && d->fuse_reduce) {
        static int* cnt = nullptr;
        if (!cnt) { if (hipMalloc(reinterpret_cast<void**>(&cnt), 65536 * sizeof(int)) != hipSuccess) return APSE_E_NOMEM; hipMemset(cnt, 0, 65536 * sizeof(int)); }
        p.tile_cnt = cnt;
    }
    if (!p.prec) return apse_launch_conv(p, cfg, (hipStream_t)stream);
    // 16-bit operands: round the filters like a context does at load (this stateless entry is a test / tool helper: the
    // rounded copy is rebuilt by a small kernel on the caller's stream in front of every call, in a buffer that only grows)
    const size_t ne = (size_t)apse_roundup(p.Cout, 128) * p.KH * p.KWCp;
    static uint16_t* d16 = nullptr;
    static size_t d16_cap = 0;
    if (ne > d16_cap) {
        hipDeviceSynchronize();
        if (d16) hipFree(d16);
        d16 = nullptr; d16_cap = 0;
        if (hipMalloc(reinterpret_cast<void**>(&d16), ne * 2) != hipSuccess) return APSE_E_NOMEM;
        d16_cap = ne;
    }
    int rc = apse_k_round16(w, d16, ne, p.prec, (hipStream_t)stream);
    if (rc) return rc;
    p.w16 = d16;
    return apse_launch_conv(p, cfg, (hipStream_t)stream);
}

int apse_conv2d(const apse_conv_desc* d, const float* x, const float* w, const float* bias, const float* res, float* y, float* ws,
                size_t ws_bytes, void* stream) {
    return conv2d_stateless(d, x, w, bias, res, y, ws, ws_bytes, nullptr, 0, 0, 0, stream);
}

int apse_conv2d_ex(const apse_conv_desc* d, const void* x, const float* w, const float* bias, const void* res, void* y, float* ws,
                   size_t ws_bytes, const int* count_dev, int hint_items, int y_ld, int deconv, void* stream) {
    return conv2d_stateless(d, x, w, bias, res, y, ws, ws_bytes, count_dev, hint_items, y_ld, deconv, stream);
}

int apse_winograd_pack_filter(const float* w, int Cout, int Cin, float* packed) {
    if (!w || !packed || Cout < 1 || Cin < 8 || pow2_at_least(Cin) != Cin) return APSE_E_INVALID;
    const std::vector<float> u = winograd_filters(w, Cout, Cin, Cin);
    memcpy(packed, u.data(), u.size() * sizeof(float));
    return APSE_OK;
}

int apse_winograd_conv2d(const apse_conv_desc* d, const float* x, const float* wu, const float* bias, float* y, void* stream) {
    if (!d || !x || !wu || !y || d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 8 || pow2_at_least(d->Cin) != d->Cin) return APSE_E_INVALID;
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.x = x; p.wu = wu; p.bias = bias; p.y = y;
    p.B = d->B; p.H = d->H; p.W = d->W; p.cin_log2 = apse_ilog2(d->Cin);
    p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad;
    p.OH = d->H; p.OW = d->W; p.Cout = d->Cout; p.relu = d->relu;
    p.M = p.B * p.OH * p.OW; p.m_per_item = p.OH * p.OW;
    p.y_ld = d->Cout; p.splitk = 1;
    p.res_mode = d->res_mode; p.prec = d->prec; p.x_st = d->x_st; p.y_st = d->y_st;      // anything but 0 is refused by the launcher
    return apse_launch_conv_winograd(p, (hipStream_t)stream);
}

int apse_winograd_conv2d_split(const apse_conv_desc* d, const float* x, const float* wu, const float* bias, float* y, float* ws,
                               size_t ws_bytes, int geometry, void* stream) {
    if (!d || !x || !wu || !y || d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 8 || pow2_at_least(d->Cin) != d->Cin) return APSE_E_INVALID;
    if (d->splitk < 1 || d->splitk > d->Cin / 8 || (geometry != 0 && geometry != 1)) return APSE_E_INVALID;
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.x = x; p.wu = wu; p.bias = bias; p.y = y; p.ws = ws;
    p.B = d->B; p.H = d->H; p.W = d->W; p.cin_log2 = apse_ilog2(d->Cin);
    p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad;
    p.OH = d->H; p.OW = d->W; p.Cout = d->Cout; p.relu = d->relu;
    p.M = p.B * p.OH * p.OW; p.m_per_item = p.OH * p.OW;
    p.y_ld = d->Cout; p.splitk = d->splitk; p.wino_geom = geometry;
    p.res_mode = d->res_mode; p.prec = d->prec; p.x_st = d->x_st; p.y_st = d->y_st;      // anything but 0 is refused by the launcher
    if (p.splitk > 1 && (!ws || (size_t)p.splitk * p.M * p.Cout * sizeof(float) > ws_bytes)) return APSE_E_INVALID;
    return apse_launch_conv_winograd(p, (hipStream_t)stream);
}

int apse_maxpool3x3s2(const float* x, float* y, int B, int H, int W, int C, void* stream) {
    return apse_k_maxpool3x3s2(x, y, B, H, W, C, 0, (hipStream_t)stream);
}

int apse_maxpool3x3s2_typed(const void* x, void* y, int B, int H, int W, int C, int storage, void* stream) {
    if (!x || !y || B < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || storage < 0 || storage > 2) return APSE_E_INVALID;
    return apse_k_maxpool3x3s2(x, y, B, H, W, C, storage, (hipStream_t)stream);
}

static int roi_align_stateless(const void* const* feats, const int* hs, const int* ws, const float* rois, int n, int per_img,
                               int out_size, int st, void* out, void* stream) {
    if (!feats || !hs || !ws || !rois || !out || n < 0 || out_size < 1 || st < 0 || st > 2) return APSE_E_INVALID;
    FpnMaps F;
    static const float sc[4] = {0.25f, 0.125f, 0.0625f, 0.03125f};
    for (int l = 0; l < 4; ++l) { F.p[l] = feats[l]; F.H[l] = hs[l]; F.W[l] = ws[l]; F.scale[l] = sc[l]; }
    F.st = st;
    // all rois live: a one-element count array is not available here, so use a device int holding n via total
    static int* total_dev = nullptr;
    if (!total_dev) hipMalloc(reinterpret_cast<void**>(&total_dev), sizeof(int));
    hipMemcpyAsync(total_dev, &n, sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream);
    hipStreamSynchronize((hipStream_t)stream);
    // roi_img derived from per_img: build on device via a tiny host vector
    std::vector<int> img(n);
    for (int i = 0; i < n; ++i) img[i] = per_img > 0 ? i / per_img : 0;
    int* img_dev = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&img_dev), sizeof(int) * (n > 0 ? n : 1)) != hipSuccess) return APSE_E_NOMEM;
    hipMemcpy(img_dev, img.data(), sizeof(int) * n, hipMemcpyHostToDevice);
    int rc = apse_k_roi_align(&F, rois, img_dev, nullptr, total_dev, 0, n, out_size, out, st, (hipStream_t)stream);
    hipStreamSynchronize((hipStream_t)stream);
    hipFree(img_dev);
    return rc;
}

int apse_roi_align(const float* const* feats, const int* hs, const int* ws, const float* rois, int n, int per_img, int out_size,
                   float* out, void* stream) {
    return roi_align_stateless(reinterpret_cast<const void* const*>(feats), hs, ws, rois, n, per_img, out_size, 0, out, stream);
}

int apse_roi_align_typed(const void* const* feats, const int* hs, const int* ws, const float* rois, int n, int per_img,
                         int out_size, int storage, void* out, void* stream) {
    return roi_align_stateless(feats, hs, ws, rois, n, per_img, out_size, storage, out, stream);
}

int apse_roi_pool(const float* feat, int H, int W, const float* rois, const int* roi_img, int n, int out_size, float scale,
                  float* out, void* stream) {
    static int* total_dev = nullptr;
    if (!total_dev) hipMalloc(reinterpret_cast<void**>(&total_dev), sizeof(int));
    hipMemcpyAsync(total_dev, &n, sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream);
    hipStreamSynchronize((hipStream_t)stream);
    return apse_k_roi_pool(feat, 0, H, W, rois, roi_img, total_dev, n, out_size, scale, out, 0, 0, (hipStream_t)stream);
}

int apse_nms_rank(const float* boxes, const float* scores, const int* valid, int n, int cat_div, int cat_mod, int ncat, float thr,
                  int topk, float* out_boxes, float* out_scores, int* out_index, int* out_count, void* stream) {
    if (ncat < 1 || ncat > 8 || n > 8192) return APSE_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int *keep_idx = nullptr, *keep_cnt = nullptr;
    uint32_t* maxc = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&keep_idx), sizeof(int) * 8 * APSE_NMS_SLOT) != hipSuccess) return APSE_E_NOMEM;
    hipMalloc(reinterpret_cast<void**>(&keep_cnt), sizeof(int) * 8);
    hipMalloc(reinterpret_cast<void**>(&maxc), sizeof(uint32_t));
    // max coordinate over the valid boxes (torchvision batched_nms): computed on the host for this stateless op
    std::vector<float> hb((size_t)n * 4);
    std::vector<int> hv(n);
    hipMemcpy(hb.data(), boxes, hb.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(hv.data(), valid, hv.size() * 4, hipMemcpyDeviceToHost);
    float m = 0.f;
    bool any = false;
    for (int i = 0; i < n; ++i)
        if (hv[i]) for (int k = 0; k < 4; ++k) { m = (!any || hb[i * 4 + k] > m) ? hb[i * 4 + k] : m; any = true; }
    uint32_t mb;
    memcpy(&mb, &m, 4);
    hipMemcpy(maxc, &mb, 4, hipMemcpyHostToDevice);
    void* scratch = nullptr;
    if (hipMalloc(&scratch, apse_nms_scratch_bytes(8)) != hipSuccess) return APSE_E_NOMEM;
    int rc = apse_k_nms_percat(boxes, scores, valid, n, cat_div, cat_mod, maxc, thr, keep_idx, keep_cnt, ncat, scratch, 0, 1, 0, s);
    if (!rc) rc = apse_k_rank_final(boxes, scores, n, keep_idx, keep_cnt, ncat, topk, out_boxes, out_scores, out_index, out_count, nullptr, 1, s);
    hipStreamSynchronize(s);
    hipFree(keep_idx); hipFree(keep_cnt); hipFree(maxc); hipFree(scratch);
    return rc;
}

// ---- the decision kernels on injected inputs: the launchers of apse_rpn_levels / apse_box_head, in their order, on scratch of
// this call (select_nms.hip).  Test / tool entries: every call allocates, synchronises and frees.
int apse_rpn_select(const float* const* heads_dev, const int* H, const int* W, int head_ld, int B, int image_h, int image_w,
                    int pre_topk, int post_topk, float nms_thr, int level_mask, unsigned long long* keys_dev, float* dec_boxes_dev,
                    float* dec_scores_dev, int* dec_valid_dev, float* props_dev, float* prop_scores_dev, int* prop_entry_dev,
                    int* prop_count_dev, void* stream) {
    if (!heads_dev || !H || !W || !dec_boxes_dev || !dec_scores_dev || !dec_valid_dev || !props_dev || !prop_scores_dev ||
        !prop_entry_dev || !prop_count_dev)
        return APSE_E_INVALID;
    level_mask &= 31;
    if (!level_mask || B < 1 || B > 64 || head_ld < 15 || pre_topk < 1 || pre_topk > 1000 || post_topk < 1) return APSE_E_INVALID;
    for (int l = 0; l < 5; ++l)
        if (!heads_dev[l] || H[l] < 1 || W[l] < 1 || (long long)H[l] * W[l] * 3 > (1ll << 30)) return APSE_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    RpnSelectPlan sel;
    rpn_select_plan(heads_dev, H, W, head_ld, pre_topk, &sel);
    DevBuf rl, fs, lists, maxc, keep_idx, keep_cnt, scratch;
    std::vector<DevBuf> stage_dev(sel.stages.size());
    if (!rl.alloc(sizeof(RpnLevels)) || !fs.alloc(5 * sizeof(int)) || !lists.alloc((size_t)B * sel.nslots * 1024 * 8) ||
        !maxc.alloc((size_t)2 * B * 4, true) || !keep_idx.alloc((size_t)B * 8 * APSE_NMS_SLOT * 4) ||
        !keep_cnt.alloc((size_t)B * 8 * 4, true) || !scratch.alloc(apse_nms_scratch_bytes(8 * B)))
        return APSE_E_NOMEM;
    hipMemcpy(rl.p, &sel.levels, sizeof(RpnLevels), hipMemcpyHostToDevice);
    hipMemcpy(fs.p, sel.final_slot, 5 * sizeof(int), hipMemcpyHostToDevice);
    for (size_t i = 0; i < sel.stages.size(); ++i) {
        if (!stage_dev[i].alloc(sel.stages[i].size() * sizeof(TopkJob))) return APSE_E_NOMEM;
        hipMemcpy(stage_dev[i].p, sel.stages[i].data(), sel.stages[i].size() * sizeof(TopkJob), hipMemcpyHostToDevice);
    }
    const float clamp = (float)log(1000.0 / 16.0);
    int rc = APSE_OK;
    for (size_t i = 0; i < sel.stages.size() && !rc; ++i)
        rc = apse_k_rpn_topk_stage(rl.as<RpnLevels>(), stage_dev[i].as<TopkJob>(), (int)sel.stages[i].size(), lists.as<uint64_t>(),
                                   sel.nslots, B, i == 0 ? maxc.as<uint32_t>() : nullptr, s);
    if (!rc) rc = apse_k_rpn_decode(rl.as<RpnLevels>(), pre_topk, lists.as<uint64_t>(), sel.nslots, fs.as<int>(), (float)image_h,
                                    (float)image_w, clamp, dec_boxes_dev, dec_scores_dev, dec_valid_dev, maxc.as<uint32_t>(),
                                    level_mask, B, s);
    if (!rc) rc = apse_k_nms_percat(dec_boxes_dev, dec_scores_dev, dec_valid_dev, 5 * pre_topk, pre_topk, 0, maxc.as<uint32_t>(),
                                    nms_thr, keep_idx.as<int>(), keep_cnt.as<int>(), 5, scratch.p, level_mask, B, 1, s);
    if (!rc) rc = apse_k_rank_final(dec_boxes_dev, dec_scores_dev, 5 * pre_topk, keep_idx.as<int>(), keep_cnt.as<int>(), 5, post_topk,
                                    props_dev, prop_scores_dev, prop_entry_dev, prop_count_dev, maxc.as<uint32_t>() + B, B, s);
    if (!rc && keys_dev) {
        hipMemsetAsync(keys_dev, 0xff, (size_t)B * 5 * pre_topk * 8, s);
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < 5; ++l)
                hipMemcpyAsync(keys_dev + ((size_t)b * 5 + l) * pre_topk,
                               lists.as<uint64_t>() + ((size_t)b * sel.nslots + sel.final_slot[l]) * 1024,
                               (size_t)sel.levels.lv[l].k * 8, hipMemcpyDeviceToDevice, s);
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = APSE_E_HIP;
    return rc;
}

// The training-time selection on injected inputs (select_nms.hip "training-time FPN selection"): apse_rpn_select's arguments and
// output layouts, lists of up to APSE_RPN_TRAIN_MAX_PRE_TOPK per level.
int apse_rpn_select_train(const float* const* heads_dev, const int* H, const int* W, int head_ld, int B, int image_h, int image_w,
                          int pre_topk, int post_topk, float nms_thr, int level_mask, unsigned long long* keys_dev,
                          float* dec_boxes_dev, float* dec_scores_dev, int* dec_valid_dev, float* props_dev, float* prop_scores_dev,
                          int* prop_entry_dev, int* prop_count_dev, void* stream) {
    if (!heads_dev || !H || !W || !dec_boxes_dev || !dec_scores_dev || !dec_valid_dev || !props_dev || !prop_scores_dev ||
        !prop_entry_dev || !prop_count_dev)
        return apse_fail_global(APSE_E_INVALID, "apse_rpn_select_train: null pointer");
    level_mask &= 31;
    if (!level_mask) return apse_fail_global(APSE_E_INVALID, "apse_rpn_select_train: empty level mask");
    if (B < 1 || B > 64) return apse_fail_global(APSE_E_INVALID, "apse_rpn_select_train: batch outside 1 .. 64");
    if (head_ld < 15) return apse_fail_global(APSE_E_INVALID, "apse_rpn_select_train: head_ld below 15");
    if (pre_topk < 1 || pre_topk > APSE_RPN_TRAIN_MAX_PRE_TOPK)
        return apse_fail_global(APSE_E_INVALID, "apse_rpn_select_train: pre_topk outside 1 .. APSE_RPN_TRAIN_MAX_PRE_TOPK (2048)");
    if (post_topk < 1 || post_topk > APSE_RPN_TRAIN_MAX_POST_TOPK)
        return apse_fail_global(APSE_E_INVALID, "apse_rpn_select_train: post_topk outside 1 .. APSE_RPN_TRAIN_MAX_POST_TOPK (2048)");
    for (int l = 0; l < 5; ++l)
        if (!heads_dev[l] || H[l] < 1 || W[l] < 1 || (long long)H[l] * W[l] * 3 > (1ll << 30))
            return apse_fail_global(APSE_E_INVALID, "apse_rpn_select_train: bad level");
    hipStream_t s = (hipStream_t)stream;
    RpnLevels L;
    rpn_levels_desc(heads_dev, H, W, head_ld, pre_topk, &L);
    DevBuf scratch;
    if (!scratch.alloc(apse_rpn_train_scratch_bytes(B))) return apse_fail_global(APSE_E_NOMEM, "apse_rpn_select_train: scratch");
    int rc = apse_k_rpn_train_select(&L, post_topk, (float)image_h, (float)image_w, (float)log(1000.0 / 16.0), nms_thr, level_mask,
                                     reinterpret_cast<uint64_t*>(keys_dev), dec_boxes_dev, dec_scores_dev, dec_valid_dev, scratch.p,
                                     props_dev, prop_scores_dev, prop_entry_dev, prop_count_dev, B, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = APSE_E_HIP;
    return rc ? apse_fail_global(rc, "apse_rpn_select_train: launch failed") : APSE_OK;
}

int apse_box_inference(const float* pred_dev, int ld, int K, const float* props_dev, const int* prop_cnt_dev, int P, int B,
                       int image_h, int image_w, float score_thresh, float nms_thr, int dets_per_image, int wide,
                       float* probs_dev, float* cand_boxes_dev, float* cand_scores_dev, int* cand_valid_dev, float* det_boxes_dev,
                       float* det_scores_dev, int* det_entry_dev, int* det_cnt_dev, float* pk_boxes_dev, float* pk_scores_dev,
                       int* pk_cls_dev, int* pk_img_dev, int* pk_roi_dev, int* pk_total_dev, int* pk_offset_dev, void* stream) {
    if (!pred_dev || !props_dev || !prop_cnt_dev || !probs_dev || !cand_boxes_dev || !cand_scores_dev || !cand_valid_dev ||
        !det_boxes_dev || !det_scores_dev || !det_entry_dev || !det_cnt_dev || !pk_boxes_dev || !pk_scores_dev || !pk_cls_dev ||
        !pk_img_dev || !pk_roi_dev || !pk_total_dev || !pk_offset_dev)
        return APSE_E_INVALID;
    if (K < 1 || K > 127 || (!wide && K > 7) || ld < 5 * K + 1 || P < 1 || P > APSE_NMS_SLOT || B < 1 || B > 64 ||
        dets_per_image < 1)
        return APSE_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int KD = dets_per_image, ncat = K > 8 ? K : 8;
    DevBuf maxc, keep_idx, keep_cnt, scratch, sums, clist;
    if (!maxc.alloc((size_t)B * 4) || !keep_idx.alloc((size_t)B * ncat * APSE_NMS_SLOT * 4) || !keep_cnt.alloc((size_t)B * ncat * 4, true) ||
        !scratch.alloc(apse_nms_scratch_bytes(ncat * B)) || !sums.alloc((size_t)B * KD * 3 * 8))
        return APSE_E_NOMEM;
    // the class counts live across calls, as a context's do: zero when allocated, and nms_prepare_list leaves them zero
    static int* ccnt = nullptr;
    static size_t ccnt_cap = 0;
    if (wide) {
        if (!clist.alloc((size_t)B * K * P * 4)) return APSE_E_NOMEM;
        if ((size_t)B * K > ccnt_cap) {
            hipDeviceSynchronize();
            if (ccnt) hipFree(ccnt);
            ccnt = nullptr; ccnt_cap = 0;
            if (hipMalloc(reinterpret_cast<void**>(&ccnt), (size_t)B * K * 4) != hipSuccess) return APSE_E_NOMEM;
            hipMemset(ccnt, 0, (size_t)B * K * 4);
            ccnt_cap = (size_t)B * K;
        }
    }
    const float wts[4] = {10.f, 10.f, 5.f, 5.f};
    const float clamp = (float)log(1000.0 / 16.0);
    hipMemsetAsync(maxc.p, 0, sizeof(uint32_t) * B, s);
    int rc;
    if (wide) {
        rc = apse_k_box_candidates_wide(pred_dev, ld, K, props_dev, prop_cnt_dev, P, (float)image_h, (float)image_w, score_thresh, wts,
                                        clamp, cand_boxes_dev, cand_scores_dev, cand_valid_dev, maxc.as<uint32_t>(), probs_dev,
                                        clist.as<int>(), ccnt, B, s);
        if (!rc) rc = apse_k_nms_lists(cand_boxes_dev, cand_scores_dev, P * K, clist.as<int>(), ccnt, P, maxc.as<uint32_t>(), nms_thr,
                                       keep_idx.as<int>(), keep_cnt.as<int>(), K, scratch.p, B, s);
        if (!rc) rc = apse_k_rank_wide(cand_boxes_dev, cand_scores_dev, P * K, keep_idx.as<int>(), keep_cnt.as<int>(), K, KD,
                                       det_boxes_dev, det_scores_dev, det_entry_dev, det_cnt_dev, B, s);
    } else {
        rc = apse_k_box_candidates(pred_dev, ld, K, props_dev, prop_cnt_dev, P, (float)image_h, (float)image_w, score_thresh, wts, clamp,
                                   cand_boxes_dev, cand_scores_dev, cand_valid_dev, maxc.as<uint32_t>(), probs_dev, B, s);
        if (!rc) rc = apse_k_nms_percat(cand_boxes_dev, cand_scores_dev, cand_valid_dev, P * K, 0, K, maxc.as<uint32_t>(), nms_thr,
                                        keep_idx.as<int>(), keep_cnt.as<int>(), K, scratch.p, 0, B, 0, s);
        if (!rc) rc = apse_k_rank_final(cand_boxes_dev, cand_scores_dev, P * K, keep_idx.as<int>(), keep_cnt.as<int>(), K, KD,
                                        det_boxes_dev, det_scores_dev, det_entry_dev, det_cnt_dev, nullptr, B, s);
    }
    if (!rc) rc = apse_k_pack_detections(det_boxes_dev, det_scores_dev, det_entry_dev, det_cnt_dev, B, KD, K, pk_boxes_dev, pk_scores_dev,
                                         pk_cls_dev, pk_img_dev, pk_roi_dev, pk_total_dev, pk_offset_dev,
                                         sums.as<unsigned long long>(), s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = APSE_E_HIP;
    return rc;
}

int apse_c4_rpn_select(const float* head_dev, int H, int W, int B, int image_h, int image_w, int pre, int post, float nms_thr,
                       float* dec_boxes_dev, float* dec_scores_dev, int* dec_valid_dev, float* props_dev, float* prop_scores_dev,
                       int* prop_entry_dev, int* prop_count_dev, void* stream) {
    if (!head_dev || !dec_boxes_dev || !dec_scores_dev || !dec_valid_dev || !props_dev || !prop_scores_dev || !prop_entry_dev ||
        !prop_count_dev || H < 1 || W < 1 || (long long)H * W * 15 > (1ll << 30) || B < 1 || B > 64)
        return APSE_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    C4Rpn R;
    c4_rpn_desc(head_dev, H, W, 80, pre, &R);
    DevBuf scratch;
    if (!scratch.alloc(apse_c4_nms_scratch_bytes(B))) return APSE_E_NOMEM;
    int rc = apse_k_c4_rpn(&R, pre, post, (float)image_h, (float)image_w, (float)log(1000.0 / 16.0), nms_thr, dec_boxes_dev,
                           dec_scores_dev, dec_valid_dev, scratch.p, props_dev, prop_scores_dev, prop_entry_dev, prop_count_dev, B, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = APSE_E_HIP;
    return rc;
}

static int dense_scratch(int H, int W, uint64_t** bits, unsigned long long** sums) {
    static uint64_t* b = nullptr;
    static unsigned long long* sm = nullptr;
    static size_t words = 0;
    const size_t need = (size_t)H * ((W + 63) / 64);
    if (need > words) {
        if (b) hipFree(b);
        if (hipMalloc(reinterpret_cast<void**>(&b), need * 8) != hipSuccess) return APSE_E_NOMEM;
        words = need;
    }
    if (!sm && hipMalloc(reinterpret_cast<void**>(&sm), 4 * sizeof(unsigned long long)) != hipSuccess) return APSE_E_NOMEM;
    *bits = b; *sums = sm;
    return APSE_OK;
}

int apse_mask_centroid_dense(const uint8_t* mask, int H, int W, int* out3, void* stream) {
    uint64_t* bits; unsigned long long* sums;
    int rc = dense_scratch(H, W, &bits, &sums);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = apse_k_dense_to_bits(mask, H, W, (W + 63) / 64, bits, sums, s);
    if (rc) return rc;
    unsigned long long h[3];
    if (hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess) return APSE_E_HIP;
    hipStreamSynchronize(s);
    out3[2] = (int)h[0];
    out3[0] = h[0] ? (int)(h[1] / h[0]) : -1;
    out3[1] = h[0] ? (int)(h[2] / h[0]) : -1;
    return APSE_OK;
}

int apse_mask_closest_dense(const uint8_t* mask, int H, int W, float px, float py, int* out2, void* stream) {
    uint64_t* bits; unsigned long long* sums;
    int rc = dense_scratch(H, W, &bits, &sums);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = apse_k_dense_to_bits(mask, H, W, (W + 63) / 64, bits, sums, s);
    if (rc) return rc;
    rc = apse_k_closest_single(bits, H, W, (W + 63) / 64, px, py, sums + 3, s);
    if (rc) return rc;
    unsigned long long best;
    if (hipMemcpyAsync(&best, sums + 3, sizeof best, hipMemcpyDeviceToHost, s) != hipSuccess) return APSE_E_HIP;
    hipStreamSynchronize(s);
    if (best == ~0ull) { out2[0] = out2[1] = -1; return APSE_OK; }
    const unsigned lin = (unsigned)(best & 0xffffffffu);
    out2[0] = (int)(lin % (unsigned)W) + 1;
    out2[1] = (int)(lin / (unsigned)W) + 1;
    return APSE_OK;
}

int apse_l2_normalize(const float* x, float* y, int n, int D, void* stream) {
    return apse_k_l2_normalize(x, y, D, nullptr, n, (hipStream_t)stream);
}
int apse_sqdist(const float* a, const float* b, int O, int N, int D, float* out, void* stream) {
    return apse_k_sqdist(a, b, O, N, D, out, (hipStream_t)stream);
}
// Lab tables of a gamma LUT, device-resident for the stateless operator: one copy PER DEVICE (keyed by hipGetDevice), rebuilt
// when the LUT changes, guarded by a mutex (the operator is a test / tool entry; a context keeps its own copy)
static int lab_tables_device(const uint8_t* lut, hipStream_t s, LabTables** out) {
    struct PerDev { LabTables* dev = nullptr; uint8_t lut[256]; bool have = false; };
    static std::mutex mu;
    static std::map<int, PerDev> cache;
    static LabTables host;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return APSE_E_HIP;
    std::lock_guard<std::mutex> lock(mu);
    PerDev& e = cache[device];
    if (!e.dev && hipMalloc(reinterpret_cast<void**>(&e.dev), sizeof(LabTables)) != hipSuccess) return APSE_E_NOMEM;
    if (!e.have || memcmp(e.lut, lut, 256) != 0) {
        hipStreamSynchronize(s);                       // an earlier launch may still read the previous tables
        lab_tables_build(&host, lut);
        if (hipMemcpy(e.dev, &host, sizeof(LabTables), hipMemcpyHostToDevice) != hipSuccess) return APSE_E_HIP;
        memcpy(e.lut, lut, 256);
        e.have = true;
    }
    *out = e.dev;
    return APSE_OK;
}

int apse_undistort_gamma(const uint8_t* src, uint8_t* dst, int B, int H, int W, const double* m, const double* dist, int ndist,
                         const uint8_t* lut, int do_undistort, int do_gamma, void* stream) {
    if (!src || !dst || (do_gamma && !lut)) return APSE_E_INVALID;
    UndistortParams p;
    int rc = fill_camera(p, H, W, m, dist, ndist, do_undistort, do_gamma);
    if (rc) return rc;
    LabTables* lab = nullptr;
    if (do_gamma && (rc = lab_tables_device(lut, (hipStream_t)stream, &lab))) return rc;
    return apse_k_undistort_gamma(&p, src, dst, lab, B, (hipStream_t)stream);
}

size_t apse_lab_tables_host(const uint8_t* lut256, void* out, size_t cap) {
    if (!lut256 || !out || cap < sizeof(LabTables)) return sizeof(LabTables);
    lab_tables_build(reinterpret_cast<LabTables*>(out), lut256);
    return sizeof(LabTables);
}

int apse_resize_normalize(const uint8_t* frames, uint8_t* tmp, float* out, uint8_t* resized, const int* hb, const int* hc, int hk,
                          const int* vb, const int* vc, int vk, int B, int H, int W, int OH, int OW, int PH, int PW,
                          const float* mean3, void* stream) {
    return apse_k_pil_resize(frames, tmp, out, 0, resized, hb, hc, hk, vb, vc, vk, B, H, W, OH, OW, PH, PW, mean3, nullptr, nullptr, nullptr, nullptr, 0, nullptr, (hipStream_t)stream);
}

// The geometry checks of every YUV entry: the frame-size limits, then the layout (yuv_source_fill)
static int yuv_source_checked(YuvSource& y, int H, int W, int pitch, int format, int matrix) {
    if (H < 1 || W < 1 || H > APSE_MAX_FRAME_H || W > APSE_MAX_FRAME_W) return apse_fail_global(APSE_E_INVALID, "YUV frame size outside 1..APSE_MAX_FRAME_H x 1..APSE_MAX_FRAME_W");
    const char* why = yuv_source_fill(y, H, W, pitch, format, matrix);
    return why ? apse_fail_global(APSE_E_INVALID, why) : APSE_OK;
}

int apse_yuv_to_bgr(const uint8_t* src, uint8_t* dst, int B, int H, int W, int pitch, int format, int matrix, void* stream) {
    if (!src || !dst || B < 1) return apse_fail_global(APSE_E_INVALID, "apse_yuv_to_bgr: null pointer or empty batch");
    YuvSource y;
    int rc = yuv_source_checked(y, H, W, pitch, format, matrix);
    if (rc) return rc;
    return apse_k_yuv_to_bgr(&y, src, dst, B, (hipStream_t)stream);
}

int apse_yuv_matrix_host(int matrix, int* out6) {
    if (matrix < 0 || matrix >= YUV_NMATRIX || !out6) return APSE_E_INVALID;
    const YuvMatrix& m = YUV_MATRICES[matrix];
    out6[0] = m.yoff; out6[1] = m.cy; out6[2] = m.cvr; out6[3] = m.cvg; out6[4] = m.cug; out6[5] = m.cub;
    return APSE_OK;
}

int apse_resize_normalize_yuv(const uint8_t* frames, int pitch, int format, int matrix, uint8_t* tmp, float* out, uint8_t* resized,
                              const int* hb, const int* hc, int hk, const int* vb, const int* vc, int vk, int B, int H, int W, int OH,
                              int OW, int PH, int PW, const float* mean3, void* stream) {
    YuvSource y;
    int rc = yuv_source_checked(y, H, W, pitch, format, matrix);
    if (rc) return rc;
    return apse_k_pil_resize(frames, tmp, out, 0, resized, hb, hc, hk, vb, vc, vk, B, H, W, OH, OW, PH, PW, mean3, nullptr, nullptr, nullptr, nullptr, 0, &y, (hipStream_t)stream);
}

}  // extern "C"
