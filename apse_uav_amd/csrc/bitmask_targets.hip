// Mask-head targets from bitmask ground truth (include/apse_hip.h "Bitmask targets"; DESIGN.md "Bitmask ground truth").
//
//   remap_windows    one wave per destination window row, one lane per pixel: destination pixel (x, y) takes the source bit at
//                    (xmap[x], ymap[y]); one __ballot per word, lane 0 stores it.  Integer only.
//   bitmask_targets  detectron2 BitMasks.crop_and_resize = ROIAlign((M, M), 1.0, 0, aligned=True) over the 0 / 1 mask, then >= 0.5.
//                    One block per RoI, the M x M cells spread over its threads.  The x side of every sample (cell column pw,
//                    grid column ix: the low pixel and the fraction) depends on the RoI alone, so the block computes it once
//                    into LDS; a cell then walks its gh x gw samples with iy outer and ix inner into ONE f32 accumulator, as
//                    ROIAlign_cpu.cpp does.  The four taps of a sample are two adjacent bits of two adjacent rows: the thread
//                    keeps two words of each row in registers and reloads them when the low pixel leaves the first word.
// Every f32 operation is rounded on its own (no FMA): the bytes equal a reference that rounds every operation.  The library is
// built with -ffp-contract=off; the pragma below keeps that true for this file under any flags.
#include "apse_common.h"
#include "apse_kernels.h"
#include "../../include/apse_hip.h"
#include "mots_window.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTargetThreads = 256;
constexpr int kXTable = 4096;          // LDS entries of the per-RoI x table (mask_size * gw); a wider grid computes x per sample
constexpr int kMaxGrid = 8192;         // samples per cell and axis; a larger grid (a box beyond 8192 * mask_size pixels) is a zero row
constexpr int kInvalid = INT_MIN;

__host__ __device__ inline bool rect_inside(const int* r, int wpr, int h, int w) {     // an empty rect is legal anywhere
    if (r[0] >= r[2] || r[1] >= r[3]) return true;
    if (r[0] < 0 || r[1] < 0 || r[2] > w || r[3] > h) return false;
    return wpr >= ((r[2] + 63) >> 6) - (r[0] >> 6);
}

// ---------------------------------------------------------------- remap_windows
__global__ void __launch_bounds__(256) remap_windows(const apse_mots_window* __restrict__ src, const int* __restrict__ xmap,
                                                     const int* __restrict__ ymap, int h, int w,
                                                     const apse_mots_window* __restrict__ dst) {
    const apse_mots_window d = dst[blockIdx.y];
    const int rows = d.rect[3] - d.rect[1];
    if (d.rect[0] >= d.rect[2] || rows <= 0 || !d.bits || !rect_inside(d.rect, d.words_per_row, h, w)) return;
    const apse_mots_window s = src[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int base = d.rect[0] >> 6;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
        const int sy = ymap[d.rect[1] + r];
        for (int c = 0; c < d.words_per_row; ++c) {
            const int x = (base + c) * 64 + lane;
            bool set = false;
            if (x >= d.rect[0] && x < d.rect[2]) {
                const int sx = xmap[x];
                if (sx >= 0) set = (window_word(s, sy, sx >> 6) >> (sx & 63)) & 1;      // 0 outside the source window
            }
            const uint64_t m = __ballot(set);
            if (lane == 0) d.bits[(size_t)r * d.words_per_row + c] = m;
        }
    }
}

// ---------------------------------------------------------------- bitmask_targets
// pre_calc_for_bilinear_interpolate for one axis: the low cell and the fraction of coordinate v over `size` cells; low = kInvalid
// outside (-1, size).  At the top (low >= size - 1) both cells are size - 1 and the fraction is 0; the caller reads cell low + 1
// with weight 0 there, which adds the same +0.
__device__ __forceinline__ void axis_prep(float v, int size, int* low, float* frac) {
    if (v < -1.0f || v > (float)size || v != v) {
        *low = kInvalid;
        *frac = 0.0f;
        return;
    }
    if (v <= 0.0f) v = 0.0f;
    int lo = (int)v;
    if (lo >= size - 1) {
        lo = size - 1;
        v = (float)lo;
    }
    *low = lo;
    *frac = v - (float)lo;
}

__device__ __forceinline__ float sample_coord(float start, int p, float bin, int i, int grid) {
    return (start + (float)p * bin) + __fdiv_rn(((float)i + 0.5f) * bin, (float)grid);
}

__global__ void __launch_bounds__(kTargetThreads) bitmask_targets(const apse_mots_window* __restrict__ windows, int n_obj, int h,
                                                                  int w, const float* __restrict__ rois,
                                                                  const int* __restrict__ matched, int M,
                                                                  uint8_t* __restrict__ out) {
    __shared__ int s_xlow[kXTable];
    __shared__ float s_xfrac[kXTable];
    const int r = blockIdx.x;
    const int tid = threadIdx.x;
    uint8_t* o = out + (size_t)r * M * M;
    const int obj = matched[r];
    apse_mots_window win = {};
    if (obj >= 0 && obj < n_obj) win = windows[obj];
    const float sw = rois[4 * r] - 0.5f, sh = rois[4 * r + 1] - 0.5f;
    const float rw = (rois[4 * r + 2] - 0.5f) - sw, rh = (rois[4 * r + 3] - 0.5f) - sh;
    const float qw = __fdiv_rn(rw, (float)M), qh = __fdiv_rn(rh, (float)M);            // the bin sizes
    const bool live = win.bits && win.rect[0] < win.rect[2] && win.rect[1] < win.rect[3] && qw > 0.0f && qh > 0.0f &&
                      qw <= (float)kMaxGrid && qh <= (float)kMaxGrid;
    if (!live) {                                             // block-uniform: no object, no pixels, or an empty sample grid
        for (int c = tid; c < M * M; c += kTargetThreads) o[c] = 0;
        return;
    }
    const int gw = (int)ceilf(qw), gh = (int)ceilf(qh);     // 1 .. kMaxGrid each
    const float count = (float)(gh * gw);
    const bool table = M * gw <= kXTable;
    if (table) {
        for (int e = tid; e < M * gw; e += kTargetThreads) {
            const int pw = e / gw;
            axis_prep(sample_coord(sw, pw, qw, e - pw * gw, gw), w, &s_xlow[e], &s_xfrac[e]);
        }
    }
    __syncthreads();
    for (int c = tid; c < M * M; c += kTargetThreads) {
        const int ph = c / M, pw = c - ph * M;
        float acc = 0.0f;
        for (int iy = 0; iy < gh; ++iy) {
            const float y = sample_coord(sh, ph, qh, iy, gh);
            if (y > (float)h) break;                         // y only grows with iy: the rest is outside too
            int ylow;
            float ly;
            axis_prep(y, h, &ylow, &ly);
            if (ylow == kInvalid) continue;                  // an invalid sample adds +0
            const float hy = 1.0f - ly;
            int cur = kInvalid;                              // word column held in a0 / b0 (a1 / b1: the next one)
            uint64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
            for (int ix = 0; ix < gw; ++ix) {
                int xlow;
                float lx;
                if (table) {
                    xlow = s_xlow[pw * gw + ix];
                    lx = s_xfrac[pw * gw + ix];
                } else {
                    const float x = sample_coord(sw, pw, qw, ix, gw);
                    if (x > (float)w) break;
                    axis_prep(x, w, &xlow, &lx);
                }
                if (xlow == kInvalid) continue;
                const int aw = xlow >> 6;
                if (aw != cur) {
                    cur = aw;
                    a0 = window_word(win, ylow, aw);
                    a1 = window_word(win, ylow, aw + 1);
                    b0 = window_word(win, ylow + 1, aw);
                    b1 = window_word(win, ylow + 1, aw + 1);
                }
                const int bl = xlow & 63, bh = (xlow + 1) & 63;
                const bool nextw = bl == 63;
                const float v1 = (float)((a0 >> bl) & 1), v2 = (float)(((nextw ? a1 : a0) >> bh) & 1);
                const float v3 = (float)((b0 >> bl) & 1), v4 = (float)(((nextw ? b1 : b0) >> bh) & 1);
                const float hx = 1.0f - lx;
                const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                acc = acc + (((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4);
            }
        }
        o[c] = __fdiv_rn(acc, count) >= 0.5f ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int apse_k_remap_windows(const apse_mots_window* src, int n, const int* xmap, const int* ymap, int h, int w,
                         const apse_mots_window* dst, hipStream_t s) {
    const int gx = (h + 3) / 4 < 64 ? (h + 3) / 4 : 64;
    remap_windows<<<dim3(gx, n), 256, 0, s>>>(src, xmap, ymap, h, w, dst);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_k_bitmask_targets(const apse_mots_window* windows, int n_obj, int h, int w, const float* rois, const int* matched, int n,
                           int mask_size, uint8_t* out, hipStream_t s) {
    bitmask_targets<<<n, kTargetThreads, 0, s>>>(windows, n_obj, h, w, rois, matched, mask_size, out);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_mots_remap_windows(const apse_mots_window* src, int n, int H, int W, const int* xmap, const int* ymap, int h, int w,
                            const apse_mots_window* dst, const apse_mots_window* dst_host, void* stream) {
    if (!frame_ok(H, W) || !frame_ok(h, w) || n < 0 || n > APSE_MOTS_MAX_OBJECTS) return APSE_E_INVALID;
    if (n == 0) return APSE_OK;
    if (!src || !xmap || !ymap || !dst || !dst_host) return APSE_E_INVALID;
    for (int k = 0; k < n; ++k)
        if (!rect_inside(dst_host[k].rect, dst_host[k].words_per_row, h, w)) return APSE_E_INVALID;
    return apse_k_remap_windows(src, n, xmap, ymap, h, w, dst, (hipStream_t)stream);
}

int apse_bitmask_targets(const apse_mots_window* windows, int n_obj, int h, int w, const float* rois, const int* matched, int n,
                         int mask_size, uint8_t* out, void* stream) {
    if (!frame_ok(h, w) || n_obj < 0 || n_obj > APSE_MOTS_MAX_OBJECTS || n < 0 || n > APSE_MASK_TRAIN_MAX_N || mask_size < 1 ||
        mask_size > APSE_BITMASK_MAX_SIZE)
        return APSE_E_INVALID;
    if (n == 0) return APSE_OK;
    if (!rois || !matched || !out || (n_obj > 0 && !windows)) return APSE_E_INVALID;
    return apse_k_bitmask_targets(windows, n_obj, h, w, rois, matched, n, mask_size, out, (hipStream_t)stream);
}

}  // extern "C"
