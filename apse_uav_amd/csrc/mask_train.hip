// Mask-head training (include/apse_hip.h "Mask-head training"): the f32 kernels behind dcnn/scripts/train/finetune_segmentation.py
// for MaskRCNNConvUpsampleHead (4 x (conv3x3 256 + ReLU) -> deconv 2x2 stride 2 + ReLU -> 1x1 predictor) and mask_rcnn_loss.
// DESIGN.md "Mask-head training" gives the rules.
//
//   pack          device-side filter packing: the checkpoint's layouts (OIHW, deconv [Cin][Cout][2][2]) -> the rows apse_conv2d
//                 reads (the bytes apse_conv_pack_weight writes on the host), and the flipped / transposed rows that turn the 3x3
//                 data gradient into a forward convolution.  The master weights stay torch leaves; nothing goes through the host.
//   conv3x3       the 256 -> 256 3x3 layers, forward and (with the flipped / transposed pack) data gradient, as an implicit GEMM on
//                 v_mfma_f32_32x32x2_f32 with the reduction summed in chains of 64: the forward error of training feeds the
//                 ReLU masks of the gradients, so it is kept near that of a blocked sum.
//   conv          the deconvolution (forward, and its data gradient as a 2x2 stride-2 convolution) and the predictor:
//                 conv_igemm_f32 through apse_launch_conv, tile shape and K split from plan constants exactly as a
//                 max_batch = 1 context chooses them for its mask head, so a result does not depend on the number of RoIs.
//   wgrad         the weight gradient as an implicit GEMM on v_mfma_f32_32x32x2_f32: dW = A^T B with the RoI pixels as the
//                 reduction, 128 x 128 tiles, 32 pixels per step, LDS double buffer, split over the reduction into chunks whose
//                 partial tiles a second kernel adds in chunk order.  One instantiation per gather: 3x3 taps of X (conv) and the
//                 2x2 taps of dY (deconvolution).
//   relu / bias   g = dY where the saved output is positive; db = column sums, rows in ascending order inside fixed slices, slices
//                 in ascending order.
//   loss          binary_cross_entropy_with_logits on the ground-truth class channel (mean over n x 784), the three logged
//                 ratios, and d = (sigmoid(x) - t) / (n x 784) for that channel only.
//   predictor     dX = d W[class] under the deconvolution's ReLU mask, dW[class] and db[class]: per-RoI sums, then RoIs in
//                 ascending order per class.
// conv3x3 and wgrad run the 128 x 128 MFMA tile and the chain-of-64 summation rule that train_tile.h describes once, for them and
// for box_train.hip's fc_gemm.
// Determinism: no float atomics; every sum has a fixed order that depends on the shapes only.
#include "apse_kernels.h"
#include "train_tile.h"
#include "../../include/apse_hip.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int kC = 256;                 // channels of the head
constexpr int kPool = 14, kUp = 28;     // RoI grid, logits grid
constexpr int kPix = kPool * kPool, kUpPix = kUp * kUp;
constexpr int kPlanDets = 8;            // APSE_EXPECTED_DETS of plan.hip: the list length a context shapes its mask-head GEMMs for

int invalid(const char* msg) { return apse_fail_global(APSE_E_INVALID, msg); }
int launched() { return hipGetLastError() == hipSuccess ? APSE_OK : apse_fail_global(APSE_E_HIP, "mask_train: kernel launch failed"); }
int pow2_at_least(int v) { int p = 4; while (p < v) p <<= 1; return p; }

// ---------------------------------------------------------------------------------------------------------------- pack
// out[o][r][s * cin_p + ci], rows padded with zeros to KWCp floats and to a multiple of 128 filters.
//   kind 0: w is OIHW [Cout][Cin][KH][KW]                                   -> value w[o][ci][r][s]
//   kind 1: w is OIHW [Cin][Cout][3][3] of the FORWARD layer; the data gradient dX = conv(dY, W') has
//           W'[o = ci_fwd][ci = co_fwd][r][s] = w[co_fwd][ci_fwd][2 - r][2 - s]
//   kind 2: w is ConvTranspose2d [Cin][Cc][2][2]; the forward runs as a 1x1 convolution with Cout = 4 Cc rows
//           o = (dy * 2 + dx) * Cc + co                                      -> value w[ci][co][dy][dx]
__global__ void pack_filter(const float* __restrict__ w, int kind, int Cout, int Cin, int KH, int KW, int cin_p, int KWCp,
                            size_t total, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pos = (int)(i % KWCp);
        const size_t orow = i / KWCp;
        const int r = (int)(orow % KH), o = (int)(orow / KH);
        const int s = pos / cin_p, ci = pos - s * cin_p;
        float v = 0.f;
        if (o < Cout && s < KW && ci < Cin) {
            if (kind == 0) v = w[(((size_t)o * Cin + ci) * KH + r) * KW + s];
            else if (kind == 1) v = w[(((size_t)ci * Cout + o) * 3 + (2 - r)) * 3 + (2 - s)];
            else { const int cc = Cout >> 2, g = o / cc, co = o - g * cc; v = w[((size_t)ci * cc + co) * 4 + g]; }
        }
        out[i] = v;
    }
}
__global__ void pack_bias(const float* __restrict__ b, int n, int n_p, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_p) out[i] = (b && i < n) ? b[i] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- wgrad
// out[m][tap][c] = sum_p A[p][m] * Bt(p, tap)[c], m and c in 0..255, p over the n * 196 pixels of the 14 x 14 RoI grids.
//   MODE 0 (3x3 convolution, 9 taps):  A = dY [n][14][14][256], Bt(p, (kh, kw)) = X[r][y + kh - 1][x + kw - 1][:] (zero outside)
//   MODE 1 (deconvolution, 4 taps):    A = X  [n][14][14][256], Bt(p, (a, b))  = dY[r][2 y + a][2 x + b][:]   (dY on 28 x 28)
// Block = train_tile.h's tile on 128 (m) x 128 (c) of one tap and one chunk of the reduction, a stage = 32 pixels.
// The f32 MFMA takes A[i = lane & 31][k = lane >> 5] and B[k = lane >> 5][j = lane & 31] in one register each: both operand
// tiles sit in LDS reduction-major (train_tile.h), so a lane's operand is one ds_read_b32.
constexpr int kLd = kLdMajor;
constexpr int kWgLds = 2 * 2 * kMajorFloats * (int)sizeof(float);    // double buffer x (A, B)

template <int MODE>
__global__ __launch_bounds__(256) void wgrad_mfma(const float* __restrict__ A, const float* __restrict__ B, int P,
                                                  int steps_per_chunk, int total_steps, int nchunks, float* __restrict__ part) {
    constexpr int NTAP = MODE == 0 ? 9 : 4;
    constexpr int TILES = 2 * NTAP * 2;
    extern __shared__ __align__(16) float lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // XCD-aware order over (chunk, tile) pairs: the tiles that read the same pixels share an L2
    const int bid = apse_xcd_remap(blockIdx.x, TILES * nchunks);
    const int chunk = bid / TILES, tile = bid - chunk * TILES;
    const int tile_m = tile / (NTAP * 2), rem = tile - tile_m * (NTAP * 2);
    const int tap = rem >> 1, m0 = tile_m * 128, c0 = (rem & 1) * 128;
    const int t0 = MODE == 0 ? tap / 3 : tap >> 1, t1 = MODE == 0 ? tap - t0 * 3 : tap & 1;
    const int step_lo = chunk * steps_per_chunk;
    const int nsteps = min(steps_per_chunk, total_steps - step_lo);
    const int p_end = min(P, (step_lo + nsteps) * kKT);

    const int srow = t >> 5, c4 = t & 31;       // staging: rows srow + 8 i, one float4 of the 128-wide row
    f32x4 ra[4], rb[4];
    auto fetch = [&](int step) {
        const int p0 = (step_lo + step) * kKT;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = p0 + srow + 8 * i;
            ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p < p_end) {
                ra[i] = *reinterpret_cast<const f32x4*>(A + (size_t)p * kC + m0 + c4 * 4);
                const int r = p / kPix, q = p - r * kPix, y = q / kPool, x = q - y * kPool;
                if (MODE == 0) {
                    const int sy = y + t0 - 1, sx = x + t1 - 1;
                    if ((unsigned)sy < (unsigned)kPool && (unsigned)sx < (unsigned)kPool)
                        rb[i] = *reinterpret_cast<const f32x4*>(B + ((size_t)r * kPix + sy * kPool + sx) * kC + c0 + c4 * 4);
                } else {
                    rb[i] = *reinterpret_cast<const f32x4*>(B + ((size_t)r * kUpPix + (2 * y + t0) * kUp + 2 * x + t1) * kC + c0 + c4 * 4);
                }
            }
        }
    };
    auto stage = [&](int buf) {
        float* as = lds + buf * (2 * kKT * kLd);
        float* bs = as + kKT * kLd;
#pragma unroll
        for (int i = 0; i < 4; ++i) {              // stage_major's layout, A and B rows interleaved
            *reinterpret_cast<f32x4*>(as + (srow + 8 * i) * kLd + c4 * 4) = ra[i];
            *reinterpret_cast<f32x4*>(bs + (srow + 8 * i) * kLd + c4 * 4) = rb[i];
        }
    };

    // two-level sum: the MFMA chain runs over kFlush steps (64 pixels), then joins the running total -- chains stay short, which
    // keeps the rounding error of a long reduction near that of a blocked sum
    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; tot[i][j][e] = 0.f; }
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, l31 = lane & 31, kh2 = lane >> 5;

    fetch(0);
    stage(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (more) fetch(s + 1);                                  // global loads of the next step fly under this step's MFMAs
        const float* as = lds + (s & 1) * (2 * kKT * kLd);
        const float* bs = as + kKT * kLd;
#pragma unroll
        for (int kk = 0; kk < kKT / 2; ++kk) {
            const int k = 2 * kk + kh2;
            const float a0 = as[k * kLd + wm + l31], a1 = as[k * kLd + wm + 32 + l31];
            const float b0 = bs[k * kLd + wn + l31], b1 = bs[k * kLd + wn + 32 + l31];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if ((s % kFlush) == kFlush - 1 || !more) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
                }
        }
        if (more) stage((s + 1) & 1);       // the other buffer: its readers (step s - 1) passed the barrier below one step ago
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh2;
                const int c = c0 + wn + j * 32 + l31;
                part[(((size_t)chunk * kC + m) * NTAP + tap) * kC + c] = tot[i][j][e];
            }
}

// ---------------------------------------------------------------------------------------------------------------- conv3x3
// Y[p][co] = relu?(bias[co] + sum_{kh,kw,ci} X[p + (kh - 1, kw - 1)][ci] * Wp[co][kh][kw * 256 + ci]) for the 256 -> 256 3x3 layers
// on 14 x 14 RoI grids: the forward of mask_fcnN and, with the flipped / transposed pack, its data gradient.  Same MFMA and block
// shape as wgrad_mfma (128 pixels x 128 channels, 4 waves of 2 x 2 tiles); here the reduction index is the contiguous one of both
// operands, so the tiles sit in LDS as [row][32 k + 4] and a lane reads row (lane & 31), column k.  72 steps of 32 k (tap-major),
// the same two-level sum: K = 2304 as 36 chains of 64.  The inference kernel runs one long chain per K split; this one is for
// training, where the forward error feeds the ReLU masks of the gradients.
constexpr int kFLd = 36;
constexpr int kFwLds = 2 * 2 * 128 * kFLd * (int)sizeof(float);

__global__ __launch_bounds__(256) void conv3x3_mfma(const float* __restrict__ X, const float* __restrict__ Wp,
                                                    const float* __restrict__ bias, int P, int relu, float* __restrict__ Y) {
    extern __shared__ __align__(16) float lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int bid = apse_xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (bid >> 1) * 128, n0 = (bid & 1) * 128;
    const int srow = t >> 3, k4 = t & 7;            // staging: rows srow + 32 i, float4 at k = 4 k4
    int py[4], px[4], pp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = m0 + srow + 32 * i;
        const int r = p / kPix, q = p - r * kPix;
        py[i] = q / kPool; px[i] = q - py[i] * kPool;
        pp[i] = p < P ? p : -1;
    }
    f32x4 ra[4], rb[4];
    auto fetch = [&](int step) {
        const int tap = step >> 3, ci0 = (step & 7) * 32 + k4 * 4;
        const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int sy = py[i] + kh - 1, sx = px[i] + kw - 1;
            if (pp[i] >= 0 && (unsigned)sy < (unsigned)kPool && (unsigned)sx < (unsigned)kPool)
                ra[i] = *reinterpret_cast<const f32x4*>(X + (size_t)(pp[i] + (kh - 1) * kPool + (kw - 1)) * kC + ci0);
            rb[i] = *reinterpret_cast<const f32x4*>(Wp + ((size_t)(n0 + srow + 32 * i) * 3 + kh) * (3 * kC) + kw * kC + ci0);
        }
    };
    auto stage = [&](int buf) {
        float* as = lds + buf * (2 * 128 * kFLd);
        float* bs = as + 128 * kFLd;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(as + (srow + 32 * i) * kFLd + k4 * 4) = ra[i];
            *reinterpret_cast<f32x4*>(bs + (srow + 32 * i) * kFLd + k4 * 4) = rb[i];
        }
    };
    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; tot[i][j][e] = 0.f; }
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, l31 = lane & 31, kh2 = lane >> 5;
    constexpr int NSTEPS = 9 * kC / 32;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int s = 0; s < NSTEPS; ++s) {
        const bool more = s + 1 < NSTEPS;
        if (more) fetch(s + 1);
        const float* as = lds + (s & 1) * (2 * 128 * kFLd);
        const float* bs = as + 128 * kFLd;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const int k = 2 * kk + kh2;
            const float a0 = as[(wm + l31) * kFLd + k], a1 = as[(wm + 32 + l31) * kFLd + k];
            const float b0 = bs[(wn + l31) * kFLd + k], b1 = bs[(wn + 32 + l31) * kFLd + k];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if ((s % kFlush) == kFlush - 1 || !more) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
                }
        }
        if (more) stage((s + 1) & 1);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = n0 + wn + j * 32 + l31;
            const float bv = bias ? bias[c] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh2;
                float v = tot[i][j][e] + bv;
                if (relu) v = v > 0.f ? v : 0.f;
                if (m < P) Y[(size_t)m * kC + c] = v;
            }
        }
}

// dw[m][c][tap] = sum over chunks, in chunk order, of part[chunk][m][tap][c]
template <int NTAP>
__global__ void wgrad_reduce(const float* __restrict__ part, int nchunks, float* __restrict__ dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kC * NTAP * kC) return;
    const int c = i & (kC - 1), tap = (i >> 8) % NTAP, m = i / (NTAP * kC);
    float v = part[i];
    for (int z = 1; z < nchunks; ++z) v += part[(size_t)z * kC * NTAP * kC + i];
    dw[((size_t)m * kC + c) * NTAP + tap] = v;
}

struct WgPlan { int total_steps, steps_per_chunk, nchunks; };
WgPlan wgrad_plan(int n, int ntap) {
    WgPlan w;
    w.total_steps = (n * kPix + kKT - 1) / kKT;
    const int tiles = 4 * ntap;
    int target = 512 / tiles;                          // about two blocks per CU
    if (target < 1) target = 1;
    const int s = w.total_steps < target ? w.total_steps : target;
    w.steps_per_chunk = (w.total_steps + s - 1) / s;
    w.nchunks = (w.total_steps + w.steps_per_chunk - 1) / w.steps_per_chunk;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------- relu / bias
__global__ void relu_grad(const f32x4* __restrict__ y, const f32x4* __restrict__ dy, size_t n4, f32x4* __restrict__ g) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 a = y[i], d = dy[i];
        g[i] = f32x4{a[0] > 0.f ? d[0] : 0.f, a[1] > 0.f ? d[1] : 0.f, a[2] > 0.f ? d[2] : 0.f, a[3] > 0.f ? d[3] : 0.f};
    }
}
// part[slice][c] = sum of g[row][c] over the slice's rows in ascending order; then db[c] = sum of the slices in ascending order
__global__ void bias_slices(const float* __restrict__ g, long rows, int rows_per_slice, float* __restrict__ part) {
    const long lo = (long)blockIdx.x * rows_per_slice;
    const long hi = lo + rows_per_slice < rows ? lo + rows_per_slice : rows;
    const int c = threadIdx.x;
    float v = 0.f;
    for (long r = lo; r < hi; ++r) v += g[r * kC + c];
    part[(size_t)blockIdx.x * kC + c] = v;
}
__global__ void bias_finish(const float* __restrict__ part, int slices, float* __restrict__ db) {
    const int c = threadIdx.x;
    float v = part[c];
    for (int s = 1; s < slices; ++s) v += part[(size_t)s * kC + c];
    db[c] = v;
}
int bias_rows_per_slice(long rows) { long r = (rows + 511) / 512; return (int)(r < 64 ? 64 : r); }

// ---------------------------------------------------------------------------------------------------------------- loss
__device__ __forceinline__ int roi_class(const int* cls, int r, int K) {
    if (K == 1) return 0;
    const int k = cls[r];
    return k < 0 ? 0 : (k >= K ? K - 1 : k);           // the caller checks the range on the host; never index outside the row
}
// One block per RoI: part[r] = {sum of the 784 loss terms, wrong pixels, positives, wrong negatives (fp), wrong positives (fn)}.
// A thread adds its pixels t, t + 256, ... in that order in f32 (at most 4 terms), the tree and everything above it run in f64.
__global__ __launch_bounds__(256) void loss_rows(const float* __restrict__ logits, int K, const int* __restrict__ cls,
                                                 const uint8_t* __restrict__ tgt, double* __restrict__ part) {
    __shared__ double red[256];
    const int r = blockIdx.x, t = threadIdx.x, k = roi_class(cls, r, K);
    float loss = 0.f;
    int wrong = 0, pos = 0, fp = 0, fn = 0;
    for (int p = t; p < kUpPix; p += 256) {
        const float x = logits[((size_t)r * kUpPix + p) * K + k];
        const bool tb = tgt[(size_t)r * kUpPix + p] != 0;
        const float tv = tb ? 1.f : 0.f;
        loss += (fmaxf(x, 0.f) - x * tv) + log1pf(expf(-fabsf(x)));
        const bool bad = (x > 0.f) != tb;
        wrong += bad; pos += tb; fp += bad && !tb; fn += bad && tb;
    }
    const double v[5] = {(double)loss, (double)wrong, (double)pos, (double)fp, (double)fn};
    for (int j = 0; j < 5; ++j) {
        const double s = block_sum_d(v[j], red);
        if (t == 0) part[(size_t)r * 5 + j] = s;
    }
}
// out = {loss_mask, mask_rcnn/accuracy, mask_rcnn/false_positive, mask_rcnn/false_negative}
__global__ __launch_bounds__(256) void loss_finish(const double* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double tot[5];
    for (int j = 0; j < 5; ++j) {
        double v = 0.0;
        for (int r = t; r < n; r += 256) v += part[(size_t)r * 5 + j];
        tot[j] = block_sum_d(v, red);
    }
    if (t == 0) {
        const double numel = (double)n * kUpPix;
        out[0] = (float)(tot[0] / numel);
        out[1] = (float)(1.0 - tot[1] / fmax(numel, 1.0));
        out[2] = (float)(tot[3] / fmax(numel - tot[2], 1.0));
        out[3] = (float)(tot[4] / fmax(tot[2], 1.0));
    }
}
// d[r][p] = (sigmoid(x) - t) * grad / (n * 784) on the ground-truth class channel
__global__ void loss_grad(const float* __restrict__ logits, int K, const int* __restrict__ cls, const uint8_t* __restrict__ tgt,
                          int n, const float* __restrict__ grad_loss, float* __restrict__ d) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * kUpPix) return;
    const int r = (int)(i / kUpPix), k = roi_class(cls, r, K);
    const float x = logits[i * K + k];
    const float tv = tgt[i] ? 1.f : 0.f;
    const float sg = 1.f / (1.f + expf(-x));
    const float go = grad_loss ? grad_loss[0] : 1.f;
    d[i] = (sg - tv) * go / (float)((size_t)n * kUpPix);
}

// ---------------------------------------------------------------------------------------------------------------- predictor
// g5[r][p][c] = a5 > 0 ? d[r][p] * Wp[class(r)][c] : 0
__global__ void pred_dx(const float* __restrict__ d, const f32x4* __restrict__ a5, const int* __restrict__ cls, int K,
                        const float* __restrict__ wp, size_t n4, f32x4* __restrict__ g5) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t px = i >> 6;
        const int c4 = (int)(i & 63), r = (int)(px / kUpPix), k = roi_class(cls, r, K);
        const f32x4 a = a5[i];
        const f32x4 w = *reinterpret_cast<const f32x4*>(wp + (size_t)k * kC + c4 * 4);
        const float dv = d[px];
        g5[i] = f32x4{a[0] > 0.f ? dv * w[0] : 0.f, a[1] > 0.f ? dv * w[1] : 0.f, a[2] > 0.f ? dv * w[2] : 0.f,
                      a[3] > 0.f ? dv * w[3] : 0.f};
    }
}
// part[r][c] = sum_p d[r][p] a5[r][p][c] (an fmaf chain per row of 28 pixels, rows added in ascending order), part[r][256] =
// sum_p d[r][p] (fixed tree)
__global__ __launch_bounds__(256) void pred_dw_rows(const float* __restrict__ d, const float* __restrict__ a5, float* __restrict__ part) {
    __shared__ float dl[kUpPix];
    __shared__ float red[256];
    const int r = blockIdx.x, c = threadIdx.x;
    float own = 0.f;
    for (int p = c; p < kUpPix; p += 256) { const float v = d[(size_t)r * kUpPix + p]; dl[p] = v; own += v; }
    red[c] = own;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (c < s) red[c] = red[c] + red[c + s];
        __syncthreads();
    }
    float v = 0.f;
    const float* a = a5 + (size_t)r * kUpPix * kC + c;
    for (int y = 0; y < kUp; ++y) {                       // two-level: one chain per row of 28 pixels, rows in ascending order
        float row = 0.f;
        for (int x = 0; x < kUp; ++x) row = fmaf(dl[y * kUp + x], a[(size_t)(y * kUp + x) * kC], row);
        v += row;
    }
    part[(size_t)r * (kC + 1) + c] = v;
    if (c == 0) part[(size_t)r * (kC + 1) + kC] = red[0];
}
// dW[k][c] = sum over the RoIs of class k in ascending order; classes without a RoI get exactly 0
__global__ __launch_bounds__(256) void pred_dw_finish(const float* __restrict__ part, const int* __restrict__ cls, int n, int K,
                                                      float* __restrict__ dw, float* __restrict__ db) {
    const int k = blockIdx.x, c = threadIdx.x;
    float v = 0.f, b = 0.f;
    for (int r = 0; r < n; ++r) {
        if (roi_class(cls, r, K) != k) continue;
        v += part[(size_t)r * (kC + 1) + c];
        if (c == 0) b += part[(size_t)r * (kC + 1) + kC];
    }
    dw[(size_t)k * kC + c] = v;
    if (c == 0) db[k] = b;
}

__global__ void roi_index_fill(int* idx, int n) {       // idx[0..n) = 0 (image of every RoI), idx[n] = n (live count)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = 0;
    else if (i == n) idx[i] = n;
}

bool n_ok(int n) { return n >= 1 && n <= APSE_MASK_TRAIN_MAX_N; }

// tile shape and K split of a mask-head convolution: from plan constants, as add_conv (detector.hip) picks them for a
// max_batch = 1 context's packed detection list
int plan_cfg(int OH, int OW, int Cout, int steps, int* sk) {
    *sk = 1;
    return apse_conv_pick_cfg(kPlanDets * OH * OW, Cout, steps, sk);
}
size_t conv_ws_bytes(int n, int H, int W, int Cout, int KH, int KW, int stride, int pad, int cin) {
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
    const int steps = KH * (apse_roundup(KW * cin, 32) / 32);
    int sk = 1;
    plan_cfg(OH, OW, Cout, steps, &sk);
    if (sk > steps) sk = steps;
    return sk > 1 ? (size_t)sk * n * OH * OW * Cout * sizeof(float) : 0;
}

}  // namespace

// index array of apse_mask_roi_features (detector.hip)
extern "C" int apse_k_mask_roi_index(int* idx, int n, hipStream_t s) {
    hipLaunchKernelGGL(roi_index_fill, dim3((n + 1 + 255) / 256), dim3(256), 0, s, idx, n);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

extern "C" {

size_t apse_mask_pack_elems(int Cout, int Cin, int KH, int KW) {
    if (Cout < 1 || Cin < 1 || KH < 1 || KW < 1) return 0;
    return (size_t)apse_roundup(Cout, 128) * KH * apse_roundup(KW * pow2_at_least(Cin), 32);
}

int apse_mask_pack_weight(const float* w, const float* bias, int kind, int Cout, int Cin, int KH, int KW, float* packed,
                          float* bias_packed, void* stream) {
    if (!w || !packed || kind < 0 || kind > 2 || Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || Cout > 4096 || Cin > 4096 || KH > 7 || KW > 7)
        return invalid("apse_mask_pack_weight: null pointer or shape outside 1..4096 channels, 1..7 taps");
    if (kind == 1 && (KH != 3 || KW != 3)) return invalid("apse_mask_pack_weight: kind 1 (data gradient) packs 3x3 filters");
    if (kind == 2 && (KH != 1 || KW != 1 || (Cout & 3))) return invalid("apse_mask_pack_weight: kind 2 (deconvolution) is 1x1 with Cout = 4 x channels");
    const int cin_p = pow2_at_least(Cin), KWCp = apse_roundup(KW * cin_p, 32);
    const size_t total = apse_mask_pack_elems(Cout, Cin, KH, KW);
    hipStream_t s = (hipStream_t)stream;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_filter, dim3((unsigned)blocks), dim3(256), 0, s, w, kind, Cout, Cin, KH, KW, cin_p, KWCp, total, packed);
    if (bias_packed) {
        const int nb = kind == 2 ? Cout / 4 : Cout, nb_p = apse_roundup(Cout, 128);
        hipLaunchKernelGGL(pack_bias, dim3((nb_p + 255) / 256), dim3(256), 0, s, bias, nb, nb_p, bias_packed);
    }
    return launched();
}

size_t apse_mask_train_workspace_bytes(int n, int K) {
    if (!n_ok(n) || K < 1 || K > APSE_MAX_CLASSES) return 0;
    size_t need = 0;
    auto up = [&](size_t v) { if (v > need) need = v; };
    up(conv_ws_bytes(n, kPool, kPool, 4 * kC, 1, 1, 1, 0, kC));           // deconvolution forward
    up(conv_ws_bytes(n, kUp, kUp, kC, 2, 2, 2, 0, kC));                   // deconvolution data gradient
    up(conv_ws_bytes(n, kUp, kUp, K, 1, 1, 1, 0, kC));                    // predictor
    const WgPlan w9 = wgrad_plan(n, 9), w4 = wgrad_plan(n, 4);
    up((size_t)w9.nchunks * kC * 9 * kC * sizeof(float));
    up((size_t)w4.nchunks * kC * 4 * kC * sizeof(float));
    up((size_t)512 * kC * sizeof(float));                                 // bias slices
    up((size_t)n * (kC + 1) * sizeof(float));                             // predictor rows
    up((size_t)n * 5 * sizeof(double));                                   // loss rows
    return need;
}

int apse_mask_conv_forward(const float* x, const float* w_packed, const float* bias_packed, int n, int H, int W, int Cin, int Cout,
                           int KH, int KW, int stride, int pad, int relu, int deconv, float* y, float* ws, size_t ws_bytes,
                           void* stream) {
    if (!n_ok(n)) return invalid("apse_mask_conv_forward: needs 1 <= n <= APSE_MASK_TRAIN_MAX_N (1024) RoIs");
    if (!x || !w_packed || !y) return invalid("apse_mask_conv_forward: null pointer");
    if (H < 1 || W < 1 || H > 64 || W > 64 || Cin < 4 || Cin > 4096 || (Cin & (Cin - 1)) || Cout < 1 || Cout > 4096 || KH < 1 ||
        KW < 1 || KH > 7 || KW > 7 || stride < 1 || stride > 2 || pad < 0 || pad > 3 || H + 2 * pad < KH || W + 2 * pad < KW)
        return invalid("apse_mask_conv_forward: shape outside the limits (maps up to 64 x 64, Cin a power of two in 4..4096, Cout <= 4096)");
    if (deconv && (KH != 1 || KW != 1 || stride != 1 || pad != 0 || (Cout & 15)))
        return invalid("apse_mask_conv_forward: the 2x2 deconvolution runs as a 1x1 convolution with Cout = 4 x channels");
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.x = x; p.w = w_packed; p.bias = bias_packed; p.y = y; p.ws = ws;
    p.B = n; p.H = H; p.W = W; p.cin_log2 = apse_ilog2(Cin);
    p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
    p.KWCp = apse_roundup(KW * Cin, 32);
    p.OH = (H + 2 * pad - KH) / stride + 1;
    p.OW = (W + 2 * pad - KW) / stride + 1;
    p.Cout = Cout; p.relu = relu;
    p.M = n * p.OH * p.OW; p.m_per_item = p.OH * p.OW;
    p.steps_total = KH * (p.KWCp / 32);
    p.out_mode = deconv ? 1 : 0;
    p.cdec = deconv ? Cout / 4 : 0;
    p.y_ld = deconv ? Cout / 4 : Cout;
    int sk = 1;
    const int cfg = plan_cfg(p.OH, p.OW, Cout, p.steps_total, &sk);
    if (sk > p.steps_total) sk = p.steps_total;
    p.splitk = sk;
    if (sk > 1 && (!ws || (size_t)sk * p.M * Cout * sizeof(float) > ws_bytes)) return invalid("apse_mask_conv_forward: workspace too small");
    const int rc = apse_launch_conv(p, cfg, (hipStream_t)stream);
    return rc ? apse_fail_global(rc, "apse_mask_conv_forward: convolution launch failed") : APSE_OK;
}

int apse_mask_conv3x3(const float* x, const float* w_packed, const float* bias_packed, int n, int relu, float* y, void* stream) {
    if (!n_ok(n)) return invalid("apse_mask_conv3x3: needs 1 <= n <= APSE_MASK_TRAIN_MAX_N (1024) RoIs");
    if (!x || !w_packed || !y) return invalid("apse_mask_conv3x3: null pointer");
    static bool attr_done = false;
    if (!attr_done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_mfma), hipFuncAttributeMaxDynamicSharedMemorySize, kFwLds);
        attr_done = true;
    }
    const int P = n * kPix;
    hipLaunchKernelGGL(conv3x3_mfma, dim3(2 * ((P + 127) / 128)), dim3(256), kFwLds, (hipStream_t)stream, x, w_packed, bias_packed, P,
                       relu, y);
    return launched();
}

int apse_mask_relu_grad(const float* y, const float* dy, long long elems, float* g, void* stream) {
    if (elems == 0) return APSE_OK;
    if (!y || !dy || !g || elems < 0 || (elems & 3)) return invalid("apse_mask_relu_grad: null pointer or a count that is not a multiple of 4");
    size_t blocks = ((size_t)(elems >> 2) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(relu_grad, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4*>(y),
                       reinterpret_cast<const f32x4*>(dy), (size_t)(elems >> 2), reinterpret_cast<f32x4*>(g));
    return launched();
}

int apse_mask_bias_grad(const float* g, long long rows, float* db, float* ws, size_t ws_bytes, void* stream) {
    if (!g || !db || !ws || rows < 1 || rows > (long long)APSE_MASK_TRAIN_MAX_N * kUpPix)
        return invalid("apse_mask_bias_grad: null pointer or rows outside 1..APSE_MASK_TRAIN_MAX_N x 784");
    const int rps = bias_rows_per_slice((long)rows);
    const int slices = (int)((rows + rps - 1) / rps);
    if (ws_bytes < (size_t)slices * kC * sizeof(float)) return invalid("apse_mask_bias_grad: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bias_slices, dim3(slices), dim3(kC), 0, s, g, (long)rows, rps, ws);
    hipLaunchKernelGGL(bias_finish, dim3(1), dim3(kC), 0, s, ws, slices, db);
    return launched();
}

int apse_mask_wgrad(const float* a, const float* b, int n, int kind, float* dw, float* ws, size_t ws_bytes, void* stream) {
    if (!n_ok(n)) return invalid("apse_mask_wgrad: needs 1 <= n <= APSE_MASK_TRAIN_MAX_N (1024) RoIs");
    if (!a || !b || !dw || !ws || kind < 0 || kind > 1) return invalid("apse_mask_wgrad: null pointer or kind not 0 (3x3) / 1 (deconvolution)");
    const int ntap = kind == 0 ? 9 : 4;
    const WgPlan w = wgrad_plan(n, ntap);
    if (ws_bytes < (size_t)w.nchunks * kC * ntap * kC * sizeof(float)) return invalid("apse_mask_wgrad: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    static bool attr_done = false;
    if (!attr_done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_mfma<0>), hipFuncAttributeMaxDynamicSharedMemorySize, kWgLds);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_mfma<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kWgLds);
        attr_done = true;
    }
    const int blocks = 4 * ntap * w.nchunks;
    const int rblocks = (kC * ntap * kC + 255) / 256;
    if (kind == 0) {
        hipLaunchKernelGGL(wgrad_mfma<0>, dim3(blocks), dim3(256), kWgLds, s, a, b, n * kPix, w.steps_per_chunk, w.total_steps, w.nchunks, ws);
        hipLaunchKernelGGL(wgrad_reduce<9>, dim3(rblocks), dim3(256), 0, s, ws, w.nchunks, dw);
    } else {
        hipLaunchKernelGGL(wgrad_mfma<1>, dim3(blocks), dim3(256), kWgLds, s, a, b, n * kPix, w.steps_per_chunk, w.total_steps, w.nchunks, ws);
        hipLaunchKernelGGL(wgrad_reduce<4>, dim3(rblocks), dim3(256), 0, s, ws, w.nchunks, dw);
    }
    return launched();
}

int apse_mask_loss_forward(const float* logits, int K, const int* classes, const uint8_t* targets, int n, float* out4, void* ws,
                           size_t ws_bytes, void* stream) {
    if (n == 0) return APSE_OK;
    if (!n_ok(n) || K < 1 || K > APSE_MAX_CLASSES) return invalid("apse_mask_loss_forward: needs 0 <= n <= APSE_MASK_TRAIN_MAX_N (1024) and 1 <= K <= APSE_MAX_CLASSES (80)");
    if (!logits || !targets || !out4 || !ws || (K > 1 && !classes)) return invalid("apse_mask_loss_forward: null pointer");
    if (ws_bytes < (size_t)n * 5 * sizeof(double)) return invalid("apse_mask_loss_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_rows, dim3(n), dim3(256), 0, s, logits, K, classes, targets, (double*)ws);
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(256), 0, s, (const double*)ws, n, out4);
    return launched();
}

int apse_mask_loss_backward(const float* logits, int K, const int* classes, const uint8_t* targets, int n, const float* grad_loss,
                            float* d, void* stream) {
    if (n == 0) return APSE_OK;
    if (!n_ok(n) || K < 1 || K > APSE_MAX_CLASSES) return invalid("apse_mask_loss_backward: needs 0 <= n <= APSE_MASK_TRAIN_MAX_N (1024) and 1 <= K <= APSE_MAX_CLASSES (80)");
    if (!logits || !targets || !d || (K > 1 && !classes)) return invalid("apse_mask_loss_backward: null pointer");
    const size_t total = (size_t)n * kUpPix;
    hipLaunchKernelGGL(loss_grad, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, K, classes,
                       targets, n, grad_loss, d);
    return launched();
}

int apse_mask_predictor_backward(const float* d, const float* a5, const int* classes, const float* w_pred, int n, int K, float* g5,
                                 float* dw, float* db, float* ws, size_t ws_bytes, void* stream) {
    if (!n_ok(n) || K < 1 || K > APSE_MAX_CLASSES) return invalid("apse_mask_predictor_backward: needs 1 <= n <= APSE_MASK_TRAIN_MAX_N (1024) and 1 <= K <= APSE_MAX_CLASSES (80)");
    if (!d || !a5 || !w_pred || !g5 || !dw || !db || !ws || (K > 1 && !classes)) return invalid("apse_mask_predictor_backward: null pointer");
    if (ws_bytes < (size_t)n * (kC + 1) * sizeof(float)) return invalid("apse_mask_predictor_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t n4 = (size_t)n * kUpPix * (kC / 4);
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(pred_dx, dim3((unsigned)blocks), dim3(256), 0, s, d, reinterpret_cast<const f32x4*>(a5), classes, K, w_pred, n4,
                       reinterpret_cast<f32x4*>(g5));
    hipLaunchKernelGGL(pred_dw_rows, dim3(n), dim3(256), 0, s, d, a5, ws);
    hipLaunchKernelGGL(pred_dw_finish, dim3(K), dim3(256), 0, s, ws, classes, n, K, dw, db);
    return launched();
}

// The targets of sampled proposals: the limits here, the kernel beside the polygon rule it shares (coco_eval.hip).
int apse_coco_mask_targets(const double* xy, const int* part_vert_off, int n_parts, const int* obj_part_off, int n_obj, int n_verts,
                      const float* rois, const int* matched, int n, int mask_size, uint8_t* targets, int* info, void* stream) {
    if (n < 0 || n > APSE_MASK_TRAIN_MAX_N) return invalid("apse_coco_mask_targets: needs 0 <= n <= APSE_MASK_TRAIN_MAX_N (1024) RoIs");
    if (mask_size != kUp) return invalid("apse_coco_mask_targets: mask_size must be 28");
    if (n_obj < 0 || n_obj > APSE_COCO_MAX_POLY_OBJECTS || n_parts < 0 || n_parts > APSE_COCO_MAX_POLY_PARTS || n_verts < 0 ||
        n_verts > APSE_COCO_MAX_POLY_VERTS)
        return invalid("apse_coco_mask_targets: n_obj, n_parts or n_verts outside [0, APSE_COCO_MAX_POLY_OBJECTS / _PARTS / _VERTS]");
    if (n == 0) return APSE_OK;
    if (!rois || !matched || !targets || !info || (n_obj > 0 && !obj_part_off) || (n_parts > 0 && !part_vert_off) ||
        (n_verts > 0 && !xy))
        return invalid("apse_coco_mask_targets: null pointer");
    return apse_k_mask_targets(xy, part_vert_off, n_parts, obj_part_off, n_obj, n_verts, rois, matched, n, targets, info,
                               (hipStream_t)stream);
}

}  // extern "C"
