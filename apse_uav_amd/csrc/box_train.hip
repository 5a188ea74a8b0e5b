// Box-head training (include/apse_hip.h "Box-head training"): the f32 kernels behind fine-tuning roi_heads.box_head.fc1 / fc2 and
// roi_heads.box_predictor.cls_score / bbox_pred of a frozen FPN detector (FastRCNNConvFCHead with two 1024-wide FC layers on
// 7 x 7 x 256 RoI features, FastRCNNOutputLayers, FastRCNNOutputs.losses of detectron2 0.1.2).  DESIGN.md "Box-head training"
// gives the rules.
//
//   match         pairwise_iou + Matcher([0.5], [0, 1]) + the class assignment of _sample_proposals: one thread per proposal over
//                 ground truths staged in LDS, best IoU with ties to the lowest index.
//   permute       the pooled features [n][7][7][256] (h, w, c) -> [n][12544] in fc1's own (c, h, w) order, once per step: every
//                 GEMM below then reads and writes the checkpoint's layouts directly.
//   gemm          C[i][j] = sum_r A(i, r) B(r, j) on v_mfma_f32_32x32x2_f32, 128 x 128 tiles, 32 reduction steps per stage, LDS
//                 double buffer, either operand stored reduction-major ([r][i]) or reduction-minor ([i][r]).  Three uses:
//                   forward   Y  = X W^T + b (+ ReLU)        A = X  [m][k] minor,  B = W  [o][k] minor
//                   dgrad     dX = dY W (+= an earlier dX)   A = dY [m][o] minor,  B = W  [o][k] major
//                   wgrad     dW = dY^T X                    A = dY [m][o] major,  B = X  [m][k] major
//                 A tile owns its outputs over the whole reduction: the gradients need no split and write no partial tiles; only
//                 the forward of a layer 4096 inputs wide or more (fc1) runs as 8 chunks of the reduction that a second kernel
//                 adds in chunk order.  Rows and columns outside the shapes are masked at the loads (exact zeros), never read.
//                 The tile, its constants and the summation order (MFMA chains of 64 reduction steps that join a running
//                 total) are described once, in train_tile.h; mask_train.hip's two MFMA kernels follow the same rule.
//   bias          db = column sums in f64, rows in ascending order inside slices of 64, slices in ascending order.
//   loss          cross_entropy (mean over the n rows) + smooth_l1 on the four columns of the ground-truth class of the
//                 foreground rows (sum / n), the logged ratios, and both gradients.
// Determinism: no float atomics; every sum has a fixed order that depends on the shapes only.
#include "apse_kernels.h"
#include "train_tile.h"
#include "../../include/apse_hip.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kFeat = 7 * 7 * 256;      // fc1's input width
constexpr int kMaxO = 1024;             // widest layer output (FC_DIM)
constexpr int kMaxK = 16384;            // widest layer input the GEMM entries take
constexpr int kMaxGt = 4096;            // ground truths per image

int invalid(const char* msg) { return apse_fail_global(APSE_E_INVALID, msg); }
int launched() { return hipGetLastError() == hipSuccess ? APSE_OK : apse_fail_global(APSE_E_HIP, "box_train: kernel launch failed"); }
bool n_ok(int n) { return n >= 1 && n <= APSE_BOX_TRAIN_MAX_N; }
bool k_ok(int K) { return K >= 1 && K <= APSE_MAX_CLASSES; }

// ---------------------------------------------------------------------------------------------------------------- match
constexpr int kGtChunk = 1024;
__global__ __launch_bounds__(256) void box_match(const float* __restrict__ props, int N, const float* __restrict__ gts,
                                                 const int* __restrict__ gcls, int G, int K, float thr, int* __restrict__ midx,
                                                 float* __restrict__ miou, int* __restrict__ labels) {
    __shared__ f32x4 sg[kGtChunk];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    f32x4 p = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < N) p = *reinterpret_cast<const f32x4*>(props + (size_t)i * 4);
    const float area_p = (p[2] - p[0]) * (p[3] - p[1]);
    float best = 0.f;
    int bi = 0;
    for (int g0 = 0; g0 < G; g0 += kGtChunk) {
        const int cnt = min(kGtChunk, G - g0);
        for (int j = threadIdx.x; j < cnt; j += blockDim.x) sg[j] = *reinterpret_cast<const f32x4*>(gts + (size_t)(g0 + j) * 4);
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const f32x4 g = sg[j];
            // detectron2 pairwise_iou(gt_boxes, proposal_boxes): boxes1 = ground truths
            const float area_g = (g[2] - g[0]) * (g[3] - g[1]);
            float w = fminf(g[2], p[2]) - fmaxf(g[0], p[0]);
            float h = fminf(g[3], p[3]) - fmaxf(g[1], p[1]);
            w = w > 0.f ? w : 0.f;
            h = h > 0.f ? h : 0.f;
            const float inter = w * h;
            const float iou = inter > 0.f ? inter / (area_g + area_p - inter) : 0.f;
            if (iou > best) { best = iou; bi = g0 + j; }           // strict: ties keep the lowest index
        }
        __syncthreads();
    }
    if (i < N) {
        int lab = K;
        if (G > 0 && best >= thr) { const int c = gcls[bi]; lab = c < 0 ? 0 : (c > K ? K : c); }
        midx[i] = bi;
        miou[i] = best;
        labels[i] = lab;
    }
}

// ---------------------------------------------------------------------------------------------------------------- permute
// out[m][c * 49 + p] = in[m][p * 256 + c]: one block per RoI through LDS (row stride 257: the transposed read is conflict-free)
__global__ __launch_bounds__(256) void permute_hwc_chw(const float* __restrict__ in, float* __restrict__ out) {
    __shared__ float tile[49 * 257];
    const float* src = in + (size_t)blockIdx.x * kFeat;
    float* dst = out + (size_t)blockIdx.x * kFeat;
    for (int i = threadIdx.x; i < kFeat; i += 256) tile[(i >> 8) * 257 + (i & 255)] = src[i];
    __syncthreads();
    for (int i = threadIdx.x; i < kFeat; i += 256) { const int c = i / 49, p = i - c * 49; dst[i] = tile[p * 257 + c]; }
}

// ---------------------------------------------------------------------------------------------------------------- gemm
// The f32 MFMA takes A[i = lane & 31][k = lane >> 5] and B[k = lane >> 5][j = lane & 31] in one register each.  A reduction-major
// operand sits in LDS as train_tile.h lays it out ([32 k][160]); a reduction-minor one as [128 i][33] (consecutive i are 33 floats
// apart: conflict-free again).
constexpr int kLdMinor = 33;
constexpr int kOpFloats = kMajorFloats;                            // 5120 >= 128 * 33
constexpr int kGemmLds = 2 * 2 * kOpFloats * (int)sizeof(float);   // double buffer x (A, B)

// four floats row[col .. col + 3] of a row with `lim` valid columns (row == nullptr: none); vec: 16-byte aligned rows
__device__ __forceinline__ f32x4 ld_masked(const float* __restrict__ row, int col, int lim, bool vec) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!row) return v;
    if (vec && col + 3 < lim) return *reinterpret_cast<const f32x4*>(row + col);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (col + e < lim) v[e] = row[col + e];
    return v;
}

template <bool MINOR>
__device__ __forceinline__ void fetch_op(const float* __restrict__ M, int ld, int idx0, int lim, int r0, int R, bool vec, int t,
                                         f32x4 (&reg)[4]) {
    if (MINOR) {                                   // M[idx][r]: rows (t >> 3) + 32 i of the tile, float4 at r0 + 4 (t & 7)
        const int row = t >> 3, k4 = t & 7;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = idx0 + row + 32 * i;
            reg[i] = ld_masked(idx < lim ? M + (size_t)idx * ld : nullptr, r0 + 4 * k4, R, vec);
        }
    } else {                                       // M[r][idx]: reduction rows (t >> 5) + 8 i, float4 at idx0 + 4 (t & 31)
        const int row = t >> 5, c4 = t & 31;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + row + 8 * i;
            reg[i] = ld_masked(r < R ? M + (size_t)r * ld : nullptr, idx0 + 4 * c4, lim, vec);
        }
    }
}
template <bool MINOR>
__device__ __forceinline__ void stage_op(float* __restrict__ s, int t, const f32x4 (&reg)[4]) {
    if (MINOR) {
        const int row = t >> 3, k4 = t & 7;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) s[(row + 32 * i) * kLdMinor + 4 * k4 + e] = reg[i][e];
    } else {
        stage_major(s, t, reg);
    }
}
template <bool MINOR>
__device__ __forceinline__ float read_op(const float* __restrict__ s, int idx, int k) {
    return MINOR ? s[idx * kLdMinor + k] : read_major(s, idx, k);
}

// C[i][j] = (accumulate ? C[i][j] : 0) + relu?(bias[j] + sum_{r < R} A(i, r) B(r, j)), i < I, j < J.  With `part` the reduction is
// split over blockIdx.y into chunks of `spc` stages and chunk z writes its bare sums to part[z][i][j] (gemm_join finishes).
template <bool AMINOR, bool BMINOR>
__global__ __launch_bounds__(256, 2) void fc_gemm(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, int I,
                                               int J, int R, const float* __restrict__ bias, int relu, int accumulate,
                                               float* __restrict__ C, int ldc, int spc, float* __restrict__ part) {
    extern __shared__ __align__(16) float lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // XCD-aware order, i fastest: the tiles that read the same columns of B share an L2
    const int bid = apse_xcd_remap(blockIdx.x, gridDim.x);
    const int tiles_i = (I + 127) >> 7;
    const int i0 = (bid % tiles_i) * 128, j0 = (bid / tiles_i) * 128;
    const bool avec = !(lda & 3) && !(reinterpret_cast<uintptr_t>(A) & 15);
    const bool bvec = !(ldb & 3) && !(reinterpret_cast<uintptr_t>(B) & 15);
    const int step_lo = blockIdx.y * spc;
    const int nsteps = min(spc, (R + kKT - 1) / kKT - step_lo);

    f32x4 ra[4], rb[4];
    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; tot[i][j][e] = 0.f; }
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, l31 = lane & 31, kh2 = lane >> 5;

    fetch_op<AMINOR>(A, lda, i0, I, step_lo * kKT, R, avec, t, ra);
    fetch_op<BMINOR>(B, ldb, j0, J, step_lo * kKT, R, bvec, t, rb);
    stage_op<AMINOR>(lds, t, ra);
    stage_op<BMINOR>(lds + kOpFloats, t, rb);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (more) {                                              // global loads of the next stage fly under this stage's MFMAs
            fetch_op<AMINOR>(A, lda, i0, I, (step_lo + s + 1) * kKT, R, avec, t, ra);
            fetch_op<BMINOR>(B, ldb, j0, J, (step_lo + s + 1) * kKT, R, bvec, t, rb);
        }
        const float* as = lds + (s & 1) * (2 * kOpFloats);
        const float* bs = as + kOpFloats;
#pragma unroll
        for (int kk = 0; kk < kKT / 2; ++kk) {
            const int k = 2 * kk + kh2;
            const float a0 = read_op<AMINOR>(as, wm + l31, k), a1 = read_op<AMINOR>(as, wm + 32 + l31, k);
            const float b0 = read_op<BMINOR>(bs, wn + l31, k), b1 = read_op<BMINOR>(bs, wn + 32 + l31, k);
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
        if (more) {                         // the other buffer: its readers (stage s - 1) passed the barrier below one stage ago
            float* an = lds + ((s + 1) & 1) * (2 * kOpFloats);
            stage_op<AMINOR>(an, t, ra);
            stage_op<BMINOR>(an + kOpFloats, t, rb);
        }
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cj = j0 + wn + j * 32 + l31;
            if (cj >= J) continue;
            const float bv = bias ? bias[cj] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ci = i0 + wm + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh2;
                if (ci >= I) continue;
                if (part) { part[((size_t)blockIdx.y * I + ci) * J + cj] = tot[i][j][e]; continue; }
                float v = tot[i][j][e] + bv;
                if (relu) v = v > 0.f ? v : 0.f;
                float* dst = C + (size_t)ci * ldc + cj;
                if (accumulate) v = *dst + v;
                *dst = v;
            }
        }
}

// C[i][j] = relu?(bias[j] + the chunks' sums in chunk order)
__global__ void gemm_join(const float* __restrict__ part, int chunks, int I, int J, const float* __restrict__ bias, int relu,
                          float* __restrict__ C) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)I * J;
    if (e >= total) return;
    float v = part[e];
    for (int z = 1; z < chunks; ++z) v += part[(size_t)z * total + e];
    if (bias) v += bias[e % J];
    if (relu) v = v > 0.f ? v : 0.f;
    C[e] = v;
}

// the forward of a layer with a long reduction (fc1: 392 stages, 8 x 8 tiles at most) is split into kFwdChunks chunks; the rule
// reads the layer's width only, so a RoI's result does not depend on how many RoIs share the call
constexpr int kFwdSplitMinK = 4096, kFwdChunks = 8;
int fwd_chunks(int Kdim) { return Kdim >= kFwdSplitMinK ? kFwdChunks : 1; }

template <bool AMINOR, bool BMINOR>
int launch_gemm(const float* A, int lda, const float* B, int ldb, int I, int J, int R, const float* bias, int relu, int accumulate,
                float* C, int ldc, hipStream_t s, int chunks = 1, float* part = nullptr) {
    static bool attr_done = false;
    if (!attr_done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fc_gemm<AMINOR, BMINOR>), hipFuncAttributeMaxDynamicSharedMemorySize, kGemmLds);
        attr_done = true;
    }
    const int blocks = ((I + 127) / 128) * ((J + 127) / 128);
    const int steps = (R + kKT - 1) / kKT;
    int spc = steps;
    if (chunks > 1) {
        spc = apse_roundup((steps + chunks - 1) / chunks, kFlush);          // whole MFMA chains per chunk
        chunks = (steps + spc - 1) / spc;
    }
    hipLaunchKernelGGL((fc_gemm<AMINOR, BMINOR>), dim3(blocks, chunks), dim3(256), kGemmLds, s, A, lda, B, ldb, I, J, R, bias, relu,
                       accumulate, C, ldc, spc, chunks > 1 ? part : nullptr);
    if (chunks > 1) {
        const size_t total = (size_t)I * J;
        hipLaunchKernelGGL(gemm_join, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, chunks, I, J, bias, relu, C);
    }
    return launched();
}

bool fc_shape_ok(int n, int O, int Kdim) { return n_ok(n) && O >= 1 && O <= kMaxO && Kdim >= 1 && Kdim <= kMaxK; }

// ---------------------------------------------------------------------------------------------------------------- bias
constexpr int kBiasRows = 64;
// part[slice][c] = sum of g[row][c] over the slice's rows in ascending order; then db[c] = sum of the slices in ascending order.
// Both sums run in f64 (a column of 1024 f32 terms summed one after the other in f32 would carry ten times the error of torch's
// blocked sum); the result is rounded to f32 once.
__global__ void bias_slices(const float* __restrict__ g, int rows, int C, double* __restrict__ part) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int lo = blockIdx.x * kBiasRows, hi = min(lo + kBiasRows, rows);
    double v = 0.0;
    for (int r = lo; r < hi; ++r) v += (double)g[(size_t)r * C + c];
    part[(size_t)blockIdx.x * C + c] = v;
}
__global__ void bias_finish(const double* __restrict__ part, int slices, int C, float* __restrict__ db) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double v = part[c];
    for (int s = 1; s < slices; ++s) v += part[(size_t)s * C + c];
    db[c] = (float)v;
}

// ---------------------------------------------------------------------------------------------------------------- loss
struct Weights4 { float w[4]; };
__device__ __forceinline__ int row_label(const int* labels, int r, int K) {
    const int k = labels[r];
    return k < 0 ? 0 : (k > K ? K : k);               // never index outside the row; K = background
}
// Box2BoxTransform.get_deltas, column j, in f32 in detectron2's order
__device__ __forceinline__ float delta_target(const float* __restrict__ p, const float* __restrict__ g, const Weights4& wt, int j) {
    const int a = j & 1;                               // 0: x, 1: y
    const float ps = p[2 + a] - p[a], gs = g[2 + a] - g[a];
    if (j < 2) {
        const float pc = p[a] + 0.5f * ps, gc = g[a] + 0.5f * gs;
        return wt.w[j] * (gc - pc) / ps;
    }
    return wt.w[j] * logf(gs / ps);
}
constexpr int kLossCols = 6;
// One thread per row: part[r] = {cross-entropy term, smooth-L1 term, argmax == label, foreground, foreground and argmax == label,
// foreground and argmax == background}.  The log-sum-exp runs in f64 on f32 logits with the row maximum subtracted.
__global__ void loss_rows(const float* __restrict__ logits, const float* __restrict__ deltas, const int* __restrict__ labels,
                          const float* __restrict__ props, const float* __restrict__ gts, int n, int K, Weights4 wt, float beta,
                          double* __restrict__ part) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int lab = row_label(labels, r, K);
    const float* x = logits + (size_t)r * (K + 1);
    float mx = x[0];
    int am = 0;
    for (int c = 1; c <= K; ++c)
        if (x[c] > mx) { mx = x[c]; am = c; }          // strict: ties keep the lowest index
    double se = 0.0;
    for (int c = 0; c <= K; ++c) se += exp((double)x[c] - (double)mx);
    const double ce = log(se) + ((double)mx - (double)x[lab]);
    const bool fg = lab < K;
    double box = 0.0;
    if (fg) {
        for (int j = 0; j < 4; ++j) {
            const float tv = delta_target(props + (size_t)r * 4, gts + (size_t)r * 4, wt, j);
            const float a = fabsf(deltas[(size_t)r * 4 * K + 4 * lab + j] - tv);
            float term = a;
            if (beta >= 1e-5f) term = a < beta ? 0.5f * (a * a) / beta : a - 0.5f * beta;
            box += (double)term;
        }
    }
    double* o = part + (size_t)r * kLossCols;
    o[0] = ce; o[1] = box; o[2] = am == lab; o[3] = fg; o[4] = fg && am == lab; o[5] = fg && am == K;
}
// out8 = {loss_cls, loss_box_reg, cls_accuracy, fg_cls_accuracy, false_negative, num_fg, num_bg, 0}
__global__ __launch_bounds__(256) void loss_finish(const double* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double tot[kLossCols];
    for (int j = 0; j < kLossCols; ++j) {
        double v = 0.0;
        for (int r = t; r < n; r += 256) v += part[(size_t)r * kLossCols + j];
        tot[j] = block_sum_d(v, red);
    }
    if (t == 0) {
        const double nn = (double)n, nfg = tot[3];
        out[0] = (float)(tot[0] / nn);
        out[1] = (float)(tot[1] / nn);
        out[2] = (float)(tot[2] / nn);
        out[3] = nfg > 0.0 ? (float)(tot[4] / nfg) : 0.f;
        out[4] = nfg > 0.0 ? (float)(tot[5] / nfg) : 0.f;
        out[5] = (float)nfg;
        out[6] = (float)(nn - nfg);
        out[7] = 0.f;
    }
}
// dlogits[r][c] = (softmax(x[r])[c] - (c == label)) / n * g_cls
__global__ void loss_grad_cls(const float* __restrict__ logits, const int* __restrict__ labels, int n, int K,
                              const float* __restrict__ g_cls, float* __restrict__ dlogits) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int lab = row_label(labels, r, K);
    const float* x = logits + (size_t)r * (K + 1);
    float mx = x[0];
    for (int c = 1; c <= K; ++c) mx = x[c] > mx ? x[c] : mx;
    double se = 0.0;
    for (int c = 0; c <= K; ++c) se += exp((double)x[c] - (double)mx);
    const double scale = (double)(g_cls ? g_cls[0] : 1.f) / (double)n;
    for (int c = 0; c <= K; ++c) {
        const double p = exp((double)x[c] - (double)mx) / se;
        dlogits[(size_t)r * (K + 1) + c] = (float)((p - (c == lab ? 1.0 : 0.0)) * scale);
    }
}
// ddeltas[r][col] = d smooth_l1 / n * g_box on the four columns of a foreground row's class, exactly 0 elsewhere
__global__ void loss_grad_box(const float* __restrict__ deltas, const int* __restrict__ labels, const float* __restrict__ props,
                              const float* __restrict__ gts, int n, int K, Weights4 wt, float beta, const float* __restrict__ g_box,
                              float* __restrict__ ddeltas) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * 4 * K) return;
    const int r = (int)(i / (4 * K)), col = (int)(i - (size_t)r * 4 * K);
    const int lab = row_label(labels, r, K);
    float v = 0.f;
    if (lab < K && (col >> 2) == lab) {
        const float d = deltas[i] - delta_target(props + (size_t)r * 4, gts + (size_t)r * 4, wt, col & 3);
        float gr = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        if (beta >= 1e-5f && fabsf(d) < beta) gr = d / beta;
        v = gr / (float)n * (g_box ? g_box[0] : 1.f);
    }
    ddeltas[i] = v;
}

}  // namespace

extern "C" {

size_t apse_box_train_workspace_bytes(int n, int K) {
    if (!n_ok(n) || !k_ok(K)) return 0;
    const size_t slices = (size_t)(n + kBiasRows - 1) / kBiasRows;
    const size_t bias = slices * kMaxO * sizeof(double), loss = (size_t)n * kLossCols * sizeof(double);
    const size_t fwd = (size_t)kFwdChunks * n * kMaxO * sizeof(float);       // fc1's forward chunks
    const size_t need = bias > loss ? bias : loss;
    return fwd > need ? fwd : need;
}

int apse_box_match(const float* proposals, int N, const float* gt_boxes, const int* gt_classes, int G, int K, float iou_thresh,
                   int* matched_idx, float* matched_iou, int* labels, void* stream) {
    if (N == 0) return APSE_OK;
    if (N < 0 || N > (1 << 20)) return invalid("apse_box_match: needs 0 <= N <= 2^20 proposals");
    if (G < 0 || G > kMaxGt) return invalid("apse_box_match: needs 0 <= G <= 4096 ground truths");
    if (!k_ok(K)) return invalid("apse_box_match: needs 1 <= K <= APSE_MAX_CLASSES (80)");
    if (!proposals || !matched_idx || !matched_iou || !labels || (G > 0 && (!gt_boxes || !gt_classes)))
        return invalid("apse_box_match: null pointer");
    hipLaunchKernelGGL(box_match, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, proposals, N, gt_boxes, gt_classes, G, K,
                       iou_thresh, matched_idx, matched_iou, labels);
    return launched();
}

int apse_box_permute_features(const float* x, int n, float* out, void* stream) {
    if (!n_ok(n)) return invalid("apse_box_permute_features: needs 1 <= n <= APSE_BOX_TRAIN_MAX_N (1024) RoIs");
    if (!x || !out || x == out) return invalid("apse_box_permute_features: null pointer or in place");
    hipLaunchKernelGGL(permute_hwc_chw, dim3(n), dim3(256), 0, (hipStream_t)stream, x, out);
    return launched();
}

int apse_box_fc_forward(const float* x, const float* w, const float* bias, int n, int O, int Kdim, int relu, float* y, float* ws,
                        size_t ws_bytes, void* stream) {
    if (!fc_shape_ok(n, O, Kdim)) return invalid("apse_box_fc_forward: needs 1 <= n <= APSE_BOX_TRAIN_MAX_N (1024), 1 <= O <= 1024, 1 <= K <= 16384");
    if (!x || !w || !y) return invalid("apse_box_fc_forward: null pointer");
    const int chunks = fwd_chunks(Kdim);
    if (chunks > 1 && (!ws || ws_bytes < (size_t)chunks * n * O * sizeof(float))) return invalid("apse_box_fc_forward: workspace too small");
    return launch_gemm<true, true>(x, Kdim, w, Kdim, n, O, Kdim, bias, relu, 0, y, O, (hipStream_t)stream, chunks, ws);
}

int apse_box_fc_dgrad(const float* dy, const float* w, int n, int O, int Kdim, int accumulate, float* dx, void* stream) {
    if (!fc_shape_ok(n, O, Kdim)) return invalid("apse_box_fc_dgrad: needs 1 <= n <= APSE_BOX_TRAIN_MAX_N (1024), 1 <= O <= 1024, 1 <= K <= 16384");
    if (!dy || !w || !dx) return invalid("apse_box_fc_dgrad: null pointer");
    return launch_gemm<true, false>(dy, O, w, Kdim, n, Kdim, O, nullptr, 0, accumulate != 0, dx, Kdim, (hipStream_t)stream);
}

int apse_box_fc_wgrad(const float* dy, const float* x, int n, int O, int Kdim, float* dw, void* stream) {
    if (!fc_shape_ok(n, O, Kdim)) return invalid("apse_box_fc_wgrad: needs 1 <= n <= APSE_BOX_TRAIN_MAX_N (1024), 1 <= O <= 1024, 1 <= K <= 16384");
    if (!dy || !x || !dw) return invalid("apse_box_fc_wgrad: null pointer");
    return launch_gemm<false, false>(dy, O, x, Kdim, O, Kdim, n, nullptr, 0, 0, dw, Kdim, (hipStream_t)stream);
}

int apse_box_bias_grad(const float* dy, int n, int O, float* db, void* ws, size_t ws_bytes, void* stream) {
    if (!n_ok(n) || O < 1 || O > kMaxO) return invalid("apse_box_bias_grad: needs 1 <= n <= APSE_BOX_TRAIN_MAX_N (1024) and 1 <= O <= 1024");
    if (!dy || !db || !ws) return invalid("apse_box_bias_grad: null pointer");
    const int slices = (n + kBiasRows - 1) / kBiasRows;
    if (ws_bytes < (size_t)slices * O * sizeof(double)) return invalid("apse_box_bias_grad: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bias_slices, dim3(slices, (O + 255) / 256), dim3(256), 0, s, dy, n, O, (double*)ws);
    hipLaunchKernelGGL(bias_finish, dim3((O + 255) / 256), dim3(256), 0, s, (const double*)ws, slices, O, db);
    return launched();
}

int apse_box_loss_forward(const float* logits, const float* deltas, const int* labels, const float* prop_boxes, const float* gt_boxes,
                          int n, int K, const float* weights4, float smooth_l1_beta, float* out8, void* ws, size_t ws_bytes,
                          void* stream) {
    if (n == 0) return APSE_OK;
    if (!n_ok(n) || !k_ok(K)) return invalid("apse_box_loss_forward: needs 0 <= n <= APSE_BOX_TRAIN_MAX_N (1024) and 1 <= K <= APSE_MAX_CLASSES (80)");
    if (!logits || !deltas || !labels || !prop_boxes || !gt_boxes || !weights4 || !out8 || !ws) return invalid("apse_box_loss_forward: null pointer");
    if (!(smooth_l1_beta >= 0.f)) return invalid("apse_box_loss_forward: smooth_l1_beta must be >= 0");
    if (ws_bytes < (size_t)n * kLossCols * sizeof(double)) return invalid("apse_box_loss_forward: workspace too small");
    Weights4 wt;
    for (int j = 0; j < 4; ++j) wt.w[j] = weights4[j];
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_rows, dim3((n + 63) / 64), dim3(64), 0, s, logits, deltas, labels, prop_boxes, gt_boxes, n, K, wt,
                       smooth_l1_beta, (double*)ws);
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(256), 0, s, (const double*)ws, n, out8);
    return launched();
}

int apse_box_loss_backward(const float* logits, const float* deltas, const int* labels, const float* prop_boxes, const float* gt_boxes,
                           int n, int K, const float* weights4, float smooth_l1_beta, const float* grad_cls, const float* grad_box,
                           float* dlogits, float* ddeltas, void* stream) {
    if (n == 0) return APSE_OK;
    if (!n_ok(n) || !k_ok(K)) return invalid("apse_box_loss_backward: needs 0 <= n <= APSE_BOX_TRAIN_MAX_N (1024) and 1 <= K <= APSE_MAX_CLASSES (80)");
    if (!logits || !deltas || !labels || !prop_boxes || !gt_boxes || !weights4 || !dlogits || !ddeltas) return invalid("apse_box_loss_backward: null pointer");
    if (!(smooth_l1_beta >= 0.f)) return invalid("apse_box_loss_backward: smooth_l1_beta must be >= 0");
    Weights4 wt;
    for (int j = 0; j < 4; ++j) wt.w[j] = weights4[j];
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_grad_cls, dim3((n + 63) / 64), dim3(64), 0, s, logits, labels, n, K, grad_cls, dlogits);
    const size_t total = (size_t)n * 4 * K;
    hipLaunchKernelGGL(loss_grad_box, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, deltas, labels, prop_boxes, gt_boxes, n, K,
                       wt, smooth_l1_beta, grad_box, ddeltas);
    return launched();
}

}  // extern "C"
