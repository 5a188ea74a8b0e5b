// Association-head training (include/apse_hip.h "Association-head training"): the f32 kernels behind
// dcnn/scripts/train/train_association_head.py -- the head's fc layer with F.normalize (dcnn/networks/association_head.py:16-31),
// forward and backward, the two online triplet losses of dcnn/online_triplet_loss/losses.py with their gradients, and the
// momentum SGD step of torch.optim.SGD.  DESIGN.md "Association-head training" gives the rules.
//
//   fc forward    split-R tile GEMM Z_s = X[:, chunk_s] W[:, chunk_s]^T (64 x 64 tiles, 4 x 4 per thread, VALU FMA) into
//                 workspace partials, then one block per row: Z = b + sum_s Z_s in s order, the row norm, E = Z / max(|Z|, eps)
//   fc backward   one block per row: dZ = (dE - E (E.dE)) / max(|Z|, eps); db = sum_i dZ (i order); dW = dZ^T X (same tile GEMM)
//   triplet       squared norms, the Gram-form distance matrix (losses.py:7-40), one block per anchor for the hardest
//                 positive / negative (batch-hard) or the O(n^2) triplet scan (batch-all), one block for the final reduction;
//                 the backward pass turns the per-row distance coefficients into dE with one block per anchor
//   sgd           one thread per element
// Determinism: no float atomics anywhere; every sum runs in a fixed order (sequential loops and fixed-shape LDS trees) and
// every max / min breaks ties by the lowest index, so two runs of a step give bit-identical results.
#include "apse_common.h"
#include "../../include/apse_hip.h"
#include <math.h>

namespace {

constexpr int kTM = 64, kTN = 64, kTR = 16;     // tile GEMM: 64 x 64 outputs, 16-deep reduction slices, 256 threads
constexpr int kRowThreads = 256;                 // per-row kernels (D <= 256)
constexpr float kNormEps = 1e-12f;               // F.normalize eps

__device__ __forceinline__ float block_sum(float v, float* red) {   // fixed-shape tree over 256 threads
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = kRowThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// C[m][n] = sum_{r in chunk z} A(m, r) B(n, r).  A(m, r) = A[m * lda + r] when A_RC (r contiguous), A[r * lda + m] otherwise;
// B likewise.  Chunk z covers r in [z * rchunk, min(R, (z + 1) * rchunk)) and writes C + z * M * N.  Each output is one fmaf
// chain in ascending r.
template <bool A_RC, bool B_RC>
__global__ void __launch_bounds__(256) tile_gemm(const float* __restrict__ A, const float* __restrict__ B, int M, int N, int R,
                                                 int rchunk, long lda, long ldb, float* __restrict__ C) {
    __shared__ __align__(16) float As[kTR][kTM + 4];
    __shared__ __align__(16) float Bs[kTR][kTN + 4];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int m0 = blockIdx.y * kTM, n0 = blockIdx.x * kTN;
    const int r_lo = blockIdx.z * rchunk, r_hi = min(R, r_lo + rchunk);
    float acc[4][4] = {};
    for (int r0 = r_lo; r0 < r_hi; r0 += kTR) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int m, r;
            if (A_RC) { m = t >> 2; r = (t & 3) * 4 + q; } else { m = t & 63; r = (t >> 6) + 4 * q; }
            const int gm = m0 + m, gr = r0 + r;
            float v = 0.f;
            if (gm < M && gr < r_hi) v = A_RC ? A[(size_t)gm * lda + gr] : A[(size_t)gr * lda + gm];
            As[r][m] = v;
            int n, rb;
            if (B_RC) { n = t >> 2; rb = (t & 3) * 4 + q; } else { n = t & 63; rb = (t >> 6) + 4 * q; }
            const int gn = n0 + n, gr2 = r0 + rb;
            float w = 0.f;
            if (gn < N && gr2 < r_hi) w = B_RC ? B[(size_t)gn * ldb + gr2] : B[(size_t)gr2 * ldb + gn];
            Bs[rb][n] = w;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kTR; ++r) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&As[r][ty * 4]);
            const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[r][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
    float* out = C + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty * 4 + i;
        if (gm >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx * 4 + j;
            if (gn < N) out[(size_t)gm * N + gn] = acc[i][j];
        }
    }
}

// one block per row i: Z = b + sum_s P[s][i] (s ascending), E = Z / max(|Z|, eps)    (association_head.py:29-30)
__global__ void __launch_bounds__(kRowThreads) fc_finish(const float* __restrict__ P, int S, const float* __restrict__ b, int n,
                                                         int D, float* __restrict__ E, float* __restrict__ inv_norm) {
    __shared__ float red[kRowThreads];
    const int i = blockIdx.x, d = threadIdx.x;
    float z = 0.f;
    if (d < D) {
        for (int s = 0; s < S; ++s) z = z + P[((size_t)s * n + i) * D + d];
        z = z + b[d];
    }
    const float ss = block_sum(d < D ? z * z : 0.f, red);
    const float den = fmaxf(sqrtf(ss), kNormEps);
    if (d < D) E[(size_t)i * D + d] = z / den;
    if (d == 0) inv_norm[i] = 1.0f / den;
}

// one block per row: dZ = (dE - E (E . dE)) * inv_norm    (backward of F.normalize above its eps)
__global__ void __launch_bounds__(kRowThreads) fc_dz(const float* __restrict__ E, const float* __restrict__ dE,
                                                     const float* __restrict__ inv_norm, int D, float* __restrict__ dZ) {
    __shared__ float red[kRowThreads];
    const int i = blockIdx.x, d = threadIdx.x;
    const size_t o = (size_t)i * D + d;
    const float e = d < D ? E[o] : 0.f, g = d < D ? dE[o] : 0.f;
    const float dot = block_sum(e * g, red);
    if (d < D) dZ[o] = (g - e * dot) * inv_norm[i];
}

// db[d] = sum_i dZ[i][d], i ascending
__global__ void __launch_bounds__(kRowThreads) fc_db(const float* __restrict__ dZ, int n, int D, float* __restrict__ db) {
    const int d = blockIdx.x * kRowThreads + threadIdx.x;
    if (d >= D) return;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s = s + dZ[(size_t)i * D + d];
    db[d] = s;
}

// ---------------------------------------------------------------- triplet losses
struct TripletWs {          // workspace layout (byte offsets from the base)
    size_t d0, gd, sq, part, pos, val, scal, total;
};

__host__ __device__ inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

__host__ __device__ inline TripletWs triplet_layout(int n) {
    TripletWs w;
    const size_t nn = (size_t)n * n;
    w.d0 = 0;                                        // raw Gram-form distances [n][n] (before the clamp)
    w.gd = align256(w.d0 + nn * 4);                  // coefficient of the loss in each distance [n][n] (before the sqrt)
    w.sq = align256(w.gd + nn * 4);                  // squared norms [n]
    w.part = align256(w.sq + (size_t)n * 4);         // per-anchor hinged loss (hard) or partial sum (all) [n]
    w.pos = align256(w.part + (size_t)n * 4);        // per-anchor positive-triplet counts [n] (u64, batch-all)
    w.val = align256(w.pos + (size_t)n * 8);         // per-anchor valid-triplet counts [n] (u64, batch-all)
    w.scal = align256(w.val + (size_t)n * 8);        // [0] = the divisor of the loss (n, or P + 1e-16 as f32)
    w.total = align256(w.scal + 16);
    return w;
}

__device__ __forceinline__ float dot_rows(const float* a, const float* b, int D) {   // one fmaf chain, ascending d
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(a[d], b[d], s);
    return s;
}

// _pairwise_distances output from the raw Gram form d0 (losses.py:33-40): the clamp at 0, then for squared=False the eq(0)
// mask, + mask * 1e-16 and (1 - mask) * sqrt
__device__ __forceinline__ float dist_of(float d0, int squared) {
    const float d = d0 < 0.f ? 0.f : d0;
    if (squared) return d;
    const float m = d == 0.f ? 1.f : 0.f;
    return (1.0f - m) * sqrtf(d + m * 1e-16f);
}

// d dist / d d0 applied to a coefficient g: 0 where the clamp fired; for squared=False also 0 where the distance is 0
// ((1 - mask) * sqrt), else g / (2 sqrt(d0)) (torch's sqrt backward)
__device__ __forceinline__ float chain_dist(float g, float d0, int squared) {
    if (d0 < 0.f) return 0.f;
    if (squared) return g;
    return d0 == 0.f ? 0.f : g / (2.0f * sqrtf(d0));
}

__global__ void __launch_bounds__(256) tri_sqnorm(const float* __restrict__ E, int n, int D, float* __restrict__ sq) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) sq[i] = dot_rows(E + (size_t)i * D, E + (size_t)i * D, D);
}

// d0[i][j] = (sq[j] - 2 G[i][j]) + sq[i], the expression order of losses.py:27; G[i][j] and sq use the same fmaf chain, so
// the diagonal is exactly 0 and equal rows give exactly 0
__global__ void __launch_bounds__(256) tri_dist(const float* __restrict__ E, const float* __restrict__ sq, int n, int D,
                                                float* __restrict__ d0) {
    __shared__ float Ei[16][APSE_ASSOC_MAX_D + 1], Ej[16][APSE_ASSOC_MAX_D + 1];
    const int t = threadIdx.x, i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    for (int k = t; k < 16 * D; k += 256) {
        const int r = k / D, c = k - r * D;
        Ei[r][c] = i0 + r < n ? E[(size_t)(i0 + r) * D + c] : 0.f;
        Ej[r][c] = j0 + r < n ? E[(size_t)(j0 + r) * D + c] : 0.f;
    }
    __syncthreads();
    const int i = i0 + (t >> 4), j = j0 + (t & 15);
    if (i >= n || j >= n) return;
    const float g = dot_rows(Ei[t >> 4], Ej[t & 15], D);
    d0[(size_t)i * n + j] = (sq[j] - 2.0f * g) + sq[i];
}

struct ArgBest { float v; int i; };

// batch_hard_triplet_loss (losses.py:102-146), one block per anchor a.  hardest positive = max_j mask_ap * d (losses.py:125),
// rowmax = max_j d (:133), hardest negative = min_j d + rowmax (1 - mask_an) (:134-137); ties -> lowest j.  part[a] = the hinged
// tl (:140-141); gd row a = the coefficients of tl in d[a][j] when tl is not clipped (tl >= 0: `tl[tl < 0] = 0` is strict):
// +mask_ap at the hardest positive, -1 at the hardest negative, -(1 - mask_an) at the row maximum.
__global__ void __launch_bounds__(256) tri_hard_rows(const double* __restrict__ labels, const float* __restrict__ d0, int n,
                                                     float margin, int squared, float* __restrict__ gd, float* __restrict__ part) {
    __shared__ ArgBest red[256];
    __shared__ float s_rowmax;
    const int a = blockIdx.x, t = threadIdx.x;
    const double la = labels[a];
    const float* row = d0 + (size_t)a * n;
    // pass 1: rowmax and the hardest positive
    ArgBest mx{-INFINITY, n}, hp{-INFINITY, n};
    for (int j = t; j < n; j += 256) {
        const float d = dist_of(row[j], squared);
        const float map = (labels[j] == la && j != a) ? 1.f : 0.f;
        const float ap = map * d;
        if (d > mx.v) mx = {d, j};          // strided ascending j per thread: the first max wins within a thread
        if (ap > hp.v) hp = {ap, j};
    }
    auto reduce = [&](ArgBest v, bool want_max) {
        red[t] = v;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) {
                const ArgBest o = red[t + s], c = red[t];
                const bool take = want_max ? (o.v > c.v || (o.v == c.v && o.i < c.i)) : (o.v < c.v || (o.v == c.v && o.i < c.i));
                if (take) red[t] = o;
            }
            __syncthreads();
        }
        const ArgBest r = red[0];
        __syncthreads();
        return r;
    };
    const ArgBest rmax = reduce(mx, true);
    const ArgBest rpos = reduce(hp, true);
    if (t == 0) s_rowmax = rmax.v;
    __syncthreads();
    const float rowmax = s_rowmax;
    // pass 2: the hardest negative
    ArgBest hn{INFINITY, n};
    for (int j = t; j < n; j += 256) {
        const float d = dist_of(row[j], squared);
        const float man = labels[j] != la ? 1.f : 0.f;
        const float an = d + rowmax * (1.0f - man);
        if (an < hn.v) hn = {an, j};
    }
    const ArgBest rneg = reduce(hn, false);
    // min(.., n - 1): only a NaN row leaves an index at its initial n
    const int jp = min(rpos.i, n - 1), jn = min(rneg.i, n - 1), jm = min(rmax.i, n - 1);
    const float tl = (rpos.v - rneg.v) + margin;
    const bool active = !(tl < 0.f);
    const float cp = active ? ((labels[jp] == la && jp != a) ? 1.f : 0.f) : 0.f;
    const float cn = active ? -1.f : 0.f;
    const float cm = active ? -(1.0f - (labels[jn] != la ? 1.f : 0.f)) : 0.f;
    for (int j = t; j < n; j += 256) {
        float g = 0.f;
        if (j == jp) g = g + cp;
        if (j == jn) g = g + cn;
        if (j == jm) g = g + cm;
        gd[(size_t)a * n + j] = g;
    }
    if (t == 0) part[a] = active ? tl : 0.f;
}

// batch_all_triplet_loss (losses.py:149-197), one block per anchor a.  Valid triplets (a, p, k): p != a, label p == label a,
// label k != label a (_get_triplet_mask, losses.py:43-67).  tl = (d[a][p] - d[a][k]) + margin.  part[a] = sum of the hinged tl
// (fixed order), pos[a] = #(tl > 1e-16), val[a] = #valid; gd row a: +#{k : tl >= 0} at each p, -#{p : tl >= 0} at each k.
__global__ void __launch_bounds__(256) tri_all_rows(const double* __restrict__ labels, const float* __restrict__ d0, int n,
                                                    float margin, int squared, float* __restrict__ gd, float* __restrict__ part,
                                                    unsigned long long* __restrict__ pos, unsigned long long* __restrict__ val) {
    __shared__ float drow[APSE_ASSOC_MAX_N];
    __shared__ unsigned char same[APSE_ASSOC_MAX_N];
    __shared__ float red[256];
    __shared__ unsigned long long redu[256];
    const int a = blockIdx.x, t = threadIdx.x;
    const double la = labels[a];
    for (int j = t; j < n; j += 256) {
        drow[j] = dist_of(d0[(size_t)a * n + j], squared);
        same[j] = labels[j] == la ? 1 : 0;
    }
    __syncthreads();
    float sum = 0.f;
    unsigned long long np = 0, nv = 0;
    for (int j = t; j < n; j += 256) {
        float g = 0.f;
        if (same[j] && j != a) {                     // j as the positive
            int c = 0;
            for (int k = 0; k < n; ++k) {
                if (same[k]) continue;
                const float tl = (drow[j] - drow[k]) + margin;
                ++nv;
                if (!(tl < 0.f)) { ++c; sum = sum + tl; }
                if (tl > 1e-16f) ++np;
            }
            g = (float)c;
        } else if (!same[j]) {                       // j as the negative
            int c = 0;
            for (int p = 0; p < n; ++p) {
                if (!same[p] || p == a) continue;
                const float tl = (drow[p] - drow[j]) + margin;
                if (!(tl < 0.f)) ++c;
            }
            g = -(float)c;
        }
        gd[(size_t)a * n + j] = g;
    }
    red[t] = sum; redu[t] = np;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { red[t] = red[t] + red[t + s]; redu[t] += redu[t + s]; }
        __syncthreads();
    }
    if (t == 0) { part[a] = red[0]; pos[a] = redu[0]; }
    __syncthreads();
    redu[t] = nv;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) redu[t] += redu[t + s];
        __syncthreads();
    }
    if (t == 0) val[a] = redu[0];
}

// one block: the anchors' parts in a fixed tree.  all == 0: loss = mean of the hinged tl (losses.py:142), divisor n.
// all == 1: loss = sum / (P + 1e-16), fraction = P / (V + 1e-16) (losses.py:186-194), divisor P + 1e-16 (f32).
__global__ void __launch_bounds__(1024) tri_finish(const float* __restrict__ part, const unsigned long long* __restrict__ pos,
                                                   const unsigned long long* __restrict__ val, int n, int all,
                                                   float* __restrict__ out, float* __restrict__ scal) {
    __shared__ float red[1024];
    __shared__ unsigned long long rp[1024], rv[1024];
    const int t = threadIdx.x;
    float s = 0.f;
    unsigned long long p = 0, v = 0;
    for (int i = t; i < n; i += 1024) {
        s = s + part[i];
        if (all) { p += pos[i]; v += val[i]; }
    }
    red[t] = s; rp[t] = p; rv[t] = v;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) { red[t] = red[t] + red[t + w]; rp[t] += rp[t + w]; rv[t] += rv[t + w]; }
        __syncthreads();
    }
    if (t != 0) return;
    if (!all) {
        const float div = (float)n;
        out[0] = red[0] / div;
        scal[0] = div;
    } else {
        const float div = (float)((double)rp[0] + 1e-16);
        out[0] = red[0] / div;
        out[1] = (float)rp[0] / ((float)rv[0] + 1e-16f);
        scal[0] = div;
    }
}

// dE[a] = (grad / divisor) * 2 sum_j w[a][j] (E[a] - E[j]),  w[a][j] = c(d0[a][j]) gd[a][j] + c(d0[j][a]) gd[j][a]:
// the backward of d0[i][j] = |E_j|^2 - 2 E_i.E_j + |E_i|^2 through both index positions; j ascending.
__global__ void __launch_bounds__(kRowThreads) tri_grad(const float* __restrict__ E, const float* __restrict__ d0,
                                                        const float* __restrict__ gd, const float* __restrict__ scal,
                                                        const float* __restrict__ grad, int n, int D, int squared,
                                                        float* __restrict__ dE) {
    const int a = blockIdx.x, d = threadIdx.x;
    const float ea = d < D ? E[(size_t)a * D + d] : 0.f;
    float acc = 0.f;
    for (int j = 0; j < n; ++j) {
        const float w = chain_dist(gd[(size_t)a * n + j], d0[(size_t)a * n + j], squared) +
                        chain_dist(gd[(size_t)j * n + a], d0[(size_t)j * n + a], squared);
        if (w != 0.f && d < D) acc = fmaf(w, ea - E[(size_t)j * D + d], acc);
    }
    const float g = (grad ? grad[0] : 1.0f) / scal[0];
    if (d < D) dE[(size_t)a * D + d] = (2.0f * acc) * g;
}

// torch.optim.SGD (torch/optim/sgd.py, _single_tensor_sgd): weight decay, momentum buffer (buf = grad on the first step,
// else momentum * buf + (1 - dampening) * grad), nesterov, p += -lr * step
__global__ void __launch_bounds__(256) sgd_step(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                long long n, float lr, float momentum, float dampening, float wd, int nesterov,
                                                int first) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float d = g[i];
    const float pv = p[i];
    if (wd != 0.f) d = d + wd * pv;
    if (momentum != 0.f) {
        const float b = first ? d : buf[i] * momentum + (1.0f - dampening) * d;
        buf[i] = b;
        d = nesterov ? d + momentum * b : b;
    }
    p[i] = pv + (-lr) * d;
}

int fc_splits(int n, int K, int D, int* rchunk) {
    const int tiles = ((n + kTM - 1) / kTM) * ((D + kTN - 1) / kTN);
    int s = (1024 + tiles - 1) / tiles;
    s = min(s, (K + 255) / 256);
    s = max(s, 1);
    int rc = (K + s - 1) / s;
    rc = (rc + kTR - 1) / kTR * kTR;
    if (rchunk) *rchunk = rc;
    return (K + rc - 1) / rc;
}

bool fc_shape_ok(int n, int K, int D) {
    return n >= 1 && n <= APSE_ASSOC_MAX_N && D >= 1 && D <= APSE_ASSOC_MAX_D && K >= 1 && K <= APSE_ASSOC_MAX_K;
}

int invalid(const char* msg) { return apse_fail_global(APSE_E_INVALID, msg); }

int launched() {
    return hipGetLastError() == hipSuccess ? APSE_OK : apse_fail_global(APSE_E_HIP, "association training kernel launch failed");
}

}  // namespace

extern "C" {

size_t apse_assoc_fc_workspace_bytes(int n, int K, int D) {
    if (!fc_shape_ok(n, K, D)) return 0;
    const size_t fwd = (size_t)fc_splits(n, K, D, nullptr) * n * D * 4;
    const size_t bwd = (size_t)n * D * 4;
    return fwd > bwd ? fwd : bwd;
}

int apse_assoc_fc_forward(const float* x, const float* w, const float* b, int n, int K, int D, float* e, float* inv_norm,
                          float* ws, size_t ws_bytes, void* stream) {
    if (!fc_shape_ok(n, K, D)) return invalid("apse_assoc_fc_forward: needs 1 <= n <= 2048, 1 <= D <= 256, 1 <= K <= 262144");
    if (!x || !w || !b || !e || !inv_norm || !ws) return invalid("apse_assoc_fc_forward: null pointer");
    if (ws_bytes < apse_assoc_fc_workspace_bytes(n, K, D)) return invalid("apse_assoc_fc_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int rc = 0;
    const int S = fc_splits(n, K, D, &rc);
    const dim3 grid((D + kTN - 1) / kTN, (n + kTM - 1) / kTM, S);
    hipLaunchKernelGGL((tile_gemm<true, true>), grid, dim3(256), 0, s, x, w, n, D, K, rc, (long)K, (long)K, ws);
    hipLaunchKernelGGL(fc_finish, dim3(n), dim3(kRowThreads), 0, s, ws, S, b, n, D, e, inv_norm);
    return launched();
}

int apse_assoc_fc_backward(const float* x, const float* e, const float* inv_norm, const float* de, int n, int K, int D, float* dw,
                           float* db, float* ws, size_t ws_bytes, void* stream) {
    if (!fc_shape_ok(n, K, D)) return invalid("apse_assoc_fc_backward: needs 1 <= n <= 2048, 1 <= D <= 256, 1 <= K <= 262144");
    if (!x || !e || !inv_norm || !de || !dw || !db || !ws) return invalid("apse_assoc_fc_backward: null pointer");
    if (ws_bytes < apse_assoc_fc_workspace_bytes(n, K, D)) return invalid("apse_assoc_fc_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fc_dz, dim3(n), dim3(kRowThreads), 0, s, e, de, inv_norm, D, ws);
    hipLaunchKernelGGL(fc_db, dim3((D + kRowThreads - 1) / kRowThreads), dim3(kRowThreads), 0, s, ws, n, D, db);
    // dW[d][k] = sum_i dZ[i][d] X[i][k]: M = D, N = K, R = n, both operands contiguous along their output index
    const dim3 grid((K + kTN - 1) / kTN, (D + kTM - 1) / kTM, 1);
    hipLaunchKernelGGL((tile_gemm<false, false>), grid, dim3(256), 0, s, ws, x, D, K, n, n, (long)D, (long)K, dw);
    return launched();
}

size_t apse_triplet_workspace_bytes(int n) {
    if (n < 1 || n > APSE_ASSOC_MAX_N) return 0;
    return triplet_layout(n).total;
}

static int triplet_forward(const double* labels, const float* e, int n, int D, float margin, int squared, float* out, void* ws,
                           size_t ws_bytes, void* stream, int all) {
    if (n == 0) return APSE_OK;
    if (n < 1 || n > APSE_ASSOC_MAX_N || D < 1 || D > APSE_ASSOC_MAX_D)
        return invalid("apse_triplet_*_forward: needs 0 <= n <= 2048 and 1 <= D <= 256");
    if (!labels || !e || !out || !ws) return invalid("apse_triplet_*_forward: null pointer");
    if (ws_bytes < apse_triplet_workspace_bytes(n)) return invalid("apse_triplet_*_forward: workspace too small");
    const TripletWs L = triplet_layout(n);
    char* base = (char*)ws;
    float *d0 = (float*)(base + L.d0), *gd = (float*)(base + L.gd), *sq = (float*)(base + L.sq), *part = (float*)(base + L.part);
    unsigned long long *pos = (unsigned long long*)(base + L.pos), *val = (unsigned long long*)(base + L.val);
    float* scal = (float*)(base + L.scal);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tri_sqnorm, dim3((n + 255) / 256), dim3(256), 0, s, e, n, D, sq);
    hipLaunchKernelGGL(tri_dist, dim3((n + 15) / 16, (n + 15) / 16), dim3(256), 0, s, e, sq, n, D, d0);
    if (all)
        hipLaunchKernelGGL(tri_all_rows, dim3(n), dim3(256), 0, s, labels, d0, n, margin, squared, gd, part, pos, val);
    else
        hipLaunchKernelGGL(tri_hard_rows, dim3(n), dim3(256), 0, s, labels, d0, n, margin, squared, gd, part);
    hipLaunchKernelGGL(tri_finish, dim3(1), dim3(1024), 0, s, part, pos, val, n, all, out, scal);
    return launched();
}

static int triplet_backward(const float* e, int n, int D, int squared, const void* ws, const float* grad, float* de,
                            void* stream) {
    if (n == 0) return APSE_OK;
    if (n < 1 || n > APSE_ASSOC_MAX_N || D < 1 || D > APSE_ASSOC_MAX_D)
        return invalid("apse_triplet_*_backward: needs 0 <= n <= 2048 and 1 <= D <= 256");
    if (!e || !ws || !de) return invalid("apse_triplet_*_backward: null pointer");
    const TripletWs L = triplet_layout(n);
    const char* base = (const char*)ws;
    hipLaunchKernelGGL(tri_grad, dim3(n), dim3(kRowThreads), 0, (hipStream_t)stream, e, (const float*)(base + L.d0),
                       (const float*)(base + L.gd), (const float*)(base + L.scal), grad, n, D, squared, de);
    return launched();
}

int apse_triplet_hard_forward(const double* labels, const float* e, int n, int D, float margin, int squared, float* loss,
                              void* ws, size_t ws_bytes, void* stream) {
    return triplet_forward(labels, e, n, D, margin, squared, loss, ws, ws_bytes, stream, 0);
}

int apse_triplet_all_forward(const double* labels, const float* e, int n, int D, float margin, int squared, float* loss_frac,
                             void* ws, size_t ws_bytes, void* stream) {
    return triplet_forward(labels, e, n, D, margin, squared, loss_frac, ws, ws_bytes, stream, 1);
}

int apse_triplet_hard_backward(const float* e, int n, int D, int squared, const void* ws, const float* grad_loss, float* de,
                               void* stream) {
    return triplet_backward(e, n, D, squared, ws, grad_loss, de, stream);
}

int apse_triplet_all_backward(const float* e, int n, int D, int squared, const void* ws, const float* grad_loss, float* de,
                              void* stream) {
    return triplet_backward(e, n, D, squared, ws, grad_loss, de, stream);
}

int apse_sgd_step(float* p, const float* g, float* buf, long long n, float lr, float momentum, float dampening,
                  float weight_decay, int nesterov, int first_step, void* stream) {
    if (n < 0) return invalid("apse_sgd_step: negative element count");
    if (n == 0) return APSE_OK;
    if (!p || !g || (momentum != 0.f && !buf)) return invalid("apse_sgd_step: null pointer");
    if (nesterov && (momentum <= 0.f || dampening != 0.f))
        return invalid("apse_sgd_step: nesterov needs a momentum and zero dampening");
    const long long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return invalid("apse_sgd_step: too many elements");
    hipLaunchKernelGGL(sgd_step, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, buf, n, lr, momentum, dampening,
                       weight_decay, nesterov, first_step);
    return launched();
}

}  // extern "C"
