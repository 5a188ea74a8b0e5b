// COCO evaluation: the per-pair and per-group arithmetic of pycocotools COCOeval (include/apse_hip.h "COCO evaluation").  The
// rules are DESIGN.md "COCO evaluation"; tests/coco_ref.py restates them as literal loops and the GPU tests compare exactly.
//
//   box_iou        one block per (image, category) group: maskApi bbIou over its [D][G] pairs
//   poly_to_bits   rleFrPoly + merge: one thread per polygon edge writes the edge's y-boundary points (the host sized every
//                  edge's share by the same column rule), then one wave per window word counts, per part, the points at or before
//                  each pixel (odd: set) and ORs the parts
//   mask_targets   PolygonMasks.crop_and_resize at 28 x 28 for mask-head training: one block per RoI transforms the matched
//                  object's vertices, takes every part through the same edge rule with its points kept in LDS, writes bytes
//   match          evaluateImg's greedy matching: one wave per (group, area range, IoU threshold), detections in order, the
//                  ground truths spread over the lanes; the pick is an (ignore class, IoU, index) max-reduction
//   accumulate     a stable LSD radix sort of every (category, maxDet) list of scores (one block per list), then one wave per
//                  (threshold, category, area range, maxDet): counts, precision envelope and the recall-threshold lookups
// Every value is f64 as pycocotools computes it (the build keeps -ffp-contract=off), there are no float atomics, and every
// reduction is an exact max or an integer sum: results are bit-reproducible.
#include "apse_kernels.h"
#include "../../include/apse_hip.h"
#include <limits.h>
#include <math.h>
#include <stdio.h>

namespace {

constexpr double kScale = 5.0;                       // rleFrPoly's upsampling
constexpr int kSortThreads = 1024;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kPolyChunks = 16;                      // blocks per polygon object (grid-stride over its window words)
constexpr double kEps = 2.220446049250313e-16;       // np.spacing(1) = 2^-52

int invalid(const char* msg) { return apse_fail_global(APSE_E_INVALID, msg); }
int launched(const char* what) { return hipGetLastError() == hipSuccess ? APSE_OK : apse_fail_global(APSE_E_HIP, what); }

// ---------------------------------------------------------------- box IoU
__global__ void __launch_bounds__(256) box_iou_kernel(const int* __restrict__ dt_off, const int* __restrict__ gt_off,
                                                      const long long* __restrict__ iou_off, const double* __restrict__ dt_box,
                                                      const double* __restrict__ gt_box, const int* __restrict__ gt_crowd,
                                                      double* __restrict__ iou) {
    const int grp = blockIdx.x;
    const int d0 = dt_off[grp], D = dt_off[grp + 1] - d0;
    const int g0 = gt_off[grp], G = gt_off[grp + 1] - g0;
    if (D <= 0 || G <= 0) return;
    double* o = iou + iou_off[grp];
    for (int p = threadIdx.x; p < D * G; p += 256) {
        const int d = p / G, g = p - d * G;
        const double* Db = dt_box + 4 * (size_t)(d0 + d);
        const double* Gb = gt_box + 4 * (size_t)(g0 + g);
        const double ga = Gb[2] * Gb[3], da = Db[2] * Db[3];
        double r = 0.0;
        const double w = fmin(Db[2] + Db[0], Gb[2] + Gb[0]) - fmax(Db[0], Gb[0]);
        if (w > 0) {
            const double h = fmin(Db[3] + Db[1], Gb[3] + Gb[1]) - fmax(Db[1], Gb[1]);
            if (h > 0) {
                const double i = w * h;
                const double u = gt_crowd[g0 + g] ? da : da + ga - i;
                r = i / u;
            }
        }
        o[p] = r;
    }
}

// ---------------------------------------------------------------- polygons
__device__ __forceinline__ int scaled(double v) { return (int)(kScale * v + .5); }   // C truncation toward zero

__device__ __forceinline__ int last_le(const int* off, int n, int v) {     // last k in [0, n) with off[k] <= v
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// An edge between two scaled vertices, as rleFrPoly walks it.  The y-boundary points it keeps from this edge's consecutive walk
// points: one per column x in [0, w-1] whose boundary u = 5x+2 | 5x+3 the walk crosses (xd == x exactly there, and nowhere
// else); consecutive edges share their scaled vertex, so no kept point spans two edges.
struct PolyEdge {
    int xs, ys, xe, ye, dx, dy;       // after orient(): in walk order
    int xa, xb;                       // the columns that hold a point: xa .. xb (none when xb < xa)
    double s;                         // the walk's slope (set by orient())
};

__device__ __forceinline__ PolyEdge poly_edge(int xs, int ys, int xe, int ye, int w) {
    PolyEdge e;
    e.xs = xs; e.ys = ys; e.xe = xe; e.ye = ye;
    e.dx = abs(xe - xs); e.dy = abs(ys - ye);
    const int lo = min(xs, xe), hi = max(xs, xe);
    e.xa = lo > 2 ? (lo + 2) / 5 : 0;                // first x with 5x+2 >= lo
    e.xb = hi >= 3 ? min(w - 1, (hi - 3) / 5) : -1;  // last x with 5x+3 <= hi
    e.s = 0.0;
    return e;
}

__device__ __forceinline__ int edge_count(const PolyEdge& e) { return e.xb >= e.xa ? e.xb - e.xa + 1 : 0; }

// rleFrPoly's flip and slope; only for an edge with points (dx > 0 there, so no division by zero)
__device__ __forceinline__ void orient(PolyEdge& e) {
    const bool flip = (e.dx >= e.dy && e.xs > e.xe) || (e.dx < e.dy && e.ys > e.ye);
    if (flip) { int t = e.xs; e.xs = e.xe; e.xe = t; t = e.ys; e.ys = e.ye; e.ye = t; }
    e.s = e.dx >= e.dy ? (double)(e.ye - e.ys) / e.dx : (double)(e.xe - e.xs) / e.dy;
}

// The point of column x (xa <= x <= xb) of an oriented edge in an image of height h: x * h + y, y in [0, h]
__device__ __forceinline__ int edge_point(const PolyEdge& e, int x, int h) {
    int vmin;
    if (e.dx >= e.dy) {                                  // u = t + xs: the pair t0 = 5x+2-xs, t0+1
        const int t0 = 5 * x + 2 - e.xs;
        const int v0 = (int)(e.ys + e.s * t0 + .5), v1 = (int)(e.ys + e.s * (t0 + 1) + .5);
        vmin = min(v0, v1);
    } else {                                             // u = (int)(xs + s t + .5): monotone in t, steps of at most 1
        int a = 1, b = e.dy;                             // first t whose u is past the boundary
        while (a < b) {
            const int mid = (a + b) >> 1;
            const int u = (int)(e.xs + e.s * mid + .5);
            const bool past = e.s >= 0 ? u >= 5 * x + 3 : u <= 5 * x + 2;
            if (past) b = mid; else a = mid + 1;
        }
        vmin = a - 1 + e.ys;                             // v = t + ys: the pair (a-1, a)
    }
    double yd = ((double)vmin + .5) / kScale - .5;
    if (yd < 0) yd = 0; else if (yd > h) yd = h;
    yd = ceil(yd);
    return x * h + (int)yd;
}

// Edge j (vertex j to the next vertex of its part) writes its points into the share the host sized for it.
__global__ void __launch_bounds__(256) poly_edges(const double* __restrict__ xy, const int* __restrict__ part_vert_off,
                                                  int n_parts, const int* __restrict__ obj_part_off, int n_obj,
                                                  const int* __restrict__ obj_hw, const int* __restrict__ edge_off, int n_verts,
                                                  int* __restrict__ toggles, int* __restrict__ info) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_verts) return;
    const int part = last_le(part_vert_off, n_parts + 1, j);
    const int obj = last_le(obj_part_off, n_obj + 1, part);
    const int h = obj_hw[2 * obj], w = obj_hw[2 * obj + 1];
    const int nxt = j + 1 < part_vert_off[part + 1] ? j + 1 : part_vert_off[part];
    PolyEdge e = poly_edge(scaled(xy[2 * j]), scaled(xy[2 * j + 1]), scaled(xy[2 * nxt]), scaled(xy[2 * nxt + 1]), w);
    const int cnt = edge_count(e);
    const int base = edge_off[j];
    if (cnt != edge_off[j + 1] - base) { info[0] = 1; return; }     // the host sized this edge differently: write nothing
    if (cnt == 0) return;
    orient(e);
    for (int x = e.xa; x <= e.xb; ++x) toggles[base + (x - e.xa)] = edge_point(e, x, h);
}

// One wave per (object, window word): pixel p = x*h + y is set in a part when an odd number of the part's points lie at or
// before p; the object is the union of its parts.
__global__ void __launch_bounds__(256) poly_bits(const int* __restrict__ obj_part_off, const int* __restrict__ part_vert_off,
                                                 const int* __restrict__ edge_off, const int* __restrict__ toggles,
                                                 const int* __restrict__ obj_hw, const apse_mots_window* __restrict__ windows) {
    const int obj = blockIdx.x;
    const apse_mots_window win = windows[obj];
    const int rows = win.rect[3] - win.rect[1];
    if (win.rect[0] >= win.rect[2] || rows <= 0 || !win.bits) return;
    const int h = obj_hw[2 * obj];
    const int lane = threadIdx.x & 63;
    const int p0 = obj_part_off[obj], p1 = obj_part_off[obj + 1];
    const int base = win.rect[0] >> 6;
    const long long items = (long long)rows * win.words_per_row;
    for (long long it = blockIdx.y * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.y * 4) {
        const int r = (int)(it / win.words_per_row), c = (int)(it - (long long)r * win.words_per_row);
        const int y = win.rect[1] + r;
        const int x = (base + c) * 64 + lane;
        const bool inside = x >= win.rect[0] && x < win.rect[2];
        const long long p = (long long)x * h + y;
        bool set = false;
        for (int q = p0; q < p1; ++q) {
            const int t0 = edge_off[part_vert_off[q]], t1 = edge_off[part_vert_off[q + 1]];
            int odd = 0;
            for (int t = t0; t < t1; ++t) odd ^= (long long)toggles[t] <= p;
            set = set || odd;
        }
        const uint64_t m = __ballot(inside && set);
        if (lane == 0) win.bits[(size_t)r * win.words_per_row + c] = m;
    }
}

// ---------------------------------------------------------------- mask-head training targets
// detectron2 PolygonMasks.crop_and_resize at kTgt x kTgt, one block per RoI: the matched object's vertices are shifted by the
// box origin and scaled by kTgt / max(extent, 0.1) in f64 (utils/COCO_utils.py crop_and_resize_polygons), then every part goes
// through the edge rule above.  No scratch and no host-sized shares: a wave owns a part and keeps its points as one word per
// column in LDS (bit y of column x = position x * kTgt + y; XOR, so a position hit twice cancels as two sorted points would).
// A pixel is set when an odd number of points lie at or before it: the prefix parity down the columns.  Parts are ORed.
constexpr int kTgt = 28;
constexpr double kCoordMax = 2147483648.0 / 5.0 - 1.0;      // utils/coco.py _COORD_MAX

__global__ void __launch_bounds__(256) mask_targets_kernel(const double* __restrict__ xy, const int* __restrict__ part_vert_off,
                                                           int n_parts, const int* __restrict__ obj_part_off, int n_obj,
                                                           int n_verts, const float* __restrict__ rois,
                                                           const int* __restrict__ matched, unsigned char* __restrict__ targets,
                                                           int* __restrict__ info) {
    __shared__ unsigned s_tog[4][kTgt];
    __shared__ unsigned s_acc[kTgt];
    __shared__ int s_bad;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kTgt) s_acc[tid] = 0u;
    if (tid == 0) s_bad = 0;
    const int obj = matched[row];
    int p0 = 0, p1 = 0;
    if (obj >= 0 && obj < n_obj) { p0 = max(obj_part_off[obj], 0); p1 = min(obj_part_off[obj + 1], n_parts); }
    const double x0 = rois[4 * row], y0 = rois[4 * row + 1];
    const double bw = (double)rois[4 * row + 2] - x0, bh = (double)rois[4 * row + 3] - y0;
    const double rw = (double)kTgt / (0.1 > bw ? 0.1 : bw), rh = (double)kTgt / (0.1 > bh ? 0.1 : bh);   // Python's max(extent, 0.1)
    __syncthreads();
    for (int q0 = p0; q0 < p1; q0 += 4) {                    // the same trip count in every wave: the barriers are uniform
        const int q = q0 + wave;
        if (lane < kTgt) s_tog[wave][lane] = 0u;
        __syncthreads();
        if (q < p1) {
            const int v0 = max(part_vert_off[q], 0), v1 = min(part_vert_off[q + 1], n_verts);
            for (int j = v0 + lane; j < v1; j += 64) {
                const int nxt = j + 1 < v1 ? j + 1 : v0;
                const double ax = (xy[2 * j] - x0) * rw, ay = (xy[2 * j + 1] - y0) * rh;
                const double bx = (xy[2 * nxt] - x0) * rw, by = (xy[2 * nxt + 1] - y0) * rh;
                if (!(fabs(ax) <= kCoordMax) || !(fabs(ay) <= kCoordMax) || !(fabs(bx) <= kCoordMax) || !(fabs(by) <= kCoordMax)) {
                    s_bad = 1;                               // the host path refuses these: the row's bytes are not meaningful
                    continue;
                }
                PolyEdge e = poly_edge(scaled(ax), scaled(ay), scaled(bx), scaled(by), kTgt);
                if (edge_count(e) == 0) continue;
                orient(e);
                for (int x = e.xa; x <= e.xb; ++x) {
                    const int pos = edge_point(e, x, kTgt);  // x * kTgt + y, y in [0, kTgt]: y == kTgt is column x + 1, bit 0
                    const int col = pos / kTgt;
                    if (col < kTgt) atomicXor(&s_tog[wave][col], 1u << (pos - col * kTgt));
                }
            }
        }
        __syncthreads();
        if (q < p1 && lane < kTgt) {
            unsigned carry = 0u;
            for (int c = 0; c < lane; ++c) carry ^= (unsigned)__popc(s_tog[wave][c]);
            unsigned m = s_tog[wave][lane];
            m ^= m << 1; m ^= m << 2; m ^= m << 4; m ^= m << 8; m ^= m << 16;      // bit y = parity of bits 0 .. y
            if (carry & 1u) m = ~m;
            atomicOr(&s_acc[lane], m & ((1u << kTgt) - 1u));
        }
        __syncthreads();
    }
    unsigned char* out = targets + (size_t)row * (kTgt * kTgt);
    for (int i = tid; i < kTgt * kTgt; i += 256) {
        const int y = i / kTgt, x = i - y * kTgt;
        out[i] = (unsigned char)((s_acc[x] >> y) & 1u);
    }
    if (tid == 0 && s_bad) info[0] = 1;
}

// ---------------------------------------------------------------- matching
struct MatchParams {
    double rng[2 * APSE_COCO_MAX_A];
    double thr[APSE_COCO_MAX_T];
    int A, T, n_dt, n_gt;
};

__device__ __forceinline__ bool better(int c1, double v1, int i1, int c2, double v2, int i2) {   // (class, IoU, index) order
    if (c1 != c2) return c1 > c2;
    if (v1 != v2) return v1 > v2;
    return i1 > i2;
}

__global__ void __launch_bounds__(64) match_kernel(const int* __restrict__ dt_off, const int* __restrict__ gt_off,
                                                   const long long* __restrict__ iou_off, const double* __restrict__ iou,
                                                   const double* __restrict__ dt_area, const long long* __restrict__ dt_id,
                                                   const double* __restrict__ gt_area, const int* __restrict__ gt_crowd,
                                                   const long long* __restrict__ gt_id, MatchParams P,
                                                   long long* __restrict__ dt_match, unsigned char* __restrict__ dt_ignore,
                                                   long long* __restrict__ gt_match, unsigned char* __restrict__ gt_ignore) {
    const int grp = blockIdx.x, a = blockIdx.y, t = blockIdx.z;
    const int lane = threadIdx.x;
    const int d0 = dt_off[grp], D = dt_off[grp + 1] - d0;
    const int g0 = gt_off[grp], G = gt_off[grp + 1] - g0;
    const double lo = P.rng[2 * a], hi = P.rng[2 * a + 1];
    const double thr = P.thr[t] < 1.0 - 1e-10 ? P.thr[t] : 1.0 - 1e-10;       // min([t, 1-1e-10])
    long long* gm = gt_match + ((size_t)a * P.T + t) * P.n_gt + g0;
    long long* dm = dt_match + ((size_t)a * P.T + t) * P.n_dt + d0;
    unsigned char* di = dt_ignore + ((size_t)a * P.T + t) * P.n_dt + d0;
    for (int g = lane; g < G; g += 64) {                     // lane g % 64 owns ground truth g: its match is never shared
        gm[g] = 0;
        if (t == 0) {
            const double ar = gt_area[g0 + g];
            gt_ignore[(size_t)a * P.n_gt + g0 + g] = (gt_crowd[g0 + g] || ar < lo || ar > hi) ? 1 : 0;
        }
    }
    const double* io = G > 0 && D > 0 ? iou + iou_off[grp] : nullptr;
    for (int d = 0; d < D; ++d) {
        int bc = -1, bi = -1;
        double bv = 0.0;
        if (io) {
            for (int g = lane; g < G; g += 64) {
                const int crowd = gt_crowd[g0 + g];
                if (gm[g] > 0 && !crowd) continue;           // matched and not crowd
                const double v = io[(size_t)d * G + g];
                if (!(v >= thr)) continue;
                const double ar = gt_area[g0 + g];
                const int c = (crowd || ar < lo || ar > hi) ? 0 : 1;       // not-ignored ground truths come first
                if (bc < 0 || better(c, v, g, bc, bv, bi)) { bc = c; bv = v; bi = g; }
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const int oc = __shfl_xor(bc, off), oi = __shfl_xor(bi, off);
                const double ov = __shfl_xor(bv, off);
                if (oc >= 0 && (bc < 0 || better(oc, ov, oi, bc, bv, bi))) { bc = oc; bv = ov; bi = oi; }
            }
        }
        long long m_id = 0;
        int m_ig = 0;
        if (bc >= 0) {
            m_id = gt_id[g0 + bi];
            m_ig = bc == 0;
            if ((bi & 63) == lane) gm[bi] = dt_id[d0 + d];
        }
        if (lane == 0) {
            const double ar = dt_area[d0 + d];
            dm[d] = m_id;
            di[d] = (m_ig || (m_id == 0 && (ar < lo || ar > hi))) ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------- accumulate: sort
__device__ __forceinline__ uint64_t desc_key(double s) {    // ascending key order = np.argsort(-s) order; NaN last
    if (s != s) return ~0ull;
    const double f = s == 0.0 ? 0.0 : -s;                    // -0 and +0 tie, as numpy compares them
    const uint64_t u = (uint64_t)__double_as_longlong(f);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

// One block per segment (maxDet, category): the concatenated list's detection indices, sorted stably by descending score.
// 8-bit digits, least significant first, in tiles of 1024 keys: a key's place is its digit's base, plus the keys of that
// digit in earlier tiles (s_run), in earlier waves of its tile (s_wcnt) and in earlier lanes of its wave.  A pass whose digit
// is the same for every key is skipped.  The result goes to out (which may be v0).
__global__ void __launch_bounds__(kSortThreads) sort_kernel(const double* __restrict__ score, const int* __restrict__ seg_off,
                                                           const int* __restrict__ seg_idx, uint64_t* __restrict__ k0,
                                                           uint64_t* __restrict__ k1, int* v0, int* v1, int* out) {
    __shared__ int s_hist[256], s_base[256], s_run[256];
    __shared__ int s_wcnt[kSortWaves][256];
    __shared__ int s_skip;
    const int seg = blockIdx.x;
    const int off = seg_off[seg], n = seg_off[seg + 1] - off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t* ka = k0 + off;
    uint64_t* kb = k1 + off;
    int* va = v0 + off;
    int* vb = v1 + off;
    for (int i = tid; i < n; i += kSortThreads) {
        const int idx = seg_idx[off + i];
        ka[i] = desc_key(score[idx]);
        va[i] = idx;
    }
    __syncthreads();
    for (int pass = 0; pass < 8; ++pass) {
        const int sh = pass * 8;
        if (tid < 256) { s_hist[tid] = 0; s_run[tid] = 0; }
        __syncthreads();
        for (int i = tid; i < n; i += kSortThreads) atomicAdd(&s_hist[(int)((ka[i] >> sh) & 255)], 1);
        __syncthreads();
        if (tid == 0) {
            int acc = 0, skip = 0;
            for (int b = 0; b < 256; ++b) { s_base[b] = acc; acc += s_hist[b]; if (s_hist[b] == n) skip = 1; }
            s_skip = skip;
        }
        __syncthreads();
        if (s_skip) continue;                                // every key has this digit: the order stays
        for (int t0 = 0; t0 < n; t0 += kSortThreads) {
            for (int e = tid; e < kSortWaves * 256; e += kSortThreads) s_wcnt[e >> 8][e & 255] = 0;
            __syncthreads();
            const int i = t0 + tid;
            const bool valid = i < n;
            uint64_t key = 0;
            int val = 0, dig = 0;
            if (valid) { key = ka[i]; val = va[i]; dig = (int)((key >> sh) & 255); }
            uint64_t match = __ballot(valid);
            for (int b = 0; b < 8; ++b) {
                const uint64_t bal = __ballot(valid && ((dig >> b) & 1));
                match &= ((dig >> b) & 1) ? bal : ~bal;
            }
            const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
            const int rank = __popcll(match & below);
            if (valid && rank == 0) s_wcnt[wave][dig] = __popcll(match);
            __syncthreads();
            if (valid) {
                int pos = s_base[dig] + s_run[dig] + rank;
                for (int w2 = 0; w2 < wave; ++w2) pos += s_wcnt[w2][dig];
                kb[pos] = key;
                vb[pos] = val;
            }
            __syncthreads();
            if (tid < 256) {
                int acc = 0;
                for (int w2 = 0; w2 < kSortWaves; ++w2) acc += s_wcnt[w2][tid];
                s_run[tid] += acc;
            }
            __syncthreads();
        }
        uint64_t* tk = ka; ka = kb; kb = tk;
        int* tv = va; va = vb; vb = tv;
    }
    int* dst = out + off;
    if (dst != va)                                           // the order ended in the other buffer (or out is the caller's)
        for (int i = tid; i < n; i += kSortThreads) dst[i] = va[i];
}

// ---------------------------------------------------------------- accumulate: precision / recall
struct AccParams {
    int T, R, K, A, M, n_dt;
};

__device__ __forceinline__ int first_above(const double* r, int R, double v) {    // first ri with r[ri] > v
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One wave per (category, area range, threshold x maxDet).  Walks the sorted list from its end: the cumulative counts at i are
// the totals minus the counts after i, and the precision envelope is the running maximum.  searchsorted(rc, recThrs, 'left')
// picks, for each recall threshold r, the first i with rc[i] >= r: that i is the one with rc[i-1] < r <= rc[i].
__global__ void __launch_bounds__(64) acc_kernel(const double* __restrict__ score, const long long* __restrict__ dt_match,
                                                 const unsigned char* __restrict__ dt_ignore, const int* __restrict__ seg_off,
                                                 const int* __restrict__ sorted_idx, const unsigned char* __restrict__ gt_ignore,
                                                 const int* __restrict__ cat_gt_off, int n_gt, const double* __restrict__ rec_thrs,
                                                 AccParams P, double* __restrict__ precision, double* __restrict__ recall,
                                                 double* __restrict__ scores) {
    __shared__ double s_q[APSE_COCO_MAX_R], s_ss[APSE_COCO_MAX_R], s_r[APSE_COCO_MAX_R];
    const int k = blockIdx.x, a = blockIdx.y;
    const int t = blockIdx.z / P.M, m = blockIdx.z - t * P.M;
    const int lane = threadIdx.x;
    const int R = P.R;
    const size_t rstride = (size_t)P.K * P.A * P.M;
    const size_t col = ((size_t)k * P.A + a) * P.M + m;
    double* prec = precision + (size_t)t * R * rstride + col;
    double* scr = scores + (size_t)t * R * rstride + col;
    int npig = 0;                                            // the category's ground truths not ignored in this area range
    const unsigned char* gi = gt_ignore + (size_t)a * n_gt;
    for (int g = cat_gt_off[k] + lane; g < cat_gt_off[k + 1]; g += 64) npig += gi[g] == 0;
    for (int off = 32; off >= 1; off >>= 1) npig += __shfl_xor(npig, off);
    if (npig == 0) {
        for (int ri = lane; ri < R; ri += 64) { prec[ri * rstride] = -1.0; scr[ri * rstride] = -1.0; }
        if (lane == 0) recall[(size_t)t * rstride + col] = -1.0;
        return;
    }
    const int seg = m * P.K + k;
    const int off0 = seg_off[seg], n = seg_off[seg + 1] - off0;
    const int* idx = sorted_idx + off0;
    const long long* dm = dt_match + ((size_t)a * P.T + t) * P.n_dt;
    const unsigned char* di = dt_ignore + ((size_t)a * P.T + t) * P.n_dt;
    for (int ri = lane; ri < R; ri += 64) { s_q[ri] = 0.0; s_ss[ri] = 0.0; s_r[ri] = rec_thrs[ri]; }
    int TP = 0, FP = 0;
    for (int i = lane; i < n; i += 64) {
        const int d = idx[i];
        if (!di[d]) { if (dm[d] != 0) ++TP; else ++FP; }
    }
    for (int off = 32; off >= 1; off >>= 1) { TP += __shfl_xor(TP, off); FP += __shfl_xor(FP, off); }
    __syncthreads();
    const double npd = (double)npig;
    int carry_tp = 0, carry_fp = 0;
    double carry_env = -1.0;
    for (int end = n; end > 0; end -= 64) {
        const int i = end - 64 + lane;
        const bool valid = i >= 0;
        int tpf = 0, fpf = 0;
        double sc = 0.0;
        if (valid) {
            const int d = idx[i];
            sc = score[d];
            if (!di[d]) { if (dm[d] != 0) tpf = 1; else fpf = 1; }
        }
        int stp = tpf, sfp = fpf;                            // inclusive suffix sums over lanes >= lane
        for (int o = 1; o < 64; o <<= 1) {
            const int a1 = __shfl_down(stp, o), b1 = __shfl_down(sfp, o);
            if (lane + o < 64) { stp += a1; sfp += b1; }
        }
        const int tp_i = TP - (carry_tp + stp) + tpf;        // np.cumsum at i
        const int fp_i = FP - (carry_fp + sfp) + fpf;
        const double tpd = (double)tp_i, fpd = (double)fp_i;
        double env = valid ? tpd / ((fpd + tpd) + kEps) : -1.0;
        for (int o = 1; o < 64; o <<= 1) {
            const double e1 = __shfl_down(env, o);
            if (lane + o < 64) env = fmax(env, e1);
        }
        env = fmax(env, carry_env);
        if (valid && (tpf || i == 0)) {                      // rc changes only here
            const double rc = tpd / npd;
            const int lo = i == 0 ? 0 : first_above(s_r, R, (double)(tp_i - tpf) / npd);
            const int hi = first_above(s_r, R, rc);
            for (int ri = lo; ri < hi; ++ri) { s_q[ri] = env; s_ss[ri] = sc; }
        }
        const int lead = end >= 64 ? 0 : 64 - end;           // first valid lane: its sums and envelope cover the tile
        carry_tp += __shfl(stp, lead);
        carry_fp += __shfl(sfp, lead);
        carry_env = __shfl(env, lead);
    }
    __syncthreads();
    for (int ri = lane; ri < R; ri += 64) { prec[ri * rstride] = s_q[ri]; scr[ri * rstride] = s_ss[ri]; }
    if (lane == 0) recall[(size_t)t * rstride + col] = n ? (double)TP / npd : 0.0;
}

bool frame_ok(int h, int w) {
    return h >= 1 && h <= APSE_MAX_FRAME_H && w >= 1 && w <= APSE_MAX_FRAME_W && (long long)h * w <= INT_MAX - 64;
}

size_t keys_bytes(long long n_keys) { return (size_t)(n_keys > 0 ? n_keys : 1) * sizeof(uint64_t); }
size_t vals_bytes(long long n_keys) { return ((size_t)(n_keys > 0 ? n_keys : 1) * sizeof(int) + 255) & ~(size_t)255; }

int sort_checks(const char* who, int n_seg, long long n_keys, int max_seg, size_t ws_bytes, const void* ws) {
    static char msg[160];
    if (n_seg < 0 || n_seg > APSE_COCO_MAX_CATS * APSE_COCO_MAX_M) {
        snprintf(msg, sizeof msg, "%s: n_seg outside [0, APSE_COCO_MAX_CATS * APSE_COCO_MAX_M]", who);
        return invalid(msg);
    }
    if (max_seg < 0 || max_seg > APSE_COCO_MAX_KEYS) {
        snprintf(msg, sizeof msg, "%s: a (category, maxDet) list outside [0, APSE_COCO_MAX_KEYS] detections", who);
        return invalid(msg);
    }
    if (n_keys < 0 || n_keys > (long long)max_seg * n_seg || n_keys > INT_MAX) {
        snprintf(msg, sizeof msg, "%s: n_keys outside [0, max_seg * lists]", who);
        return invalid(msg);
    }
    if (!ws || ws_bytes < 2 * keys_bytes(n_keys) + 2 * vals_bytes(n_keys)) {
        snprintf(msg, sizeof msg, "%s: workspace smaller than apse_coco_accumulate_workspace_bytes", who);
        return invalid(msg);
    }
    return APSE_OK;
}

void launch_sort(const double* score, const int* seg_off, int n_seg, const int* seg_idx, long long n_keys, int* out, void* ws,
                 hipStream_t st) {
    uint64_t* k0 = reinterpret_cast<uint64_t*>(ws);
    uint64_t* k1 = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(ws) + keys_bytes(n_keys));
    int* v0 = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + 2 * keys_bytes(n_keys));
    int* v1 = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + 2 * keys_bytes(n_keys) + vals_bytes(n_keys));
    sort_kernel<<<n_seg, kSortThreads, 0, st>>>(score, seg_off, seg_idx, k0, k1, v0, v1, out ? out : v0);
}

}  // namespace

extern "C" {

int apse_k_mask_targets(const double* xy, const int* part_vert_off, int n_parts, const int* obj_part_off, int n_obj, int n_verts,
                        const float* rois, const int* matched, int n, uint8_t* targets, int* info, hipStream_t s) {
    mask_targets_kernel<<<n, 256, 0, s>>>(xy, part_vert_off, n_parts, obj_part_off, n_obj, n_verts, rois, matched, targets, info);
    return launched("apse_coco_mask_targets: launch failed");
}

int apse_coco_box_iou(const int* dt_off, const int* gt_off, const long long* iou_off, int n_groups, int max_dt, int max_gt,
                      const double* dt_box, const double* gt_box, const int* gt_crowd, double* iou, void* stream) {
    if (n_groups < 0 || n_groups > APSE_COCO_MAX_GROUPS) return invalid("apse_coco_box_iou: n_groups outside [0, APSE_COCO_MAX_GROUPS]");
    if (max_dt < 0 || max_dt > APSE_COCO_MAX_DET) return invalid("apse_coco_box_iou: max_dt outside [0, APSE_COCO_MAX_DET]");
    if (max_gt < 0 || max_gt > APSE_COCO_MAX_GT) return invalid("apse_coco_box_iou: max_gt outside [0, APSE_COCO_MAX_GT]");
    if (n_groups == 0) return APSE_OK;
    if (!dt_off || !gt_off || !iou_off || (max_dt > 0 && max_gt > 0 && (!dt_box || !gt_box || !gt_crowd || !iou)))
        return invalid("apse_coco_box_iou: NULL pointer");
    box_iou_kernel<<<n_groups, 256, 0, (hipStream_t)stream>>>(dt_off, gt_off, iou_off, dt_box, gt_box, gt_crowd, iou);
    return launched("apse_coco_box_iou: launch failed");
}

int apse_coco_poly_to_bits(const double* xy, const int* part_vert_off, int n_parts, const int* obj_part_off, int n_obj,
                           const int* obj_hw, const int* obj_hw_host, const int* edge_off, int n_verts, int* toggles,
                           const apse_mots_window* windows, int* info, void* stream) {
    if (n_obj < 0 || n_obj > APSE_COCO_MAX_POLY_OBJECTS)
        return invalid("apse_coco_poly_to_bits: n_obj outside [0, APSE_COCO_MAX_POLY_OBJECTS]");
    if (n_parts < 0 || n_parts > APSE_COCO_MAX_POLY_PARTS)
        return invalid("apse_coco_poly_to_bits: n_parts outside [0, APSE_COCO_MAX_POLY_PARTS]");
    if (n_verts < 0 || n_verts > APSE_COCO_MAX_POLY_VERTS)
        return invalid("apse_coco_poly_to_bits: n_verts outside [0, APSE_COCO_MAX_POLY_VERTS]");
    if (n_obj > 0 && !obj_hw_host) return invalid("apse_coco_poly_to_bits: NULL obj_hw_host");
    for (int i = 0; i < n_obj; ++i)
        if (!frame_ok(obj_hw_host[2 * i], obj_hw_host[2 * i + 1]))
            return invalid("apse_coco_poly_to_bits: an image size outside the frame limits");
    if (n_obj == 0) return APSE_OK;
    if (!part_vert_off || !obj_part_off || !obj_hw || !edge_off || !windows || !info || (n_verts > 0 && (!xy || !toggles)))
        return invalid("apse_coco_poly_to_bits: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_verts > 0)
        poly_edges<<<(n_verts + 255) / 256, 256, 0, st>>>(xy, part_vert_off, n_parts, obj_part_off, n_obj, obj_hw, edge_off,
                                                         n_verts, toggles, info);
    poly_bits<<<dim3(n_obj, kPolyChunks), 256, 0, st>>>(obj_part_off, part_vert_off, edge_off, toggles, obj_hw, windows);
    return launched("apse_coco_poly_to_bits: launch failed");
}

int apse_coco_match(const int* dt_off, const int* gt_off, const long long* iou_off, int n_groups, int max_dt, int max_gt,
                    const double* iou, const double* dt_area, const long long* dt_id, int n_dt, const double* gt_area,
                    const int* gt_crowd, const long long* gt_id, int n_gt, const double* area_rng_host, int A,
                    const double* iou_thrs_host, int T, long long* dt_match, unsigned char* dt_ignore, long long* gt_match,
                    unsigned char* gt_ignore, void* stream) {
    if (n_groups < 0 || n_groups > APSE_COCO_MAX_GROUPS) return invalid("apse_coco_match: n_groups outside [0, APSE_COCO_MAX_GROUPS]");
    if (max_dt < 0 || max_dt > APSE_COCO_MAX_DET) return invalid("apse_coco_match: max_dt outside [0, APSE_COCO_MAX_DET]");
    if (max_gt < 0 || max_gt > APSE_COCO_MAX_GT) return invalid("apse_coco_match: max_gt outside [0, APSE_COCO_MAX_GT]");
    if (A < 1 || A > APSE_COCO_MAX_A) return invalid("apse_coco_match: A outside [1, APSE_COCO_MAX_A]");
    if (T < 1 || T > APSE_COCO_MAX_T) return invalid("apse_coco_match: T outside [1, APSE_COCO_MAX_T]");
    if (n_dt < 0 || n_gt < 0 || (long long)n_dt * A * T > INT_MAX || (long long)n_gt * A * T > INT_MAX)
        return invalid("apse_coco_match: n_dt * A * T or n_gt * A * T past 2^31 - 1");
    if (!area_rng_host || !iou_thrs_host) return invalid("apse_coco_match: NULL area ranges or thresholds");
    if (n_groups == 0) return APSE_OK;
    if (!dt_off || !gt_off || !iou_off || (n_dt > 0 && (!dt_area || !dt_id || !dt_match || !dt_ignore)) ||
        (n_gt > 0 && (!gt_area || !gt_crowd || !gt_id || !gt_match || !gt_ignore)) || (n_dt > 0 && n_gt > 0 && !iou))
        return invalid("apse_coco_match: NULL pointer");
    MatchParams P;
    for (int i = 0; i < 2 * A; ++i) P.rng[i] = area_rng_host[i];
    for (int i = 0; i < T; ++i) P.thr[i] = iou_thrs_host[i];
    P.A = A; P.T = T; P.n_dt = n_dt; P.n_gt = n_gt;
    match_kernel<<<dim3(n_groups, A, T), 64, 0, (hipStream_t)stream>>>(dt_off, gt_off, iou_off, iou, dt_area, dt_id, gt_area,
                                                                      gt_crowd, gt_id, P, dt_match, dt_ignore, gt_match, gt_ignore);
    return launched("apse_coco_match: launch failed");
}

size_t apse_coco_accumulate_workspace_bytes(long long n_keys) {
    if (n_keys < 0 || n_keys > INT_MAX) return 0;
    return 2 * keys_bytes(n_keys) + 2 * vals_bytes(n_keys);
}

int apse_coco_sort_lists(const double* score, const int* seg_off, int n_seg, const int* seg_idx, long long n_keys, int max_seg,
                         int* sorted_idx, void* ws, size_t ws_bytes, void* stream) {
    const int rc = sort_checks("apse_coco_sort_lists", n_seg, n_keys, max_seg, ws_bytes, ws);
    if (rc != APSE_OK) return rc;
    if (n_seg == 0 || n_keys == 0) return APSE_OK;
    if (!score || !seg_off || !seg_idx || !sorted_idx) return invalid("apse_coco_sort_lists: NULL pointer");
    launch_sort(score, seg_off, n_seg, seg_idx, n_keys, sorted_idx, ws, (hipStream_t)stream);
    return launched("apse_coco_sort_lists: launch failed");
}

int apse_coco_accumulate(const double* dt_score, const long long* dt_match, const unsigned char* dt_ignore, int n_dt,
                         const unsigned char* gt_ignore, int n_gt, const int* cat_gt_off, const int* seg_off,
                         const int* seg_idx, long long n_keys, int max_seg, const double* rec_thrs, int T, int R, int K, int A,
                         int M, double* precision, double* recall, double* scores, void* ws, size_t ws_bytes, void* stream) {
    if (T < 1 || T > APSE_COCO_MAX_T) return invalid("apse_coco_accumulate: T outside [1, APSE_COCO_MAX_T]");
    if (R < 1 || R > APSE_COCO_MAX_R) return invalid("apse_coco_accumulate: R outside [1, APSE_COCO_MAX_R]");
    if (K < 1 || K > APSE_COCO_MAX_CATS) return invalid("apse_coco_accumulate: K outside [1, APSE_COCO_MAX_CATS]");
    if (A < 1 || A > APSE_COCO_MAX_A) return invalid("apse_coco_accumulate: A outside [1, APSE_COCO_MAX_A]");
    if (M < 1 || M > APSE_COCO_MAX_M) return invalid("apse_coco_accumulate: M outside [1, APSE_COCO_MAX_M]");
    if (max_seg < 0 || max_seg > APSE_COCO_MAX_KEYS)
        return invalid("apse_coco_accumulate: a (category, maxDet) list outside [0, APSE_COCO_MAX_KEYS] detections");
    if (n_dt < 0 || n_gt < 0 || (long long)n_dt * A * T > INT_MAX || (long long)n_gt * A > INT_MAX)
        return invalid("apse_coco_accumulate: n_dt * A * T or n_gt * A past 2^31 - 1");
    if (n_keys < 0 || n_keys > (long long)max_seg * K * M || n_keys > INT_MAX)
        return invalid("apse_coco_accumulate: n_keys outside [0, max_seg * K * M]");
    if (!ws || ws_bytes < apse_coco_accumulate_workspace_bytes(n_keys))
        return invalid("apse_coco_accumulate: workspace smaller than apse_coco_accumulate_workspace_bytes");
    if (!cat_gt_off || !seg_off || !rec_thrs || !precision || !recall || !scores || (n_keys > 0 && (!seg_idx || !dt_score)) ||
        (n_dt > 0 && (!dt_match || !dt_ignore)) || (n_gt > 0 && !gt_ignore))
        return invalid("apse_coco_accumulate: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    int* v0 = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + 2 * keys_bytes(n_keys));     // the sorted lists
    if (n_keys > 0) launch_sort(dt_score, seg_off, K * M, seg_idx, n_keys, nullptr, ws, st);
    AccParams P;
    P.T = T; P.R = R; P.K = K; P.A = A; P.M = M; P.n_dt = n_dt;
    acc_kernel<<<dim3(K, A, T * M), 64, 0, st>>>(dt_score, dt_match, dt_ignore, seg_off, v0, gt_ignore, cat_gt_off, n_gt,
                                               rec_thrs, P, precision, recall, scores);
    return launched("apse_coco_accumulate: launch failed");
}

}  // extern "C"
