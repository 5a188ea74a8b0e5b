// MOTS evaluation: the mask arithmetic of mots_tools/mots_eval on bit windows (include/apse_hip.h "MOTS evaluation").  The
// rules are DESIGN.md "MOTS evaluation"; tests/mots_ref.py restates them in numpy and the GPU tests compare exactly.
//
//   split_idmap   four launches: table reset (65536 values), per-segment statistics (one wave per 64-pixel row segment; one
//                 __ballot per value present in it, integer atomics for bbox and area), one 1024-thread block that scans the
//                 values in ascending order and packs the windows, and the bits (one wave per window row: one __ballot per word)
//   rle_to_bits   one wave per window row, one lane per pixel: the run holding the pixel is an upper_bound over the run ends
//   overlaps      one block per pair: popcounts of the words of a's window against b's (or the OR of the union list's) words
//   shift_overlaps  one block per pair: the same counts with a translated by (dx, dy) and cropped to the frame (the mask-IoU
//                 association metric, utils/mask_utils.py): a funnel shift of two of a's words against each word of b
//   render_idmap  one wave per 64-pixel row segment: each lane keeps the owner of its pixel over the objects in index order
// Only integer arithmetic and order-independent integer atomics: every result is exact and bit-reproducible.
#include "apse_common.h"
#include "../../include/apse_hip.h"
#include "mots_window.h"
#include <limits.h>
#include <string.h>

namespace {

constexpr int kValues = 65536;
constexpr int kScanThreads = 1024;
constexpr int kPerThread = kValues / kScanThreads;
constexpr int kBitsBlocks = 1024;      // grid of split_bits (grid-stride over window rows)

struct SplitTables {                   // workspace layout
    int minx[kValues], maxx[kValues], miny[kValues], maxy[kValues], area[kValues];
    int rowstart[APSE_MOTS_MAX_OBJECTS + 1];
};

struct RenderValues {
    uint16_t v[APSE_MOTS_MAX_OBJECTS];
};

// ---------------------------------------------------------------- split_idmap
__global__ void __launch_bounds__(256) split_reset(SplitTables* t) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    t->minx[v] = INT_MAX; t->miny[v] = INT_MAX; t->maxx[v] = -1; t->maxy[v] = -1; t->area[v] = 0;
}

__global__ void __launch_bounds__(256) split_stats(const uint16_t* __restrict__ idmap, int H, int W, SplitTables* t) {
    const int wpr = (W + 63) >> 6;
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= H * wpr) return;                              // whole waves leave together
    const int lane = threadIdx.x & 63;
    const int y = seg / wpr, wc = seg - y * wpr;
    const int x = wc * 64 + lane;
    const int v = x < W ? (int)idmap[(size_t)y * W + x] : 0;
    uint64_t pending = __ballot(v != 0);
    while (pending) {
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const int vv = __shfl(v, leader);
        const uint64_t m = __ballot(v == vv);
        if (lane == leader) {
            atomicAdd(&t->area[vv], __popcll(m));
            atomicMin(&t->minx[vv], wc * 64 + __ffsll((unsigned long long)m) - 1);
            atomicMax(&t->maxx[vv], wc * 64 + 63 - __clzll((long long)m));
            atomicMin(&t->miny[vv], y);
            atomicMax(&t->maxy[vv], y);
        }
        pending &= ~m;
    }
}

// One block: values in ascending order -> index, window, pool offset (exclusive scans of count, rows and words).
__global__ void __launch_bounds__(kScanThreads) split_scan(SplitTables* t, int max_values, uint64_t* pool, size_t pool_words,
                                                           int* values, apse_mots_window* windows, int* info) {
    __shared__ int s_cnt[kScanThreads], s_rows[kScanThreads];
    __shared__ long long s_words[kScanThreads];
    const int tid = threadIdx.x;
    int cnt = 0, rows = 0;
    long long words = 0;
    for (int i = 0; i < kPerThread; ++i) {
        const int v = tid * kPerThread + i;
        if (v == 0 || t->area[v] == 0) continue;
        ++cnt;
        rows += t->maxy[v] - t->miny[v] + 1;
        words += (long long)(t->maxy[v] - t->miny[v] + 1) * ((t->maxx[v] >> 6) - (t->minx[v] >> 6) + 1);
    }
    s_cnt[tid] = cnt; s_rows[tid] = rows; s_words[tid] = words;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {       // inclusive Hillis-Steele scan
        int c = 0, r = 0;
        long long w = 0;
        if (tid >= off) { c = s_cnt[tid - off]; r = s_rows[tid - off]; w = s_words[tid - off]; }
        __syncthreads();
        s_cnt[tid] += c; s_rows[tid] += r; s_words[tid] += w;
        __syncthreads();
    }
    const int n = s_cnt[kScanThreads - 1];
    const long long total_words = s_words[kScanThreads - 1];
    int idx = s_cnt[tid] - cnt, roff = s_rows[tid] - rows;
    long long woff = s_words[tid] - words;
    for (int i = 0; i < kPerThread; ++i) {
        const int v = tid * kPerThread + i;
        if (v == 0 || t->area[v] == 0) continue;
        const int x0 = t->minx[v], x1 = t->maxx[v] + 1, y0 = t->miny[v], y1 = t->maxy[v] + 1;
        const int wpr = ((x1 - 1) >> 6) - (x0 >> 6) + 1;
        if (idx < max_values) {
            values[idx] = v;
            apse_mots_window w;
            w.rect[0] = x0; w.rect[1] = y0; w.rect[2] = x1; w.rect[3] = y1;
            w.words_per_row = wpr;
            w.area = t->area[v];
            w.bits = pool + woff;
            windows[idx] = w;
            t->rowstart[idx] = roff;
        }
        ++idx;
        roff += y1 - y0;
        woff += (long long)(y1 - y0) * wpr;
    }
    if (tid == kScanThreads - 1) {
        const int ok = n <= max_values && total_words <= (long long)pool_words;
        t->rowstart[n < max_values ? n : max_values] = ok ? s_rows[kScanThreads - 1] : 0;   // 0 rows: split_bits writes nothing
        info[0] = n;
        info[1] = (int)(total_words < INT_MAX ? total_words : INT_MAX);
        info[2] = ok;
    }
}

__global__ void __launch_bounds__(256) split_bits(const uint16_t* __restrict__ idmap, int H, int W, const SplitTables* t,
                                                  const int* values, const apse_mots_window* windows, const int* info,
                                                  int max_values) {
    const int n = min(info[0], max_values);
    const int total = t->rowstart[n];
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * 4;
    for (int item = blockIdx.x * 4 + (threadIdx.x >> 6); item < total; item += nwaves) {
        int lo = 0, hi = n - 1;                              // last k with rowstart[k] <= item
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (t->rowstart[mid] <= item) lo = mid; else hi = mid - 1;
        }
        const apse_mots_window w = windows[lo];
        const int v = values[lo];
        const int r = item - t->rowstart[lo];
        const int y = w.rect[1] + r;
        const int base = w.rect[0] >> 6;
        for (int c = 0; c < w.words_per_row; ++c) {
            const int x = (base + c) * 64 + lane;
            const bool set = x < W && (int)idmap[(size_t)y * W + x] == v;
            const uint64_t m = __ballot(set);
            if (lane == 0) w.bits[(size_t)r * w.words_per_row + c] = m;
        }
    }
}

// ---------------------------------------------------------------- rle_to_bits
__global__ void __launch_bounds__(256) rle_bits(const int* __restrict__ ends, const int* __restrict__ ends_off, int h,
                                                const apse_mots_window* windows) {
    const apse_mots_window w = windows[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int rows = w.rect[3] - w.rect[1];
    if (w.rect[0] >= w.rect[2] || rows <= 0 || !w.bits) return;
    const int r0 = ends_off[blockIdx.y], r1 = ends_off[blockIdx.y + 1];
    const int base = w.rect[0] >> 6;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
        const int y = w.rect[1] + r;
        for (int c = 0; c < w.words_per_row; ++c) {
            const int x = (base + c) * 64 + lane;
            bool set = false;
            if (x >= w.rect[0] && x < w.rect[2]) {
                const int p = x * h + y;                     // column-major pixel index
                int lo = r0, hi = r1;                        // first run whose end is > p
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ends[mid] <= p) lo = mid + 1; else hi = mid;
                }
                set = lo < r1 && ((lo - r0) & 1);
            }
            const uint64_t m = __ballot(set);
            if (lane == 0) w.bits[(size_t)r * w.words_per_row + c] = m;
        }
    }
}

// ---------------------------------------------------------------- overlaps
__global__ void __launch_bounds__(256) overlaps_kernel(const apse_mots_window* windows, const int* pairs, const int* union_idx,
                                                       int n_union, int* out) {
    __shared__ int s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const int p = blockIdx.x;
    const apse_mots_window a = windows[pairs[2 * p]];
    const int bi = pairs[2 * p + 1];
    int inter = 0, area_a = 0, area_b = 0;
    const int ax0 = a.rect[0] >> 6;
    const int arows = a.rect[3] - a.rect[1];
    const long long awords = a.rect[0] < a.rect[2] && arows > 0 ? (long long)arows * a.words_per_row : 0;
    for (long long i = threadIdx.x; i < awords; i += 256) {
        const int r = (int)(i / a.words_per_row), c = (int)(i - (long long)r * a.words_per_row);
        const int y = a.rect[1] + r, aw = ax0 + c;
        const uint64_t wa = window_word(a, y, aw);
        if (!wa) continue;
        area_a += __popcll(wa);
        uint64_t wb = 0;
        if (bi >= 0) {
            wb = window_word(windows[bi], y, aw);
        } else {
            for (int u = 0; u < n_union; ++u) wb |= window_word(windows[union_idx[u]], y, aw);
        }
        inter += __popcll(wa & wb);
    }
    if (bi >= 0) {
        const apse_mots_window b = windows[bi];
        const int brows = b.rect[3] - b.rect[1];
        const long long bwords = b.rect[0] < b.rect[2] && brows > 0 ? (long long)brows * b.words_per_row : 0;
        for (long long i = threadIdx.x; i < bwords; i += 256) {
            const int r = (int)(i / b.words_per_row), c = (int)(i - (long long)r * b.words_per_row);
            area_b += __popcll(window_word(b, b.rect[1] + r, (b.rect[0] >> 6) + c));
        }
    }
    if (inter) atomicAdd(&s_sum[0], inter);
    if (area_a) atomicAdd(&s_sum[1], area_a);
    if (area_b) atomicAdd(&s_sum[2], area_b);
    __syncthreads();
    if (threadIdx.x == 0) {
        out[3 * p] = s_sum[0];
        out[3 * p + 1] = s_sum[1];
        out[3 * p + 2] = bi >= 0 ? s_sum[2] : -1;
    }
}

// ---------------------------------------------------------------- shift_overlaps
__device__ __forceinline__ int wave_sum(int v) {             // wave64 butterfly: every lane must arrive
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// bits lo..hi-1 of a word for 64-bit bounds that may lie anywhere: the part of [lo, hi) inside [0, 64)
__device__ __forceinline__ uint64_t clip_mask(long long lo, long long hi) {
    lo = lo < 0 ? 0 : lo;
    hi = hi > 64 ? 64 : hi;
    return lo < hi ? span_mask((int)lo, (int)hi) : 0;
}

// T(a) = a moved by (dx, dy), zero fill, cropped to the H x W frame.  |T(a)| is counted over a's own words (each word keeps
// the pixels whose target column is inside the frame); |T(a) & b| over b's words, where the word of T(a) at absolute word
// column bw is the funnel shift of a's words q and q + 1 with bw * 64 - dx = q * 64 + off, 0 <= off < 64 (floor division:
// the offset is never negative, and off == 0 takes no second word, so no shift by 64 occurs).
__global__ void __launch_bounds__(256) shift_overlaps_kernel(const apse_mots_window* windows, int n_windows, const int* quads,
                                                             int H, int W, int* out) {
    __shared__ int s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const int p = blockIdx.x;
    const int ia = quads[4 * p], ib = quads[4 * p + 1];
    apse_mots_window a = {}, b = {};                         // an index outside the list: the empty mask
    if (ia >= 0 && ia < n_windows) a = windows[ia];
    if (ib >= 0 && ib < n_windows) b = windows[ib];
    const long long dx = quads[4 * p + 2], dy = quads[4 * p + 3];
    int inter = 0, area_t = 0, area_b = 0;
    const int ax0 = a.rect[0] >> 6;
    const int arows = a.rect[3] - a.rect[1];
    const long long awords = a.rect[0] < a.rect[2] && arows > 0 && a.bits ? (long long)arows * a.words_per_row : 0;
    for (long long i = threadIdx.x; i < awords; i += 256) {
        const int r = (int)(i / a.words_per_row), c = (int)(i - (long long)r * a.words_per_row);
        const int y = a.rect[1] + r, aw = ax0 + c;
        const long long ty = y + dy;
        if (ty < 0 || ty >= H) continue;
        const long long x0 = (long long)aw * 64 + dx;        // target column of bit 0
        area_t += __popcll(window_word(a, y, aw) & clip_mask(-x0, W - x0));
    }
    const int bx0 = b.rect[0] >> 6;
    const int brows = b.rect[3] - b.rect[1];
    const long long bwords = b.rect[0] < b.rect[2] && brows > 0 && b.bits ? (long long)brows * b.words_per_row : 0;
    for (long long i = threadIdx.x; i < bwords; i += 256) {
        const int r = (int)(i / b.words_per_row), c = (int)(i - (long long)r * b.words_per_row);
        const int y = b.rect[1] + r, bw = bx0 + c;
        const uint64_t wb = window_word(b, y, bw);
        if (!wb) continue;
        area_b += __popcll(wb);
        const long long sy = y - dy;                          // source row in a
        if (y < 0 || y >= H || sy < a.rect[1] || sy >= a.rect[3]) continue;
        const long long s = (long long)bw * 64 - dx;         // source column of bit 0
        const long long q = s >= 0 ? s >> 6 : -((-s + 63) >> 6);
        const int off = (int)(s - q * 64);
        uint64_t t = window_word(a, (int)sy, (int)q) >> off;
        if (off) t |= window_word(a, (int)sy, (int)q + 1) << (64 - off);
        t &= clip_mask(-(long long)bw * 64, W - (long long)bw * 64);
        inter += __popcll(t & wb);
    }
    inter = wave_sum(inter);
    area_t = wave_sum(area_t);
    area_b = wave_sum(area_b);
    if ((threadIdx.x & 63) == 0) {                           // one LDS add per wave and count
        atomicAdd(&s_sum[0], inter);
        atomicAdd(&s_sum[1], area_t);
        atomicAdd(&s_sum[2], area_b);
    }
    __syncthreads();
    if (threadIdx.x < 3) out[3 * p + threadIdx.x] = s_sum[threadIdx.x];
}

// ---------------------------------------------------------------- render_idmap
__global__ void __launch_bounds__(256) render_idmap_kernel(const apse_mots_object* __restrict__ objs, int n, int H, int W,
                                                           uint16_t* __restrict__ idmap, RenderValues vals) {
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= H) return;
    const int lane = threadIdx.x & 63;
    const int aw = blockIdx.x;
    const int x = aw * 64 + lane;
    int owner = -1;
    float best = 0.0f;
    for (int k = 0; k < n; ++k) {                            // index order: a later object wins a tie
        const apse_mots_object o = objs[k];
        if (!o.bits || y < o.rect[1] || y >= o.rect[3] || o.rect[0] >= o.rect[2]) continue;
        const int c = aw - (o.rect[0] >> 6);
        if (c < 0 || c >= o.words_per_row) continue;
        const uint64_t word = o.bits[(size_t)(y - o.rect[1]) * o.words_per_row + c];
        const bool set = x >= o.rect[0] && x < o.rect[2] && ((word >> lane) & 1);
        if (set && (owner < 0 || !(best > o.score))) {       // the pair rule: i keeps the overlap only if score[i] > score[j]
            owner = k;
            best = o.score;
        }
    }
    if (x < W) idmap[(size_t)y * W + x] = owner < 0 ? (uint16_t)0 : vals.v[owner];
}

}  // namespace

extern "C" {

size_t apse_mots_split_workspace_bytes(void) { return sizeof(SplitTables); }

int apse_mots_split_idmap(const uint16_t* idmap, int H, int W, int max_values, uint64_t* pool, size_t pool_words, int* values,
                          apse_mots_window* windows, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (!idmap || !frame_ok(H, W) || max_values < 1 || max_values > APSE_MOTS_MAX_OBJECTS) return APSE_E_INVALID;
    if (!values || !windows || !info || !ws || ws_bytes < sizeof(SplitTables) || (pool_words > 0 && !pool)) return APSE_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    SplitTables* t = reinterpret_cast<SplitTables*>(ws);
    const int segs = H * ((W + 63) >> 6);
    split_reset<<<kValues / 256, 256, 0, st>>>(t);
    split_stats<<<(segs + 3) / 4, 256, 0, st>>>(idmap, H, W, t);
    split_scan<<<1, kScanThreads, 0, st>>>(t, max_values, pool, pool_words, values, windows, info);
    split_bits<<<kBitsBlocks, 256, 0, st>>>(idmap, H, W, t, values, windows, info, max_values);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_mots_rle_to_bits(const int* ends, const int* ends_off, int n, int h, int w, const apse_mots_window* windows,
                          void* stream) {
    if (!frame_ok(h, w) || n < 0 || n > APSE_MOTS_MAX_OBJECTS || (n > 0 && (!ends || !ends_off || !windows))) return APSE_E_INVALID;
    if (n == 0) return APSE_OK;
    const int gx = (h + 3) / 4 < 64 ? (h + 3) / 4 : 64;
    rle_bits<<<dim3(gx, n), 256, 0, (hipStream_t)stream>>>(ends, ends_off, h, windows);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_mots_overlaps(const apse_mots_window* windows, int n_windows, const int* pairs, int npairs, const int* union_idx,
                       int n_union, int* out, void* stream) {
    if (n_windows < 0 || npairs < 0 || npairs > APSE_MOTS_MAX_PAIRS || n_union < 0 || n_union > APSE_MOTS_MAX_UNION)
        return APSE_E_INVALID;
    if (npairs > 0 && (!windows || !pairs || !out || n_windows < 1)) return APSE_E_INVALID;
    if (n_union > 0 && !union_idx) return APSE_E_INVALID;
    if (npairs == 0) return APSE_OK;
    overlaps_kernel<<<npairs, 256, 0, (hipStream_t)stream>>>(windows, pairs, union_idx, n_union, out);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_mots_shift_overlaps(const apse_mots_window* windows, int n_windows, const int* quads, int npairs, int H, int W,
                             int* out, void* stream) {
    if (!frame_ok(H, W) || n_windows < 0 || npairs < 0 || npairs > APSE_MOTS_MAX_PAIRS) return APSE_E_INVALID;
    if (npairs > 0 && (!windows || !quads || !out || n_windows < 1)) return APSE_E_INVALID;
    if (npairs == 0) return APSE_OK;
    shift_overlaps_kernel<<<npairs, 256, 0, (hipStream_t)stream>>>(windows, n_windows, quads, H, W, out);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_mots_render_idmap(const apse_mots_object* objects, const int* values_host, int n, int H, int W, uint16_t* idmap,
                           void* stream) {
    if (!idmap || !frame_ok(H, W) || n < 0 || n > APSE_MOTS_MAX_OBJECTS || (n > 0 && (!objects || !values_host)))
        return APSE_E_INVALID;
    RenderValues vals;
    memset(&vals, 0, sizeof vals);
    for (int k = 0; k < n; ++k) {
        if (values_host[k] < 0 || values_host[k] > 65535) return APSE_E_INVALID;
        vals.v[k] = (uint16_t)values_host[k];
    }
    render_idmap_kernel<<<dim3((W + 63) >> 6, (H + 3) / 4), 256, 0, (hipStream_t)stream>>>(objects, n, H, W, idmap, vals);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

}  // extern "C"
