// Decision kernels of the dcnn hot path (gfx950): top-k, box decoding, NMS, final ranking.
// Everything here is f32 with -ffp-contract=off so that, given identical inputs, the index
// results are identical to the CPU oracle's (each product and sum rounded separately, IEEE
// division).  Ordering rule everywhere: score descending, ties by ascending input index
// (DESIGN.md "Tie-breaks").
//
// Restates (from detectron2 0.1.2 / torchvision 0.6, reached from
// /root/reference/dcnn/networks/track_rcnn.py:46,51):
//   RPNOutputs.predict_proposals + find_top_rpn_proposals  -> rpn_topk_stage, rpn_decode,
//                                                             nms_percat, rank_final
//   FastRCNNOutputs.inference / fast_rcnn_inference_single_image -> box_candidates,
//                                                             nms_percat, rank_final
#include "apse_kernels.h"

#define TK_N 4096          // elements sorted per block in the top-k tournament
#define NMS_MAX APSE_NMS_SLOT   // boxes per category (<= 1000 by construction); the host sizes the keep lists by the same constant

__device__ __forceinline__ uint32_t mono_key(float f) {   // order-preserving float -> uint
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mono_inv(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}
// ascending sort of this composite = score descending, index ascending.  The two zeros are one score (-0.0 == +0.0, as a
// stable sort of the floats has it): the key carries +0, so a tie between them goes by index and comp_score returns +0.
__device__ __forceinline__ uint64_t comp_key(float score, uint32_t idx) {
    score = score == 0.f ? 0.f : score;
    return ((uint64_t)(~mono_key(score)) << 32) | idx;
}
__device__ __forceinline__ float comp_score(uint64_t k) { return mono_inv(~(uint32_t)(k >> 32)); }

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {   // l must be wave-uniform
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// Bitonic sort of N = 1024 * EPT 64-bit keys in LDS, ascending, by a 1024-thread block.  Thread t owns the EPT consecutive
// keys a[EPT t ..] in registers: a compare-exchange distance j < EPT stays inside the thread, j < 64 EPT inside the wave
// (64-bit lane exchange), and only j >= 64 EPT goes through LDS with a block barrier -- 10 of the 78 steps for N = 4096
// (EPT = 4), 10 of 55 for N = 1024 (EPT = 1).  The all-LDS form paid a barrier per step and ran at ~0.55 us a step with one
// block per CU (rpn_topk_stage 43 us per 4096 keys).  Same network, same result (the keys are distinct).
template <int EPT>
__device__ __forceinline__ void block_bitonic_sort(uint64_t* a, int tid) {
    constexpr int N = 1024 * EPT;
    uint64_t e[EPT];
#pragma unroll
    for (int s = 0; s < EPT; ++s) e[s] = a[tid * EPT + s];
    for (int k = 2; k <= N; k <<= 1) {
        int j = k >> 1;
        if (j >= 64 * EPT) {
            __syncthreads();                               // every thread has taken its keys out of LDS
#pragma unroll
            for (int s = 0; s < EPT; ++s) a[tid * EPT + s] = e[s];
            __syncthreads();
            for (; j >= 64 * EPT; j >>= 1) {
                for (int pidx = tid; pidx < N / 2; pidx += 1024) {
                    const int i = ((pidx & ~(j - 1)) << 1) | (pidx & (j - 1));
                    const int l = i | j;
                    const bool asc = (i & k) == 0;
                    const uint64_t x = a[i], y = a[l];
                    if ((x > y) == asc) { a[i] = y; a[l] = x; }
                }
                __syncthreads();
            }
#pragma unroll
            for (int s = 0; s < EPT; ++s) e[s] = a[tid * EPT + s];
        }
        for (; j >= EPT; j >>= 1) {                        // partner key lives in lane ^ (j / EPT), same register slot
            const int tj = j / EPT;
            const bool lower = (tid & tj) == 0;
#pragma unroll
            for (int s = 0; s < EPT; ++s) {
                const bool asc = ((tid * EPT + s) & k) == 0;
                const uint64_t o = __shfl_xor(e[s], tj);
                const bool take_min = lower == asc;
                e[s] = ((o < e[s]) == take_min) ? o : e[s];
            }
        }
#pragma unroll
        for (int jj = EPT / 2; jj >= 1; jj >>= 1) {        // both keys in this thread
            if (jj > (k >> 1)) continue;
#pragma unroll
            for (int s = 0; s < EPT; ++s) {
                if (s & jj) continue;
                const bool asc = ((tid * EPT + s) & k) == 0;
                const uint64_t x = e[s], y = e[s | jj];
                if ((x > y) == asc) { e[s] = y; e[s | jj] = x; }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < EPT; ++s) a[tid * EPT + s] = e[s];
    __syncthreads();
}

// ---------------------------------------------------------------- RPN top-k tournament
// RpnLevel, RpnLevels, TopkJob: apse_kernels.h (filled by plan.hip)

// lists: [B][nslots][1024] u64.  kind 0: sort one 4096-element chunk of raw logits (bitonic, LDS).
// kind 1: merge up to four sorted lists by rank (position + binary-search counts in the other lists):
// no sort, no barriers after the load.  `zero_word` (stage 0 only): image b's max-coordinate cell is
// cleared here so the decode kernel's atomicMax needs no separate memset.
__global__ __launch_bounds__(1024) void rpn_topk_stage(const RpnLevels* __restrict__ Lp, const TopkJob* __restrict__ jobs,
                                                       uint64_t* __restrict__ lists, int nslots,
                                                       uint32_t* __restrict__ zero_word) {
    __shared__ uint64_t a[TK_N];
    const TopkJob* job = jobs + blockIdx.x;
    const int b = blockIdx.y, tid = threadIdx.x;
    uint64_t* pool = lists + (size_t)b * nslots * 1024;
    if (zero_word && blockIdx.x == 0 && tid == 0) zero_word[b] = 0u;
    if (job->kind == 0) {
        const RpnLevel* lv = &Lp->lv[job->level];
        const int head_ld = Lp->head_ld;
        const float* head = lv->head + (size_t)b * lv->H * lv->W * head_ld;
        const int jb = job->begin, jc = job->count;
        for (int i = tid; i < TK_N; i += 1024) {
            uint64_t k = ~0ull;
            if (i < jc) {
                const int e = jb + i;
                const int pix = e / 3, an = e - pix * 3;
                k = comp_key(head[(size_t)pix * head_ld + an], (uint32_t)e);
            }
            a[i] = k;
        }
        __syncthreads();
        block_bitonic_sort<TK_N / 1024>(a, tid);
        if (tid < job->dst_count) pool[(size_t)job->dst * 1024 + tid] = a[tid];
    } else {
        const int ns = job->nsrc;
        int cnt[4];
        for (int s = 0; s < 4; ++s) cnt[s] = s < ns ? job->src_count[s] : 0;
        for (int s = 0; s < ns; ++s)
            if (tid < cnt[s]) a[s * 1024 + tid] = pool[(size_t)job->src[s] * 1024 + tid];
        __syncthreads();
        const int K = job->dst_count;
        uint64_t* dst = pool + (size_t)job->dst * 1024;
        for (int s = 0; s < ns; ++s) {
            if (tid >= cnt[s]) continue;
            const uint64_t key = a[s * 1024 + tid];
            int rank = tid;
            for (int o = 0; o < ns; ++o) {
                if (o == s) continue;
                int lo = 0, hi = cnt[o];
                const uint64_t* ko = a + o * 1024;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (ko[mid] < key) lo = mid + 1; else hi = mid; }
                rank += lo;
            }
            if (rank < K) dst[rank] = key;
        }
    }
}

// Decode the selected anchors of every level: Box2BoxTransform.apply_deltas (weights 1,1,1,1),
// clip to the image, nonempty flag, and the running max coordinate of the kept boxes.
// out arrays are [B][5*pre_topk].  scores: the logit as the sort key carries it (a zero is +0 whatever its sign).
__global__ __launch_bounds__(256) void rpn_decode(const RpnLevels* __restrict__ Lp, const uint64_t* __restrict__ lists, int nslots,
                                                  const int* __restrict__ final_slot, float img_h, float img_w,
                                                  float scale_clamp, float* __restrict__ boxes, float* __restrict__ scores,
                                                  int* __restrict__ valid, uint32_t* __restrict__ maxc, int level_mask) {
    const int b = blockIdx.z, l = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int pre_topk = Lp->pre_topk, head_ld = Lp->head_ld;
    if (i >= pre_topk) return;
    const RpnLevel lv = Lp->lv[l];
    const size_t o = (size_t)b * 5 * pre_topk + (size_t)l * pre_topk + i;
    if (i >= lv.k || !((level_mask >> l) & 1)) { valid[o] = 0; scores[o] = 0.f; return; }
    const uint64_t key = lists[((size_t)b * nslots + final_slot[l]) * 1024 + i];
    const uint32_t e = (uint32_t)key;
    const float sc = comp_score(key);
    const int pix = e / 3, an = e - pix * 3;
    const int y = pix / lv.W, x = pix - y * lv.W;
    const float sx = (float)(x * lv.stride), sy = (float)(y * lv.stride);
    const float ax0 = sx + lv.base[an][0], ay0 = sy + lv.base[an][1];
    const float ax1 = sx + lv.base[an][2], ay1 = sy + lv.base[an][3];
    const float* d = lv.head + ((size_t)b * lv.H * lv.W + pix) * head_ld + 3 + an * 4;
    const float w = ax1 - ax0, h = ay1 - ay0;
    const float cx = ax0 + 0.5f * w, cy = ay0 + 0.5f * h;
    float dx = d[0] / 1.0f, dy = d[1] / 1.0f, dw = d[2] / 1.0f, dh = d[3] / 1.0f;
    dw = dw > scale_clamp ? scale_clamp : dw;
    dh = dh > scale_clamp ? scale_clamp : dh;
    const float pcx = dx * w + cx, pcy = dy * h + cy;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    float x0 = pcx - 0.5f * pw, y0 = pcy - 0.5f * ph, x1 = pcx + 0.5f * pw, y1 = pcy + 0.5f * ph;
    x0 = fminf(fmaxf(x0, 0.f), img_w);
    y0 = fminf(fmaxf(y0, 0.f), img_h);
    x1 = fminf(fmaxf(x1, 0.f), img_w);
    y1 = fminf(fmaxf(y1, 0.f), img_h);
    const int ok = ((x1 - x0) > 0.f) && ((y1 - y0) > 0.f);
    boxes[o * 4 + 0] = x0; boxes[o * 4 + 1] = y0; boxes[o * 4 + 2] = x1; boxes[o * 4 + 3] = y1;
    scores[o] = sc;
    valid[o] = ok;
    if (ok) {
        const float m = fmaxf(fmaxf(x0, x1), fmaxf(y0, y1));   // all >= 0 after the clip
        atomicMax(maxc + b, __float_as_uint(m));
    }
}

// ---------------------------------------------------------------- per-category NMS
// Entries: boxes/scores/valid are [B][n_total]; the category of entry e is
// cat_div ? e / cat_div : e % cat_mod.  Within a category, entries are ordered by (score desc,
// entry index asc); IoU is evaluated on boxes shifted by cat * (max_coord + 1) in f32 (torchvision
// batched_nms); `iou > thr` suppresses.  torchvision numbers the categories the call is given: with cat_mask != 0 (the RPN's
// level mask) category c counts as the number of mask bits below c, with cat_mask == 0 as c itself.  Three launches:
//   nms_prepare : one block per (category, image): ordered compaction + sort -> sorted shifted boxes
//   nms_matrix  : 64x64 tiles of the upper-triangular suppression bit matrix, one wave each
//   nms_scan    : one block per (category, image): greedy scan, 64 rows at a time
// scratch per (image, category): entry[1024] int, box[4][1024] f32, area[1024] f32, mask[1024][16] u64, n.
struct NmsScratch {
    int* entry; float* box; float* area; uint64_t* mask; int* n;
};

// Sorted keys -> the category's slot of the NMS scratch: boxes shifted by cat * (max_coord + 1) in f32 (torchvision batched_nms
// numbers the categories that are present in the call: `cat` is the slot's rank among them), their areas, entry ids, count.
__device__ __forceinline__ void nms_store_sorted(const uint64_t* keys, int n, int cat, uint32_t maxc_bits,
                                                 const float* __restrict__ boxes, NmsScratch S, size_t slot, int tid) {
    const float off = (float)cat * (__uint_as_float(maxc_bits) + 1.0f);
    float* bx = S.box + slot * 4 * NMS_MAX;
    if (tid < n) {
        const uint32_t e = (uint32_t)keys[tid];
        const float x0 = boxes[e * 4 + 0] + off, y0 = boxes[e * 4 + 1] + off;
        const float x1 = boxes[e * 4 + 2] + off, y1 = boxes[e * 4 + 3] + off;
        bx[tid] = x0; bx[NMS_MAX + tid] = y0; bx[2 * NMS_MAX + tid] = x1; bx[3 * NMS_MAX + tid] = y1;
        S.area[slot * NMS_MAX + tid] = (x1 - x0) * (y1 - y0);
        S.entry[slot * NMS_MAX + tid] = (int)e;
    }
    if (tid == 0) S.n[slot] = n;
}

__global__ __launch_bounds__(1024) void nms_prepare(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                    const int* __restrict__ valid, int n_total, int cat_div, int cat_mod,
                                                    const uint32_t* __restrict__ maxc, NmsScratch S, int ncat, int cat_mask,
                                                    int presorted) {
    __shared__ uint64_t keys[NMS_MAX];
    __shared__ int wsum[17];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    boxes += (size_t)b * n_total * 4;
    scores += (size_t)b * n_total;
    valid += (size_t)b * n_total;
    const size_t slot = (size_t)b * ncat + c;
    if (tid == 0) wsum[16] = 0;
    keys[tid] = ~0ull;
    __syncthreads();
    for (int base = 0; base < n_total; base += 1024) {
        const int e = base + tid;
        bool f = false;
        if (e < n_total) {
            const int cat = cat_div ? e / cat_div : e % cat_mod;
            f = (cat == c) && valid[e];
        }
        const uint64_t bal = __ballot(f);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = wsum[16];
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
        if (f && pos < NMS_MAX) keys[pos] = comp_key(scores[e], (uint32_t)e);
        __syncthreads();
        if (tid == 0) { int t = wsum[16]; for (int w = 0; w < 16; ++w) t += wsum[w]; wsum[16] = t; }
        __syncthreads();
    }
    int n = wsum[16];
    n = n < NMS_MAX ? n : NMS_MAX;
    // presorted: the entries of a category already come in (score desc, entry asc) order -- the RPN stage, whose entry
    // l * pre_topk + i is rank i of level l's top-k list (sorted by the same key; ties by anchor index = by i) -- so the ordered
    // compaction above IS the sorted list and the 55 barrier steps of the bitonic network are skipped
    if (!presorted) block_bitonic_sort<NMS_MAX / 1024>(keys, tid);
    nms_store_sorted(keys, n, cat_mask ? __popc(cat_mask & ((1 << c) - 1)) : c, maxc[b], boxes, S, slot, tid);
}

// Wide box inference (K > 8): the same as nms_prepare, but category c of image b reads only its own candidate list
// (written by box_candidates_wide: clist[b][c][0 .. ccnt[b][c]) = entry ids, in arrival order) instead of scanning all P * K
// entries.  The sort makes the arrival order irrelevant (the keys are distinct).  The block leaves its count at zero for the
// next forward.
__global__ __launch_bounds__(1024) void nms_prepare_list(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                         int n_total, const int* __restrict__ clist, int* __restrict__ ccnt,
                                                         int list_stride, const uint32_t* __restrict__ maxc, NmsScratch S,
                                                         int ncat) {
    __shared__ uint64_t keys[NMS_MAX];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    boxes += (size_t)b * n_total * 4;
    scores += (size_t)b * n_total;
    const size_t slot = (size_t)b * ncat + c;
    int n = ccnt[slot];
    n = n < list_stride ? n : list_stride;              // list_stride <= NMS_MAX (launcher)
    const int* src = clist + slot * list_stride;
    uint64_t k = ~0ull;
    if (tid < n) { const int e = src[tid]; k = comp_key(scores[e], (uint32_t)e); }
    keys[tid] = k;
    __syncthreads();                                    // every thread has read the count
    if (tid == 0) ccnt[slot] = 0;
    block_bitonic_sort<NMS_MAX / 1024>(keys, tid);
    nms_store_sorted(keys, n, c, maxc[b], boxes, S, slot, tid);
}

// grid (16 column chunks, 16 row chunks, ncat*B), 64 threads: thread t owns row 64*ic + t.
__global__ __launch_bounds__(64) void nms_matrix(NmsScratch S, float thr) {
    __shared__ float cb[5][64];
    const int jc = blockIdx.x, ic = blockIdx.y;
    const size_t slot = blockIdx.z;
    const int n = S.n[slot];
    if (jc < ic || 64 * ic >= n || 64 * jc >= n) return;
    const int t = threadIdx.x;
    const float* bx = S.box + slot * 4 * NMS_MAX;
    const float* ar = S.area + slot * NMS_MAX;
    const int j = 64 * jc + t;
    if (j < n) {
        cb[0][t] = bx[j]; cb[1][t] = bx[NMS_MAX + j]; cb[2][t] = bx[2 * NMS_MAX + j]; cb[3][t] = bx[3 * NMS_MAX + j];
        cb[4][t] = ar[j];
    }
    __syncthreads();
    const int i = 64 * ic + t;
    uint64_t bits = 0;
    if (i < n) {
        const float ix0 = bx[i], iy0 = bx[NMS_MAX + i], ix1 = bx[2 * NMS_MAX + i], iy1 = bx[3 * NMS_MAX + i];
        const float ia = ar[i];
        const int jend = (n - 64 * jc) < 64 ? (n - 64 * jc) : 64;
        for (int jj = 0; jj < jend; ++jj) {
            if (64 * jc + jj <= i) continue;
            const float xx0 = fmaxf(ix0, cb[0][jj]), yy0 = fmaxf(iy0, cb[1][jj]);
            const float xx1 = fminf(ix1, cb[2][jj]), yy1 = fminf(iy1, cb[3][jj]);
            const float ww = fmaxf(0.f, xx1 - xx0), hh = fmaxf(0.f, yy1 - yy0);
            const float inter = ww * hh;
            const float ovr = inter / (ia + cb[4][jj] - inter);
            if (ovr > thr) bits |= (1ull << jj);
        }
    }
    S.mask[(slot * NMS_MAX + i) * 16 + jc] = bits;
}

__device__ __forceinline__ uint64_t wave_or64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// Greedy scan, one block per (category, image).  Wave 0 resolves the 64 rows of a chunk on the
// diagonal word (scalar readlanes), then wave w ORs the kept rows' word w into the removed bitmap.
__global__ __launch_bounds__(1024) void nms_scan(NmsScratch S, int* __restrict__ keep_idx, int* __restrict__ keep_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* mask = reinterpret_cast<uint64_t*>(smem);          // [n][16]
    __shared__ uint64_t removed[16];
    __shared__ uint64_t keepbits_s;
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n[slot];
    const int nw = (n + 63) >> 6;
    const uint64_t* gm = S.mask + slot * NMS_MAX * 16;
    for (int i = tid; i < n * 16; i += 1024) {
        const int r = i >> 4, w = i & 15;
        mask[i] = (w >= (r >> 6) && w < nw) ? gm[i] : 0ull;       // lower-triangle words were never written
    }
    if (tid < 16) removed[tid] = 0;
    __syncthreads();
    int kept = 0;
    int* out = keep_idx + slot * NMS_MAX;
    const int* entry = S.entry + slot * NMS_MAX;
    for (int ch = 0; ch < nw; ++ch) {
        const int rows_here = (n - 64 * ch) < 64 ? (n - 64 * ch) : 64;
        if (wave == 0) {
            const int row = 64 * ch + lane;
            const uint64_t diag = row < n ? mask[(size_t)row * 16 + ch] : 0ull;
            uint64_t rem = removed[ch];
            uint64_t keepbits = 0;
            // visit only rows that are still alive: the next kept row is the lowest clear bit of `rem` above the
            // last one (a removed row never suppresses anything), so the loop runs once per KEPT row, not per row
            uint64_t alive = ~rem & (rows_here == 64 ? ~0ull : ((1ull << rows_here) - 1ull));
            while (alive) {
                const int r = __builtin_ctzll(alive);
                keepbits |= (1ull << r);
                rem |= readlane64(diag, r) | (1ull << r);
                alive &= ~rem;
            }
            if ((keepbits >> lane) & 1ull) out[kept + __popcll(keepbits & ((1ull << lane) - 1ull))] = entry[row];
            kept += __popcll(keepbits);
            if (lane == 0) keepbits_s = keepbits;
        }
        __syncthreads();
        if (wave > ch && wave < nw) {
            const uint64_t kb = keepbits_s;
            uint64_t v = 0;
            if (lane < rows_here && ((kb >> lane) & 1ull)) v = mask[(size_t)(64 * ch + lane) * 16 + wave];
            v = wave_or64(v);
            if (lane == 0) removed[wave] |= v;
        }
        __syncthreads();
    }
    if (tid == 0) keep_cnt[slot] = kept;
}

// Final ranking by merging: each category's kept list is already sorted by (score desc, entry asc),
// so the global rank of an element is its own position plus, for every other list, the number of
// keys that precede it (binary search).  No barriers after the load; first K ranks are written.
// Grid (image, category): every block loads all lists of its image (the searches need them) and ranks the elements of ITS
// list -- the ncat x 4 dependent binary searches of one block were 8 of this launch's 21 us at batch 1.
__global__ __launch_bounds__(1024) void rank_merge(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                   int n_total, const int* __restrict__ keep_idx,
                                                   const int* __restrict__ keep_cnt, int ncat, int K,
                                                   float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                   int* __restrict__ out_entry, int* __restrict__ out_count,
                                                   uint32_t* __restrict__ zero_word) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);      // [ncat][NMS_MAX]
    const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    if (zero_word && c == 0 && tid == 0) zero_word[b] = 0u;      // next stage's max-coordinate cell
    __shared__ int cnt[8];
    boxes += (size_t)b * n_total * 4;
    scores += (size_t)b * n_total;
    if (tid < ncat) cnt[tid] = keep_cnt[b * ncat + tid];
    __syncthreads();
    int total = 0;
    for (int o = 0; o < ncat; ++o) {
        const int* src = keep_idx + ((size_t)b * ncat + o) * NMS_MAX;
        if (tid < cnt[o]) { const int e = src[tid]; keys[o * NMS_MAX + tid] = comp_key(scores[e], (uint32_t)e); }
        total += cnt[o];
    }
    __syncthreads();
    const int nout = total < K ? total : K;
    if (tid < cnt[c]) {
        const uint64_t key = keys[c * NMS_MAX + tid];
        int rank = tid;
        for (int o = 0; o < ncat; ++o) {
            if (o == c) continue;
            int lo = 0, hi = cnt[o];
            const uint64_t* ko = keys + o * NMS_MAX;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (ko[mid] < key) lo = mid + 1; else hi = mid; }
            rank += lo;
        }
        if (rank < K) {
            const uint32_t e = (uint32_t)key;
            float* ob = out_boxes + ((size_t)b * K + rank) * 4;
            ob[0] = boxes[e * 4 + 0]; ob[1] = boxes[e * 4 + 1]; ob[2] = boxes[e * 4 + 2]; ob[3] = boxes[e * 4 + 3];
            out_scores[(size_t)b * K + rank] = scores[e];
            out_entry[(size_t)b * K + rank] = (int)e;
        }
    }
    if (c != 0) return;
    for (int i = nout + tid; i < K; i += 1024) {
        float* ob = out_boxes + ((size_t)b * K + i) * 4;
        ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
        out_scores[(size_t)b * K + i] = 0.f;
        out_entry[(size_t)b * K + i] = -1;
    }
    if (tid == 0) out_count[b] = nout;
}

// ---------------------------------------------------------------- box head post-processing
// One thread per ROI: softmax over K+1 logits, per-class box decoding (weights wx,wy,ww,wh), clip,
// score filter.  pred: [B*P][ld] with logits at [0..K] (background last) and deltas at [K+1 ..].
// Candidate slot = roi*K + class (== torch nonzero() order).
__global__ __launch_bounds__(256) void box_candidates(const float* __restrict__ pred, int ld, int K,
                                                      const float* __restrict__ props, const int* __restrict__ prop_cnt,
                                                      int P, float img_h, float img_w, float thresh, float wx, float wy,
                                                      float ww, float wh, float scale_clamp, float* __restrict__ cboxes,
                                                      float* __restrict__ cscores, int* __restrict__ cvalid,
                                                      uint32_t* __restrict__ maxc, float* __restrict__ probs_out) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P) return;
    const size_t roi = (size_t)b * P + r;
    const bool live = r < prop_cnt[b];
    const float* lg = pred + roi * ld;
    float mx = lg[0];
    for (int k = 1; k <= K; ++k) mx = fmaxf(mx, lg[k]);
    float ex[8], sum = 0.f;
    for (int k = 0; k <= K; ++k) { ex[k] = expf(lg[k] - mx); sum += ex[k]; }
    const float* pb = props + roi * 4;
    const float w = pb[2] - pb[0], h = pb[3] - pb[1];
    const float cx = pb[0] + 0.5f * w, cy = pb[1] + 0.5f * h;
    for (int k = 0; k < K; ++k) {
        const size_t slot = roi * K + k;
        const float p = ex[k] / sum;
        if (probs_out) probs_out[roi * (K + 1) + k] = p;
        const float* d = lg + (K + 1) + 4 * k;
        float dx = d[0] / wx, dy = d[1] / wy, dw = d[2] / ww, dh = d[3] / wh;
        dw = dw > scale_clamp ? scale_clamp : dw;
        dh = dh > scale_clamp ? scale_clamp : dh;
        const float pcx = dx * w + cx, pcy = dy * h + cy;
        const float pw = expf(dw) * w, ph = expf(dh) * h;
        float x0 = pcx - 0.5f * pw, y0 = pcy - 0.5f * ph, x1 = pcx + 0.5f * pw, y1 = pcy + 0.5f * ph;
        x0 = fminf(fmaxf(x0, 0.f), img_w);
        y0 = fminf(fmaxf(y0, 0.f), img_h);
        x1 = fminf(fmaxf(x1, 0.f), img_w);
        y1 = fminf(fmaxf(y1, 0.f), img_h);
        const int ok = live && (p > thresh);
        cboxes[slot * 4 + 0] = x0; cboxes[slot * 4 + 1] = y0; cboxes[slot * 4 + 2] = x1; cboxes[slot * 4 + 3] = y1;
        cscores[slot] = p;
        cvalid[slot] = ok;
        if (ok) atomicMax(maxc + b, __float_as_uint(fmaxf(fmaxf(x0, x1), fmaxf(y0, y1))));
    }
    if (probs_out) probs_out[roi * (K + 1) + K] = ex[K] / sum;
}

// Wide form (K > 8, up to 127 classes): one wave per ROI, lane l owns logits l and l + 64 (class k, or the background at k = K).
// Softmax max and sum are wave reductions (xor butterflies: every lane ends with the same bits, whatever the launch), then each
// lane decodes, clips and filters its classes exactly as box_candidates does.  Same outputs in the same layout (slot
// roi * K + k, probs_out, maxc), plus a class-major list of the passing entries: clist[b][k][pos] = r * K + k with pos from
// ccnt[b][k] (arrival order; nms_prepare_list sorts, and zeroes the counts again).
__global__ __launch_bounds__(256) void box_candidates_wide(const float* __restrict__ pred, int ld, int K,
                                                           const float* __restrict__ props, const int* __restrict__ prop_cnt,
                                                           int P, float img_h, float img_w, float thresh, float wx, float wy,
                                                           float ww, float wh, float scale_clamp, float* __restrict__ cboxes,
                                                           float* __restrict__ cscores, int* __restrict__ cvalid,
                                                           uint32_t* __restrict__ maxc, float* __restrict__ probs_out,
                                                           int* __restrict__ clist, int* __restrict__ ccnt) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= P) return;                                  // wave-uniform
    const size_t roi = (size_t)b * P + r;
    const bool live = r < prop_cnt[b];
    const float* lg = pred + roi * ld;
    const int k0 = lane, k1 = lane + 64;
    const float l0 = k0 <= K ? lg[k0] : -INFINITY, l1 = k1 <= K ? lg[k1] : -INFINITY;
    float mx = fmaxf(l0, l1);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float e0 = k0 <= K ? expf(l0 - mx) : 0.f, e1 = k1 <= K ? expf(l1 - mx) : 0.f;
    float sum = e0 + e1;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float* pb = props + roi * 4;
    const float w = pb[2] - pb[0], h = pb[3] - pb[1];
    const float cx = pb[0] + 0.5f * w, cy = pb[1] + 0.5f * h;
    uint32_t m = 0u;
    bool any = false;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int k = half ? k1 : k0;
        const float ex = half ? e1 : e0;
        if (k > K) continue;
        const float p = ex / sum;
        if (probs_out) probs_out[roi * (K + 1) + k] = p;
        if (k == K) continue;                            // background: probability only
        const size_t slot = roi * K + k;
        const float* d = lg + (K + 1) + 4 * k;
        float dx = d[0] / wx, dy = d[1] / wy, dw = d[2] / ww, dh = d[3] / wh;
        dw = dw > scale_clamp ? scale_clamp : dw;
        dh = dh > scale_clamp ? scale_clamp : dh;
        const float pcx = dx * w + cx, pcy = dy * h + cy;
        const float pw = expf(dw) * w, ph = expf(dh) * h;
        float x0 = pcx - 0.5f * pw, y0 = pcy - 0.5f * ph, x1 = pcx + 0.5f * pw, y1 = pcy + 0.5f * ph;
        x0 = fminf(fmaxf(x0, 0.f), img_w);
        y0 = fminf(fmaxf(y0, 0.f), img_h);
        x1 = fminf(fmaxf(x1, 0.f), img_w);
        y1 = fminf(fmaxf(y1, 0.f), img_h);
        const int ok = live && (p > thresh);
        cboxes[slot * 4 + 0] = x0; cboxes[slot * 4 + 1] = y0; cboxes[slot * 4 + 2] = x1; cboxes[slot * 4 + 3] = y1;
        cscores[slot] = p;
        cvalid[slot] = ok;
        if (ok) {
            const uint32_t mk = __float_as_uint(fmaxf(fmaxf(x0, x1), fmaxf(y0, y1)));   // >= 0 after the clip: uint order = float order
            m = mk > m ? mk : m;
            any = true;
            const size_t ci = (size_t)b * K + k;
            const int pos = atomicAdd(ccnt + ci, 1);     // < P: one entry per ROI and class
            if (pos < P) clist[ci * P + pos] = r * K + k;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = __shfl_xor(m, o);
        m = t > m ? t : m;
    }
    if (__ballot(any) && lane == 0) atomicMax(maxc + b, m);
}

// Final top-`K` of the wide box inference (any number of categories up to 128): each category's kept list is sorted by (score desc, entry
// asc), so only its first K entries can reach the output.  One block per image loads at most ncat * K keys (<= 8000 for 80
// classes and 100 detections), pads them to the next power of two of 1024 .. 8192 and sorts them in LDS; the first
// min(total kept, K) keys are the output, in the order and layout of rank_merge (zero-filled tail, entry -1).
__global__ __launch_bounds__(1024) void rank_sort_wide(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                       int n_total, const int* __restrict__ keep_idx,
                                                       const int* __restrict__ keep_cnt, int ncat, int K,
                                                       float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                       int* __restrict__ out_entry, int* __restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);      // [<= 8192]
    __shared__ int cnt[128], beg[129];
    const int b = blockIdx.x, tid = threadIdx.x;
    boxes += (size_t)b * n_total * 4;
    scores += (size_t)b * n_total;
    if (tid < ncat) cnt[tid] = keep_cnt[b * ncat + tid];
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int o = 0; o < ncat; ++o) { beg[o] = t; t += cnt[o] < K ? cnt[o] : K; }
        beg[ncat] = t;
    }
    __syncthreads();
    int total = 0;
    for (int o = 0; o < ncat; ++o) total += cnt[o];
    const int nload = beg[ncat];                             // <= ncat * K <= 8192 (checked by the launcher)
    const int N = nload <= 1024 ? 1024 : nload <= 2048 ? 2048 : nload <= 4096 ? 4096 : 8192;
    for (int i = tid; i < N; i += 1024) keys[i] = ~0ull;
    __syncthreads();
    // wave w loads categories w, w + 16, ..: lanes over the entries of one category
    for (int o = tid >> 6; o < ncat; o += 16) {
        const int n = beg[o + 1] - beg[o];
        const int* src = keep_idx + ((size_t)b * ncat + o) * NMS_MAX;
        for (int i = tid & 63; i < n; i += 64) { const int e = src[i]; keys[beg[o] + i] = comp_key(scores[e], (uint32_t)e); }
    }
    __syncthreads();
    if (N == 1024) block_bitonic_sort<1>(keys, tid);
    else if (N == 2048) block_bitonic_sort<2>(keys, tid);
    else if (N == 4096) block_bitonic_sort<4>(keys, tid);
    else block_bitonic_sort<8>(keys, tid);
    const int nout = total < K ? total : K;
    for (int i = tid; i < K; i += 1024) {
        float* ob = out_boxes + ((size_t)b * K + i) * 4;
        if (i < nout) {
            const uint32_t e = (uint32_t)keys[i];
            ob[0] = boxes[e * 4 + 0]; ob[1] = boxes[e * 4 + 1]; ob[2] = boxes[e * 4 + 2]; ob[3] = boxes[e * 4 + 3];
            out_scores[(size_t)b * K + i] = scores[e];
            out_entry[(size_t)b * K + i] = (int)e;
        } else {
            ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
            out_scores[(size_t)b * K + i] = 0.f;
            out_entry[(size_t)b * K + i] = -1;
        }
    }
    if (tid == 0) out_count[b] = nout;
}

// ---------------------------------------------------------------- C4: single-level RPN selection and long-list NMS
// detectron2's C4 RPN (Res5ROIHeads models) runs on one stride-16 map with 15 anchors per cell and keeps the top
// PRE_NMS_TOPK_TEST = 6000 logits of up to H * W * 15 (59220 at 47 x 84) before an NMS over that one list.  The FPN
// tournament (4096-key chunks, 1024-slot lists) and the 1024-box NMS slots do not reach that far, so this path has its own:
//   c4_rpn_select : one block per image.  Radix select of the k-th smallest composite key (comp_key: score descending,
//                   anchor index ascending -- distinct keys, so "key <= kth" is exactly k elements), compaction of those
//                   k into LDS, one bitonic sort of <= 8192 keys, then Box2BoxTransform decode + clip + nonempty flag.
//   c4_nms_prepare: ordered compaction of the valid decoded boxes (they arrive sorted) into the long NMS slot.
//   c4_nms_matrix : 64 x 64 tiles of the suppression bit matrix (the same IoU arithmetic as nms_matrix).
//   c4_nms_scan   : greedy scan, 64 rows per step, the bit matrix read from HBM; stops once post_topk boxes are kept
//                   (keep[:post_topk] of the full scan), then writes the proposals.
#define C4_SORT_N 8192      // keys sorted in LDS per image (>= rpn_pre_topk <= 6000)
#define C4_NMS_MAX 6144     // boxes of the long NMS slot (>= 6000)
#define C4_NMS_WORDS (C4_NMS_MAX / 64)


__global__ __launch_bounds__(1024) void c4_rpn_select(const C4Rpn R, float img_h, float img_w, float scale_clamp,
                                                     float* __restrict__ boxes, float* __restrict__ scores,
                                                     int* __restrict__ valid, int pre) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* a = reinterpret_cast<uint64_t*>(smem);                    // [C4_SORT_N]
    unsigned* hist = reinterpret_cast<unsigned*>(smem + C4_SORT_N * 8);  // [16 waves][256]
    __shared__ uint64_t prefix_s;
    __shared__ unsigned rank_s, fill_s;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const float* head = R.head + (size_t)b * R.H * R.W * R.ld;
    const int n = R.n, k = R.k;
    auto key_of = [&](int e) -> uint64_t {
        const int pix = e / 15, an = e - pix * 15;
        return comp_key(head[(size_t)pix * R.ld + an], (uint32_t)e);
    };
    // radix select, 8 bits per pass from the top: after pass p the top 8 (p + 1) bits of the k-th smallest key are known
    if (tid == 0) { prefix_s = 0; rank_s = (unsigned)(k - 1); }
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int i = tid; i < 16 * 256; i += 1024) hist[i] = 0u;
        __syncthreads();
        const uint64_t prefix = prefix_s;
        for (int e = tid; e < n; e += 1024) {
            const uint64_t key = key_of(e);
            if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[wave * 256 + (int)((key >> shift) & 255u)], 1u);
        }
        __syncthreads();
        if (tid < 256) {
            unsigned t = 0;
            for (int w = 0; w < 16; ++w) t += hist[w * 256 + tid];
            hist[tid] = t;                                                 // wave 0's row now holds the totals
        }
        __syncthreads();
        if (tid == 0) {
            unsigned r = rank_s;
            int d = 0;
            for (; d < 255 && r >= hist[d]; ++d) r -= hist[d];
            rank_s = r;
            prefix_s = prefix | ((uint64_t)d << shift);
            fill_s = 0u;
        }
        __syncthreads();
    }
    const uint64_t kth = prefix_s;
    for (int i = tid; i < C4_SORT_N; i += 1024) a[i] = ~0ull;
    __syncthreads();
    for (int e = tid; e < n; e += 1024) {
        const uint64_t key = key_of(e);
        if (key <= kth) a[atomicAdd(&fill_s, 1u)] = key;                   // exactly k keys (distinct keys)
    }
    __syncthreads();
    block_bitonic_sort<C4_SORT_N / 1024>(a, tid);
    for (int i = tid; i < pre; i += 1024) {
        const size_t o = (size_t)b * pre + i;
        if (i >= k) { valid[o] = 0; scores[o] = 0.f; continue; }
        const uint64_t key = a[i];
        const uint32_t e = (uint32_t)key;
        const int pix = e / 15, an = e - pix * 15;
        const int y = pix / R.W, x = pix - y * R.W;
        const float sx = (float)(x * R.stride), sy = (float)(y * R.stride);
        const float ax0 = sx + R.base[an][0], ay0 = sy + R.base[an][1];
        const float ax1 = sx + R.base[an][2], ay1 = sy + R.base[an][3];
        const float* d = head + (size_t)pix * R.ld + 15 + an * 4;
        const float w = ax1 - ax0, h = ay1 - ay0;
        const float cx = ax0 + 0.5f * w, cy = ay0 + 0.5f * h;
        float dx = d[0] / 1.0f, dy = d[1] / 1.0f, dw = d[2] / 1.0f, dh = d[3] / 1.0f;
        dw = dw > scale_clamp ? scale_clamp : dw;
        dh = dh > scale_clamp ? scale_clamp : dh;
        const float pcx = dx * w + cx, pcy = dy * h + cy;
        const float pw = expf(dw) * w, ph = expf(dh) * h;
        float x0 = pcx - 0.5f * pw, y0 = pcy - 0.5f * ph, x1 = pcx + 0.5f * pw, y1 = pcy + 0.5f * ph;
        x0 = fminf(fmaxf(x0, 0.f), img_w);
        y0 = fminf(fmaxf(y0, 0.f), img_h);
        x1 = fminf(fmaxf(x1, 0.f), img_w);
        y1 = fminf(fmaxf(y1, 0.f), img_h);
        boxes[o * 4 + 0] = x0; boxes[o * 4 + 1] = y0; boxes[o * 4 + 2] = x1; boxes[o * 4 + 3] = y1;
        scores[o] = comp_score(key);
        valid[o] = ((x1 - x0) > 0.f) && ((y1 - y0) > 0.f);
    }
}

// One long NMS slot per image: box [4][C4_NMS_MAX], area, entry, n; mask [C4_NMS_MAX][C4_NMS_WORDS] u64.
struct C4Nms { float* box; float* area; int* entry; int* n; uint64_t* mask; };

// The decoded list is in (score desc, anchor asc) order already; the valid boxes keep that order (a single category: the
// batched_nms offset is 0 * (max + 1) = 0, so the boxes go in unshifted).
__global__ __launch_bounds__(1024) void c4_nms_prepare(const float* __restrict__ boxes, const int* __restrict__ valid, int pre,
                                                      C4Nms S) {
    __shared__ int wsum[17];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    boxes += (size_t)b * pre * 4;
    valid += (size_t)b * pre;
    float* bx = S.box + (size_t)b * 4 * C4_NMS_MAX;
    if (tid == 0) wsum[16] = 0;
    __syncthreads();
    for (int base = 0; base < pre; base += 1024) {
        const int e = base + tid;
        const bool f = e < pre && valid[e];
        const uint64_t bal = __ballot(f);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = wsum[16];
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
        if (f && pos < C4_NMS_MAX) {
            const float x0 = boxes[e * 4 + 0], y0 = boxes[e * 4 + 1], x1 = boxes[e * 4 + 2], y1 = boxes[e * 4 + 3];
            bx[pos] = x0; bx[C4_NMS_MAX + pos] = y0; bx[2 * C4_NMS_MAX + pos] = x1; bx[3 * C4_NMS_MAX + pos] = y1;
            S.area[(size_t)b * C4_NMS_MAX + pos] = (x1 - x0) * (y1 - y0);
            S.entry[(size_t)b * C4_NMS_MAX + pos] = e;
        }
        __syncthreads();
        if (tid == 0) { int t = wsum[16]; for (int w = 0; w < 16; ++w) t += wsum[w]; wsum[16] = t; }
        __syncthreads();
    }
    if (tid == 0) S.n[b] = wsum[16] < C4_NMS_MAX ? wsum[16] : C4_NMS_MAX;
}

// grid (C4_NMS_WORDS column chunks, C4_NMS_WORDS row chunks, B), 64 threads: thread t owns row 64 * ic + t.
__global__ __launch_bounds__(64) void c4_nms_matrix(C4Nms S, float thr) {
    __shared__ float cb[5][64];
    const int jc = blockIdx.x, ic = blockIdx.y, b = blockIdx.z;
    const int n = S.n[b];
    if (jc < ic || 64 * ic >= n || 64 * jc >= n) return;
    const int t = threadIdx.x;
    const float* bx = S.box + (size_t)b * 4 * C4_NMS_MAX;
    const float* ar = S.area + (size_t)b * C4_NMS_MAX;
    const int j = 64 * jc + t;
    if (j < n) {
        cb[0][t] = bx[j]; cb[1][t] = bx[C4_NMS_MAX + j]; cb[2][t] = bx[2 * C4_NMS_MAX + j]; cb[3][t] = bx[3 * C4_NMS_MAX + j];
        cb[4][t] = ar[j];
    }
    __syncthreads();
    const int i = 64 * ic + t;
    if (i >= n) return;
    uint64_t bits = 0;
    const float ix0 = bx[i], iy0 = bx[C4_NMS_MAX + i], ix1 = bx[2 * C4_NMS_MAX + i], iy1 = bx[3 * C4_NMS_MAX + i];
    const float ia = ar[i];
    const int jend = (n - 64 * jc) < 64 ? (n - 64 * jc) : 64;
    for (int jj = 0; jj < jend; ++jj) {
        if (64 * jc + jj <= i) continue;
        const float xx0 = fmaxf(ix0, cb[0][jj]), yy0 = fmaxf(iy0, cb[1][jj]);
        const float xx1 = fminf(ix1, cb[2][jj]), yy1 = fminf(iy1, cb[3][jj]);
        const float ww = fmaxf(0.f, xx1 - xx0), hh = fmaxf(0.f, yy1 - yy0);
        const float inter = ww * hh;
        const float ovr = inter / (ia + cb[4][jj] - inter);
        if (ovr > thr) bits |= (1ull << jj);
    }
    S.mask[((size_t)b * C4_NMS_MAX + i) * C4_NMS_WORDS + jc] = bits;
}

// Greedy scan, one block per image.  Wave 0 resolves the 64 rows of a chunk on the diagonal word; then the waves OR the kept
// rows' words right of the diagonal into the removed bitmap.  The scan ends as soon as `post` rows are kept: the kept list is in
// processing order, so that is keep[:post] of the full scan.  Output: proposals [B][post] (boxes, scores, entry = rank in the
// decoded list; zeros and -1 past the count) and the per-image count.
__global__ __launch_bounds__(1024) void c4_nms_scan(C4Nms S, const float* __restrict__ dboxes, const float* __restrict__ dscores,
                                                   int pre, int post, float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                   int* __restrict__ out_entry, int* __restrict__ out_count) {
    __shared__ uint64_t removed[C4_NMS_WORDS];
    __shared__ uint64_t keepbits_s;
    __shared__ int kept_s;
    __shared__ int keep[1024];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n[b];
    const int nw = (n + 63) >> 6;
    const uint64_t* gm = S.mask + (size_t)b * C4_NMS_MAX * C4_NMS_WORDS;
    const int* entry = S.entry + (size_t)b * C4_NMS_MAX;
    for (int i = tid; i < C4_NMS_WORDS; i += 1024) removed[i] = 0ull;
    if (tid == 0) kept_s = 0;
    __syncthreads();
    int kept = 0;                                   // wave 0's running count
    for (int ch = 0; ch < nw; ++ch) {
        const int rows_here = (n - 64 * ch) < 64 ? (n - 64 * ch) : 64;
        if (wave == 0) {
            const int row = 64 * ch + lane;
            const uint64_t diag = row < n ? gm[(size_t)row * C4_NMS_WORDS + ch] : 0ull;
            uint64_t rem = removed[ch];
            uint64_t keepbits = 0;
            uint64_t alive = ~rem & (rows_here == 64 ? ~0ull : ((1ull << rows_here) - 1ull));
            while (alive) {
                const int r = __builtin_ctzll(alive);
                keepbits |= (1ull << r);
                rem |= readlane64(diag, r) | (1ull << r);
                alive &= ~rem;
            }
            const int pos = kept + __popcll(keepbits & ((1ull << lane) - 1ull));
            if (((keepbits >> lane) & 1ull) && pos < post) keep[pos] = entry[row];
            kept += __popcll(keepbits);
            if (lane == 0) { keepbits_s = keepbits; kept_s = kept; }
        }
        __syncthreads();
        if (kept_s >= post) break;                  // block-uniform
        const uint64_t kb = keepbits_s;
        for (int w = ch + 1 + wave; w < nw; w += 16) {
            uint64_t v = 0;
            if (lane < rows_here && ((kb >> lane) & 1ull)) v = gm[(size_t)(64 * ch + lane) * C4_NMS_WORDS + w];
            v = wave_or64(v);
            if (lane == 0) removed[w] |= v;
        }
        __syncthreads();
    }
    const int cnt = kept_s < post ? kept_s : post;
    dboxes += (size_t)b * pre * 4;
    dscores += (size_t)b * pre;
    for (int i = tid; i < post; i += 1024) {
        float* ob = out_boxes + ((size_t)b * post + i) * 4;
        if (i < cnt) {
            const int e = keep[i];
            ob[0] = dboxes[e * 4 + 0]; ob[1] = dboxes[e * 4 + 1]; ob[2] = dboxes[e * 4 + 2]; ob[3] = dboxes[e * 4 + 3];
            out_scores[(size_t)b * post + i] = dscores[e];
            out_entry[(size_t)b * post + i] = e;
        } else {
            ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
            out_scores[(size_t)b * post + i] = 0.f;
            out_entry[(size_t)b * post + i] = -1;
        }
    }
    if (tid == 0) out_count[b] = cnt;
}

// ---------------------------------------------------------------- training-time FPN selection
// find_top_rpn_proposals with the training limits (PRE_NMS_TOPK_TRAIN 2000 per level, POST_NMS_TOPK_TRAIN 1000): the rules of the
// FPN path above, but lists of up to TR_MAX = 2048 keys per (level, image), which the 1024-slot tournament lists, the 1024-box
// NMS slot and the 64 KiB rank merge do not hold.  One slot per (level, image), slot = image * 5 + level:
//   train_rpn_select : one block per slot.  A level of more than TR_MAX anchors: radix select of the k-th smallest composite
//                      key, as c4_rpn_select does, leaving as soon as the remaining bin is wholly inside the top k (random
//                      scores: after the four score bytes); then one bitonic sort of <= 2048 keys in LDS, the key list, and
//                      rpn_decode's arithmetic on the sorted anchors (decode, clip, nonempty flag, running max coordinate).
//   train_nms_prepare: ordered compaction of the slot's valid boxes (they arrive sorted), shifted by cat * (max_coord + 1).
//   train_nms_matrix : 64 x 64 tiles of the suppression bit matrix in HBM, [2048][32] u64 per slot (nms_matrix's arithmetic).
//   train_nms_scan   : greedy scan per slot; stops once post_topk rows are kept (an element behind post_topk others of its own
//                      sorted list has a merged rank >= post_topk, so the merge below never sees it).
//   train_rank_merge : rank merge over the five kept lists (80 KiB of keys in LDS), first post_topk.
// The FPN and C4 kernels above are not touched by this path.
#define TR_MAX 2048         // keys of a level's list and boxes of an NMS slot (APSE_RPN_TRAIN_MAX_PRE_TOPK, include/apse_hip.h)
#define TR_WORDS (TR_MAX / 64)

__global__ __launch_bounds__(1024) void train_rpn_select(const RpnLevels L, float img_h, float img_w, float scale_clamp,
                                                        uint64_t* __restrict__ keys_out, float* __restrict__ boxes,
                                                        float* __restrict__ scores, int* __restrict__ valid,
                                                        uint32_t* __restrict__ maxc, int level_mask) {
    __shared__ uint64_t a[TR_MAX];
    __shared__ unsigned hist[16 * 256];                                  // [16 waves][256]
    __shared__ uint64_t prefix_s;
    __shared__ unsigned rank_s, fill_s;
    __shared__ int done_s;
    const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const RpnLevel& lv = L.lv[l];
    const int head_ld = L.head_ld, pre = L.pre_topk;
    const float* head = lv.head + (size_t)b * lv.H * lv.W * head_ld;
    const int n = lv.n, k = lv.k;
    auto key_of = [&](int e) -> uint64_t {
        const int pix = e / 3, an = e - pix * 3;
        return comp_key(head[(size_t)pix * head_ld + an], (uint32_t)e);
    };
    if (tid == 0) { prefix_s = ~0ull; rank_s = (unsigned)(k - 1); fill_s = 0u; done_s = 0; }
    __syncthreads();
    // radix select, 8 bits per pass from the top.  The keys are distinct, so the last pass always ends with one key in the bin
    for (int pass = 0; pass < 8 && n > TR_MAX; ++pass) {
        const int shift = 56 - 8 * pass;
        const uint64_t prefix = pass == 0 ? 0ull : prefix_s;
        for (int i = tid; i < 16 * 256; i += 1024) hist[i] = 0u;
        __syncthreads();
        for (int e = tid; e < n; e += 1024) {
            const uint64_t key = key_of(e);
            if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[wave * 256 + (int)((key >> shift) & 255u)], 1u);
        }
        __syncthreads();
        if (tid < 256) {
            unsigned t = 0;
            for (int w = 0; w < 16; ++w) t += hist[w * 256 + tid];
            hist[tid] = t;                                                 // wave 0's row now holds the totals
        }
        __syncthreads();
        if (tid == 0) {
            unsigned r = rank_s;
            int d = 0;
            for (; d < 255 && r >= hist[d]; ++d) r -= hist[d];
            rank_s = r;
            const uint64_t p = prefix | ((uint64_t)d << shift);
            // the whole bin is inside the top k: every key up to the bin's last possible one is selected
            if (r + 1u == hist[d]) { prefix_s = p | ((1ull << shift) - 1ull); done_s = 1; }
            else prefix_s = p;
        }
        __syncthreads();
        if (done_s) break;                                                 // block-uniform
    }
    const uint64_t kth = prefix_s;                                         // all ones for a level that fits the list whole
    for (int i = tid; i < TR_MAX; i += 1024) a[i] = ~0ull;
    __syncthreads();
    for (int e = tid; e < n; e += 1024) {
        const uint64_t key = key_of(e);
        if (key <= kth) { const unsigned pos = atomicAdd(&fill_s, 1u); if (pos < TR_MAX) a[pos] = key; }      // exactly k keys
    }
    __syncthreads();
    block_bitonic_sort<TR_MAX / 1024>(a, tid);
    const bool on = (level_mask >> l) & 1;
    for (int i = tid; i < pre; i += 1024) {
        const size_t o = (size_t)b * 5 * pre + (size_t)l * pre + i;
        if (keys_out) keys_out[o] = i < k ? a[i] : ~0ull;
        if (i >= k || !on) { valid[o] = 0; scores[o] = 0.f; continue; }
        const uint64_t key = a[i];
        const uint32_t e = (uint32_t)key;
        const float sc = comp_score(key);
        const int pix = e / 3, an = e - pix * 3;
        const int y = pix / lv.W, x = pix - y * lv.W;
        const float sx = (float)(x * lv.stride), sy = (float)(y * lv.stride);
        const float ax0 = sx + lv.base[an][0], ay0 = sy + lv.base[an][1];
        const float ax1 = sx + lv.base[an][2], ay1 = sy + lv.base[an][3];
        const float* d = head + (size_t)pix * head_ld + 3 + an * 4;
        const float w = ax1 - ax0, h = ay1 - ay0;
        const float cx = ax0 + 0.5f * w, cy = ay0 + 0.5f * h;
        float dx = d[0] / 1.0f, dy = d[1] / 1.0f, dw = d[2] / 1.0f, dh = d[3] / 1.0f;
        dw = dw > scale_clamp ? scale_clamp : dw;
        dh = dh > scale_clamp ? scale_clamp : dh;
        const float pcx = dx * w + cx, pcy = dy * h + cy;
        const float pw = expf(dw) * w, ph = expf(dh) * h;
        float x0 = pcx - 0.5f * pw, y0 = pcy - 0.5f * ph, x1 = pcx + 0.5f * pw, y1 = pcy + 0.5f * ph;
        x0 = fminf(fmaxf(x0, 0.f), img_w);
        y0 = fminf(fmaxf(y0, 0.f), img_h);
        x1 = fminf(fmaxf(x1, 0.f), img_w);
        y1 = fminf(fmaxf(y1, 0.f), img_h);
        const int ok = ((x1 - x0) > 0.f) && ((y1 - y0) > 0.f);
        boxes[o * 4 + 0] = x0; boxes[o * 4 + 1] = y0; boxes[o * 4 + 2] = x1; boxes[o * 4 + 3] = y1;
        scores[o] = sc;
        valid[o] = ok;
        if (ok) {
            const float m = fmaxf(fmaxf(x0, x1), fmaxf(y0, y1));   // all >= 0 after the clip
            atomicMax(maxc + b, __float_as_uint(m));
        }
    }
}

// Per slot: box [4][TR_MAX] (shifted), area, entry, n; mask [TR_MAX][TR_WORDS] u64; keep [TR_MAX] and its count.
struct TrainNms { float* box; float* area; int* entry; int* n; uint64_t* mask; int* keep; int* keep_cnt; };

// grid (5, B).  Level l's entries l * pre .. l * pre + pre - 1 are in (score desc, anchor asc) order already; the valid ones
// keep it.  The category of a level is its rank among the levels of the mask (torchvision numbers the categories it is given).
__global__ __launch_bounds__(1024) void train_nms_prepare(const float* __restrict__ boxes, const int* __restrict__ valid, int pre,
                                                         const uint32_t* __restrict__ maxc, int level_mask, TrainNms S) {
    __shared__ int wsum[17];
    const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t slot = (size_t)b * 5 + l;
    boxes += (size_t)b * 5 * pre * 4;
    valid += (size_t)b * 5 * pre;
    const float off = (float)__popc(level_mask & ((1 << l) - 1)) * (__uint_as_float(maxc[b]) + 1.0f);
    float* bx = S.box + slot * 4 * TR_MAX;
    if (tid == 0) wsum[16] = 0;
    __syncthreads();
    for (int base = 0; base < pre; base += 1024) {
        const int i = base + tid, e = l * pre + i;
        const bool f = i < pre && valid[e];
        const uint64_t bal = __ballot(f);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int o = wsum[16];
        for (int w = 0; w < wave; ++w) o += wsum[w];
        const int pos = o + __popcll(bal & ((1ull << lane) - 1ull));
        if (f && pos < TR_MAX) {
            const float x0 = boxes[e * 4 + 0] + off, y0 = boxes[e * 4 + 1] + off;
            const float x1 = boxes[e * 4 + 2] + off, y1 = boxes[e * 4 + 3] + off;
            bx[pos] = x0; bx[TR_MAX + pos] = y0; bx[2 * TR_MAX + pos] = x1; bx[3 * TR_MAX + pos] = y1;
            S.area[slot * TR_MAX + pos] = (x1 - x0) * (y1 - y0);
            S.entry[slot * TR_MAX + pos] = e;
        }
        __syncthreads();
        if (tid == 0) { int t = wsum[16]; for (int w = 0; w < 16; ++w) t += wsum[w]; wsum[16] = t; }
        __syncthreads();
    }
    if (tid == 0) S.n[slot] = wsum[16] < TR_MAX ? wsum[16] : TR_MAX;
}

// grid (TR_WORDS column chunks, TR_WORDS row chunks, 5 B), 64 threads: thread t owns row 64 * ic + t.
__global__ __launch_bounds__(64) void train_nms_matrix(TrainNms S, float thr) {
    __shared__ float cb[5][64];
    const int jc = blockIdx.x, ic = blockIdx.y;
    const size_t slot = blockIdx.z;
    const int n = S.n[slot];
    if (jc < ic || 64 * ic >= n || 64 * jc >= n) return;
    const int t = threadIdx.x;
    const float* bx = S.box + slot * 4 * TR_MAX;
    const float* ar = S.area + slot * TR_MAX;
    const int j = 64 * jc + t;
    if (j < n) {
        cb[0][t] = bx[j]; cb[1][t] = bx[TR_MAX + j]; cb[2][t] = bx[2 * TR_MAX + j]; cb[3][t] = bx[3 * TR_MAX + j];
        cb[4][t] = ar[j];
    }
    __syncthreads();
    const int i = 64 * ic + t;
    if (i >= n) return;
    uint64_t bits = 0;
    const float ix0 = bx[i], iy0 = bx[TR_MAX + i], ix1 = bx[2 * TR_MAX + i], iy1 = bx[3 * TR_MAX + i];
    const float ia = ar[i];
    const int jend = (n - 64 * jc) < 64 ? (n - 64 * jc) : 64;
    for (int jj = 0; jj < jend; ++jj) {
        if (64 * jc + jj <= i) continue;
        const float xx0 = fmaxf(ix0, cb[0][jj]), yy0 = fmaxf(iy0, cb[1][jj]);
        const float xx1 = fminf(ix1, cb[2][jj]), yy1 = fminf(iy1, cb[3][jj]);
        const float ww = fmaxf(0.f, xx1 - xx0), hh = fmaxf(0.f, yy1 - yy0);
        const float inter = ww * hh;
        const float ovr = inter / (ia + cb[4][jj] - inter);
        if (ovr > thr) bits |= (1ull << jj);
    }
    S.mask[(slot * TR_MAX + i) * TR_WORDS + jc] = bits;
}

// Greedy scan, grid (5, B), the bit matrix read from HBM (only words on and right of the diagonal of rows < n: those the matrix
// kernel wrote).  Kept entries in processing order -> keep [slot][TR_MAX], at most `post` of them.
__global__ __launch_bounds__(1024) void train_nms_scan(TrainNms S, int post) {
    __shared__ uint64_t removed[TR_WORDS];
    __shared__ uint64_t keepbits_s;
    __shared__ int kept_s;
    const size_t slot = (size_t)blockIdx.y * 5 + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n[slot];
    const int nw = (n + 63) >> 6;
    const uint64_t* gm = S.mask + slot * TR_MAX * TR_WORDS;
    const int* entry = S.entry + slot * TR_MAX;
    int* keep = S.keep + slot * TR_MAX;
    if (tid < TR_WORDS) removed[tid] = 0ull;
    if (tid == 0) kept_s = 0;
    __syncthreads();
    int kept = 0;                                   // wave 0's running count
    for (int ch = 0; ch < nw; ++ch) {
        const int rows_here = (n - 64 * ch) < 64 ? (n - 64 * ch) : 64;
        if (wave == 0) {
            const int row = 64 * ch + lane;
            const uint64_t diag = row < n ? gm[(size_t)row * TR_WORDS + ch] : 0ull;
            uint64_t rem = removed[ch];
            uint64_t keepbits = 0;
            uint64_t alive = ~rem & (rows_here == 64 ? ~0ull : ((1ull << rows_here) - 1ull));
            while (alive) {
                const int r = __builtin_ctzll(alive);
                keepbits |= (1ull << r);
                rem |= readlane64(diag, r) | (1ull << r);
                alive &= ~rem;
            }
            const int pos = kept + __popcll(keepbits & ((1ull << lane) - 1ull));
            if (((keepbits >> lane) & 1ull) && pos < post) keep[pos] = entry[row];
            kept += __popcll(keepbits);
            if (lane == 0) { keepbits_s = keepbits; kept_s = kept; }
        }
        __syncthreads();
        if (kept_s >= post) break;                  // block-uniform
        const uint64_t kb = keepbits_s;
        for (int w = ch + 1 + wave; w < nw; w += 16) {
            uint64_t v = 0;
            if (lane < rows_here && ((kb >> lane) & 1ull)) v = gm[(size_t)(64 * ch + lane) * TR_WORDS + w];
            v = wave_or64(v);
            if (lane == 0) removed[w] |= v;
        }
        __syncthreads();
    }
    if (tid == 0) S.keep_cnt[slot] = kept_s < post ? kept_s : post;
}

// rank_merge over five lists of up to TR_MAX keys: grid (image, level), every block loads the five lists of its image and ranks
// the elements of its own (position + binary-search counts in the other four).  K <= TR_MAX.
__global__ __launch_bounds__(1024) void train_rank_merge(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                        int n_total, TrainNms S, int K, float* __restrict__ out_boxes,
                                                        float* __restrict__ out_scores, int* __restrict__ out_entry,
                                                        int* __restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);      // [5][TR_MAX]
    __shared__ int cnt[5];
    const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    boxes += (size_t)b * n_total * 4;
    scores += (size_t)b * n_total;
    if (tid < 5) cnt[tid] = S.keep_cnt[b * 5 + tid];
    __syncthreads();
    int total = 0;
    for (int o = 0; o < 5; ++o) {
        const int* src = S.keep + ((size_t)b * 5 + o) * TR_MAX;
        for (int i = tid; i < cnt[o]; i += 1024) { const int e = src[i]; keys[o * TR_MAX + i] = comp_key(scores[e], (uint32_t)e); }
        total += cnt[o];
    }
    __syncthreads();
    const int nout = total < K ? total : K;
    for (int i = tid; i < cnt[c]; i += 1024) {
        const uint64_t key = keys[c * TR_MAX + i];
        int rank = i;
        for (int o = 0; o < 5; ++o) {
            if (o == c) continue;
            int lo = 0, hi = cnt[o];
            const uint64_t* ko = keys + o * TR_MAX;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (ko[mid] < key) lo = mid + 1; else hi = mid; }
            rank += lo;
        }
        if (rank < K) {
            const uint32_t e = (uint32_t)key;
            float* ob = out_boxes + ((size_t)b * K + rank) * 4;
            ob[0] = boxes[e * 4 + 0]; ob[1] = boxes[e * 4 + 1]; ob[2] = boxes[e * 4 + 2]; ob[3] = boxes[e * 4 + 3];
            out_scores[(size_t)b * K + rank] = scores[e];
            out_entry[(size_t)b * K + rank] = (int)e;
        }
    }
    if (c != 0) return;
    for (int i = nout + tid; i < K; i += 1024) {
        float* ob = out_boxes + ((size_t)b * K + i) * 4;
        ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
        out_scores[(size_t)b * K + i] = 0.f;
        out_entry[(size_t)b * K + i] = -1;
    }
    if (tid == 0) out_count[b] = nout;
}

// Pack per-image detections into one dense list (image id kept per entry) so the mask tail's
// GEMMs see a contiguous M.  det_* are [B][Kd]; packed_* are [B*Kd].
__global__ void pack_detections(const float* __restrict__ det_boxes, const float* __restrict__ det_scores,
                                const int* __restrict__ det_entry, const int* __restrict__ det_cnt, int B, int Kd,
                                int ncls, float* __restrict__ pk_boxes, float* __restrict__ pk_scores,
                                int* __restrict__ pk_cls, int* __restrict__ pk_img, int* __restrict__ pk_roi,
                                int* __restrict__ pk_total, int* __restrict__ pk_offset,
                                unsigned long long* __restrict__ zero_sums) {
    __shared__ int offs[65];
    // the mask tail's per-detection integer sums (paste_masks adds into them)
    if (zero_sums) for (int i = threadIdx.x; i < B * Kd * 3; i += blockDim.x) zero_sums[i] = 0ull;
    if (threadIdx.x == 0) {
        int t = 0;
        for (int b = 0; b < B; ++b) { offs[b] = t; pk_offset[b] = t; t += det_cnt[b]; }
        offs[B] = t;
        pk_offset[B] = t;
        *pk_total = t;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B * Kd; i += blockDim.x) {
        const int b = i / Kd, k = i - b * Kd;
        if (k < det_cnt[b]) {
            const int o = offs[b] + k;
            const float* s = det_boxes + (size_t)i * 4;
            pk_boxes[o * 4 + 0] = s[0]; pk_boxes[o * 4 + 1] = s[1]; pk_boxes[o * 4 + 2] = s[2]; pk_boxes[o * 4 + 3] = s[3];
            pk_scores[o] = det_scores[i];
            const int e = det_entry[i];
            pk_cls[o] = e % ncls;
            pk_roi[o] = e / ncls;
            pk_img[o] = b;
        }
    }
}

extern "C" {
int apse_k_rpn_topk_stage(const RpnLevels* L_dev, const TopkJob* jobs_dev, int njobs, uint64_t* lists, int nslots, int B,
                          uint32_t* zero_word, hipStream_t s) {
    if (njobs <= 0) return APSE_OK;
    hipLaunchKernelGGL(rpn_topk_stage, dim3(njobs, B), dim3(1024), 0, s, L_dev, jobs_dev, lists, nslots, zero_word);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_rpn_decode(const RpnLevels* L_dev, int pre_topk, const uint64_t* lists, int nslots, const int* final_slot_dev,
                      float img_h, float img_w, float scale_clamp, float* boxes, float* scores, int* valid, uint32_t* maxc,
                      int level_mask, int B, hipStream_t s) {
    hipLaunchKernelGGL(rpn_decode, dim3((pre_topk + 255) / 256, 5, B), dim3(256), 0, s, L_dev, lists, nslots, final_slot_dev,
                       img_h, img_w, scale_clamp, boxes, scores, valid, maxc, level_mask);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
size_t apse_nms_scratch_bytes(int slots) {
    return (size_t)slots * (NMS_MAX * 4 + 4 * NMS_MAX * 4 + NMS_MAX * 4 + (size_t)NMS_MAX * 16 * 8 + 16);
}
static NmsScratch carve(void* scratch, int slots) {
    NmsScratch S;
    char* p = reinterpret_cast<char*>(scratch);
    S.mask = reinterpret_cast<uint64_t*>(p); p += (size_t)slots * NMS_MAX * 16 * 8;
    S.box = reinterpret_cast<float*>(p); p += (size_t)slots * 4 * NMS_MAX * 4;
    S.area = reinterpret_cast<float*>(p); p += (size_t)slots * NMS_MAX * 4;
    S.entry = reinterpret_cast<int*>(p); p += (size_t)slots * NMS_MAX * 4;
    S.n = reinterpret_cast<int*>(p);
    return S;
}
int apse_k_nms_percat(const float* boxes, const float* scores, const int* valid, int n_total, int cat_div, int cat_mod,
                      const uint32_t* maxc, float thr, int* keep_idx, int* keep_cnt, int ncat, void* scratch, int cat_mask,
                      int B, int presorted, hipStream_t s) {
    static bool done = false;
    if (!done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&nms_scan), hipFuncAttributeMaxDynamicSharedMemorySize,
                            NMS_MAX * 16 * 8);
        done = true;
    }
    NmsScratch S = carve(scratch, ncat * B);
    hipLaunchKernelGGL(nms_prepare, dim3(ncat, B), dim3(1024), 0, s, boxes, scores, valid, n_total, cat_div, cat_mod, maxc, S,
                       ncat, cat_mask, presorted);
    hipLaunchKernelGGL(nms_matrix, dim3(16, 16, ncat * B), dim3(64), 0, s, S, thr);
    hipLaunchKernelGGL(nms_scan, dim3(ncat, B), dim3(1024), NMS_MAX * 16 * 8, s, S, keep_idx, keep_cnt);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_rank_final(const float* boxes, const float* scores, int n_total, const int* keep_idx, const int* keep_cnt,
                      int ncat, int K, float* out_boxes, float* out_scores, int* out_entry, int* out_count,
                      uint32_t* zero_word, int B, hipStream_t s) {
    static bool done = false;
    if (!done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_merge), hipFuncAttributeMaxDynamicSharedMemorySize,
                            8 * NMS_MAX * 8);
        done = true;
    }
    if (ncat > 8) return APSE_E_INVALID;
    hipLaunchKernelGGL(rank_merge, dim3(B, ncat), dim3(1024), (size_t)ncat * NMS_MAX * 8, s, boxes, scores, n_total, keep_idx, keep_cnt,
                       ncat, K, out_boxes, out_scores, out_entry, out_count, zero_word);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_box_candidates(const float* pred, int ld, int K, const float* props, const int* prop_cnt, int P, float img_h,
                          float img_w, float thresh, const float* wts, float scale_clamp, float* cboxes, float* cscores,
                          int* cvalid, uint32_t* maxc, float* probs_out, int B, hipStream_t s) {
    if (K > 7) return APSE_E_INVALID;
    hipLaunchKernelGGL(box_candidates, dim3((P + 255) / 256, B), dim3(256), 0, s, pred, ld, K, props, prop_cnt, P, img_h,
                       img_w, thresh, wts[0], wts[1], wts[2], wts[3], scale_clamp, cboxes, cscores, cvalid, maxc, probs_out);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_box_candidates_wide(const float* pred, int ld, int K, const float* props, const int* prop_cnt, int P, float img_h,
                               float img_w, float thresh, const float* wts, float scale_clamp, float* cboxes, float* cscores,
                               int* cvalid, uint32_t* maxc, float* probs_out, int* clist, int* ccnt, int B, hipStream_t s) {
    if (K < 1 || K > 127 || ld < 5 * K + 1 || P > NMS_MAX) return APSE_E_INVALID;
    hipLaunchKernelGGL(box_candidates_wide, dim3((P + 3) / 4, B), dim3(256), 0, s, pred, ld, K, props, prop_cnt, P, img_h, img_w,
                       thresh, wts[0], wts[1], wts[2], wts[3], scale_clamp, cboxes, cscores, cvalid, maxc, probs_out, clist, ccnt);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_rank_wide(const float* boxes, const float* scores, int n_total, const int* keep_idx, const int* keep_cnt, int ncat,
                     int K, float* out_boxes, float* out_scores, int* out_entry, int* out_count, int B, hipStream_t s) {
    if (ncat < 1 || ncat > 128 || K < 1 || (size_t)ncat * K > 8192) return APSE_E_INVALID;      // one block sorts <= 8192 keys
    static bool done = false;
    if (!done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_sort_wide), hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 8);
        done = true;
    }
    hipLaunchKernelGGL(rank_sort_wide, dim3(B), dim3(1024), 8192 * 8, s, boxes, scores, n_total, keep_idx, keep_cnt, ncat, K,
                       out_boxes, out_scores, out_entry, out_count);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_nms_lists(const float* boxes, const float* scores, int n_total, const int* clist, int* ccnt, int list_stride,
                     const uint32_t* maxc, float thr, int* keep_idx, int* keep_cnt, int ncat, void* scratch, int B, hipStream_t s) {
    static bool done = false;
    if (!done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&nms_scan), hipFuncAttributeMaxDynamicSharedMemorySize,
                            NMS_MAX * 16 * 8);
        done = true;
    }
    if (list_stride > NMS_MAX) return APSE_E_INVALID;
    NmsScratch S = carve(scratch, ncat * B);
    hipLaunchKernelGGL(nms_prepare_list, dim3(ncat, B), dim3(1024), 0, s, boxes, scores, n_total, clist, ccnt, list_stride, maxc, S,
                       ncat);
    hipLaunchKernelGGL(nms_matrix, dim3(16, 16, ncat * B), dim3(64), 0, s, S, thr);
    hipLaunchKernelGGL(nms_scan, dim3(ncat, B), dim3(1024), NMS_MAX * 16 * 8, s, S, keep_idx, keep_cnt);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
size_t apse_c4_nms_scratch_bytes(int B) {
    return (size_t)B * ((size_t)C4_NMS_MAX * C4_NMS_WORDS * 8 + (size_t)C4_NMS_MAX * 4 * 4 + (size_t)C4_NMS_MAX * 4 * 2 + 16);
}
static C4Nms c4_carve(void* scratch, int B) {
    C4Nms S;
    char* p = reinterpret_cast<char*>(scratch);
    S.mask = reinterpret_cast<uint64_t*>(p); p += (size_t)B * C4_NMS_MAX * C4_NMS_WORDS * 8;
    S.box = reinterpret_cast<float*>(p); p += (size_t)B * 4 * C4_NMS_MAX * 4;
    S.area = reinterpret_cast<float*>(p); p += (size_t)B * C4_NMS_MAX * 4;
    S.entry = reinterpret_cast<int*>(p); p += (size_t)B * C4_NMS_MAX * 4;
    S.n = reinterpret_cast<int*>(p);
    return S;
}
// C4 proposals: select + decode (dec_* [B][pre]), long NMS, keep[:post] -> props [B][post], counts.  pre <= 6000, post <= 1000.
int apse_k_c4_rpn(const C4Rpn* R, int pre, int post, float img_h, float img_w, float scale_clamp, float thr, float* dec_boxes,
                  float* dec_scores, int* dec_valid, void* scratch, float* props, float* prop_scores, int* prop_entry,
                  int* prop_count, int B, hipStream_t s) {
    if (pre < 1 || pre > 6000 || R->k > pre || post < 1 || post > 1000) return APSE_E_INVALID;
    static bool done = false;
    const size_t lds = (size_t)C4_SORT_N * 8 + 16 * 256 * 4;
    if (!done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&c4_rpn_select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        done = true;
    }
    hipLaunchKernelGGL(c4_rpn_select, dim3(B), dim3(1024), lds, s, *R, img_h, img_w, scale_clamp, dec_boxes, dec_scores, dec_valid, pre);
    C4Nms S = c4_carve(scratch, B);
    hipLaunchKernelGGL(c4_nms_prepare, dim3(B), dim3(1024), 0, s, dec_boxes, dec_valid, pre, S);
    hipLaunchKernelGGL(c4_nms_matrix, dim3(C4_NMS_WORDS, C4_NMS_WORDS, B), dim3(64), 0, s, S, thr);
    hipLaunchKernelGGL(c4_nms_scan, dim3(B), dim3(1024), 0, s, S, dec_boxes, dec_scores, pre, post, props, prop_scores, prop_entry,
                       prop_count);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
size_t apse_rpn_train_scratch_bytes(int B) {
    const size_t slots = (size_t)B * 5;
    return slots * ((size_t)TR_MAX * TR_WORDS * 8 + (size_t)TR_MAX * 4 * 4 + (size_t)TR_MAX * 4 * 3 + 8) + (size_t)B * 4 + 16;
}
static TrainNms train_carve(void* scratch, int B, uint32_t** maxc) {
    TrainNms S;
    const size_t slots = (size_t)B * 5;
    char* p = reinterpret_cast<char*>(scratch);
    S.mask = reinterpret_cast<uint64_t*>(p); p += slots * TR_MAX * TR_WORDS * 8;
    S.box = reinterpret_cast<float*>(p); p += slots * 4 * TR_MAX * 4;
    S.area = reinterpret_cast<float*>(p); p += slots * TR_MAX * 4;
    S.entry = reinterpret_cast<int*>(p); p += slots * TR_MAX * 4;
    S.keep = reinterpret_cast<int*>(p); p += slots * TR_MAX * 4;
    S.n = reinterpret_cast<int*>(p); p += slots * 4;
    S.keep_cnt = reinterpret_cast<int*>(p); p += slots * 4;
    *maxc = reinterpret_cast<uint32_t*>(p);
    return S;
}
// Training-time FPN proposals: L (host; pre_topk and every level's k filled, rpn_select_plan) -> key lists (keys may be null),
// dec_* [B][5 * pre], props [B][post], counts.  1 <= pre, post <= TR_MAX; scratch of apse_rpn_train_scratch_bytes(B).
int apse_k_rpn_train_select(const RpnLevels* L, int post, float img_h, float img_w, float scale_clamp, float thr, int level_mask,
                            uint64_t* keys, float* dec_boxes, float* dec_scores, int* dec_valid, void* scratch, float* props,
                            float* prop_scores, int* prop_entry, int* prop_count, int B, hipStream_t s) {
    const int pre = L->pre_topk;
    if (pre < 1 || pre > TR_MAX || post < 1 || post > TR_MAX || B < 1) return APSE_E_INVALID;
    for (int l = 0; l < 5; ++l)
        if (L->lv[l].k > pre || L->lv[l].k > L->lv[l].n) return APSE_E_INVALID;
    static bool done = false;
    if (!done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&train_rank_merge), hipFuncAttributeMaxDynamicSharedMemorySize,
                            5 * TR_MAX * 8);
        done = true;
    }
    uint32_t* maxc;
    TrainNms S = train_carve(scratch, B, &maxc);
    if (hipMemsetAsync(maxc, 0, (size_t)B * 4, s) != hipSuccess) return APSE_E_HIP;
    hipLaunchKernelGGL(train_rpn_select, dim3(5, B), dim3(1024), 0, s, *L, img_h, img_w, scale_clamp, keys, dec_boxes, dec_scores,
                       dec_valid, maxc, level_mask);
    hipLaunchKernelGGL(train_nms_prepare, dim3(5, B), dim3(1024), 0, s, dec_boxes, dec_valid, pre, maxc, level_mask, S);
    hipLaunchKernelGGL(train_nms_matrix, dim3(TR_WORDS, TR_WORDS, 5 * B), dim3(64), 0, s, S, thr);
    hipLaunchKernelGGL(train_nms_scan, dim3(5, B), dim3(1024), 0, s, S, post);
    hipLaunchKernelGGL(train_rank_merge, dim3(B, 5), dim3(1024), (size_t)5 * TR_MAX * 8, s, dec_boxes, dec_scores, 5 * pre, S, post,
                       props, prop_scores, prop_entry, prop_count);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_pack_detections(const float* det_boxes, const float* det_scores, const int* det_entry, const int* det_cnt, int B,
                           int Kd, int ncls, float* pk_boxes, float* pk_scores, int* pk_cls, int* pk_img, int* pk_roi,
                           int* pk_total, int* pk_offset, unsigned long long* zero_sums, hipStream_t s) {
    if (B > 64) return APSE_E_INVALID;
    hipLaunchKernelGGL(pack_detections, dim3(1), dim3(256), 0, s, det_boxes, det_scores, det_entry, det_cnt, B, Kd, ncls,
                       pk_boxes, pk_scores, pk_cls, pk_img, pk_roi, pk_total, pk_offset, zero_sums);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
}
