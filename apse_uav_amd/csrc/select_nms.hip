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
//
// Every rule has one definition, shared by the three entries (FPN inference, C4 inference, FPN training):
//   decode_box           Box2BoxTransform.apply_deltas + clip          (RPN anchors with weights 1, box head with its own)
//   decode_selected      key -> pixel, anchor -> decode -> nonempty flag -> stores -> running max coordinate
//   radix_select_kth     k-th smallest composite key of a head map too long for one sort
//   block_ordered_pos    ordered compaction of a flagged list
//   nms_matrix<MAX>      the suppression bit matrix: the only IoU in the file
//   resolve_diag         the greedy step of every scan
//   rank_merge<MAX>      final ranking of the kept lists (count_below: the binary search of every merge)
// One NMS, three slot lengths: NMS_MAX (FPN and box head, one slot per category and image, matrix scanned from LDS),
// C4_NMS_MAX (one slot per image) and TR_MAX (one per level and image), the long two scanned from HBM.
#include "apse_kernels.h"

#define TK_N 4096          // elements sorted per block in the top-k tournament
#define NMS_MAX APSE_NMS_SLOT   // boxes per category (<= 1000 by construction); the host sizes the keep lists by the same constant
#define C4_SORT_N 8192     // C4: keys sorted in LDS per image (>= rpn_pre_topk <= 6000)
#define C4_NMS_MAX 6144    // C4: boxes of the image's one NMS slot (>= 6000)
#define TR_MAX 2048        // training: keys of a level's list and boxes of its NMS slot (APSE_RPN_TRAIN_MAX_PRE_TOPK, include/apse_hip.h)

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

// Number of keys below `key` in the ascending list ko[0 .. n): the rank a merge adds for that list.
__device__ __forceinline__ int count_below(const uint64_t* ko, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (ko[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}

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

// ---------------------------------------------------------------- box decoding
struct Box4 { float x0, y0, x1, y1; };

// Box2BoxTransform.apply_deltas on one box (an anchor or a proposal) and four deltas d[0..3] with weights (wx, wy, ww, wh),
// then Boxes.clip to the image.  Each product and sum is rounded on its own, in this order; with weight 1 the division is
// exact.
__device__ __forceinline__ Box4 decode_box(float bx0, float by0, float bx1, float by1, const float* __restrict__ d, float wx,
                                           float wy, float ww, float wh, float scale_clamp, float img_h, float img_w) {
    const float w = bx1 - bx0, h = by1 - by0;
    const float cx = bx0 + 0.5f * w, cy = by0 + 0.5f * h;
    float dx = d[0] / wx, dy = d[1] / wy, dw = d[2] / ww, dh = d[3] / wh;
    dw = dw > scale_clamp ? scale_clamp : dw;
    dh = dh > scale_clamp ? scale_clamp : dh;
    const float pcx = dx * w + cx, pcy = dy * h + cy;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    Box4 q = {pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw, pcy + 0.5f * ph};
    q.x0 = fminf(fmaxf(q.x0, 0.f), img_w);
    q.y0 = fminf(fmaxf(q.y0, 0.f), img_h);
    q.x1 = fminf(fmaxf(q.x1, 0.f), img_w);
    q.y1 = fminf(fmaxf(q.y1, 0.f), img_h);
    return q;
}
__device__ __forceinline__ uint32_t max_coord_bits(const Box4& q) {   // all >= 0 after the clip: uint order = float order
    return __float_as_uint(fmaxf(fmaxf(q.x0, q.x1), fmaxf(q.y0, q.y1)));
}

// One selected RPN anchor -> entry o of the decoded list.  The key's index is e = pixel * A + anchor on a map of width W whose
// rows (`head`: this image's, `ld` floats each) hold A logits and then A x 4 deltas; the anchor is the cell anchor base[a] moved
// to the pixel.  Decode with weights 1, nonempty flag, the score as the key carries it (a zero is +0 whatever its sign), and,
// where the entry has one (`maxc`), the running max coordinate of the image's flagged boxes.
template <int A>
__device__ __forceinline__ void decode_selected(uint64_t key, int W, int stride, const float (*base)[4],
                                                const float* __restrict__ head, int ld, float img_h, float img_w,
                                                float scale_clamp, size_t o, float* __restrict__ boxes,
                                                float* __restrict__ scores, int* __restrict__ valid, uint32_t* maxc) {
    const uint32_t e = (uint32_t)key;
    const int pix = e / A, an = e - pix * A;
    const int y = pix / W, x = pix - y * W;
    const float sx = (float)(x * stride), sy = (float)(y * stride);
    const Box4 q = decode_box(sx + base[an][0], sy + base[an][1], sx + base[an][2], sy + base[an][3],
                              head + (size_t)pix * ld + A + an * 4, 1.0f, 1.0f, 1.0f, 1.0f, scale_clamp, img_h, img_w);
    const int ok = ((q.x1 - q.x0) > 0.f) && ((q.y1 - q.y0) > 0.f);
    boxes[o * 4 + 0] = q.x0; boxes[o * 4 + 1] = q.y0; boxes[o * 4 + 2] = q.x1; boxes[o * 4 + 3] = q.y1;
    scores[o] = comp_score(key);
    valid[o] = ok;
    if (maxc && ok) atomicMax(maxc, max_coord_bits(q));
}

// k-th smallest (1 <= k <= n) of the n distinct composite keys key_of(0 .. n-1), by a 1024-thread block: radix select, eight
// bits per pass from the top, a histogram per wave in hist[16][256].  Returns a bound with exactly k keys <= it: the k-th key
// itself after the last pass, or, as soon as the bin that holds it lies wholly inside the top k, that bin's last possible key
// (random scores: after the four score bytes).  Ends on a barrier.
template <class KeyOf>
__device__ __forceinline__ uint64_t radix_select_kth(int n, int k, KeyOf key_of, unsigned* hist, int tid) {
    __shared__ uint64_t prefix_s;
    __shared__ unsigned rank_s;
    __shared__ int done_s;
    const int wave = tid >> 6;
    if (tid == 0) { prefix_s = 0ull; rank_s = (unsigned)(k - 1); done_s = 0; }
    __syncthreads();
    for (int pass = 0; pass < 8; ++pass) {                 // the keys are distinct: the last pass ends with one key in the bin
        const int shift = 56 - 8 * pass;
        const uint64_t prefix = prefix_s;
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
    return prefix_s;
}

// Ordered compaction by a 1024-thread block, one call per 1024 candidates: the position of this thread's flagged candidate =
// the flagged ones of earlier calls (running total in wsum[16], zeroed by the caller before a barrier) + those of lower threads
// in this call.  Ends on a barrier with the total advanced, so wsum[16] is the count after the last call.
__device__ __forceinline__ int block_ordered_pos(bool f, int* wsum, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const uint64_t bal = __ballot(f);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = wsum[16];
    for (int w = 0; w < wave; ++w) off += wsum[w];
    __syncthreads();
    if (tid == 0) { int t = wsum[16]; for (int w = 0; w < 16; ++w) t += wsum[w]; wsum[16] = t; }
    __syncthreads();
    return off + __popcll(bal & ((1ull << lane) - 1ull));
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
                rank += count_below(a + o * 1024, cnt[o], key);
            }
            if (rank < K) dst[rank] = key;
        }
    }
}

// Decode the selected anchors of every level (decode_selected).  out arrays are [B][5*pre_topk].
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
    decode_selected<3>(key, lv.W, lv.stride, lv.base, lv.head + (size_t)b * lv.H * lv.W * head_ld, head_ld, img_h, img_w,
                       scale_clamp, o, boxes, scores, valid, maxc + b);
}

// ---------------------------------------------------------------- per-category NMS
// Entries: boxes/scores/valid are [B][n_total]; the category of entry e is
// cat_div ? e / cat_div : e % cat_mod.  Within a category, entries are ordered by (score desc,
// entry index asc); IoU is evaluated on boxes shifted by cat * (max_coord + 1) in f32 (torchvision
// batched_nms); `iou > thr` suppresses.  torchvision numbers the categories the call is given: with cat_mask != 0 (the RPN's
// level mask) category c counts as the number of mask bits below c, with cat_mask == 0 as c itself.
// One slot per list, of MAX boxes (NMS_MAX, C4_NMS_MAX or TR_MAX), and three launches:
//   prepare     : one block per slot -> the list's boxes in order, shifted, with areas, entry ids and the count n
//                 (nms_prepare / nms_prepare_list sort a category's entries; long_nms_prepare compacts a sorted list)
//   nms_matrix  : 64x64 tiles of the upper-triangular suppression bit matrix, one wave each
//   scan        : one block per slot: greedy scan, 64 rows at a time (nms_scan with the matrix in LDS; the long slots from HBM)
// A slot: entry[MAX] int, box[4][MAX] f32, area[MAX] f32, mask[MAX][MAX / 64] u64, n.
struct NmsSlots {
    int* entry; float* box; float* area; uint64_t* mask; int* n;
};

// Entry e of `boxes` -> row `pos` of a slot: shifted by `off`, with its area.
template <int MAX>
__device__ __forceinline__ void slot_put(const NmsSlots& S, size_t slot, int pos, uint32_t e, const float* __restrict__ boxes,
                                         float off) {
    float* bx = S.box + slot * 4 * MAX;
    const float x0 = boxes[e * 4 + 0] + off, y0 = boxes[e * 4 + 1] + off;
    const float x1 = boxes[e * 4 + 2] + off, y1 = boxes[e * 4 + 3] + off;
    bx[pos] = x0; bx[MAX + pos] = y0; bx[2 * MAX + pos] = x1; bx[3 * MAX + pos] = y1;
    S.area[slot * MAX + pos] = (x1 - x0) * (y1 - y0);
    S.entry[slot * MAX + pos] = (int)e;
}
// The batched_nms shift of category `cat` (its rank among the categories present in the call): cat * (max_coord + 1) in f32.
__device__ __forceinline__ float cat_shift(int cat, uint32_t maxc_bits) {
    return (float)cat * (__uint_as_float(maxc_bits) + 1.0f);
}

// Sorted keys -> the category's slot.
__device__ __forceinline__ void nms_store_sorted(const uint64_t* keys, int n, int cat, uint32_t maxc_bits,
                                                 const float* __restrict__ boxes, NmsSlots S, size_t slot, int tid) {
    const float off = cat_shift(cat, maxc_bits);
    if (tid < n) slot_put<NMS_MAX>(S, slot, tid, (uint32_t)keys[tid], boxes, off);
    if (tid == 0) S.n[slot] = n;
}

__global__ __launch_bounds__(1024) void nms_prepare(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                    const int* __restrict__ valid, int n_total, int cat_div, int cat_mod,
                                                    const uint32_t* __restrict__ maxc, NmsSlots S, int ncat, int cat_mask,
                                                    int presorted) {
    __shared__ uint64_t keys[NMS_MAX];
    __shared__ int wsum[17];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
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
        const int pos = block_ordered_pos(f, wsum, tid);
        if (f && pos < NMS_MAX) keys[pos] = comp_key(scores[e], (uint32_t)e);
    }
    __syncthreads();
    int n = wsum[16];
    n = n < NMS_MAX ? n : NMS_MAX;
    // presorted: the entries of a category already come in (score desc, entry asc) order -- the RPN stage, whose entry
    // l * pre_topk + i is rank i of level l's top-k list (sorted by the same key; ties by anchor index = by i) -- so the ordered
    // compaction above IS the sorted list and the 55 barrier steps of the bitonic network are skipped
    if (!presorted) block_bitonic_sort<NMS_MAX / 1024>(keys, tid);
    nms_store_sorted(keys, n, cat_mask ? __popc(cat_mask & ((1 << c) - 1)) : c, maxc[b], boxes, S, slot, tid);
}

// Long lists (C4, training): grid (lists per image, B), list l of image b = entries l * pre .. l * pre + pre - 1 of `boxes`,
// which are in (score desc, anchor asc) order already; the flagged ones keep it.  The category of a list is its rank among the
// lists of cat_mask; C4's one list has no max coordinate (maxc null) and shift 0.
template <int MAX>
__global__ __launch_bounds__(1024) void long_nms_prepare(const float* __restrict__ boxes, const int* __restrict__ valid, int pre,
                                                         const uint32_t* __restrict__ maxc, int cat_mask, NmsSlots S) {
    __shared__ int wsum[17];
    const int l = blockIdx.x, nl = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t slot = (size_t)b * nl + l;
    boxes += (size_t)b * nl * pre * 4;
    valid += (size_t)b * nl * pre;
    const float off = maxc ? cat_shift(__popc(cat_mask & ((1 << l) - 1)), maxc[b]) : 0.f;
    if (tid == 0) wsum[16] = 0;
    __syncthreads();
    for (int base = 0; base < pre; base += 1024) {
        const int i = base + tid, e = l * pre + i;
        const bool f = i < pre && valid[e];
        const int pos = block_ordered_pos(f, wsum, tid);
        if (f && pos < MAX) slot_put<MAX>(S, slot, pos, (uint32_t)e, boxes, off);
    }
    if (tid == 0) S.n[slot] = wsum[16] < MAX ? wsum[16] : MAX;
}

// Wide box inference (K > 8): the same as nms_prepare, but category c of image b reads only its own candidate list
// (written by box_candidates_wide: clist[b][c][0 .. ccnt[b][c]) = entry ids, in arrival order) instead of scanning all P * K
// entries.  The sort makes the arrival order irrelevant (the keys are distinct).  The block leaves its count at zero for the
// next forward.
__global__ __launch_bounds__(1024) void nms_prepare_list(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                         int n_total, const int* __restrict__ clist, int* __restrict__ ccnt,
                                                         int list_stride, const uint32_t* __restrict__ maxc, NmsSlots S,
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

// grid (MAX / 64 column chunks, MAX / 64 row chunks, slots), 64 threads: thread t owns row 64*ic + t of a tile on or right of
// the diagonal.  A live tile's rows i >= n (i <= MAX - 1: inside the slot) get a zero word that no scan reads: every scan
// stops at row n.  The store stays because with it the 1024 tile, the one on the frame's path, is the code it has always
// been; it costs the last row chunk's tiles at most 63 words each.
template <int MAX>
__global__ __launch_bounds__(64) void nms_matrix(NmsSlots S, float thr) {
    __shared__ float cb[5][64];
    const int jc = blockIdx.x, ic = blockIdx.y;
    const size_t slot = blockIdx.z;
    const int n = S.n[slot];
    if (jc < ic || 64 * ic >= n || 64 * jc >= n) return;
    const int t = threadIdx.x;
    const float* bx = S.box + slot * 4 * MAX;
    const float* ar = S.area + slot * MAX;
    const int j = 64 * jc + t;
    if (j < n) {
        cb[0][t] = bx[j]; cb[1][t] = bx[MAX + j]; cb[2][t] = bx[2 * MAX + j]; cb[3][t] = bx[3 * MAX + j];
        cb[4][t] = ar[j];
    }
    __syncthreads();
    const int i = 64 * ic + t;
    uint64_t bits = 0;
    if (i < n) {
        const float ix0 = bx[i], iy0 = bx[MAX + i], ix1 = bx[2 * MAX + i], iy1 = bx[3 * MAX + i];
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
    S.mask[(slot * MAX + i) * (MAX / 64) + jc] = bits;
}

__device__ __forceinline__ uint64_t wave_or64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// The greedy step, by wave 0 of a scan: lane l holds the diagonal word of row l of a 64-row chunk (`diag`: which later rows of
// the chunk row l suppresses), `rem` the rows that kept rows of earlier chunks removed.  Returns the rows kept (wave-uniform).
// Only rows that are still alive are visited: the next kept row is the lowest clear bit of `rem` above the last one (a removed
// row never suppresses anything), so the loop runs once per KEPT row, not per row.
__device__ __forceinline__ uint64_t resolve_diag(uint64_t diag, uint64_t rem, int rows_here) {
    uint64_t keepbits = 0;
    uint64_t alive = ~rem & (rows_here == 64 ? ~0ull : ((1ull << rows_here) - 1ull));
    while (alive) {
        const int r = __builtin_ctzll(alive);
        keepbits |= (1ull << r);
        rem |= readlane64(diag, r) | (1ull << r);
        alive &= ~rem;
    }
    return keepbits;
}

// Greedy scan, one block per (category, image).  Wave 0 resolves the 64 rows of a chunk on the
// diagonal word (scalar readlanes), then wave w ORs the kept rows' word w into the removed bitmap.
__global__ __launch_bounds__(1024) void nms_scan(NmsSlots S, int* __restrict__ keep_idx, int* __restrict__ keep_cnt) {
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
            const uint64_t keepbits = resolve_diag(diag, removed[ch], rows_here);
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

// Greedy scan of a long slot by one 1024-thread block, the bit matrix read from HBM (only words on and right of the diagonal
// of rows < n: those nms_matrix wrote).  Wave 0 resolves the 64 rows of a chunk on the diagonal word; then the waves OR the
// kept rows' words right of the diagonal into the removed bitmap.  The scan ends as soon as `post` rows are kept: the kept
// list is in processing order, so that is keep[:post] of the full scan.  keep[0 .. post) (LDS or HBM) receives the kept
// entries; returns their count (block-uniform, <= post), behind a barrier.
template <int MAX>
__device__ __forceinline__ int long_nms_scan(const NmsSlots& S, size_t slot, int post, int* keep) {
    constexpr int WORDS = MAX / 64;
    __shared__ uint64_t removed[WORDS];
    __shared__ uint64_t keepbits_s;
    __shared__ int kept_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n[slot];
    const int nw = (n + 63) >> 6;
    const uint64_t* gm = S.mask + slot * MAX * WORDS;
    const int* entry = S.entry + slot * MAX;
    for (int i = tid; i < WORDS; i += 1024) removed[i] = 0ull;
    if (tid == 0) kept_s = 0;
    __syncthreads();
    int kept = 0;                                   // wave 0's running count
    for (int ch = 0; ch < nw; ++ch) {
        const int rows_here = (n - 64 * ch) < 64 ? (n - 64 * ch) : 64;
        if (wave == 0) {
            const int row = 64 * ch + lane;
            const uint64_t diag = row < n ? gm[(size_t)row * WORDS + ch] : 0ull;
            const uint64_t keepbits = resolve_diag(diag, removed[ch], rows_here);
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
            if (lane < rows_here && ((kb >> lane) & 1ull)) v = gm[(size_t)(64 * ch + lane) * WORDS + w];
            v = wave_or64(v);
            if (lane == 0) removed[w] |= v;
        }
        __syncthreads();
    }
    return kept_s < post ? kept_s : post;
}

// C4: grid (B), slot = image.  The kept list stays in LDS and becomes the proposals [B][post]: boxes, scores, entry = rank in
// the decoded list; zeros and -1 past the count; the per-image count.  post <= 1024.
__global__ __launch_bounds__(1024) void long_nms_scan_proposals(NmsSlots S, const float* __restrict__ dboxes,
                                                                const float* __restrict__ dscores, int pre, int post,
                                                                float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                                int* __restrict__ out_entry, int* __restrict__ out_count) {
    __shared__ int keep[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cnt = long_nms_scan<C4_NMS_MAX>(S, b, post, keep);
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

// Training: grid (5, B), slot = image * 5 + level.  The kept list goes to keep_idx [slot][TR_MAX] for rank_merge: an element
// behind `post` others of its own sorted list has a merged rank >= post, so the merge never misses what the early stop left out.
__global__ __launch_bounds__(1024) void long_nms_scan_keep(NmsSlots S, int post, int* __restrict__ keep_idx,
                                                           int* __restrict__ keep_cnt) {
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int cnt = long_nms_scan<TR_MAX>(S, slot, post, keep_idx + slot * TR_MAX);
    if (threadIdx.x == 0) keep_cnt[slot] = cnt;
}

// Final ranking by merging: each category's kept list (up to MAX entries) is already sorted by (score desc, entry asc),
// so the global rank of an element is its own position plus, for every other list, the number of
// keys that precede it (binary search).  No barriers after the load; first K ranks are written.
// Grid (image, category): every block loads all lists of its image (the searches need them) and ranks the elements of ITS
// list -- the ncat x 4 dependent binary searches of one block were 8 of this launch's 21 us at batch 1.
// ncat <= 8; ncat * MAX keys of dynamic LDS (64 KiB for eight lists of NMS_MAX, 80 KiB for the five of TR_MAX).
template <int MAX>
__global__ __launch_bounds__(1024) void rank_merge(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                   int n_total, const int* __restrict__ keep_idx,
                                                   const int* __restrict__ keep_cnt, int ncat, int K,
                                                   float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                   int* __restrict__ out_entry, int* __restrict__ out_count,
                                                   uint32_t* __restrict__ zero_word) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);      // [ncat][MAX]
    const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    if (zero_word && c == 0 && tid == 0) zero_word[b] = 0u;      // next stage's max-coordinate cell
    __shared__ int cnt[8];
    boxes += (size_t)b * n_total * 4;
    scores += (size_t)b * n_total;
    if (tid < ncat) cnt[tid] = keep_cnt[b * ncat + tid];
    __syncthreads();
    int total = 0;
    for (int o = 0; o < ncat; ++o) {
        const int* src = keep_idx + ((size_t)b * ncat + o) * MAX;
#pragma unroll
        for (int s = 0; s < MAX / 1024; ++s) {               // thread t owns positions t, t + 1024, .. of every list
            const int i = tid + 1024 * s;
            if (i < cnt[o]) { const int e = src[i]; keys[o * MAX + i] = comp_key(scores[e], (uint32_t)e); }
        }
        total += cnt[o];
    }
    __syncthreads();
    const int nout = total < K ? total : K;
#pragma unroll
    for (int s = 0; s < MAX / 1024; ++s) {
        const int i = tid + 1024 * s;
        if (i >= cnt[c]) continue;
        const uint64_t key = keys[c * MAX + i];
        int rank = i;
        for (int o = 0; o < ncat; ++o) {
            if (o == c) continue;
            rank += count_below(keys + o * MAX, cnt[o], key);
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
    const float px0 = pb[0], py0 = pb[1], px1 = pb[2], py1 = pb[3];
    for (int k = 0; k < K; ++k) {
        const size_t slot = roi * K + k;
        const float p = ex[k] / sum;
        if (probs_out) probs_out[roi * (K + 1) + k] = p;
        const Box4 q = decode_box(px0, py0, px1, py1, lg + (K + 1) + 4 * k, wx, wy, ww, wh, scale_clamp, img_h, img_w);
        const int ok = live && (p > thresh);
        cboxes[slot * 4 + 0] = q.x0; cboxes[slot * 4 + 1] = q.y0; cboxes[slot * 4 + 2] = q.x1; cboxes[slot * 4 + 3] = q.y1;
        cscores[slot] = p;
        cvalid[slot] = ok;
        if (ok) atomicMax(maxc + b, max_coord_bits(q));
    }
    if (probs_out) probs_out[roi * (K + 1) + K] = ex[K] / sum;
}

// Wide form (K > 8, up to 127 classes): one wave per ROI, lane l owns logits l and l + 64 (class k, or the background at k = K).
// Softmax max and sum are wave reductions (xor butterflies: every lane ends with the same bits, whatever the launch), then each
// lane decodes (decode_box), clips and filters its classes.  The outputs and layout of box_candidates (slot
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
    const float px0 = pb[0], py0 = pb[1], px1 = pb[2], py1 = pb[3];
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
        const Box4 q = decode_box(px0, py0, px1, py1, lg + (K + 1) + 4 * k, wx, wy, ww, wh, scale_clamp, img_h, img_w);
        const int ok = live && (p > thresh);
        cboxes[slot * 4 + 0] = q.x0; cboxes[slot * 4 + 1] = q.y0; cboxes[slot * 4 + 2] = q.x1; cboxes[slot * 4 + 3] = q.y1;
        cscores[slot] = p;
        cvalid[slot] = ok;
        if (ok) {
            const uint32_t mk = max_coord_bits(q);
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

// ---------------------------------------------------------------- long lists: C4 and training-time selection
// detectron2's C4 RPN (Res5ROIHeads models) runs on one stride-16 map with 15 anchors per cell and keeps the top
// PRE_NMS_TOPK_TEST = 6000 logits of up to H * W * 15 (59220 at 47 x 84) before an NMS over that one list; training keeps
// PRE_NMS_TOPK_TRAIN = 2000 per FPN level (up to TR_MAX) and POST_NMS_TOPK_TRAIN = 1000 of the merge.  The tournament's
// 4096-key chunks and 1024-key lists do not reach that far, so one block selects a whole list: radix_select_kth (the keys are
// distinct, so "key <= bound" is exactly k elements), compaction of those k into LDS, one bitonic sort, decode_selected on the
// sorted keys.  Then the NMS above on a long slot -- long_nms_prepare, nms_matrix, long_nms_scan -- and, for the five lists of
// training, rank_merge<TR_MAX>.

// C4: one block per image, n = H * W * 15 keys -> dec_* [B][pre] (k = min(pre, n) live entries, the rest flagged off).
__global__ __launch_bounds__(1024) void c4_rpn_select(const C4Rpn R, float img_h, float img_w, float scale_clamp,
                                                     float* __restrict__ boxes, float* __restrict__ scores,
                                                     int* __restrict__ valid, int pre) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* a = reinterpret_cast<uint64_t*>(smem);                    // [C4_SORT_N]
    unsigned* hist = reinterpret_cast<unsigned*>(smem + C4_SORT_N * 8);  // [16 waves][256]
    __shared__ unsigned fill_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* head = R.head + (size_t)b * R.H * R.W * R.ld;
    const int n = R.n, k = R.k;
    auto key_of = [&](int e) -> uint64_t {
        const int pix = e / 15, an = e - pix * 15;
        return comp_key(head[(size_t)pix * R.ld + an], (uint32_t)e);
    };
    if (tid == 0) fill_s = 0u;
    const uint64_t kth = radix_select_kth(n, k, key_of, hist, tid);
    for (int i = tid; i < C4_SORT_N; i += 1024) a[i] = ~0ull;
    __syncthreads();
    for (int e = tid; e < n; e += 1024) {
        const uint64_t key = key_of(e);
        if (key <= kth) a[atomicAdd(&fill_s, 1u)] = key;                   // exactly k <= pre < C4_SORT_N keys
    }
    __syncthreads();
    block_bitonic_sort<C4_SORT_N / 1024>(a, tid);
    for (int i = tid; i < pre; i += 1024) {
        const size_t o = (size_t)b * pre + i;
        if (i >= k) { valid[o] = 0; scores[o] = 0.f; continue; }
        decode_selected<15>(a[i], R.W, R.stride, R.base, head, R.ld, img_h, img_w, scale_clamp, o, boxes, scores, valid, nullptr);
    }
}

// Training: grid (5, B), one block per (level, image), n = H * W * 3 keys -> the key list (keys_out may be null) and dec_*
// [B][5 * pre], with the image's running max coordinate.  A level of at most TR_MAX anchors is sorted whole.
__global__ __launch_bounds__(1024) void train_rpn_select(const RpnLevels L, float img_h, float img_w, float scale_clamp,
                                                        uint64_t* __restrict__ keys_out, float* __restrict__ boxes,
                                                        float* __restrict__ scores, int* __restrict__ valid,
                                                        uint32_t* __restrict__ maxc, int level_mask) {
    __shared__ uint64_t a[TR_MAX];
    __shared__ unsigned hist[16 * 256];                                  // [16 waves][256]
    __shared__ unsigned fill_s;
    const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const RpnLevel& lv = L.lv[l];
    const int head_ld = L.head_ld, pre = L.pre_topk;
    const float* head = lv.head + (size_t)b * lv.H * lv.W * head_ld;
    const int n = lv.n, k = lv.k;
    auto key_of = [&](int e) -> uint64_t {
        const int pix = e / 3, an = e - pix * 3;
        return comp_key(head[(size_t)pix * head_ld + an], (uint32_t)e);
    };
    if (tid == 0) fill_s = 0u;
    const uint64_t kth = n > TR_MAX ? radix_select_kth(n, k, key_of, hist, tid) : ~0ull;
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
        decode_selected<3>(a[i], lv.W, lv.stride, lv.base, head, head_ld, img_h, img_w, scale_clamp, o, boxes, scores, valid,
                           maxc + b);
    }
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

// ---------------------------------------------------------------- host side
// A scratch layout is written once, as a walk that takes its arrays in order.  With a base the walk hands out the pointers;
// without one it only adds up the sizes: the byte count and the carve cannot disagree.
struct ScratchWalk {
    void* base;
    size_t bytes = 0;
    template <class T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(static_cast<char*>(base) + bytes) : nullptr;
        bytes += count * sizeof(T);
        return p;
    }
};
// `slots` NMS slots of `len` boxes.  The 64-bit words come first; everything after them is 4-byte data.
static NmsSlots walk_slots(ScratchWalk& w, size_t slots, size_t len) {
    NmsSlots S;
    S.mask = w.take<uint64_t>(slots * len * (len / 64));
    S.box = w.take<float>(slots * 4 * len);
    S.area = w.take<float>(slots * len);
    S.entry = w.take<int>(slots * len);
    S.n = w.take<int>(slots);
    return S;
}
// Training-time selection: five slots of TR_MAX per image, their kept lists for the merge, the images' max-coordinate cells.
struct TrainScratch { NmsSlots S; int* keep; int* keep_cnt; uint32_t* maxc; };
static TrainScratch walk_train(ScratchWalk& w, size_t B) {
    TrainScratch T;
    T.S = walk_slots(w, B * 5, TR_MAX);
    T.keep = w.take<int>(B * 5 * TR_MAX);
    T.keep_cnt = w.take<int>(B * 5);
    T.maxc = w.take<uint32_t>(B);
    return T;
}

// A kernel opts in to its largest dynamic LDS size (`Bytes`) once, before its first launch.
template <auto Kernel, int Bytes>
static void allow_dynamic_lds() {
    static const hipError_t once =
        hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, Bytes);
    (void)once;
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
    ScratchWalk w{nullptr};
    walk_slots(w, (size_t)slots, NMS_MAX);
    return w.bytes;
}
int apse_k_nms_percat(const float* boxes, const float* scores, const int* valid, int n_total, int cat_div, int cat_mod,
                      const uint32_t* maxc, float thr, int* keep_idx, int* keep_cnt, int ncat, void* scratch, int cat_mask,
                      int B, int presorted, hipStream_t s) {
    allow_dynamic_lds<&nms_scan, NMS_MAX * 16 * 8>();
    ScratchWalk w{scratch};
    const NmsSlots S = walk_slots(w, (size_t)ncat * B, NMS_MAX);
    hipLaunchKernelGGL(nms_prepare, dim3(ncat, B), dim3(1024), 0, s, boxes, scores, valid, n_total, cat_div, cat_mod, maxc, S,
                       ncat, cat_mask, presorted);
    hipLaunchKernelGGL(nms_matrix<NMS_MAX>, dim3(NMS_MAX / 64, NMS_MAX / 64, ncat * B), dim3(64), 0, s, S, thr);
    hipLaunchKernelGGL(nms_scan, dim3(ncat, B), dim3(1024), NMS_MAX * 16 * 8, s, S, keep_idx, keep_cnt);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_rank_final(const float* boxes, const float* scores, int n_total, const int* keep_idx, const int* keep_cnt,
                      int ncat, int K, float* out_boxes, float* out_scores, int* out_entry, int* out_count,
                      uint32_t* zero_word, int B, hipStream_t s) {
    allow_dynamic_lds<&rank_merge<NMS_MAX>, 8 * NMS_MAX * 8>();
    if (ncat > 8) return APSE_E_INVALID;
    hipLaunchKernelGGL(rank_merge<NMS_MAX>, dim3(B, ncat), dim3(1024), (size_t)ncat * NMS_MAX * 8, s, boxes, scores, n_total,
                       keep_idx, keep_cnt, ncat, K, out_boxes, out_scores, out_entry, out_count, zero_word);
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
    allow_dynamic_lds<&rank_sort_wide, 8192 * 8>();
    hipLaunchKernelGGL(rank_sort_wide, dim3(B), dim3(1024), 8192 * 8, s, boxes, scores, n_total, keep_idx, keep_cnt, ncat, K,
                       out_boxes, out_scores, out_entry, out_count);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
int apse_k_nms_lists(const float* boxes, const float* scores, int n_total, const int* clist, int* ccnt, int list_stride,
                     const uint32_t* maxc, float thr, int* keep_idx, int* keep_cnt, int ncat, void* scratch, int B, hipStream_t s) {
    allow_dynamic_lds<&nms_scan, NMS_MAX * 16 * 8>();
    if (list_stride > NMS_MAX) return APSE_E_INVALID;
    ScratchWalk w{scratch};
    const NmsSlots S = walk_slots(w, (size_t)ncat * B, NMS_MAX);
    hipLaunchKernelGGL(nms_prepare_list, dim3(ncat, B), dim3(1024), 0, s, boxes, scores, n_total, clist, ccnt, list_stride, maxc, S,
                       ncat);
    hipLaunchKernelGGL(nms_matrix<NMS_MAX>, dim3(NMS_MAX / 64, NMS_MAX / 64, ncat * B), dim3(64), 0, s, S, thr);
    hipLaunchKernelGGL(nms_scan, dim3(ncat, B), dim3(1024), NMS_MAX * 16 * 8, s, S, keep_idx, keep_cnt);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
size_t apse_c4_nms_scratch_bytes(int B) {
    ScratchWalk w{nullptr};
    walk_slots(w, (size_t)B, C4_NMS_MAX);
    return w.bytes;
}
// C4 proposals: select + decode (dec_* [B][pre]), long NMS, keep[:post] -> props [B][post], counts.  pre <= 6000, post <= 1000.
int apse_k_c4_rpn(const C4Rpn* R, int pre, int post, float img_h, float img_w, float scale_clamp, float thr, float* dec_boxes,
                  float* dec_scores, int* dec_valid, void* scratch, float* props, float* prop_scores, int* prop_entry,
                  int* prop_count, int B, hipStream_t s) {
    if (pre < 1 || pre > 6000 || R->k > pre || post < 1 || post > 1000) return APSE_E_INVALID;
    constexpr int lds = C4_SORT_N * 8 + 16 * 256 * 4;
    allow_dynamic_lds<&c4_rpn_select, lds>();
    hipLaunchKernelGGL(c4_rpn_select, dim3(B), dim3(1024), lds, s, *R, img_h, img_w, scale_clamp, dec_boxes, dec_scores, dec_valid, pre);
    ScratchWalk w{scratch};
    const NmsSlots S = walk_slots(w, (size_t)B, C4_NMS_MAX);
    hipLaunchKernelGGL(long_nms_prepare<C4_NMS_MAX>, dim3(1, B), dim3(1024), 0, s, dec_boxes, dec_valid, pre,
                       static_cast<const uint32_t*>(nullptr), 0, S);
    hipLaunchKernelGGL(nms_matrix<C4_NMS_MAX>, dim3(C4_NMS_MAX / 64, C4_NMS_MAX / 64, B), dim3(64), 0, s, S, thr);
    hipLaunchKernelGGL(long_nms_scan_proposals, dim3(B), dim3(1024), 0, s, S, dec_boxes, dec_scores, pre, post, props, prop_scores,
                       prop_entry, prop_count);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
size_t apse_rpn_train_scratch_bytes(int B) {
    ScratchWalk w{nullptr};
    walk_train(w, (size_t)B);
    return w.bytes;
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
    allow_dynamic_lds<&rank_merge<TR_MAX>, 5 * TR_MAX * 8>();
    ScratchWalk w{scratch};
    const TrainScratch T = walk_train(w, (size_t)B);
    if (hipMemsetAsync(T.maxc, 0, (size_t)B * 4, s) != hipSuccess) return APSE_E_HIP;
    hipLaunchKernelGGL(train_rpn_select, dim3(5, B), dim3(1024), 0, s, *L, img_h, img_w, scale_clamp, keys, dec_boxes, dec_scores,
                       dec_valid, T.maxc, level_mask);
    hipLaunchKernelGGL(long_nms_prepare<TR_MAX>, dim3(5, B), dim3(1024), 0, s, dec_boxes, dec_valid, pre,
                       static_cast<const uint32_t*>(T.maxc), level_mask, T.S);
    hipLaunchKernelGGL(nms_matrix<TR_MAX>, dim3(TR_MAX / 64, TR_MAX / 64, 5 * B), dim3(64), 0, s, T.S, thr);
    hipLaunchKernelGGL(long_nms_scan_keep, dim3(5, B), dim3(1024), 0, s, T.S, post, T.keep, T.keep_cnt);
    hipLaunchKernelGGL(rank_merge<TR_MAX>, dim3(B, 5), dim3(1024), (size_t)5 * TR_MAX * 8, s, dec_boxes, dec_scores, 5 * pre,
                       static_cast<const int*>(T.keep), static_cast<const int*>(T.keep_cnt), 5, post, props, prop_scores,
                       prop_entry, prop_count, static_cast<uint32_t*>(nullptr));
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
