// Result writers: tracked or detected masks -> cropped windows, COCO RLE run ends and the compressed counts string, on the
// bit windows (include/apse_hip.h "Result writers"; the rules are DESIGN.md "Result writers").
//
//   crop_overlaps  one block per object: the objects that beat it and meet its window are listed in LDS in index order
//                  (ballot + prefix), then every word of its window loses the OR of their words at the same absolute word
//                  column; mass and coordinate sums are block reductions.  No atomics anywhere
//   bits_to_rle    five launches: per-object cell layout (one block), per-cell transition counts (one wave per 64 columns x
//                  kSegRows rows: each lane loads one row and forms row ^ row_above, 64 ballots transpose that to one lane
//                  per column), tile scan, one block that scans the tile sums and writes ends_off / info, and the writes
//                  (the count pass again, now storing p = x * h + y)
//   rle_pack       four launches: bytes per value, the same two scans, the bytes
// A cell is (object, column, row segment) in that order, so cell order is ascending p within an object.  Every output
// position is a count followed by a scan: nothing is handed out by atomics, integer arithmetic only, so two runs are
// bit-identical.
#include "apse_common.h"
#include "../../include/apse_hip.h"
#include "mots_window.h"

namespace {

constexpr int kSegRows = APSE_MOTS_RLE_SEG_ROWS;   // rows of one cell
constexpr int kTile = 1024;                        // values of one scan tile (256 threads x 4)
constexpr int kScanThreads = 1024;

struct RleHeader {                                 // start of the bits_to_rle workspace
    long long cells;                               // cells the device windows need
    long long ok;                                  // 1: they fit the workspace the caller sized
};

struct RleGeom {                                   // the part of the frame where a window can hold a transition
    int x0, y0;
    int cols;                                      // columns x0 .. min(x1, w - 1); 0: none (empty, NULL bits or illegal window)
    int rows;                                      // `extra` + rows y0 .. min(y1, h - 1)
    int extra;                                     // 1: row 0 comes first (y0 > 0 and y1 == h: the column seam closes a run there)
    int segs;
};

// rect inside the frame and enough words per row; an empty rect is legal whatever else it says
__host__ __device__ inline bool rect_legal(const int* r, int wpr, int h, int w) {
    if (r[0] >= r[2] || r[1] >= r[3]) return true;
    if (r[0] < 0 || r[1] < 0 || r[2] > w || r[3] > h) return false;
    return wpr >= ((r[2] + 63) >> 6) - (r[0] >> 6);
}

__host__ __device__ inline RleGeom rle_geom(const apse_mots_window& win, int h, int w) {
    RleGeom g = {0, 0, 0, 0, 0, 0};
    const int* r = win.rect;
    if (r[0] >= r[2] || r[1] >= r[3] || !win.bits || !rect_legal(r, win.words_per_row, h, w)) return g;
    g.x0 = r[0];
    g.y0 = r[1];
    g.cols = (r[2] < w - 1 ? r[2] : w - 1) - r[0] + 1;
    g.extra = r[1] > 0 && r[3] == h;
    g.rows = g.extra + (r[3] < h - 1 ? r[3] : h - 1) - r[1] + 1;
    g.segs = (g.rows + kSegRows - 1) / kSegRows;
    return g;
}

__host__ __device__ inline long long tiles_of(long long values) { return (values + kTile - 1) / kTile; }

// ---------------------------------------------------------------- crop_overlaps
__device__ __forceinline__ apse_mots_window as_window(const apse_mots_object& o) {
    apse_mots_window w;
    w.rect[0] = o.rect[0]; w.rect[1] = o.rect[1]; w.rect[2] = o.rect[2]; w.rect[3] = o.rect[3];
    w.words_per_row = o.words_per_row;
    w.area = 0;
    w.bits = const_cast<uint64_t*>(o.bits);
    return w;
}

__device__ __forceinline__ int bit_index_sum(uint64_t v) {   // sum of the indices of the set bits
    return __popcll(v & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(v & 0xCCCCCCCCCCCCCCCCull) +
           4 * __popcll(v & 0xF0F0F0F0F0F0F0F0ull) + 8 * __popcll(v & 0xFF00FF00FF00FF00ull) +
           16 * __popcll(v & 0xFFFF0000FFFF0000ull) + 32 * __popcll(v & 0xFFFFFFFF00000000ull);
}

__global__ void __launch_bounds__(256) crop_kernel(const apse_mots_object* __restrict__ objs, int n, int H, int W, uint64_t* pool,
                                                   long long pool_words, const long long* __restrict__ pool_off,
                                                   long long* __restrict__ stats) {
    __shared__ int s_list[APSE_MOTS_MAX_OBJECTS];
    __shared__ int s_n, s_wave[4];
    __shared__ long long s_red[4][256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const apse_mots_object me = objs[k];
    const apse_mots_window mw = as_window(me);
    const bool live = me.rect[0] < me.rect[2] && me.rect[1] < me.rect[3] && rect_legal(me.rect, me.words_per_row, H, W);
    const int rows = live ? me.rect[3] - me.rect[1] : 0;
    const long long words = (long long)rows * me.words_per_row;
    const long long off = pool_off[k];
    const bool room = off >= 0 && off <= pool_words && words <= pool_words - off;   // else: nothing written, stats -1
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (live && room && me.bits) {                           // uniform over the block
        const int c0 = me.rect[0] >> 6, c1 = (me.rect[2] - 1) >> 6;
        const int lane = tid & 63, wave = tid >> 6;
        for (int j0 = 0; j0 < n; j0 += 256) {                // the objects that take pixels from k, in index order: ballot + prefix
            const int j = j0 + tid;
            bool take = false;
            if (j < n && j != k) {
                const apse_mots_object o = objs[j];
                take = o.bits && o.rect[0] < o.rect[2] && o.rect[1] < o.rect[3] && rect_legal(o.rect, o.words_per_row, H, W) &&
                       (o.score > me.score || (o.score == me.score && j > k)) &&
                       o.rect[1] < me.rect[3] && o.rect[3] > me.rect[1] && (o.rect[0] >> 6) <= c1 && ((o.rect[2] - 1) >> 6) >= c0;
            }
            const uint64_t m = __ballot(take);
            if (lane == 0) s_wave[wave] = __popcll(m);
            __syncthreads();
            int at = s_n + __popcll(m & ((1ull << lane) - 1));
            for (int q = 0; q < wave; ++q) at += s_wave[q];
            if (take) s_list[at] = j;
            __syncthreads();
            if (tid == 0) s_n += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            __syncthreads();
        }
    }
    __syncthreads();
    const int nl = s_n;
    long long mass_in = 0, mass = 0, sx = 0, sy = 0;
    if (room && me.bits) {                                   // NULL bits: no words are reserved for it, none are written
        for (long long i = tid; i < words; i += 256) {
            const int r = (int)(i / me.words_per_row), c = (int)(i - (long long)r * me.words_per_row);
            const int y = me.rect[1] + r, aw = (me.rect[0] >> 6) + c;
            uint64_t v = window_word(mw, y, aw);
            mass_in += __popcll(v);
            for (int l = 0; l < nl && v; ++l) v &= ~window_word(as_window(objs[s_list[l]]), y, aw);
            pool[off + i] = v;
            const int pc = __popcll(v);
            mass += pc;
            sx += (long long)pc * (aw * 64 + 1) + bit_index_sum(v);
            sy += (long long)pc * (y + 1);
        }
    }
    s_red[0][tid] = mass_in; s_red[1][tid] = mass; s_red[2][tid] = sx; s_red[3][tid] = sy;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int q = 0; q < 4; ++q) s_red[q][tid] += s_red[q][tid + s];
        __syncthreads();
    }
    if (tid < 4) stats[4 * k + tid] = room ? s_red[tid][0] : -1;
}

// ---------------------------------------------------------------- scans (shared by bits_to_rle and rle_pack)
// values [0, total) in tiles of kTile: each value is replaced by its exclusive prefix inside its tile; tile_sum[t] = the tile's sum
__global__ void __launch_bounds__(256) scan_tiles(uint32_t* v, const long long* total64, const int* total32, long long limit,
                                                  long long* tile_sum) {
    __shared__ uint32_t s[256];
    const long long total = total64 ? *total64 : (long long)*total32;
    if (total < 0 || total > limit) return;
    const int tid = threadIdx.x;
    const long long ntiles = tiles_of(total);
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long base = t * kTile + tid * 4;
        uint32_t a[4], sum = 0;
        for (int j = 0; j < 4; ++j) {
            a[j] = base + j < total ? v[base + j] : 0;
            sum += a[j];
        }
        s[tid] = sum;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                  // inclusive Hillis-Steele scan
            const uint32_t add = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        uint32_t run = s[tid] - sum;
        for (int j = 0; j < 4; ++j) {
            if (base + j < total) v[base + j] = run;
            run += a[j];
        }
        if (tid == 255) tile_sum[t] = s[255];
        __syncthreads();
    }
}

// one block of kScanThreads: tile_sum[0, ntiles) -> exclusive prefixes in place; returns the grand total to every thread
__device__ long long scan_tile_sums(long long* tile_sum, long long ntiles) {
    __shared__ long long s[kScanThreads];
    __shared__ long long s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (long long b = 0; b < ntiles; b += kScanThreads) {
        const long long mine = b + tid < ntiles ? tile_sum[b + tid] : 0;
        s[tid] = mine;
        __syncthreads();
        for (int o = 1; o < kScanThreads; o <<= 1) {
            const long long add = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        const long long carry = s_carry;
        if (b + tid < ntiles) tile_sum[b + tid] = carry + s[tid] - mine;
        __syncthreads();
        if (tid == kScanThreads - 1) s_carry = carry + s[tid];
        __syncthreads();
    }
    return s_carry;
}

__device__ __forceinline__ int saturate_int(long long v) { return v > INT_MAX ? INT_MAX : (int)v; }

// ---------------------------------------------------------------- bits_to_rle
__global__ void __launch_bounds__(kScanThreads) rle_layout(const apse_mots_window* __restrict__ windows, int n, int h, int w,
                                                           long long cells_cap, RleHeader* hdr, long long* cell_off) {
    __shared__ long long s[kScanThreads];
    const int tid = threadIdx.x;
    long long mine = 0;
    if (tid < n) {
        const RleGeom g = rle_geom(windows[tid], h, w);
        mine = (long long)g.cols * g.segs;
    }
    s[tid] = mine;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {
        const long long add = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    if (tid < n) cell_off[tid] = s[tid] - mine;
    if (tid == kScanThreads - 1) {
        cell_off[n] = s[tid];
        hdr->cells = s[tid];
        hdr->ok = s[tid] <= cells_cap;
    }
}

// The cells of object blockIdx.y, one wave per (word column, row segment), one lane per column.  WRITE = false: counts[cell] =
// transitions of the cell; WRITE = true: their pixel indices p = x * h + y, ascending, from the cell's scanned position.
template <bool WRITE>
__global__ void __launch_bounds__(256) rle_cells(const apse_mots_window* __restrict__ windows, int h, int w, const RleHeader* hdr,
                                                 const long long* __restrict__ cell_off, uint32_t* counts,
                                                 const long long* __restrict__ tile_sum, const int* __restrict__ ends_off,
                                                 const int* __restrict__ info, int* __restrict__ ends) {
    if (!hdr->ok) return;
    if (WRITE && !info[1]) return;
    const int k = blockIdx.y;
    if (WRITE && blockIdx.x == 0 && threadIdx.x == 0) ends[ends_off[k + 1] - 1] = h * w;   // the end of the last run
    const apse_mots_window win = windows[k];
    const RleGeom g = rle_geom(win, h, w);
    if (!g.cols) return;
    const int lane = threadIdx.x & 63;
    const int aw0 = g.x0 >> 6;
    const int wcols = ((g.x0 + g.cols - 1) >> 6) - aw0 + 1;
    const int items = wcols * g.segs;
    const long long base = cell_off[k];
    for (int item = blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += gridDim.x * 4) {
        const int c = item / g.segs, sgm = item - c * g.segs;
        const int aw = aw0 + c;
        const int x = aw * 64 + lane;
        const bool mine = x >= g.x0 && x < g.x0 + g.cols;
        const long long cell = base + (long long)(x - g.x0) * g.segs + sgm;
        long long pos = 0;
        if (WRITE && mine) pos = tile_sum[cell / kTile] + counts[cell] + k;   // k: one closing end per earlier object
        // lane r: the transitions of row i0 + r of this word column; 64 ballots hand lane b the rows of column b
        static_assert(kSegRows == 64, "one row per lane");
        const int i0 = sgm * kSegRows;
        const int i = i0 + lane;
        uint64_t t = 0;
        if (i < g.rows) {
            const int y = i < g.extra ? 0 : g.y0 + i - g.extra;
            const uint64_t prev = y == 0                      // the pixel before (x, 0) is (x - 1, h - 1)
                ? (window_word(win, h - 1, aw) << 1) | (window_word(win, h - 1, aw - 1) >> 63)
                : window_word(win, y - 1, aw);
            t = window_word(win, y, aw) ^ prev;
        }
        uint64_t rows_set = 0;
        for (int b = 0; b < 64; ++b) {
            const uint64_t m = __ballot((t >> b) & 1);
            if (lane == b) rows_set = m;
        }
        if (WRITE) {
            while (mine && rows_set) {                       // ascending rows: ascending p
                const int r = __ffsll((unsigned long long)rows_set) - 1;
                rows_set &= rows_set - 1;
                const int ii = i0 + r;
                ends[pos++] = x * h + (ii < g.extra ? 0 : g.y0 + ii - g.extra);
            }
        }
        const uint32_t cnt = __popcll(rows_set);
        if (!WRITE && mine) counts[cell] = cnt;
    }
}

__global__ void __launch_bounds__(kScanThreads) rle_finish(const RleHeader* hdr, const long long* __restrict__ cell_off,
                                                           const uint32_t* __restrict__ counts, long long* tile_sum, int n,
                                                           int cap, int* ends_off, int* info) {
    const int tid = threadIdx.x;
    if (!hdr->ok) {                                          // device windows that differ from the host copy: nothing written
        for (int k = tid; k <= n; k += kScanThreads) ends_off[k] = 0;
        if (tid == 0) { info[0] = -1; info[1] = 0; }
        return;
    }
    const long long cells = hdr->cells;
    const long long grand = scan_tile_sums(tile_sum, tiles_of(cells));
    __syncthreads();
    for (int k = tid; k <= n; k += kScanThreads) {
        const long long c = cell_off[k];
        ends_off[k] = saturate_int((c < cells ? tile_sum[c / kTile] + counts[c] : grand) + k);
    }
    if (tid == 0) {
        info[0] = saturate_int(grand + n);
        info[1] = grand + n <= cap;
    }
}

// ---------------------------------------------------------------- rle_pack
// value i of the flat list: the count's difference to the count two back (from the fourth count of its object on)
__device__ __forceinline__ int pack_value(const int* __restrict__ ends, const int* __restrict__ ends_off, int n, int i) {
    int lo = 0, hi = n - 1;                                  // last k with ends_off[k] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ends_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const int j = i - ends_off[lo];
    int x = ends[i] - (j > 0 ? ends[i - 1] : 0);
    if (j > 2) x -= ends[i - 2] - ends[i - 3];
    return x;
}

__global__ void __launch_bounds__(256) pack_cells(const int* __restrict__ ends, const int* __restrict__ ends_off, int n,
                                                  int limit, uint32_t* lens, const long long* __restrict__ tile_sum,
                                                  const int* __restrict__ info, char* __restrict__ chars, int write) {
    const int total = ends_off[n];
    if (total < 0 || total > limit) return;
    if (write && !info[1]) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        int x = pack_value(ends, ends_off, n, (int)i);
        long long pos = write ? tile_sum[i / kTile] + lens[i] : 0;
        uint32_t len = 0;
        bool more = true;
        while (more) {
            int c = x & 0x1f;
            x >>= 5;                                         // arithmetic: negative differences sign-extend
            more = (c & 0x10) ? x != -1 : x != 0;
            if (more) c |= 0x20;
            if (write) chars[pos++] = (char)(c + 48);
            ++len;
        }
        if (!write) lens[i] = len;
    }
}

__global__ void __launch_bounds__(kScanThreads) pack_finish(const int* __restrict__ ends_off, int n, int limit,
                                                            const uint32_t* __restrict__ lens, long long* tile_sum, int cap,
                                                            int* chars_off, int* info) {
    const int tid = threadIdx.x;
    const int total = ends_off[n];
    if (total < 0 || total > limit) {                        // the run ends were not written (or do not fit the workspace)
        for (int k = tid; k <= n; k += kScanThreads) chars_off[k] = 0;
        if (tid == 0) { info[0] = -1; info[1] = 0; }
        return;
    }
    const long long grand = scan_tile_sums(tile_sum, tiles_of(total));
    __syncthreads();
    for (int k = tid; k <= n; k += kScanThreads) {
        const int e = ends_off[k];
        chars_off[k] = saturate_int(e < total ? tile_sum[e / kTile] + lens[e] : grand);
    }
    if (tid == 0) {
        info[0] = saturate_int(grand);
        info[1] = grand <= cap;
    }
}

struct RleLayout {                                           // byte offsets into the bits_to_rle workspace
    long long cells;
    int max_items;                                           // most (word column, segment) items of one object
    size_t cell_off, tile_sum, counts, bytes;
};

bool rle_layout_host(const apse_mots_window* wh, int n, int h, int w, RleLayout* L) {
    long long cells = 0;
    int max_items = 1;
    for (int k = 0; k < n; ++k) {
        if (!rect_legal(wh[k].rect, wh[k].words_per_row, h, w)) return false;
        const RleGeom g = rle_geom(wh[k], h, w);
        if (!g.cols) continue;
        cells += (long long)g.cols * g.segs;
        const long long items = (long long)(((g.x0 + g.cols - 1) >> 6) - (g.x0 >> 6) + 1) * g.segs;
        if (items > max_items) max_items = (int)(items < INT_MAX ? items : INT_MAX);
    }
    L->cells = cells;
    L->max_items = max_items;
    L->cell_off = sizeof(RleHeader);
    L->tile_sum = L->cell_off + sizeof(long long) * (size_t)(n + 1);
    L->counts = L->tile_sum + sizeof(long long) * (size_t)(tiles_of(cells) + 1);
    L->bytes = L->counts + sizeof(uint32_t) * (size_t)(tiles_of(cells) * kTile);
    return true;
}

size_t pack_ws_bytes(int max_ends, size_t* lens_off) {
    *lens_off = sizeof(long long) * (size_t)(tiles_of(max_ends) + 1);
    return *lens_off + sizeof(uint32_t) * (size_t)(tiles_of(max_ends) * kTile);
}

}  // namespace

extern "C" {

int apse_mots_crop_overlaps(const apse_mots_object* objects, const apse_mots_object* objects_host, int n, int H, int W,
                            uint64_t* pool, size_t pool_words, const long long* pool_off, long long* stats, void* stream) {
    if (!frame_ok(H, W) || n < 0 || n > APSE_MOTS_MAX_OBJECTS) return APSE_E_INVALID;
    if (n == 0) return APSE_OK;
    if (!objects || !objects_host || !pool_off || !stats || (pool_words > 0 && !pool) || pool_words > (size_t)LLONG_MAX)
        return APSE_E_INVALID;
    for (int k = 0; k < n; ++k)
        if (!rect_legal(objects_host[k].rect, objects_host[k].words_per_row, H, W)) return APSE_E_INVALID;
    crop_kernel<<<n, 256, 0, (hipStream_t)stream>>>(objects, n, H, W, pool, (long long)pool_words, pool_off, stats);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

size_t apse_mots_rle_workspace_bytes(const apse_mots_window* windows_host, int n, int h, int w) {
    RleLayout L;
    if (!frame_ok(h, w) || n < 0 || n > APSE_MOTS_MAX_OBJECTS || (n > 0 && !windows_host)) return 0;
    if (!rle_layout_host(windows_host, n, h, w, &L)) return 0;
    return L.bytes;
}

int apse_mots_bits_to_rle(const apse_mots_window* windows, const apse_mots_window* windows_host, int n, int h, int w, int* ends,
                          int cap, int* ends_off, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (!frame_ok(h, w) || n < 0 || n > APSE_MOTS_MAX_OBJECTS || cap < 0) return APSE_E_INVALID;
    if (n == 0) return APSE_OK;
    if (!windows || !windows_host || !ends_off || !info || !ws || (cap > 0 && !ends)) return APSE_E_INVALID;
    RleLayout L;
    if (!rle_layout_host(windows_host, n, h, w, &L) || ws_bytes < L.bytes) return APSE_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    RleHeader* hdr = reinterpret_cast<RleHeader*>(base);
    long long* cell_off = reinterpret_cast<long long*>(base + L.cell_off);
    long long* tile_sum = reinterpret_cast<long long*>(base + L.tile_sum);
    uint32_t* counts = reinterpret_cast<uint32_t*>(base + L.counts);
    const int gx = (L.max_items + 3) / 4 < 256 ? (L.max_items + 3) / 4 : 256;
    const long long ntiles = tiles_of(L.cells);
    const int gt = ntiles < 1 ? 1 : (ntiles < 1024 ? (int)ntiles : 1024);
    rle_layout<<<1, kScanThreads, 0, st>>>(windows, n, h, w, L.cells, hdr, cell_off);
    rle_cells<false><<<dim3(gx, n), 256, 0, st>>>(windows, h, w, hdr, cell_off, counts, tile_sum, ends_off, info, ends);
    scan_tiles<<<gt, 256, 0, st>>>(counts, &hdr->cells, nullptr, L.cells, tile_sum);
    rle_finish<<<1, kScanThreads, 0, st>>>(hdr, cell_off, counts, tile_sum, n, cap, ends_off, info);
    rle_cells<true><<<dim3(gx, n), 256, 0, st>>>(windows, h, w, hdr, cell_off, counts, tile_sum, ends_off, info, ends);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

size_t apse_mots_rle_pack_workspace_bytes(int max_ends) {
    size_t lens_off;
    return max_ends < 0 ? 0 : pack_ws_bytes(max_ends, &lens_off);
}

int apse_mots_rle_pack(const int* ends, const int* ends_off, int n, int max_ends, char* chars, int cap, int* chars_off,
                       int* info, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || n > APSE_MOTS_MAX_OBJECTS || max_ends < 0 || cap < 0) return APSE_E_INVALID;
    if (n == 0) return APSE_OK;
    if (!ends_off || !chars_off || !info || !ws || (max_ends > 0 && !ends) || (cap > 0 && !chars)) return APSE_E_INVALID;
    size_t lens_off;
    if (ws_bytes < pack_ws_bytes(max_ends, &lens_off)) return APSE_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    long long* tile_sum = reinterpret_cast<long long*>(ws);
    uint32_t* lens = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + lens_off);
    const long long ntiles = tiles_of(max_ends);
    const int gt = ntiles < 1 ? 1 : (ntiles < 1024 ? (int)ntiles : 1024);
    const int gb = gt * 4;                                   // 256 threads per block: a tile is four blocks' worth
    pack_cells<<<gb, 256, 0, st>>>(ends, ends_off, n, max_ends, lens, tile_sum, info, chars, 0);
    scan_tiles<<<gt, 256, 0, st>>>(lens, nullptr, ends_off + n, max_ends, tile_sum);
    pack_finish<<<1, kScanThreads, 0, st>>>(ends_off, n, max_ends, lens, tile_sum, cap, chars_off, info);
    pack_cells<<<gb, 256, 0, st>>>(ends, ends_off, n, max_ends, lens, tile_sum, info, chars, 1);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

}  // extern "C"
