// Track renderer: boxes, bit-packed masks and labels drawn onto u8 frames (include/apse_hip.h "track renderer").  The rules are
// DESIGN.md "Track rendering"; tests/render_ref.py restates them in numpy and the GPU tests compare byte for byte.  Every decision
// is integer arithmetic (or an f32 comparison of the caller's box with a host-made table), so no device rounding choice shows.
//
// Three launches after a memset of the count workspace:
//   render_stats     per item and 64-row band of its mask window: row popcounts (plain stores) and column counts (integer atomics,
//                    order-independent) into the workspace -- a window can span the whole frame, so the counts live in HBM;
//   render_anchor    one wave per item: bounding box and medians of the set pixels from those counts, the label anchor, scale and
//                    layout, the box rectangles, the item's reach; one RenderItemDev per item;
//   render_composite 64 x 16 pixel tiles: the items whose reach meets the tile, in draw order, as an LDS list; a tile with an empty
//                    list returns without touching the frame.  Out of place, the frames are copied first (hipMemcpyAsync), so the
//                    composite always works in place on `out` and its traffic scales with the drawn area.  Pixels are addressed
//                    as single bytes (3 per pixel), so any frame width works without alignment requirements.
#include "apse_common.h"
#include "../../include/apse_hip.h"
#include "render_font.h"
#include <math.h>
#include <limits.h>
#include <string.h>

namespace {

__constant__ uint8_t c_font[APSE_FONT_COUNT * APSE_FONT_ROWS] = {APSE_FONT_5X7_ROWS};
const uint8_t h_font[APSE_FONT_COUNT * APSE_FONT_ROWS] = {APSE_FONT_5X7_ROWS};

constexpr int kStatRows = 64;      // rows of one render_stats block
constexpr int kTileW = 64, kTileH = 16;
constexpr int kLabelStage = 256;      // label bytes render_anchor stages in LDS
constexpr int kAnchorStage = 12288;   // ints of window counts render_anchor stages in LDS (48 KiB)
constexpr float kCoordClamp = 1.0e8f;   // box coordinates are clamped to +-1e8 before any integer conversion

struct RenderItemDev {
    int reach[4];                  // frame-clipped union of box outline, mask rect and label background; x0 >= x1: nothing drawn
    int bo[4], bi[4];              // box outline: outer and inner rectangle
    int mr[4];                     // mask window rect clipped to the frame (empty: no mask)
    int bg[4];                     // label background
    const uint64_t* bits;
    int wbase, ry0, wpr;           // word column of the window's word 0, its first row, words per row
    int s, top, nlines, col;       // glyph scale, first text row, lines, colour (bytes in frame order)
    int dark, light, image, pad0;
    int left[APSE_RENDER_MAX_LINES], off[APSE_RENDER_MAX_LINES], len[APSE_RENDER_MAX_LINES];
};

struct RenderParams {
    const apse_render_item* items;
    const uint8_t* labels;
    size_t label_bytes;
    RenderItemDev* dev;
    int* counts;                   // [n][H + W]: rows then columns, frame coordinates
    uint8_t* out;
    int B, H, W, n, bgr, t_box, t_edge, nbreaks;
    float breaks[APSE_RENDER_MAX_BREAKS];
};

size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

__device__ __forceinline__ uint64_t span_mask(int lo, int hi) {   // bits lo..hi-1 of a word, 0 <= lo < hi <= 64
    const uint64_t up = hi >= 64 ? ~0ull : ((1ull << hi) - 1);
    return up & ~((1ull << lo) - 1);
}

__device__ __forceinline__ uint64_t mask_word(const RenderItemDev& d, int y, int aw) {
    const int w = aw - d.wbase;
    if (w < 0 || w >= d.wpr) return 0;
    return d.bits[(size_t)(y - d.ry0) * d.wpr + w];
}

__device__ __forceinline__ int round_coord(float v) {          // floor(v + 0.5) in f32
    return (int)floorf(fminf(fmaxf(v, -kCoordClamp), kCoordClamp) + 0.5f);
}

__device__ __forceinline__ int twice_coord(float v) {          // floor(2v + 0.5) in f32
    return (int)floorf(2.0f * fminf(fmaxf(v, -kCoordClamp), kCoordClamp) + 0.5f);
}

// ---------------------------------------------------------------- mask statistics
__global__ void __launch_bounds__(256) render_stats(RenderParams p) {
    const int k = blockIdx.y;
    const apse_render_item& it = p.items[k];
    if (!it.bits) return;
    const int x0 = max(it.rect[0], 0), x1 = min(it.rect[2], p.W);
    const int y0 = max(it.rect[1], 0) + blockIdx.x * kStatRows, y1 = min(min(it.rect[3], p.H), y0 + kStatRows);
    if (x0 >= x1 || y0 >= y1) return;
    const int wbase = it.rect[0] >> 6, wpr = it.words_per_row;
    const uint64_t* bits = it.bits;
    int* rows = p.counts + (size_t)k * (p.H + p.W);
    int* cols = rows + p.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int aw0 = x0 >> 6, aw1 = (x1 - 1) >> 6;
    for (int y = y0 + wave; y < y1; y += 4) {
        const uint64_t* row = bits + (size_t)(y - it.rect[1]) * wpr;
        int c = 0;
        for (int aw = aw0 + lane; aw <= aw1; aw += 64) {
            const int w = aw - wbase;
            if (w < 0 || w >= wpr) continue;
            const uint64_t m = span_mask(max(x0 - 64 * aw, 0), min(x1 - 64 * aw, 64));
            c += __popcll(row[w] & m);
        }
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) rows[y] = c;
    }
    for (int x = x0 + threadIdx.x; x < x1; x += 256) {
        const int w = (x >> 6) - wbase;
        if (w < 0 || w >= wpr) continue;
        const int sh = x & 63;
        const uint64_t* col = bits + (size_t)(y0 - it.rect[1]) * wpr + w;
        int c = 0;
#pragma unroll 16
        for (int r = 0; r < y1 - y0; ++r) c += (int)((col[(size_t)r * wpr] >> sh) & 1);
        if (c) atomicAdd(cols + x, c);
    }
}

// ---------------------------------------------------------------- anchor, scale, layout (one wave per item)
struct Scan { int total, first, last; };

// cnt[i] is the count at position lo + i, i < len
__device__ Scan wave_scan(const int* cnt, int lo, int len) {
    const int lane = threadIdx.x & 63;
    int total = 0, first = INT_MAX, last = -1;
    for (int b = 0; b < len; b += 64) {
        const int i = b + lane, x = lo + i;
        const int v = i < len ? cnt[i] : 0;
        total += v;
        if (v) { first = min(first, x); last = max(last, x); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        total += __shfl_xor(total, o);
        first = min(first, __shfl_xor(first, o));
        last = max(last, __shfl_xor(last, o));
    }
    return {total, first, last};
}

// position of the k-th (0-based) set pixel along the counts (k < total)
__device__ int wave_kth(const int* cnt, int lo, int len, int k) {
    const int lane = threadIdx.x & 63;
    int cum = 0, found = INT_MAX;
    for (int b = 0; b < len; b += 64) {
        const int i = b + lane, x = lo + i;
        const int v = i < len ? cnt[i] : 0;
        int inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (v && cum + inc - v <= k && k < cum + inc) found = x;
        cum += __shfl(inc, 63);
        if (cum > k) break;
    }
    for (int o = 32; o > 0; o >>= 1) found = min(found, __shfl_xor(found, o));
    return found;
}

__device__ __forceinline__ int floor_half(int v) { return v >> 1; }   // floor(v / 2), arithmetic shift

__global__ void __launch_bounds__(64) render_anchor(RenderParams p) {
    const int k = blockIdx.x;
    const apse_render_item it = p.items[k];
    const int lane = threadIdx.x;
    const int H = p.H, W = p.W;
    int mr[4] = {0, 0, 0, 0};
    if (it.bits) {
        mr[0] = max(it.rect[0], 0); mr[1] = max(it.rect[1], 0);
        mr[2] = min(it.rect[2], W); mr[3] = min(it.rect[3], H);
        if (mr[0] >= mr[2] || mr[1] >= mr[3]) mr[0] = mr[1] = mr[2] = mr[3] = 0;
    }
    // set pixels of the mask: count, bounding box, doubled medians
    const int ny = mr[3] - mr[1], nx = mr[2] - mr[0];
    const int* rows = p.counts + (size_t)k * (H + W) + mr[1];
    const int* cols = p.counts + (size_t)k * (H + W) + H + mr[0];
    __shared__ int staged[kAnchorStage];
    if (ny + nx <= kAnchorStage) {               // the usual window: the six scans below read LDS, the counts are loaded once
#pragma unroll 8
        for (int i = lane; i < ny; i += 64) staged[i] = rows[i];
#pragma unroll 8
        for (int i = lane; i < nx; i += 64) staged[ny + i] = cols[i];
        __syncthreads();
        rows = staged;
        cols = staged + ny;
    }
    int M = 0, A2x = 0, A2y = 0;
    int mb[4] = {0, 0, 0, 0};
    if (nx > 0) {
        const Scan sy = wave_scan(rows, mr[1], ny);
        const Scan sx = wave_scan(cols, mr[0], nx);
        M = sy.total;
        if (M > 0) {
            mb[0] = sx.first; mb[1] = sy.first; mb[2] = sx.last + 1; mb[3] = sy.last + 1;
            A2x = wave_kth(cols, mr[0], nx, (M - 1) / 2) + wave_kth(cols, mr[0], nx, M / 2);
            A2y = wave_kth(rows, mr[1], ny, (M - 1) / 2) + wave_kth(rows, mr[1], ny, M / 2);
        }
    }
    // the label's first bytes to LDS in one parallel load (lane 0 parses them below)
    int off = it.label_off, len = it.label_len;
    if (off < 0 || len < 0 || (size_t)off > p.label_bytes) len = 0;
    else if ((size_t)off + (size_t)len > p.label_bytes) len = (int)(p.label_bytes - (size_t)off);
    __shared__ uint8_t text[kLabelStage];
    for (int i = lane; i < min(len, kLabelStage); i += 64) text[i] = p.labels[off + i];
    __syncthreads();
    if (lane != 0) return;
    RenderItemDev& d = p.dev[k];
    // label box B, anchor, alignment (track_visualizer.py:165-182)
    float bx0, by0, bx1, by1;
    bool centred = M > 0;
    if (M > 0) {
        bx0 = (float)mb[0]; by0 = (float)mb[1]; bx1 = (float)mb[2]; by1 = (float)mb[3];
    } else {
        bx0 = fminf(fmaxf(it.box[0], -kCoordClamp), kCoordClamp); by0 = fminf(fmaxf(it.box[1], -kCoordClamp), kCoordClamp);
        bx1 = fminf(fmaxf(it.box[2], -kCoordClamp), kCoordClamp); by1 = fminf(fmaxf(it.box[3], -kCoordClamp), kCoordClamp);
        A2x = twice_coord(bx0); A2y = twice_coord(by0);
    }
    const float bh = by1 - by0;
    if ((bx1 - bx0) * bh < 1000.0f || bh < 40.0f) {
        float ax = bx0, ay = by1;
        if (by1 >= (float)(H - 5)) { ax = bx1; ay = by0; }
        A2x = twice_coord(ax); A2y = twice_coord(ay);
    }
    int s = 1;
    for (int i = 0; i < p.nbreaks; ++i) s += bh >= p.breaks[i];
    d.s = s;
    d.top = floor_half(A2y);
    // lines of the label
    int nl = 0;
    int bgx0 = INT_MAX, bgx1 = INT_MIN;
    if (len > 0) {
        int start = 0;
        for (int i = 0; i <= len && nl < APSE_RENDER_MAX_LINES; ++i) {
            if (i == len || (i < kLabelStage ? text[i] : p.labels[off + i]) == '\n') {
                const int n = i - start;
                const int w = s * max(6 * n - 1, 0);
                const int left = centred ? floor_half(A2x - w) : floor_half(A2x);
                d.left[nl] = left; d.off[nl] = off + start; d.len[nl] = n;
                bgx0 = min(bgx0, left - s); bgx1 = max(bgx1, left + w + s);
                ++nl;
                start = i + 1;
            }
        }
    }
    for (int i = nl; i < APSE_RENDER_MAX_LINES; ++i) { d.left[i] = 0; d.off[i] = 0; d.len[i] = 0; }
    d.nlines = nl;
    if (nl) { d.bg[0] = bgx0; d.bg[1] = d.top; d.bg[2] = bgx1; d.bg[3] = d.top + 9 * s * nl; }
    else { d.bg[0] = d.bg[1] = d.bg[2] = d.bg[3] = 0; }
    // box outline
    const int a = p.t_box / 2, b = p.t_box - a;
    const int R0 = round_coord(it.box[0]), R1 = round_coord(it.box[1]), R2 = round_coord(it.box[2]), R3 = round_coord(it.box[3]);
    d.bo[0] = R0 - a; d.bo[1] = R1 - a; d.bo[2] = R2 + a; d.bo[3] = R3 + a;
    d.bi[0] = R0 + b; d.bi[1] = R1 + b; d.bi[2] = R2 - b; d.bi[3] = R3 - b;
    for (int i = 0; i < 4; ++i) d.mr[i] = mr[i];
    d.bits = it.bits; d.wbase = it.rect[0] >> 6; d.ry0 = it.rect[1]; d.wpr = it.words_per_row;
    // reach: frame-clipped union of the three rectangles
    int r[4] = {INT_MAX, INT_MAX, INT_MIN, INT_MIN};
    const int* rects[3] = {d.bo, d.mr, d.bg};
    for (int q = 0; q < 3; ++q) {
        const int c0 = max(rects[q][0], 0), c1 = max(rects[q][1], 0), c2 = min(rects[q][2], W), c3 = min(rects[q][3], H);
        if (c0 >= c2 || c1 >= c3) continue;
        r[0] = min(r[0], c0); r[1] = min(r[1], c1); r[2] = max(r[2], c2); r[3] = max(r[3], c3);
    }
    if (r[0] >= r[2]) r[0] = r[1] = r[2] = r[3] = 0;
    for (int i = 0; i < 4; ++i) d.reach[i] = r[i];
    // colours in frame byte order
    int col = 0, dark = 0, light = 0;
    for (int ch = 0; ch < 3; ++ch) {
        const int c = it.rgb[p.bgr ? 2 - ch : ch];
        col |= c << (8 * ch);
        dark |= ((c * 77 + 128) >> 8) << (8 * ch);
        light |= (c + (((255 - c) * 179 + 128) >> 8)) << (8 * ch);
    }
    d.col = col; d.dark = dark; d.light = light; d.image = it.image; d.pad0 = 0;
}

// ---------------------------------------------------------------- composite
__device__ __forceinline__ bool in_rect(const int* r, int x, int y) { return x >= r[0] && x < r[2] && y >= r[1] && y < r[3]; }

__device__ __forceinline__ int blend(int p, int c, int a) { return (a * c + (256 - a) * p + 128) >> 8; }

// every pixel of [xa, xb] (inclusive) in row y of the mask is set
__device__ bool row_all_set(const RenderItemDev& d, int y, int xa, int xb) {
    for (int aw = xa >> 6; aw <= (xb >> 6); ++aw) {
        const uint64_t m = span_mask(max(xa - 64 * aw, 0), min(xb + 1 - 64 * aw, 64));
        if ((mask_word(d, y, aw) & m) != m) return false;
    }
    return true;
}

__global__ void __launch_bounds__(256) render_composite(RenderParams p) {
    __shared__ short list[APSE_RENDER_MAX_ITEMS];
    __shared__ int wcnt[4];
    __shared__ int total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH, img = blockIdx.z;
    const int tx1 = min(tx0 + kTileW, p.W), ty1 = min(ty0 + kTileH, p.H);
    if (tid == 0) total = 0;
    __syncthreads();
    for (int c0 = 0; c0 < p.n; c0 += 256) {
        const int k = c0 + tid;
        bool hit = false;
        if (k < p.n && p.dev[k].image == img) {
            const int* r = p.dev[k].reach;
            hit = r[0] < tx1 && r[2] > tx0 && r[1] < ty1 && r[3] > ty0;
        }
        const uint64_t m = __ballot(hit);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int base = total;
        for (int w = 0; w < wave; ++w) base += wcnt[w];
        if (hit) list[base + __popcll(m & ((1ull << lane) - 1))] = (short)k;
        __syncthreads();
        if (tid == 0) total += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    const int cnt = total;
    if (cnt == 0) return;
    const int x = tx0 + lane;
    if (x >= p.W) return;
    const int te = p.t_edge;
    for (int y = ty0 + wave; y < ty1; y += 4) {
        uint8_t* px = p.out + (((size_t)img * p.H + y) * p.W + x) * 3;
        int c0 = px[0], c1 = px[1], c2 = px[2];
        const int o0 = c0, o1 = c1, o2 = c2;
        // boxes and masks, in draw order
        for (int i = 0; i < cnt; ++i) {
            const RenderItemDev& d = p.dev[list[i]];
            if (!in_rect(d.reach, x, y)) continue;
            if (in_rect(d.bo, x, y) && !in_rect(d.bi, x, y)) {
                c0 = blend(c0, d.col & 255, 128); c1 = blend(c1, (d.col >> 8) & 255, 128); c2 = blend(c2, (d.col >> 16) & 255, 128);
            }
            if (in_rect(d.mr, x, y) && ((mask_word(d, y, x >> 6) >> (x & 63)) & 1)) {
                bool edge = y - te < d.mr[1] || y + te >= d.mr[3] || x - te < d.mr[0] || x + te >= d.mr[2];
                for (int yy = y - te; !edge && yy <= y + te; ++yy) edge = !row_all_set(d, yy, x - te, x + te);
                if (edge) {
                    c0 = d.dark & 255; c1 = (d.dark >> 8) & 255; c2 = (d.dark >> 16) & 255;
                } else {
                    c0 = blend(c0, d.col & 255, 128); c1 = blend(c1, (d.col >> 8) & 255, 128); c2 = blend(c2, (d.col >> 16) & 255, 128);
                }
            }
        }
        // labels, in draw order
        for (int i = 0; i < cnt; ++i) {
            const RenderItemDev& d = p.dev[list[i]];
            if (!in_rect(d.bg, x, y)) continue;
            c0 = blend(c0, 0, 205); c1 = blend(c1, 0, 205); c2 = blend(c2, 0, 205);
            const int s = d.s, line = (y - d.top) / (9 * s);
            if (line >= d.nlines) continue;
            const int gy = (y - d.top - 9 * s * line) / s - 1;
            const int rx = x - d.left[line];
            if (gy < 0 || gy >= APSE_FONT_ROWS || rx < 0) continue;
            const int j = rx / (6 * s);
            if (j >= d.len[line]) continue;
            const int gx = (rx - 6 * s * j) / s;
            if (gx >= APSE_FONT_W) continue;
            int ch = p.labels[d.off[line] + j];
            if (ch < APSE_FONT_FIRST || ch >= APSE_FONT_FIRST + APSE_FONT_COUNT) ch = '?';
            if ((c_font[(ch - APSE_FONT_FIRST) * APSE_FONT_ROWS + gy] >> (APSE_FONT_W - 1 - gx)) & 1) {
                c0 = d.light & 255; c1 = (d.light >> 8) & 255; c2 = (d.light >> 16) & 255;
            }
        }
        if (c0 != o0 || c1 != o1 || c2 != o2) { px[0] = (uint8_t)c0; px[1] = (uint8_t)c1; px[2] = (uint8_t)c2; }
    }
}

__global__ void __launch_bounds__(256) render_pack(const uint8_t* mask, int H, int W, uint64_t* words) {
    const int wpr = (W + 63) >> 6;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * wpr) return;
    const int y = (int)(i / wpr), w = (int)(i % wpr);
    const uint8_t* row = mask + (size_t)y * W;
    uint64_t v = 0;
    const int xe = min(64, W - 64 * w);
    for (int b = 0; b < xe; ++b) v |= (uint64_t)(row[64 * w + b] != 0) << b;
    words[i] = v;
}

}  // namespace

extern "C" {

size_t apse_render_workspace_bytes(int H, int W, int n) {
    if (H < 1 || W < 1 || n < 0) return 0;
    return align256((size_t)n * sizeof(RenderItemDev)) + (size_t)n * ((size_t)H + W) * sizeof(int) + 256;
}

int apse_render_instances(const uint8_t* frames, uint8_t* out, int B, int H, int W, int bgr, const apse_render_item* items, int n,
                          const uint8_t* labels, size_t label_bytes, const float* breaks, int nbreaks, void* ws, size_t ws_bytes,
                          void* stream) {
    if (!frames || !out || B < 1 || H < 1 || H > APSE_MAX_FRAME_H || W < 1 || W > APSE_MAX_FRAME_W) return APSE_E_INVALID;
    if (n < 0 || n > APSE_RENDER_MAX_ITEMS || (n > 0 && (!items || !ws)) || (label_bytes > 0 && !labels)) return APSE_E_INVALID;
    if (nbreaks < 0 || nbreaks > APSE_RENDER_MAX_BREAKS || (nbreaks > 0 && !breaks)) return APSE_E_INVALID;
    if (n > 0 && ws_bytes < apse_render_workspace_bytes(H, W, n)) return APSE_E_INVALID;
    const size_t bytes = (size_t)B * H * W * 3;
    if (out != frames && out < frames + bytes && frames < out + bytes) return APSE_E_INVALID;   // partial overlap
    hipStream_t st = (hipStream_t)stream;
    if (out != frames && hipMemcpyAsync(out, frames, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return APSE_E_HIP;
    if (n == 0) return APSE_OK;
    RenderParams p;
    memset(&p, 0, sizeof p);
    p.items = items; p.labels = labels; p.label_bytes = label_bytes;
    p.dev = reinterpret_cast<RenderItemDev*>(ws);
    p.counts = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + align256((size_t)n * sizeof(RenderItemDev)));
    p.out = out;
    p.B = B; p.H = H; p.W = W; p.n = n; p.bgr = bgr != 0;
    // frame constants (DESIGN.md "Track rendering"), f64 on the host
    const int D = (int)fmax(floor(sqrt((double)H * (double)W) / 90.0), 10.0);
    p.t_box = D / 4 > 1 ? D / 4 : 1;
    p.t_edge = D / 15 > 1 ? D / 15 : 1;
    p.nbreaks = nbreaks;
    for (int i = 0; i < nbreaks; ++i) p.breaks[i] = breaks[i];
    if (hipMemsetAsync(p.counts, 0, (size_t)n * ((size_t)H + W) * sizeof(int), st) != hipSuccess) return APSE_E_HIP;
    render_stats<<<dim3((H + kStatRows - 1) / kStatRows, n), 256, 0, st>>>(p);
    render_anchor<<<n, 64, 0, st>>>(p);
    render_composite<<<dim3((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, B), 256, 0, st>>>(p);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_render_pack_mask(const uint8_t* mask, int H, int W, uint64_t* words, void* stream) {
    if (!mask || !words || H < 1 || H > APSE_MAX_FRAME_H || W < 1 || W > APSE_MAX_FRAME_W) return APSE_E_INVALID;
    const size_t total = (size_t)H * ((W + 63) >> 6);
    render_pack<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(mask, H, W, words);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

size_t apse_render_font_host(uint8_t* out, size_t cap) {
    if (out && cap >= sizeof h_font) memcpy(out, h_font, sizeof h_font);
    return sizeof h_font;
}

}  // extern "C"
