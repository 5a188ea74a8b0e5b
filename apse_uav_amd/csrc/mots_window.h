// Bit-window helpers shared by the MOTS kernels (mots.hip, rle_encode.hip): the window layout of include/apse_hip.h
// "MOTS evaluation".
#pragma once
#include "apse_common.h"
#include "../../include/apse_hip.h"
#include <limits.h>

namespace {

__device__ __forceinline__ uint64_t span_mask(int lo, int hi) {   // bits lo..hi-1 of a word, 0 <= lo < hi <= 64
    const uint64_t up = hi >= 64 ? ~0ull : ((1ull << hi) - 1);
    return up & ~((1ull << lo) - 1);
}

// word at absolute word column aw of row y of a window, restricted to its rect's pixels (0 outside the window)
__device__ __forceinline__ uint64_t window_word(const apse_mots_window& w, int y, int aw) {
    if (y < w.rect[1] || y >= w.rect[3] || w.rect[0] >= w.rect[2] || !w.bits) return 0;
    const int c = aw - (w.rect[0] >> 6);
    if (c < 0 || c >= w.words_per_row) return 0;
    const int lo = max(w.rect[0] - aw * 64, 0), hi = min(w.rect[2] - aw * 64, 64);
    if (lo >= hi) return 0;
    return w.bits[(size_t)(y - w.rect[1]) * w.words_per_row + c] & span_mask(lo, hi);
}

inline bool frame_ok(int H, int W) {                                // as apse_create: 32-bit pixel (and RLE run end) indices
    return H >= 1 && H <= APSE_MAX_FRAME_H && W >= 1 && W <= APSE_MAX_FRAME_W && (long long)H * W <= INT_MAX - 64;
}

}  // namespace
