// Training augmentation on resized u8 BGR images (include/apse_hip.h "Training augmentation"): detectron2's RandomFlip,
// RandomBrightness, RandomSaturation, RandomContrast and RandomLighting as the reference's DatasetMapper chains them.  The rules
// are DESIGN.md "Training augmentation"; tests/augment_ref.py restates them in numpy with explicit dtypes and the GPU tests compare
// every byte.
//
//   augment_sum     pass 1: brightness + saturation per pixel, the u8 results summed per image (the contrast step blends with
//                   the mean of the WHOLE image after saturation).  Flat over the image, grid-stride; an integer sum, so any
//                   order gives the same bits: per-thread u32, wave shuffle, LDS, one no-return 64-bit atomic add per block.
//   augment_write   pass 2: recomputes the first two steps (6 bytes read per pixel in all instead of 3 read + 3 written + 3
//                   read), derives mean and the contrast offset from the sum on the device, finishes contrast and lighting and
//                   writes the u8 image and / or the f32 CHW planes, mirrored when the image is flipped.
// A thread handles a run of 4 pixels of one row = 12 bytes = three dwords; the ragged end of a row (W % 4 pixels) goes bytewise.
// Rows have any width, so a run has no alignment: the 12 bytes move through memcpy of align 1, which gfx950 serves with one
// dwordx3 access (unaligned global access is on for amdhsa).
//
// The mix of f32 and f64 is the specification (numpy 1.18 value-based casting under detectron2 0.1.2), not a choice: the build
// keeps -ffp-contract=off, and every product and sum below is written as one operation of the stated type.
#include "apse_kernels.h"
#include "../../include/apse_hip.h"
#include <stdio.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
// pass 1 blocks per image at most: one atomic each on the image's sum word.  Measured at 2160 x 3840 (both passes):
// 512 -> 0.071 ms, 2048 -> 0.075 ms, 8192 -> 0.146 ms (the atomics on one word serialise)
constexpr int kSumBlocks = 512;

int invalid(const char* msg) { return apse_fail_global(APSE_E_INVALID, msg); }

__device__ __forceinline__ uint8_t clip_u8(float x) { return (uint8_t)(int)fminf(fmaxf(x, 0.0f), 255.0f); }
__device__ __forceinline__ uint8_t clip_u8(double x) { return (uint8_t)(int)fmin(fmax(x, 0.0), 255.0); }

// brightness then saturation of one pixel (channels 0, 1, 2 of the BGR image), each ending in clip + truncation
__device__ __forceinline__ void bright_sat(const AugmentImage& a, uint8_t& c0, uint8_t& c1, uint8_t& c2) {
    const uint8_t b0 = clip_u8(a.wb * (float)c0), b1 = clip_u8(a.wb * (float)c1), b2 = clip_u8(a.wb * (float)c2);
    const double g01 = (double)b0 * 0.299 + (double)b1 * 0.587;
    const double gray = g01 + (double)b2 * 0.114;
    const double t = a.one_minus_ws * gray;
    c0 = clip_u8(t + (double)(a.ws * (float)b0));
    c1 = clip_u8(t + (double)(a.ws * (float)b1));
    c2 = clip_u8(t + (double)(a.ws * (float)b2));
}

// contrast (offset s, f32) then lighting (f64) of one value of channel ch
__device__ __forceinline__ uint8_t contrast_light(const AugmentImage& a, float s, int ch, uint8_t v) {
    const uint8_t c = clip_u8(s + a.wc * (float)v);
    return clip_u8(a.vec[ch] + (double)c);
}

// n pixels (1..4) at p -> px[12]; a whole run is one 12-byte access
__device__ __forceinline__ void load_run(const uint8_t* p, int n, uint8_t (&px)[12]) {
    if (n == 4) {
        uint32_t d[3];
        __builtin_memcpy(d, p, 12);
#pragma unroll
        for (int i = 0; i < 12; ++i) px[i] = (uint8_t)(d[i >> 2] >> (8 * (i & 3)));
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) px[i] = i < 3 * n ? p[i] : (uint8_t)0;
    }
}

__global__ void __launch_bounds__(kThreads) augment_sum(const uint8_t* __restrict__ src, int npix, AugmentBatch P,
                                                        unsigned long long* __restrict__ sums) {
    const int b = blockIdx.y;
    const AugmentImage& a = P.im[b];
    const uint8_t* img = src + (size_t)b * npix * 3;
    const int items = (npix + 3) >> 2;
    unsigned int acc = 0;                  // at most 12 * 255 per item and items / (gridDim.x * 256) < 2^20 items per thread
    for (int it = blockIdx.x * kThreads + threadIdx.x; it < items; it += gridDim.x * kThreads) {
        const int n = min(4, npix - 4 * it);
        uint8_t px[12];
        load_run(img + (size_t)it * 12, n, px);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n) {
                bright_sat(a, px[3 * j], px[3 * j + 1], px[3 * j + 2]);
                acc += (unsigned int)px[3 * j] + px[3 * j + 1] + px[3 * j + 2];
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ unsigned int part[kThreads / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) t += part[w];
        if (t) atomicAdd(&sums[b], t);     // result unused: a no-return atomic
    }
}

__global__ void __launch_bounds__(kThreads) augment_write(const uint8_t* __restrict__ src, int H, int W, int runs_per_row,
                                                          AugmentBatch P, const unsigned long long* __restrict__ sums,
                                                          uint8_t* __restrict__ out_u8, float* __restrict__ out_chw) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= H * runs_per_row) return;
    const AugmentImage& a = P.im[b];
    const int y = t / runs_per_row, x = (t - y * runs_per_row) * 4;
    const int n = min(4, W - x);
    const size_t npix = (size_t)H * W;
    const size_t row = (size_t)b * npix + (size_t)y * W;

    uint8_t px[12];
    load_run(src + (row + x) * 3, n, px);
    // mean of the image after saturation, and the contrast offset: f64 product, rounded to f32 once
    const double mean = (double)sums[b] / (double)(3ull * npix);
    const float s = (float)(a.one_minus_wc * mean);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bright_sat(a, px[3 * j], px[3 * j + 1], px[3 * j + 2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[3 * j + c] = contrast_light(a, s, c, px[3 * j + c]);
    }
    // the run lands at xo .. xo + n - 1; flipped, both the run and the order inside it are mirrored
    const int xo = a.flip ? W - x - n : x;
    uint8_t o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int sj = a.flip ? n - 1 - j : j;     // n == 4 on the dword path; the ragged path reads j < n only
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v = sj == k ? px[3 * k + c] : v;
            o[3 * j + c] = v;
        }
    }
    if (out_u8) {
        uint8_t* q = out_u8 + (row + xo) * 3;
        if (n == 4) {
            uint32_t d[3] = {0, 0, 0};
#pragma unroll
            for (int i = 0; i < 12; ++i) d[i >> 2] |= (uint32_t)o[i] << (8 * (i & 3));
            __builtin_memcpy(q, d, 12);
        } else {
#pragma unroll
            for (int i = 0; i < 9; ++i)
                if (i < 3 * n) q[i] = o[i];
        }
    }
    if (out_chw) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* q = out_chw + ((size_t)b * 3 + c) * npix + (size_t)y * W + xo;
            if (n == 4 && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
                f32x4 v4 = {(float)o[c], (float)o[3 + c], (float)o[6 + c], (float)o[9 + c]};
                *reinterpret_cast<f32x4*>(q) = v4;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) q[j] = (float)o[3 * j + c];
            }
        }
    }
}

}  // namespace

extern "C" {

int apse_k_augment(const uint8_t* src, int B, int H, int W, const AugmentBatch* P, uint8_t* out_u8, float* out_chw,
                   unsigned long long* sums, hipStream_t s) {
    if (hipMemsetAsync(sums, 0, (size_t)B * sizeof(unsigned long long), s) != hipSuccess) return APSE_E_HIP;
    const int npix = H * W;                                   // < 2^31 by the frame bounds
    const int items = (npix + 3) / 4;
    const int sum_blocks = min(kSumBlocks, (items + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(augment_sum, dim3(sum_blocks, B), dim3(kThreads), 0, s, src, npix, *P, sums);
    const int rpr = (W + 3) / 4;
    const int blocks = (int)(((long long)H * rpr + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(augment_write, dim3(blocks, B), dim3(kThreads), 0, s, src, H, W, rpr, *P, sums, out_u8, out_chw);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_augment_u8(const uint8_t* src, int B, int H, int W, const apse_augment_params* params, uint8_t* out_u8, float* out_chw,
                    unsigned long long* sums, void* stream) {
    char msg[160];
    if (H < 1 || W < 1 || H > APSE_MAX_FRAME_H || W > APSE_MAX_FRAME_W) {
        snprintf(msg, sizeof msg, "apse_augment_u8: image %d x %d outside 1..%d x 1..%d", H, W, APSE_MAX_FRAME_H, APSE_MAX_FRAME_W);
        return invalid(msg);
    }
    if (B < 1 || B > APSE_AUGMENT_MAX_BATCH) {
        snprintf(msg, sizeof msg, "apse_augment_u8: batch %d outside 1..%d", B, APSE_AUGMENT_MAX_BATCH);
        return invalid(msg);
    }
    if (!src || !sums || !params) return invalid("apse_augment_u8: src, params and sums must not be NULL");
    if (!out_u8 && !out_chw) return invalid("apse_augment_u8: out_u8 and out_chw are both NULL");
    const size_t bytes = (size_t)B * H * W * 3;
    if (out_u8 && reinterpret_cast<uintptr_t>(out_u8) < reinterpret_cast<uintptr_t>(src) + bytes &&
        reinterpret_cast<uintptr_t>(src) < reinterpret_cast<uintptr_t>(out_u8) + bytes)
        return invalid("apse_augment_u8: out_u8 overlaps src (pass 2 reads src again)");
    AugmentBatch P;
    memset(&P, 0, sizeof P);
    static_assert(sizeof(P.im) / sizeof(P.im[0]) == APSE_AUGMENT_MAX_BATCH && sizeof(AugmentBatch) <= 3840, "the per-image parameters travel as a kernel argument (4 KiB in all)");
    for (int b = 0; b < B; ++b) {
        const apse_augment_params& p = params[b];
        AugmentImage& a = P.im[b];
        a.flip = p.flip != 0;
        a.wb = (float)p.brightness;
        a.ws = (float)p.saturation;
        a.wc = (float)p.contrast;
        a.one_minus_ws = 1.0 - p.saturation;
        a.one_minus_wc = 1.0 - p.contrast;
        for (int c = 0; c < 3; ++c) a.vec[c] = p.lighting_vec[c];
    }
    return apse_k_augment(src, B, H, W, &P, out_u8, out_chw, sums, (hipStream_t)stream);
}

}  // extern "C"
