// Optional frame pre-processing (gfx950): undistort + Lab-L gamma, one kernel, u8 BGR in -> u8 BGR out.
// Replaces preprocess_img of /root/reference/dcnn/scripts/tests/visualize_uav.py:56-71 (cv2.undistort,
// cvtColor RGB2LAB, LUT on L, cvtColor LAB2RGB; same maths in aruco_detect.py:250-259).
// The per-pixel arithmetic lives in preproc_pixel.h; inside a context the same function feeds the horizontal resize pass
// directly (apse_set_camera -> pil_resize_h<true>), so this stand-alone form (24.9 MB read + 24.9 MB written per 4K frame)
// is the stateless operator of the tests / FramePreprocessor only.
#include "apse_kernels.h"
#include "preproc_pixel.h"

__global__ __launch_bounds__(256) void undistort_gamma(const UndistortParams p, const uint8_t* __restrict__ src,
                                                       uint8_t* __restrict__ dst, const LabTables* __restrict__ lab) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int b = blockIdx.z;
    if (x >= p.W) return;
    const uint8_t* s = src + (size_t)b * p.H * p.W * 3;
    int c0, c1, c2;
    undistort_gamma_pixel(p, s, lab, x, y, c0, c1, c2);
    uint8_t* o = dst + (((size_t)b * p.H + y) * p.W + x) * 3;
    o[0] = (uint8_t)c0; o[1] = (uint8_t)c1; o[2] = (uint8_t)c2;
}

// YUV 4:2:0 (NV12 with a pitch / packed I420) -> BGR [B][H][W][3], the stand-alone form of yuv_quad_bgr (preproc_pixel.h): what
// a context with a camera set runs in front of its fused undistort pass, and utils/preprocess.yuv_to_bgr.  A thread owns a
// 4 x 2 block of pixels -- two luma dwords, the one chroma row under them fetched once, 2 x 12 output bytes -- through dword
// loads / stores where the row it touches is dword-aligned and the four pixels exist, and byte by byte otherwise (an odd pitch,
// an offset pointer, a width that is no multiple of 4: the last columns; an odd height: the last row has no partner).  Every
// byte read is a luma byte (x, y) or a chroma byte of sample (x >> 1, y >> 1) of an existing pixel: nothing past the batch.
__global__ __launch_bounds__(256) void yuv_to_bgr(const YuvSource p, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                  size_t frame_bytes) {
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int y0 = blockIdx.y * 2, b = blockIdx.z;
    if (x0 >= p.W) return;
    const int n = p.W - x0 < 4 ? p.W - x0 : 4, np = (n + 1) >> 1;
    const uint8_t* f = src + (size_t)b * frame_bytes;
    const int CH = (p.H + 1) >> 1, CW = (p.W + 1) >> 1, cy = y0 >> 1;
    int U[2] = {128, 128}, V[2] = {128, 128};
    if (p.format == 0) {
        const uint8_t* c = f + (size_t)(p.H + cy) * p.pitch + x0;          // (x0 >> 1) pairs of two bytes
        if (n == 4 && (reinterpret_cast<uintptr_t>(c) & 3) == 0) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(c);
            U[0] = w & 0xffu; V[0] = (w >> 8) & 0xffu; U[1] = (w >> 16) & 0xffu; V[1] = w >> 24;
        } else {
            for (int j = 0; j < np; ++j) { U[j] = c[2 * j]; V[j] = c[2 * j + 1]; }
        }
    } else {
        const uint8_t* cu = f + (size_t)p.H * p.W + (size_t)cy * CW + (x0 >> 1);
        const uint8_t* cv = cu + (size_t)CH * CW;
        for (int j = 0; j < np; ++j) { U[j] = cu[j]; V[j] = cv[j]; }
    }
    const int lp = p.format == 0 ? p.pitch : p.W;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        if (y >= p.H) break;
        const uint8_t* l = f + (size_t)y * lp + x0;
        uint32_t y4 = 0;
        if (n == 4 && (reinterpret_cast<uintptr_t>(l) & 3) == 0) y4 = *reinterpret_cast<const uint32_t*>(l);
        else for (int k = 0; k < n; ++k) y4 |= (uint32_t)l[k] << (8 * k);
        uint32_t o3[3];
        yuv_quad_bgr(p.m, y4, U[0], V[0], U[1], V[1], o3);
        uint8_t* o = dst + (((size_t)b * p.H + y) * p.W + x0) * 3;
        if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
            o4[0] = o3[0]; o4[1] = o3[1]; o4[2] = o3[2];
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (k < n * 3) o[k] = (uint8_t)(o3[k >> 2] >> (8 * (k & 3)));
        }
    }
}
extern "C" int apse_k_yuv_to_bgr(const YuvSource* p, const uint8_t* src, uint8_t* dst, int B, hipStream_t s) {
    hipLaunchKernelGGL(yuv_to_bgr, dim3(((p->W + 3) / 4 + 255) / 256, (p->H + 1) / 2, B), dim3(256), 0, s, *p, src, dst, yuv_frame_bytes(*p));
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

// Built once per camera (apse_set_camera): the remap table of the fused path.
// The compact form (4 bytes per pixel, preproc_pixel.h); *overflow counts pixels inside the frame whose displacement does not fit.
__global__ __launch_bounds__(256) void undistort_build_map_compact(const UndistortParams p, uint32_t* __restrict__ map, int* __restrict__ overflow) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= p.W) return;
    map[(size_t)y * p.W + x] = undistort_map_compact(p, x, y, overflow);
}
extern "C" int apse_k_undistort_build_map_compact(const UndistortParams* p, void* map, int* overflow_dev, hipStream_t s) {
    hipLaunchKernelGGL(undistort_build_map_compact, dim3((p->W + 255) / 256, p->H), dim3(256), 0, s, *p, reinterpret_cast<uint32_t*>(map), overflow_dev);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

extern "C" int apse_k_undistort_gamma(const UndistortParams* p, const uint8_t* src, uint8_t* dst, const LabTables* lab, int B,
                                      hipStream_t s) {
    hipLaunchKernelGGL(undistort_gamma, dim3((p->W + 255) / 256, p->H, B), dim3(256), 0, s, *p, src, dst, lab);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
