// What the training GEMMs (mask_train.hip: wgrad_mfma, conv3x3_mfma; box_train.hip: fc_gemm) share.  Internal device header:
// included by those two files, and by rpn_train.hip for block_sum_d.
//
// The tile.  A block of 256 threads owns a 128 x 128 tile of C = A B: 4 waves as 2 x 2, each 2 x 2 MFMA tiles of 32 x 32
// (v_mfma_f32_32x32x2_f32).  The reduction runs in stages of kKT = 32 steps through an LDS double buffer; the global loads of
// the next stage fly under the MFMAs of the current one.  Inside a stage, MFMA kk takes reduction steps 2 kk (lanes 0..31) and
// 2 kk + 1 (lanes 32..63).
//
// The summation order (DESIGN.md "Mask-head training").  The MFMA chain runs over kFlush = 2 stages (64 reduction steps), then
// joins the running total, and once more after the last stage -- chains stay short, which keeps the rounding error of a long
// reduction near that of a blocked sum.  The order depends on the number of stages only; the lattice and determinism tests of
// both trainers lean on it, and launch_gemm (box_train.hip) cuts its forward chunks at whole chains.
//
// The stage loop itself is still written out in each of the three kernels.  One shared, inlined loop taking fetch / stage / read
// callables computes the same bits, but hipcc (ROCm 7.2) schedules it differently: it pairs wgrad_mfma's LDS reads inside a
// k step instead of across k steps and carries 94 more register moves per stage (3.5 % slower at 64 and 256 RoIs), and fc1's
// forward runs 2-5 % slower.  The code generation of these kernels is that touchy throughout: wgrad_mfma keeps its own staging
// loop (stage_major's layout with the A and B stores interleaved; A first, then B, cost 0.6 us of 74 at 16 RoIs), and a shared
// helper for the C/D row formula rescheduled all three fc_gemm.  Whoever writes a fourth kernel of this kind copies the loop of
// fc_gemm and keeps these constants.
#pragma once
#include "apse_common.h"

#ifdef __HIPCC__
constexpr int kKT = 32;                  // reduction steps per stage
constexpr int kFlush = 2;                // stages per MFMA chain before it joins the running total

// Reduction-major operand layout: element (idx, k) of a 128-wide operand tile sits at s[k * kLdMajor + idx].  A lane's operand is
// one ds_read_b32, the 32 lanes of a k read consecutive floats, and with a row stride of 160 floats the two k rows of one
// instruction fall into different bank halves.  Thread t stages rows (t >> 5) + 8 i, one float4 at column 4 (t & 31).
constexpr int kLdMajor = 160;
constexpr int kMajorFloats = kKT * kLdMajor;
__device__ __forceinline__ void stage_major(float* __restrict__ s, int t, const f32x4 (&reg)[4]) {
    const int row = t >> 5, c4 = t & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(s + (row + 8 * i) * kLdMajor + c4 * 4) = reg[i];
}
__device__ __forceinline__ float read_major(const float* __restrict__ s, int idx, int k) { return s[k * kLdMajor + idx]; }

__device__ __forceinline__ double block_sum_d(double v, double* red) {       // fixed-shape tree over 256 threads
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
#endif
