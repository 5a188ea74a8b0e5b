// Fused f32 Winograd F(2x2, 3x3) convolution for gfx950 (CDNA4), exact-f32 MFMA (v_mfma_f32_32x32x2_f32).
//
// Takes the 3x3 / stride 1 / pad 1 layers of the f32 mode that the plan names (FPN outputs p2 / p3, RPN conv at p2 / p3 and, in
// plans of large frames, the trunk's conv2 layers and the p4 pair: plan.hip add_conv).  16 instead of 36 multiplies per 2x2
// output block: 2.25x fewer matrix-pipe FLOPs.
//
//   U[xi][co][ci] = (G g G^T)[i][j]   filters, transformed once on the host (float64, rounded once), xi = 4 i + j
//   V[xi][t][ci]  = (B^T d B)[i][j]   input tile t (4x4 pixels, stride 2), computed here on VALU per k-slice
//   M[xi][t][co]  = sum_ci V * U      16 independent GEMMs on the matrix pipe, channels ascending
//   Y[t][co]      = A^T M A + bias    (2x2 output pixels), ReLU optional
// Nothing transformed goes through HBM: V lives in LDS for one k-slice, M in accumulators until the epilogue.
//
// Block = 512 threads = 8 waves, one block per CU (128 KiB LDS).  Block tile = 64 Winograd tiles (WTR x WTC tile rows x
// columns: 16 x 4 = 32 x 8 output pixels, or 8 x 8 = 16 x 16) x 64 output channels.  Wave w owns xi = 2w, 2w+1: 2 xi x 2 M-tiles x 2 N-tiles of 32x32
// = 128 accumulators per lane.  Per k-slice of 8 channels (double-buffered, one barrier):
//   - 512 threads = (tile t, transform row i, channel group cg of 4): two input rows x 4 pixels x 4 channels through a
//     buffer descriptor (out-of-image taps get an offset past the range: zeros, i.e. the padding and partial tiles at odd
//     H / W), row combination then column combination -> V[4 i + j][t][cg] into LDS
//   - the U slice [16][64 co][8] is one contiguous 2 KiB run per xi (global layout [Cin/8][16][Cout][8])
//   - LDS rows are 8 floats (32 B): the 16-byte half a lane reads is XOR-swizzled with (row >> 3) & 1, so the ds_read_b128
//     fragment reads (lane half h takes channels 4 h .. 4 h + 3 for the four k-steps) are bank-conflict-free
// Schedule of the k loop (one basic block per slice; 256 VGPRs, no scratch, 2 waves per SIMD): slice s + 1 sits in one register set,
// fetched a slice ahead; its U hand-over, row transform and column transform + V hand-over are pinned in front of MFMA groups
// 1, 2 and 3 of slice s (sched_barrier), each followed by the fetch of slice s + 2 into the registers it freed.  The second
// xi's fragments are read behind the first xi's MFMAs, and the slice's last MFMA group runs after the barrier, behind the
// next slice's first fragment reads.  Every accumulator still takes its products channel-ascending, one k-step after the
// other, and the transforms keep their operation order: the bits are those of the unscheduled loop.  The loop carries no
// address arithmetic: the slice displacement of the twelve fetches is their scalar offset, and the loop runs two slices per
// round so that the LDS buffer parity is a constant of each copy (instruction offsets); the only vector ALU work of a slice
// is the transform (32 instructions; profiles/r11b_resource_usage.txt).
// Epilogue: per 32-channel half of the N tile the accumulators go to LDS as [16][64 t][32 co]; each thread then owns one
// tile x 4 channels, applies A^T . A, bias, ReLU and stores the 2x2 pixels as dwordx4 (pixels past H / W are dropped).
// No atomics: a tile's result depends on nothing but its inputs (not on batch, grid or history).  The Cin split (SPLIT, below)
// writes partial tiles into workspace slabs that conv_splitk_reduce4 sums in a fixed order.
#include "apse_common.h"
#include <type_traits>

namespace {
constexpr int WT = 64;                    // Winograd tiles per block: WTR rows x WTC columns, a template parameter of the kernel
constexpr int WN = 64;                    // output channels per block
constexpr int KC = 8;                     // channels per k-slice
constexpr int NTHR = 512;
// MFMA group (0..6 of a slice's eight) in front of which each piece of the next slice's staging is issued: the U hand-over,
// the row transform, the column transform + V hand-over.  Measured at out2 shape: 1/2/3 353.7 us, 0/1/2 361.4, 2/3/4 358.4,
// 0/2/4 368.4 (HISTORY.md)
constexpr int G_U = 1, G_ROWS = 2, G_V = 3;
constexpr int SLICE_F = 16 * WT * KC;     // floats of V (and of U: WN == WT) per k-slice buffer
constexpr size_t WINO_LDS = (size_t)2 * 2 * SLICE_F * sizeof(float);     // [2 buffers][V, U] = 128 KiB
static_assert(WN == WT, "V and U slices share one size");
static_assert((size_t)16 * WT * 32 * sizeof(float) <= WINO_LDS, "epilogue chunk must fit the staging LDS");
}

// <WTR, WTC>: block geometry, <16, 4> = 32 x 8 output pixels (geometry 0), <8, 8> = 16 x 16 (geometry 1: fewer blocks on small
// maps, 18 instead of 22 at 48 x 84).  SPLIT: the Cin split.  blockIdx.y = z multiplies only the k-slices [s_begin, s_end) of its
// share (whole 8-channel slices divided as evenly as possible, larger shares first), applies A^T . A but neither bias nor ReLU and
// writes its 2x2 pixels into slab z of the workspace (p.ws + z M Cout, dense NHWC, ld = Cout): the layout conv_splitk_reduce4
// sums, z ascending, then bias, then ReLU.  The output transform is linear, so the partial Y tiles add up to the whole one.
template <int WTR, int WTC, bool SPLIT>
__global__ __launch_bounds__(NTHR) void conv_winograd_f32(const ConvParams p) {
    static_assert(WTR * WTC == WT, "64 tiles per block");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Vs = reinterpret_cast<float*>(smem);          // [2][16][WT][KC]
    float* Us = Vs + 2 * SLICE_F;                         // [2][16][WN][KC]
    float* Cs = reinterpret_cast<float*>(smem);          // epilogue view [16][WT][32]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;

    // block -> (image, tile strip, N tile) in XCD-aware order: the four N tiles of one input patch run on the same L2
    const int tiles_y = (p.OH + 2 * WTR - 1) / (2 * WTR), tiles_x = (p.OW + 2 * WTC - 1) / (2 * WTC);
    const int nblk = p.Cout / WN;
    const int nwg = p.B * tiles_y * tiles_x * nblk;
    const int bid = apse_xcd_remap(blockIdx.x, nwg);
    const int nb = bid % nblk;
    int rest = bid / nblk;
    const int bx = rest % tiles_x; rest /= tiles_x;
    const int by = rest % tiles_y;
    const int b = rest / tiles_y;
    const int oy0 = by * 2 * WTR, ox0 = bx * 2 * WTC, n0 = nb * WN;
    const int C = 1 << p.cin_log2;
    int s_begin = 0, s_end = C / KC;
    if constexpr (SPLIT) {
        const int z = blockIdx.y, share = s_end / p.splitk, extra = s_end % p.splitk;
        s_begin = z * share + (z < extra ? z : extra);
        s_end = s_begin + share + (z < extra ? 1 : 0);
    }
    const int nsteps = s_end - s_begin;

    // ---- staging roles
    // input: thread = (transform row i, tile t, channel group cg); rows ra / rb of the 4x4 tile give row i of B^T d.  The row
    // index i = wave >> 1 is wave-uniform: rows ra / rb combine as ra + sgn * rb with sgn = +-1 in an SGPR (the product is
    // exact, so the fma rounds exactly like the add / subtract it stands for)
    const int cg = tid & 1, t = (tid >> 1) & (WT - 1), ti = wave >> 1;
    const int ra = ti == 0 ? 0 : (ti == 2 ? 2 : 1);
    const int rb = ti == 0 ? 2 : (ti == 1 ? 2 : (ti == 2 ? 1 : 3));
    const float sgn = ti == 1 ? 1.f : -1.f;
    const int iy_a = oy0 + 2 * (t / WTC) - 1 + ra, iy_b = oy0 + 2 * (t / WTC) - 1 + rb;
    const int ix0 = ox0 + 2 * (t % WTC) - 1;
    const __amdgpu_buffer_rsrc_t xrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)((((unsigned)(p.B * p.H * p.W)) << p.cin_log2) * 4u), 0x00020000);
    // an empty range for the fetches of slices past the last one, which the loop issues unconditionally: zeros, no memory access
    const __amdgpu_buffer_rsrc_t xnone = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, 0, 0x00020000);
    // byte offset of channel 0 of the thread's channel group at each of its 8 taps; a tap outside the image gets a base past
    // any range (the launcher keeps the activation tensor below 2 GiB), so every k-slice's load of it returns zeros
    unsigned xoff[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int iy = r ? iy_b : iy_a;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ix = ix0 + c;
            const bool in = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            xoff[r][c] = in ? ((((unsigned)((b * p.H + iy) * p.W + ix)) << p.cin_log2) + (unsigned)(cg * 4)) * 4u : 0x80000000u;
        }
    }
    // U: four 16-byte pieces per thread, piece q = tid + 512 k: xi = q >> 7, row co = (q >> 1) & 63, half q & 1.  Read through
    // a descriptor of the whole U (16 * Cout * Cin floats, slice-major): a slice past the last one is out of its range
    // (of a split: of the slices in front of s_end, so that the fetches past the share read nothing of the next split's)
    const unsigned ustep = (unsigned)(16 * p.Cout * KC * 4);     // bytes per k-slice of the global U
    const __amdgpu_buffer_rsrc_t ursrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.wu), 0, SPLIT ? (int)((unsigned)s_end * ustep) : (int)((((unsigned)(16 * p.Cout)) << p.cin_log2) * 4u), 0x00020000);
    unsigned uoff[4], ulds[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = tid + NTHR * k;
        const int xi = q >> 7, co = (q >> 1) & 63, h = q & 1;
        uoff[k] = (unsigned)(((xi * p.Cout + n0 + co) * KC + h * 4) * 4);
        ulds[k] = (unsigned)((xi * WN + co) * KC + ((h ^ ((co >> 3) & 1)) * 4));
    }
    const int vlds = (4 * ti * WT + t) * KC + (cg ^ ((t >> 3) & 1)) * 4;

    // one register set: a slice is fetched one slice ahead of the MFMAs that use it and handed to LDS inside the MFMA stream
    // of the slice before (see the loop)
    // The slice's displacement kb is wave-uniform and rides in the loads' scalar offset: the twelve per-lane offsets stay what
    // they were in front of the loop.  A tap outside the image keeps its base of 2 GiB, past any range with or without kb; a
    // slice past the last one (of a split: past the share) reads through the empty range.
    const __amdgpu_buffer_rsrc_t unone = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wu), 0, 0, 0x00020000);
    f32x4 xr[2][4], ur[4];
    auto fetch_u = [&](int s) {
        const int kb = (int)((unsigned)(s_begin + s) * ustep);
        const __amdgpu_buffer_rsrc_t rs = s < nsteps ? ursrc : unone;
#pragma unroll
        for (int k = 0; k < 4; ++k) ur[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)uoff[k], kb, 0));
    };
    auto fetch_x = [&](int s) {
        const int kb = (s_begin + s) * KC * 4;
        const __amdgpu_buffer_rsrc_t rs = s < nsteps ? xrsrc : xnone;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                xr[r][c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)xoff[r][c], kb, 0));
    };
    auto write_u = [&](int buf) {
#pragma unroll
        for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4*>(Us + buf * SLICE_F + ulds[k]) = ur[k];
    };
    // row i of B^T d (4 pixels x 4 channels), in place in xr[0]
    auto xform_rows = [&]() {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) xr[0][c][e] = __builtin_fmaf(xr[1][c][e], sgn, xr[0][c][e]);
    };
    // the column combinations: V[4 i + j]
    auto write_v = [&](int buf) {
        const f32x4 v[4] = {xr[0][0] - xr[0][2], xr[0][1] + xr[0][2], xr[0][2] - xr[0][1], xr[0][1] - xr[0][3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(Vs + buf * SLICE_F + vlds + j * WT * KC) = v[j];
    };

    f32x16 acc[2][2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[a][i][j][v] = 0.f;

    fetch_u(0);
    fetch_x(0);
    write_u(0);
    xform_rows();
    write_v(0);
    __builtin_amdgcn_sched_barrier(0);                   // the loop counts on this order: U of a slice is requested before its taps
    fetch_u(1);
    __builtin_amdgcn_sched_barrier(0);
    fetch_x(1);
    __syncthreads();
    // The k loop.  Slice s is multiplied from LDS buffer s & 1 while slice s + 1, fetched during slice s - 1, goes through the
    // transform into the other buffer and slice s + 2 is requested, each piece pinned into its own gap of the MFMA stream: the
    // two waves of a SIMD and the eight waves of the block do not all stop multiplying at once, and the last MFMA group of a
    // slice runs behind the barrier, over the next slice's first fragment reads.  One basic block per slice: the last two slices hand over
    // and fetch past the end (zeros into a buffer nobody reads) rather than branch.
    const int fsw = (fh ^ ((fr >> 3) & 1)) * 4;          // swizzled half of the fragment rows (row & 15 == fr & 15)
    const int frag = (2 * wave * WT + fr) * KC + fsw;
    f32x4 af[2][2], bf[2][2];
    auto read_frags = [&](int buf, int a) {
#pragma unroll
        for (int i = 0; i < 2; ++i) af[a][i] = *reinterpret_cast<const f32x4*>(Vs + buf * SLICE_F + frag + (a * WT + 32 * i) * KC);
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[a][j] = *reinterpret_cast<const f32x4*>(Us + buf * SLICE_F + frag + (a * WN + 32 * j) * KC);
    };
    auto mfma_group = [&](int a, int k) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[a][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a][i][k], bf[a][j][k], acc[a][i][j], 0, 0, 0);
    };
    read_frags(0, 0);
    // one slice; BUF = s & 1 is a compile-time constant (the loop below runs two slices per round), so every LDS address of
    // the slice is a per-lane base fixed in front of the loop plus an instruction offset
    auto slice = [&](auto BUF, int s) {
        constexpr int buf = decltype(BUF)::value;
        read_frags(buf, 1);                              // lands behind the first xi's MFMAs
#pragma unroll
        for (int g = 0; g < 7; ++g) {                    // MFMA groups 0..6 of the slice: (xi, k-step) = (g >> 2, g & 3)
            __builtin_amdgcn_sched_barrier(0);
            if (g == G_U) { write_u(buf ^ 1); fetch_u(s + 2); }
            if (g == G_ROWS) xform_rows();
            if (g == G_V) { write_v(buf ^ 1); fetch_x(s + 2); }
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(g >> 2, g & 3);
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                  // buf ^ 1 is complete; buf is in registers and may be rewritten
        read_frags(buf ^ 1, 0);                          // the next slice's first fragments, behind this slice's last group
        __builtin_amdgcn_sched_barrier(0);
        mfma_group(1, 3);
    };
    for (int s = 0; s < nsteps; s += 2) {
        slice(std::integral_constant<int, 0>{}, s);
        if (s + 1 < nsteps) slice(std::integral_constant<int, 1>{}, s + 1);
    }

    // ---- epilogue, one 32-channel half of the N tile at a time
    const int et = tid >> 3, eg = tid & 7;               // tile, group of 4 channels
    const int oy = oy0 + 2 * (et / WTC), ox = ox0 + 2 * (et % WTC);
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int row = 32 * i + (v & 3) + 8 * (v >> 2) + 4 * fh;
                    Cs[((2 * wave + a) * WT + row) * 32 + fr] = acc[a][i][j][v];
                }
        __syncthreads();
        f32x4 m[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = *reinterpret_cast<const f32x4*>(Cs + (k * WT + et) * 32 + eg * 4);
        f32x4 s0[4], s1[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s0[c] = m[c] + m[4 + c] + m[8 + c];
            s1[c] = m[4 + c] - m[8 + c] - m[12 + c];
        }
        const int co = n0 + 32 * j + 4 * eg;
        if constexpr (SPLIT) {
            // a partial sum: plain stores (the reduce kernel reads the slabs next), bias and ReLU are the reduce's
            float* slab = p.ws + (size_t)blockIdx.y * p.M * p.Cout;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const f32x4 val = dy ? (dx ? s1[1] - s1[2] - s1[3] : s1[0] + s1[1] + s1[2]) : (dx ? s0[1] - s0[2] - s0[3] : s0[0] + s0[1] + s0[2]);
                    if (oy + dy < p.OH && ox + dx < p.OW)
                        *reinterpret_cast<f32x4*>(slab + ((size_t)(b * p.OH + oy + dy) * p.OW + ox + dx) * p.Cout + co) = val;
                }
            __syncthreads();
            continue;
        }
        const f32x4 bias4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 y[2][2] = {{s0[0] + s0[1] + s0[2], s0[1] - s0[2] - s0[3]}, {s1[0] + s1[1] + s1[2], s1[1] - s1[2] - s1[3]}};
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                f32x4 val = y[dy][dx] + bias4;
                if (p.relu) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) val[k] = apse_relu(val[k]);
                }
                if (oy + dy < p.OH && ox + dx < p.OW)
                    APSE_NT_STORE(val, reinterpret_cast<f32x4*>(p.y + ((size_t)(b * p.OH + oy + dy) * p.OW + ox + dx) * p.y_ld + p.y_coff + co));
            }
        __syncthreads();                                  // Cs is rewritten by the next half
    }
}

// the layers this kernel handles: f32 in / out, 3x3 / stride 1 / pad 1, whole 64-channel N tiles, 8-channel k-slices, plain
// NHWC output with 16-byte aligned rows, no residual, activations below 2 GiB (32-bit descriptor offsets, see xoff); a Cin
// split of at most one share per k-slice, block geometry 0 (<16, 4>) or 1 (<8, 8>)
bool apse_conv_winograd_ok(const ConvParams& p, int max_items) {
    return p.prec == 0 && p.x_st == 0 && p.y_st == 0 && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.out_mode == 0 &&
           p.res_mode == 0 && p.Cout % WN == 0 && p.cin_log2 >= 3 && p.splitk >= 1 && p.splitk <= (1 << p.cin_log2) / KC &&
           (p.wino_geom == 0 || p.wino_geom == 1) && p.OH == p.H && p.OW == p.W &&
           (p.y_ld & 3) == 0 && (p.y_coff & 3) == 0 && ((((size_t)max_items * p.H * p.W) << p.cin_log2) * 4 < 0x7fff0000ull);
}

// spatial blocks x N tiles of one image in geometry p.wino_geom (64 Winograd tiles x 64 output channels each); a split launch
// runs p.splitk times as many
int apse_conv_winograd_blocks(const ConvParams& p) {
    const int wtr = p.wino_geom ? 8 : 16, wtc = p.wino_geom ? 8 : 4;
    return ((p.OH + 2 * wtr - 1) / (2 * wtr)) * ((p.OW + 2 * wtc - 1) / (2 * wtc)) * (p.Cout / WN);
}

template <int WTR, int WTC, bool SPLIT>
static void launch_wino(const ConvParams& p, int grid, hipStream_t s) {
    static bool attr_done = false;
    if (!attr_done) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_winograd_f32<WTR, WTC, SPLIT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)WINO_LDS);
        attr_done = true;
    }
    hipLaunchKernelGGL((conv_winograd_f32<WTR, WTC, SPLIT>), dim3(grid, SPLIT ? p.splitk : 1), dim3(NTHR), WINO_LDS, s, p);
}

// ev0 / ev1 bracket the Winograd kernel itself; the reduce pass of a split launch follows ev1 (as in apse_launch_conv)
int apse_launch_conv_winograd(const ConvParams& p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (!p.wu || !apse_conv_winograd_ok(p, p.B) || p.m_count) return APSE_E_INVALID;
    const bool split = p.splitk > 1;
    // the slabs are [splitk][M][Cout] with M = B OH OW, summed four columns at a time with 32-bit element indices
    if (split && (!p.ws || p.tile_cnt || p.M != p.B * p.OH * p.OW || (size_t)p.M * p.Cout >= 0x7fffffffull)) return APSE_E_INVALID;
    const int grid = p.B * apse_conv_winograd_blocks(p);
    if (ev0) hipEventRecord(ev0, s);
    if (p.wino_geom == 0) { if (split) launch_wino<16, 4, true>(p, grid, s); else launch_wino<16, 4, false>(p, grid, s); }
    else { if (split) launch_wino<8, 8, true>(p, grid, s); else launch_wino<8, 8, false>(p, grid, s); }
    if (ev1) hipEventRecord(ev1, s);
    if (split) apse_launch_splitk_reduce4(p, s);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}
