// RPN-head training (include/apse_hip.h "RPN-head training"): the f32 kernels behind fine-tuning proposal_generator.rpn_head.conv /
// objectness_logits / anchor_deltas of a frozen FPN detector (StandardRPNHead, RPNOutputs._get_ground_truth and RPNOutputs.losses of
// detectron2 0.1.2).  DESIGN.md "RPN-head training" gives the rules.
//
//   labels   pairwise_iou + Matcher([0.3, 0.7], [0, -1, 1], allow_low_quality_matches = True) over the anchors of the five levels,
//            which are generated here from (level, y, x, a) exactly as rpn_decode (select_nms.hip) generates them.  Three launches:
//              label_pass<false>  one thread per anchor (four anchors each, 1024 per block) over ground truths staged in LDS: the
//                                 best ground truth (ties to the lowest index), the thresholded label, and per block and ground
//                                 truth the maximum IoU of the block's anchors (an integer max in LDS on the bits of IoU >= 0)
//              gt_max_reduce      per ground truth the maximum of the blocks' maxima, in block order
//              label_pass<true>   the same IoUs again; an anchor whose IoU to some ground truth EQUALS that ground truth's maximum
//                                 gets label 1 (Matcher.set_low_quality_matches_, literally: a maximum of 0 included)
//   gather   X[s] = the 3 x 3 x 256 patch around sampled anchor s on its own level in (c, kh, kw) order, zeros outside the map:
//            rpn_head.conv becomes an FC layer on box_train.hip's GEMM entries with the checkpoint's weight as it is.
//   loss     binary cross-entropy with logits on column `slot` of the S rows + smooth_l1 on columns 4 slot .. 4 slot + 3 of the
//            positive rows against Box2BoxTransform(1, 1, 1, 1).get_deltas(anchor, gt), both sums x 1 / norm; the logged counts;
//            and both gradients, exactly 0 outside a row's own columns.
// Determinism: no float atomics; every sum has a fixed order that depends on the shapes only.
#include "apse_kernels.h"
#include "train_tile.h"
#include "../../include/apse_hip.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kMaxGt = 4096;                // ground truths per image
constexpr int kMaxAnchors = 1 << 22;
constexpr int kMaxRows = 1 << 20;           // sampled anchors per call (gather, loss)
constexpr int kGtChunk = 1024;
constexpr int kPerThread = 4, kPerBlock = 256 * kPerThread;      // anchors per thread / block of the labelling passes
constexpr int kPatch = 9 * 256;             // floats per gathered row

int invalid(const char* msg) { return apse_fail_global(APSE_E_INVALID, msg); }
int launched() { return hipGetLastError() == hipSuccess ? APSE_OK : apse_fail_global(APSE_E_HIP, "rpn_train: kernel launch failed"); }

// ---------------------------------------------------------------------------------------------------------------- anchors
// Anchor i of the (level, y, x, a) order: the box rpn_decode computes for the same element, and its level / position / slot.
struct AnchorAt { f32x4 box; int level, y, x, slot; };
__device__ __forceinline__ AnchorAt anchor_at(const RpnAnchorGrid& g, int i) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k) l += i >= g.off[k];
    const int e = i - g.off[l];
    const int pix = e / 3, an = e - pix * 3;
    const int y = pix / g.W[l], x = pix - y * g.W[l];
    const float sx = (float)(x * g.stride[l]), sy = (float)(y * g.stride[l]);
    AnchorAt r;
    r.box = f32x4{sx + g.base[l][an][0], sy + g.base[l][an][1], sx + g.base[l][an][2], sy + g.base[l][an][3]};
    r.level = l; r.y = y; r.x = x; r.slot = an;
    return r;
}

// detectron2 pairwise_iou(gt_boxes, anchors): boxes1 = ground truths (the formula apse_box_match documents)
__device__ __forceinline__ float iou_gt_anchor(const f32x4 g, const f32x4 p, float area_p) {
    const float area_g = (g[2] - g[0]) * (g[3] - g[1]);
    float w = fminf(g[2], p[2]) - fmaxf(g[0], p[0]);
    float h = fminf(g[3], p[3]) - fmaxf(g[1], p[1]);
    w = w > 0.f ? w : 0.f;
    h = h > 0.f ? h : 0.f;
    const float inter = w * h;
    return inter > 0.f ? inter / (area_g + area_p - inter) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- labels
// FINAL = false: matched_idx, matched_iou, the thresholded label and blockmax[block][g].  FINAL = true: label 1 where an IoU equals
// gtmax[g].  Both passes evaluate iou_gt_anchor on the same operands, so the comparison is between identical bits.
template <bool FINAL>
__global__ __launch_bounds__(256) void label_pass(RpnAnchorGrid grid, int A, const float* __restrict__ gts, int G, float lo, float hi,
                                                  uint32_t* __restrict__ blockmax, const float* __restrict__ gtmax,
                                                  int* __restrict__ labels, int* __restrict__ midx, float* __restrict__ miou) {
    __shared__ f32x4 sg[kGtChunk];
    __shared__ uint32_t smax[kGtChunk];          // FINAL: the bits of gtmax; else the block's running maxima
    const int t = threadIdx.x;
    f32x4 p[kPerThread];
    float area[kPerThread], best[kPerThread];
    int bi[kPerThread];
    bool live[kPerThread], low[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = blockIdx.x * kPerBlock + k * 256 + t;
        live[k] = i < A;
        p[k] = live[k] ? anchor_at(grid, i).box : f32x4{0.f, 0.f, 0.f, 0.f};
        area[k] = (p[k][2] - p[k][0]) * (p[k][3] - p[k][1]);
        best[k] = 0.f; bi[k] = 0; low[k] = false;
    }
    for (int g0 = 0; g0 < G; g0 += kGtChunk) {
        const int cnt = min(kGtChunk, G - g0);
        for (int j = t; j < cnt; j += 256) {
            const float* gb = gts + (size_t)(g0 + j) * 4;          // element loads: the caller's boxes need no 16-byte alignment
            sg[j] = f32x4{gb[0], gb[1], gb[2], gb[3]};
            smax[j] = FINAL ? __float_as_uint(gtmax[g0 + j]) : 0u;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const f32x4 g = sg[j];
#pragma unroll
            for (int k = 0; k < kPerThread; ++k) {
                if (!live[k]) continue;
                const float iou = iou_gt_anchor(g, p[k], area[k]);
                if (FINAL) {
                    low[k] = low[k] || iou == __uint_as_float(smax[j]);
                } else {
                    if (iou > best[k]) { best[k] = iou; bi[k] = g0 + j; }      // strict: ties keep the lowest index
                    if (iou > 0.f) atomicMax(&smax[j], __float_as_uint(iou));   // IoU >= 0: its bits order as the values do
                }
            }
        }
        __syncthreads();
        if (!FINAL)
            for (int j = t; j < cnt; j += 256) blockmax[(size_t)blockIdx.x * G + g0 + j] = smax[j];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = blockIdx.x * kPerBlock + k * 256 + t;
        if (!live[k]) continue;
        if (FINAL) {
            if (low[k]) labels[i] = 1;
        } else {
            midx[i] = bi[k];
            miou[i] = best[k];
            labels[i] = G == 0 ? 0 : (best[k] >= hi ? 1 : (best[k] >= lo ? -1 : 0));
        }
    }
}

// gtmax[g] = max over the blocks, in block order, of blockmax[block][g]
__global__ void gt_max_reduce(const uint32_t* __restrict__ blockmax, int blocks, int G, float* __restrict__ gtmax) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    uint32_t v = 0u;
    for (int b = 0; b < blocks; ++b) { const uint32_t u = blockmax[(size_t)b * G + g]; v = u > v ? u : v; }
    gtmax[g] = __uint_as_float(v);
}

int label_blocks(int A) { return (A + kPerBlock - 1) / kPerBlock; }
size_t label_ws_bytes(int A, int G) { return ((size_t)label_blocks(A) + 1) * (size_t)G * sizeof(uint32_t); }

// ---------------------------------------------------------------------------------------------------------------- gather
// One block per sampled anchor: the nine taps' 256 channels are read as rows of the NHWC map (thread = channel) into LDS and written
// out in (c, kh, kw) order.  An index outside 0 .. A - 1 gives a zero row, slot 0, a zero box and level -1; nothing is read for it.
__global__ __launch_bounds__(256) void rpn_gather(RpnAnchorGrid grid, RpnGatherMaps maps, int A, const int* __restrict__ idx, float* __restrict__ X,
                                                  int* __restrict__ slots, float* __restrict__ boxes, int* __restrict__ levels) {
    __shared__ float tile[9 * 257];
    const int s = blockIdx.x, t = threadIdx.x;
    const int i = idx[s];
    const bool ok = i >= 0 && i < A;
    AnchorAt a;
    a.box = f32x4{0.f, 0.f, 0.f, 0.f}; a.level = -1; a.y = 0; a.x = 0; a.slot = 0;
    if (ok) a = anchor_at(grid, i);
    if (ok) {
        const int H = grid.H[a.level], W = grid.W[a.level];
        const float* map = maps.p[a.level];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = a.y + tap / 3 - 1, xx = a.x + tap % 3 - 1;
            float v = 0.f;                                                   // zero padding of the 3 x 3 convolution
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = map[((size_t)yy * W + xx) * 256 + t];
            tile[tap * 257 + t] = v;
        }
    } else {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) tile[tap * 257 + t] = 0.f;
    }
    __syncthreads();
    float* row = X + (size_t)s * kPatch;
    for (int o = t; o < kPatch; o += 256) { const int c = o / 9, tap = o - c * 9; row[o] = tile[tap * 257 + c]; }
    if (t == 0) {
        slots[s] = a.slot;
        levels[s] = a.level;
        for (int j = 0; j < 4; ++j) boxes[(size_t)s * 4 + j] = a.box[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------- loss
__device__ __forceinline__ int row_slot(const int* slots, int r) {
    const int a = slots[r];
    return a < 0 ? 0 : (a > 2 ? 2 : a);                 // never index outside the row
}
// Box2BoxTransform(1, 1, 1, 1).get_deltas, column j, in f32 in detectron2's order
__device__ __forceinline__ float delta_target(const float* __restrict__ p, const float* __restrict__ g, int j) {
    const int a = j & 1;                               // 0: x, 1: y
    const float ps = p[2 + a] - p[a], gs = g[2 + a] - g[a];
    if (j < 2) {
        const float pc = p[a] + 0.5f * ps, gc = g[a] + 0.5f * gs;
        return 1.0f * (gc - pc) / ps;
    }
    return 1.0f * logf(gs / ps);
}
constexpr int kLossCols = 6;
// One thread per row: part[r] = {BCE term, smooth-L1 term, positive, negative, positive and logit > 0, negative and logit < 0}.
// A row whose label is negative is ignored.  The BCE term is max(x, 0) - x y + log1p(exp(-|x|)) in f64 on the f32 logit.
__global__ void loss_rows(const float* __restrict__ logits, const float* __restrict__ deltas, const int* __restrict__ slots,
                          const int* __restrict__ labels, const float* __restrict__ anchors, const float* __restrict__ gts, int S,
                          float beta, double* __restrict__ part) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S) return;
    const int a = row_slot(slots, r), lab = labels[r];
    const float xf = logits[(size_t)r * 3 + a];
    const bool pos = lab > 0, neg = lab == 0;
    double bce = 0.0, loc = 0.0;
    if (pos || neg) {
        const double x = (double)xf;
        bce = (x > 0.0 ? x : 0.0) - (pos ? x : 0.0) + log1p(exp(-fabs(x)));
    }
    if (pos) {
        for (int j = 0; j < 4; ++j) {
            const float tv = delta_target(anchors + (size_t)r * 4, gts + (size_t)r * 4, j);
            const float d = fabsf(deltas[(size_t)r * 12 + 4 * a + j] - tv);
            float term = d;
            if (beta >= 1e-5f) term = d < beta ? 0.5f * (d * d) / beta : d - 0.5f * beta;
            loc += (double)term;
        }
    }
    double* o = part + (size_t)r * kLossCols;
    o[0] = bce; o[1] = loc; o[2] = pos; o[3] = neg; o[4] = pos && xf > 0.f; o[5] = neg && xf < 0.f;
}
// out8 = {loss_rpn_cls, loss_rpn_loc, num_pos, num_neg, positive rows with logit > 0 / num_pos, negative rows with logit < 0 / num_neg, 0, 0}
__global__ __launch_bounds__(256) void loss_finish(const double* __restrict__ part, int S, int norm, float* __restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double tot[kLossCols];
    for (int j = 0; j < kLossCols; ++j) {
        double v = 0.0;
        for (int r = t; r < S; r += 256) v += part[(size_t)r * kLossCols + j];
        tot[j] = block_sum_d(v, red);
    }
    if (t == 0) {
        const double inv = 1.0 / (double)norm;
        out[0] = (float)(tot[0] * inv);
        out[1] = (float)(tot[1] * inv);
        out[2] = (float)tot[2];
        out[3] = (float)tot[3];
        out[4] = tot[2] > 0.0 ? (float)(tot[4] / tot[2]) : 0.f;
        out[5] = tot[3] > 0.0 ? (float)(tot[5] / tot[3]) : 0.f;
        out[6] = 0.f;
        out[7] = 0.f;
    }
}
// dlogits[r][c] = (sigmoid(x) - y) / norm * g_cls on column slot, ddeltas[r][c] = d smooth_l1 / norm * g_loc on columns 4 slot ..
// 4 slot + 3 of a positive row; exactly 0 elsewhere.  One thread per element of the 15 columns.
__global__ void loss_grad(const float* __restrict__ logits, const float* __restrict__ deltas, const int* __restrict__ slots,
                          const int* __restrict__ labels, const float* __restrict__ anchors, const float* __restrict__ gts, int S,
                          int norm, float beta, const float* __restrict__ g_cls, const float* __restrict__ g_loc,
                          float* __restrict__ dlogits, float* __restrict__ ddeltas) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)S * 15) return;
    const int r = (int)(i / 15), col = (int)(i - (size_t)r * 15);
    const int a = row_slot(slots, r), lab = labels[r];
    if (col < 3) {
        float v = 0.f;
        if (col == a && lab >= 0) {
            const double x = (double)logits[(size_t)r * 3 + a];
            const double sg = x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x));
            v = (float)((sg - (lab > 0 ? 1.0 : 0.0)) * ((double)(g_cls ? g_cls[0] : 1.f) / (double)norm));
        }
        dlogits[(size_t)r * 3 + col] = v;
        return;
    }
    const int dc = col - 3;
    float v = 0.f;
    if (lab > 0 && (dc >> 2) == a) {
        const float d = deltas[(size_t)r * 12 + dc] - delta_target(anchors + (size_t)r * 4, gts + (size_t)r * 4, dc & 3);
        float gr = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        if (beta >= 1e-5f && fabsf(d) < beta) gr = d / beta;
        v = gr / (float)norm * (g_loc ? g_loc[0] : 1.f);
    }
    ddeltas[(size_t)r * 12 + dc] = v;
}

bool grid_from_shapes(const int* H5, const int* W5, RpnAnchorGrid* g, long long* A) {
    static const int sizes[5] = {32, 64, 128, 256, 512};
    long long off = 0;
    for (int l = 0; l < 5; ++l) {
        if (H5[l] < 1 || W5[l] < 1 || H5[l] > 65536 || W5[l] > 65536) return false;
        g->H[l] = H5[l]; g->W[l] = W5[l]; g->stride[l] = 4 << l;
        g->off[l] = (int)off;
        off += 3ll * H5[l] * W5[l];
        if (off > kMaxAnchors) return false;
        apse_cell_anchors3(sizes[l], g->base[l]);
    }
    g->off[5] = (int)off;
    *A = off;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- weight refresh
// apse_set_rpn_head: the packing of plan.hip's pack_oihw and winograd_filters on the device, the same operations on the same
// operands (a copy; float64 products and sums rounded separately, one rounding to f32), so the bits are those of plan time.
// OIHW [Cout][Cin][KH][KW] -> rows row0 .. row0 + Cout - 1 of the tiled layout [.][KH][KWCp], run = (kw, cin_p).  One thread per
// element, in the order of the output; the padding the plan zeroed is not written.
__global__ __launch_bounds__(256) void pack_oihw_dev(const float* __restrict__ w, int Cout, int Cin, int KH, int KW, int cin_p,
                                                     int KWCp, int row0, float* __restrict__ out) {
    const size_t total = (size_t)Cout * KH * KW * Cin;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ci = (int)(i % Cin);
    const int s = (int)((i / Cin) % KW);
    const int r = (int)((i / ((size_t)Cin * KW)) % KH);
    const int o = (int)(i / ((size_t)Cin * KW * KH));
    out[((size_t)(row0 + o) * KH + r) * KWCp + s * cin_p + ci] = w[(((size_t)o * Cin + ci) * KH + r) * KW + s];
}

// U = G g G^T per (cout, cin), stored [cin_p / 8][16][Cout][8] (xi = 4 i + j).  One thread per (cout, cin).
__global__ __launch_bounds__(256) void winograd_filters_dev(const float* __restrict__ oihw, int Cout, int Cin, float* __restrict__ u) {
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Cout * Cin) return;
    const int o = idx % Cout, ci = idx / Cout;               // neighbouring threads write neighbouring 32-byte runs
    const float* gp = oihw + ((size_t)o * Cin + ci) * 9;
    double g[9];
    for (int k = 0; k < 9; ++k) g[k] = (double)gp[k];
    double t[4][3];                                          // G g
    for (int i = 0; i < 4; ++i)
        for (int s = 0; s < 3; ++s) t[i][s] = G[i][0] * g[s] + G[i][1] * g[3 + s] + G[i][2] * g[6 + s];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const double v = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];      // (G g) G^T
            u[(((size_t)(ci / 8) * 16 + 4 * i + j) * Cout + o) * 8 + (ci & 7)] = (float)v;
        }
}

}  // namespace

extern "C" {

int apse_k_pack_oihw(const float* w, int Cout, int Cin, int KH, int KW, int cin_p, int KWCp, int row0, float* out, hipStream_t s) {
    const size_t total = (size_t)Cout * KH * KW * Cin;
    hipLaunchKernelGGL(pack_oihw_dev, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, Cout, Cin, KH, KW, cin_p, KWCp, row0, out);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

int apse_k_winograd_filters(const float* oihw, int Cout, int Cin, float* u, hipStream_t s) {
    hipLaunchKernelGGL(winograd_filters_dev, dim3((Cout * Cin + 255) / 256), dim3(256), 0, s, oihw, Cout, Cin, u);
    return hipGetLastError() == hipSuccess ? APSE_OK : APSE_E_HIP;
}

size_t apse_rpn_train_workspace_bytes(int A, int G, int S) {
    if (A < 0 || A > kMaxAnchors || G < 0 || G > kMaxGt || S < 0 || S > kMaxRows) return 0;
    const size_t lab = label_ws_bytes(A, G), loss = (size_t)S * kLossCols * sizeof(double);
    const size_t need = lab > loss ? lab : loss;
    return need > 256 ? need : 256;
}

int apse_rpn_anchor_labels(const int* level_h5, const int* level_w5, const float* gt_boxes, int G, float iou_lo, float iou_hi,
                           int* labels, int* matched_idx, float* matched_iou, void* ws, size_t ws_bytes, void* stream) {
    if (!level_h5 || !level_w5 || !labels || !matched_idx || !matched_iou) return invalid("apse_rpn_anchor_labels: null pointer");
    if (G < 0 || G > kMaxGt) return invalid("apse_rpn_anchor_labels: needs 0 <= G <= 4096 ground truths");
    RpnAnchorGrid grid;
    long long A = 0;
    if (!grid_from_shapes(level_h5, level_w5, &grid, &A))
        return invalid("apse_rpn_anchor_labels: needs five levels of at least 1 x 1 and A = 3 sum(H W) <= 2^22 anchors");
    if (!(iou_lo <= iou_hi)) return invalid("apse_rpn_anchor_labels: needs iou_lo <= iou_hi");
    if (G > 0 && !gt_boxes) return invalid("apse_rpn_anchor_labels: null pointer");
    if (G > 0 && !ws) return invalid("apse_rpn_anchor_labels: null workspace");
    if (G > 0 && ws_bytes < label_ws_bytes((int)A, G)) return invalid("apse_rpn_anchor_labels: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int blocks = label_blocks((int)A);
    uint32_t* blockmax = reinterpret_cast<uint32_t*>(ws);
    float* gtmax = reinterpret_cast<float*>(blockmax + (size_t)blocks * G);
    hipLaunchKernelGGL(label_pass<false>, dim3(blocks), dim3(256), 0, s, grid, (int)A, gt_boxes, G, iou_lo, iou_hi, blockmax, nullptr,
                       labels, matched_idx, matched_iou);
    if (G > 0) {
        hipLaunchKernelGGL(gt_max_reduce, dim3((G + 255) / 256), dim3(256), 0, s, blockmax, blocks, G, gtmax);
        hipLaunchKernelGGL(label_pass<true>, dim3(blocks), dim3(256), 0, s, grid, (int)A, gt_boxes, G, iou_lo, iou_hi, nullptr, gtmax,
                           labels, matched_idx, matched_iou);
    }
    return launched();
}

int apse_k_rpn_gather(const RpnAnchorGrid* grid, const RpnGatherMaps* maps, const int* anchor_idx, int S, float* x, int* slots,
                      float* anchor_boxes, int* levels, hipStream_t s) {
    hipLaunchKernelGGL(rpn_gather, dim3(S), dim3(256), 0, s, *grid, *maps, grid->off[5], anchor_idx, x, slots, anchor_boxes, levels);
    return launched();
}

int apse_rpn_loss_forward(const float* logits, const float* deltas, const int* slots, const int* labels, const float* anchor_boxes,
                          const float* gt_boxes, int S, int norm, float smooth_l1_beta, float* out8, void* ws, size_t ws_bytes,
                          void* stream) {
    if (S == 0) return APSE_OK;
    if (S < 0 || S > kMaxRows) return invalid("apse_rpn_loss_forward: needs 0 <= S <= 2^20 rows");
    if (norm < 1) return invalid("apse_rpn_loss_forward: needs norm >= 1");
    if (!logits || !deltas || !slots || !labels || !anchor_boxes || !gt_boxes || !out8) return invalid("apse_rpn_loss_forward: null pointer");
    if (!ws) return invalid("apse_rpn_loss_forward: null workspace");
    if (!(smooth_l1_beta >= 0.f)) return invalid("apse_rpn_loss_forward: smooth_l1_beta must be >= 0");
    if (ws_bytes < (size_t)S * kLossCols * sizeof(double)) return invalid("apse_rpn_loss_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_rows, dim3((S + 63) / 64), dim3(64), 0, s, logits, deltas, slots, labels, anchor_boxes, gt_boxes, S,
                       smooth_l1_beta, (double*)ws);
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(256), 0, s, (const double*)ws, S, norm, out8);
    return launched();
}

int apse_rpn_loss_backward(const float* logits, const float* deltas, const int* slots, const int* labels, const float* anchor_boxes,
                           const float* gt_boxes, int S, int norm, float smooth_l1_beta, const float* grad_cls, const float* grad_loc,
                           float* dlogits, float* ddeltas, void* stream) {
    if (S == 0) return APSE_OK;
    if (S < 0 || S > kMaxRows) return invalid("apse_rpn_loss_backward: needs 0 <= S <= 2^20 rows");
    if (norm < 1) return invalid("apse_rpn_loss_backward: needs norm >= 1");
    if (!logits || !deltas || !slots || !labels || !anchor_boxes || !gt_boxes || !dlogits || !ddeltas) return invalid("apse_rpn_loss_backward: null pointer");
    if (!(smooth_l1_beta >= 0.f)) return invalid("apse_rpn_loss_backward: smooth_l1_beta must be >= 0");
    const size_t total = (size_t)S * 15;
    hipLaunchKernelGGL(loss_grad, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, deltas, slots, labels,
                       anchor_boxes, gt_boxes, S, norm, smooth_l1_beta, grad_cls, grad_loc, dlogits, ddeltas);
    return launched();
}

}  // extern "C"
