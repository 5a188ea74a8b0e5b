// Launch plans of the detector context: weight packing and the steps, tensors and buffers of the FPN plan (build_plan) and the
// C4 plan (build_plan_c4).  Runs once per context, at apse_finalize_weights; what it builds is replayed by run_plan (detector.hip).
#include "detector_ctx.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#define APSE_WINO_MIN_BLOCKS 128  // f32 Winograd layers: fewest blocks per image (see add_conv)
// the trunk's f32 Winograd layers (winograd_trunk_layer): fewest Winograd tiles per image of the plan's res4-stride map,
// ceil(H / 2) ceil(W / 2).  A 16:9 frame at the 800 / 1333 resize has 24 x 42 = 1008; 600 / 1000 has 576, KITTI 546.
#define APSE_WINO_TRUNK_MIN_TILES 1000
#define APSE_WINO_GRID 256        // blocks a trunk Winograd launch may have per image: one per CU
#define APSE_EXPECTED_DETS 8      // list length the packed-list GEMMs are shaped for (static: see add_conv)

// ------------------------------------------------------------------------------------------------
// weight packing: OIHW (+ per-channel scale) -> [Cout_p][KH][KWCp], run = (kw, cin_p)
void pack_oihw(const float* w, int Cout, int Cin, int KH, int KW, int cin_p, const float* scale, float* out, int KWCp) {
    for (int o = 0; o < Cout; ++o) {
        const float sc = scale ? scale[o] : 1.0f;
        for (int r = 0; r < KH; ++r)
            for (int s = 0; s < KW; ++s)
                for (int ci = 0; ci < Cin; ++ci)
                    out[((size_t)o * KH + r) * KWCp + s * cin_p + ci] = w[(((size_t)o * Cin + ci) * KH + r) * KW + s] * sc;
    }
}

static const HostW* getw(apse_ctx* c, const std::string& n) {
    auto it = c->hw.find(n);
    return it == c->hw.end() ? nullptr : &it->second;
}

static Tens make_t(apse_ctx* c, const std::string& name, int items, int H, int W, int C, int st = 0) {
    Tens t;
    t.H = H; t.W = W; t.C = C; t.st = st;
    const size_t elems = (size_t)items * H * W * C;
    t.p = dalloc<float>(c, st ? (elems + 1) / 2 : elems);          // 16-bit storage: half the bytes
    c->t[name] = t;
    return t;
}

// One convolution step, built by add_conv from reference weights `wnames` (OIHW) with optional FrozenBN `wname.norm.*`.  The
// leading fields are given positionally (ConvSpec{name, {weights}, KH, KW, stride, pad, relu}); every other field has the
// default most layers take and is set by name where a layer differs.
struct ConvSpec {
    std::string name; std::vector<std::string> wnames;   // one or more OIHW weights concatenated along Cout
    int KH, KW, stride, pad, relu;
    int fc_h = 0, fc_w = 0;   // >0: weight is [Cout][C*fc_h*fc_w] flattened (c,h,w): treat as fc_h x fc_w valid conv
    int deconv = 0;
    int s2d = 0;              // stem on the space-to-depth(2) input: the 7x7 / stride-2 filter is re-indexed as 4x4 / stride-1 over 12 channels
    std::string out_name;     // name of the output tensor in apse_ctx::t; empty: the layer's name
    int items = 1;            // items per image (1, rpn_post_topk, dets_per_image)
    const Tens* res = nullptr; int res_mode = 0;   // residual input and how it is added (ConvParams::res_mode)
    int y_ld = 0;             // > 0: row length of the output, wider than Cout (fused heads)
    int count_kind = 0;       // which device count limits the rows of a launch (ConvStep::count_kind)
    float* out_ptr = nullptr;         // write here (f32) instead of allocating; the output gets no entry in apse_ctx::t
    const Tens* out_view = nullptr;   // the output is this slice of a larger allocation (pointer and storage type taken from it)
};

// 16-bit storage mode: every activation the bulk GEMMs produce lives in HBM in the operand type; the narrow
// decision heads (Cout <= 32) and the association FC keep f32 outputs.
// f32 -> bf16 (dtype 1) / f16 (dtype 2) bits, round-to-nearest-even like the in-kernel converts; a NaN stays a NaN
static uint16_t round16(float v, int dtype) {
    if (dtype == 2) {
        const _Float16 hval = (_Float16)v;
        uint16_t r;
        memcpy(&r, &hval, 2);
        return r;
    }
    uint32_t b;
    memcpy(&b, &v, 4);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((b >> 16) | 0x40);
    return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}
static int storage_type(const apse_ctx* c) { return (c->cfg.compute_dtype >= 1 && c->cfg.storage16) ? c->cfg.compute_dtype : 0; }

// f32 layers that run as fused Winograd F(2x2,3x3) (conv_winograd.hip): the terminal 3x3 layers at p2 / p3 -- the FPN outputs and
// the RPN conv, whose results feed no further 3x3 chain (conv_winograd_f32)
static bool winograd_layer(const std::string& n) {
    return n == "backbone.fpn_output2" || n == "backbone.fpn_output3" || n == "rpn_t2" || n == "rpn_t3";
}
// ... and, in plans of large frames only (APSE_WINO_TRUNK_MIN_TILES), 3x3 layers of the trunk and of the res4-stride level: the
// bottlenecks' conv2 of res2, res3 and res5, the FPN output and the RPN conv at p4, with a Cin split and the block geometry that
// fill the card.  res4's 23 conv2 layers stay on the direct kernel: with them the 64-frame given-boxes sequence at 4K missed its
// exact CSV text in one centroid cell ("In the trunk")
static bool winograd_trunk_layer(const std::string& n) {
    static const std::string trunk = "backbone.bottom_up.res", c2 = ".conv2";
    if (n == "backbone.fpn_output4" || n == "rpn_t4") return true;
    return n.size() > trunk.size() + c2.size() && n.compare(0, trunk.size(), trunk) == 0 && n[trunk.size()] != '4' &&
           n.compare(n.size() - c2.size(), c2.size(), c2) == 0;
}
// Geometry and Cin split of a trunk Winograd layer: the grid (blocks per image x split) nearest to APSE_WINO_GRID from below; a map
// that has more blocks than that unsplit runs unsplit.  Equal grids: the unsplit launch keeps <16, 4>, a split one takes <8, 8>
// (the squarer patch has the smaller halo).  A plan constant: shape only.
static void winograd_trunk_shape(ConvParams& p) {
    const int slices = (1 << p.cin_log2) / 8;
    int best = -1;
    for (int g = 0; g < 2; ++g) {
        ConvParams q = p;
        q.wino_geom = g;
        const int nb = apse_conv_winograd_blocks(q);
        int sk = nb >= APSE_WINO_GRID ? 1 : APSE_WINO_GRID / nb;
        if (sk > slices) sk = slices;
        const int grid = nb * sk, over = grid > APSE_WINO_GRID;
        const int score = over ? -grid : grid;           // any grid within the bound beats one above it; above it, the smaller
        const bool better = best == -1 || score > best || (score == best && sk > 1);
        if (better) { best = score; p.wino_geom = g; p.splitk = sk; }
    }
}
// U = G g G^T per (cout, cin) in float64, rounded to f32 once, stored [cin_p / 8][16][Cout][8] (xi = 4 i + j): the B-operand
// staging of conv_winograd_f32 reads one contiguous 2 KiB run per xi and k-slice.  Channels past Cin are zero.
std::vector<float> winograd_filters(const float* oihw, int Cout, int Cin, int cin_p) {
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> u((size_t)16 * Cout * cin_p, 0.f);
    for (int o = 0; o < Cout; ++o)
        for (int ci = 0; ci < Cin; ++ci) {
            const float* g = oihw + ((size_t)o * Cin + ci) * 9;
            double t[4][3];                                  // G g
            for (int i = 0; i < 4; ++i)
                for (int s = 0; s < 3; ++s) t[i][s] = G[i][0] * g[s] + G[i][1] * g[3 + s] + G[i][2] * g[6 + s];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    const double v = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];      // (G g) G^T
                    u[(((size_t)(ci / 8) * 16 + 4 * i + j) * Cout + o) * 8 + (ci & 7)] = (float)v;
                }
        }
    return u;
}

static int add_conv(apse_ctx* c, std::vector<Step>& plan, const ConvSpec& sp, const Tens& in, Tens* out) {
    const std::string& out_name = sp.out_name.empty() ? sp.name : sp.out_name;
    // gather rows
    std::vector<float> rows;    // OIHW concatenated
    std::vector<float> bias;
    int Cout = 0, Cin = 0;
    const int KH = sp.KH, KW = sp.KW;
    for (const auto& wn : sp.wnames) {
        const HostW* w = getw(c, wn + ".weight");
        if (!w) return fail(c, APSE_E_MISSING, "missing weight " + wn + ".weight");
        int co, ci;
        std::vector<float> oihw;
        if (sp.fc_h > 0) {
            co = (int)w->shape[0];
            const int flat = (int)w->shape[1];
            ci = flat / (sp.fc_h * sp.fc_w);
            oihw = w->v;                      // [co][c][h][w] already (c,h,w) flattened == OIHW
        } else if (sp.deconv) {
            // ConvTranspose2d weight [Cin][Cout][2][2] -> rows n = (dy*2+dx)*Cout + co, K = ci (1x1)
            ci = (int)w->shape[0];
            const int cc = (int)w->shape[1];
            co = 4 * cc;
            oihw.assign((size_t)co * ci, 0.f);
            for (int i = 0; i < ci; ++i)
                for (int o = 0; o < cc; ++o)
                    for (int dy = 0; dy < 2; ++dy)
                        for (int dx = 0; dx < 2; ++dx)
                            oihw[((size_t)((dy * 2 + dx) * cc + o)) * ci + i] = w->v[(((size_t)i * cc + o) * 2 + dy) * 2 + dx];
        } else if (w->shape.size() == 2) {
            co = (int)w->shape[0]; ci = (int)w->shape[1]; oihw = w->v;
        } else if (sp.s2d) {
            // out(oy, ox) = sum w7[ky][kx][c] x[2 oy - 3 + ky][2 ox - 3 + kx][c]; with input row 2 Y + dy, Y = oy - 2 + r (r = 0..3):
            // ky = 2 r + dy - 1, kx = 2 s + dx - 1 (taps outside 0..6 do not exist: zero), channel (2 dy + dx) 3 + c
            if (w->shape.size() != 4 || w->shape[2] != 7 || w->shape[3] != 7 || w->shape[1] != 3 || KH != 4 || KW != 4)
                return fail(c, APSE_E_INVALID, "space-to-depth stem needs a 7x7 filter over 3 channels: " + wn);
            co = (int)w->shape[0]; ci = 12;
            oihw.assign((size_t)co * 12 * 16, 0.f);
            for (int o = 0; o < co; ++o)
                for (int ch = 0; ch < 3; ++ch)
                    for (int r = 0; r < 4; ++r)
                        for (int sx = 0; sx < 4; ++sx)
                            for (int dy = 0; dy < 2; ++dy)
                                for (int dx = 0; dx < 2; ++dx) {
                                    const int ky = 2 * r + dy - 1, kx = 2 * sx + dx - 1;
                                    if (ky < 0 || ky > 6 || kx < 0 || kx > 6) continue;
                                    oihw[(((size_t)o * 12 + (dy * 2 + dx) * 3 + ch) * 4 + r) * 4 + sx] = w->v[(((size_t)o * 3 + ch) * 7 + ky) * 7 + kx];
                                }
        } else {
            co = (int)w->shape[0]; ci = (int)w->shape[1]; oihw = w->v;
            if ((int)w->shape[2] != KH || (int)w->shape[3] != KW) return fail(c, APSE_E_INVALID, "kernel size mismatch " + wn);
        }
        if (Cin && ci != Cin) return fail(c, APSE_E_INVALID, "Cin mismatch in fused conv " + sp.name);
        Cin = ci;
        // FrozenBN fold (detectron2 FrozenBatchNorm2d, eps 1e-5): scale = g * rsqrt(var + eps), bias = b - mean*scale
        const HostW* g = getw(c, wn + ".norm.weight");
        std::vector<float> scale;
        const int nb = sp.deconv ? co / 4 : co;
        std::vector<float> b(nb, 0.f);
        if (g) {
            const HostW* be = getw(c, wn + ".norm.bias");
            const HostW* mu = getw(c, wn + ".norm.running_mean");
            const HostW* var = getw(c, wn + ".norm.running_var");
            if (!be || !mu || !var) return fail(c, APSE_E_MISSING, "incomplete norm for " + wn);
            scale.resize(co);
            for (int o = 0; o < co; ++o) {
                scale[o] = g->v[o] * (1.0f / sqrtf(var->v[o] + 1e-5f));
                b[o] = be->v[o] - mu->v[o] * scale[o];
            }
            const size_t per = (size_t)ci * KH * KW;
            for (int o = 0; o < co; ++o)
                for (size_t k = 0; k < per; ++k) oihw[(size_t)o * per + k] *= scale[o];
        } else {
            const HostW* bw = getw(c, wn + ".bias");
            if (bw) for (int o = 0; o < nb; ++o) b[o] = bw->v[o];
        }
        rows.insert(rows.end(), oihw.begin(), oihw.end());
        bias.insert(bias.end(), b.begin(), b.end());
        Cout += co;
    }
    const int cin_p = in.C;
    if (pow2_at_least(Cin) != cin_p && Cin != cin_p) return fail(c, APSE_E_INVALID, "input channels mismatch at " + sp.name);
    if (sp.s2d && (in.C != 16 || sp.stride != 1 || sp.pad != 2)) return fail(c, APSE_E_INVALID, "space-to-depth stem geometry");
    const int KWC = KW * cin_p, KWCp = apse_roundup(KWC, 32);
    const int Cout_p = apse_roundup(Cout, 128);
    std::vector<float> packed((size_t)Cout_p * KH * KWCp, 0.f);
    pack_oihw(rows.data(), Cout, Cin, KH, KW, cin_p, nullptr, packed.data(), KWCp);
    std::vector<float> bias_p(Cout_p, 0.f);
    for (size_t i = 0; i < bias.size(); ++i) bias_p[i] = bias[i];
    // bf16 or f16 operands; the box and mask predictors are decision layers and stay f32 at any width (up to 6 classes they are
    // narrow anyway: Cout <= 32)
    const bool use_bf16 = (c->cfg.compute_dtype >= 1 && Cout > 32 && sp.name != "assoc_fc" && sp.name != "box_pred" &&
                           sp.name != "mask_logits");
    float* wd = nullptr;
    uint16_t* wd16 = nullptr;
    if (use_bf16) {
        // filters pre-rounded to the 16-bit operand type (round-to-nearest-even, as the in-kernel converts do)
        std::vector<uint16_t> p16(packed.size());
        for (size_t i = 0; i < packed.size(); ++i) p16[i] = round16(packed[i], c->cfg.compute_dtype);
        wd16 = dupload(c, p16);
    } else {
        wd = dupload(c, packed);
    }
    float* bd = dupload(c, bias_p);
    if ((!wd && !wd16) || !bd) return fail(c, APSE_E_NOMEM, "weight upload failed at " + sp.name);

    Step st;
    st.kind = S_CONV;
    ConvStep& cs = st.c;
    memset(&cs.p, 0, sizeof(cs.p));
    cs.name = sp.name;
    cs.b_mult = sp.items;
    cs.count_kind = sp.count_kind;
    ConvParams& p = cs.p;
    p.x = in.p; p.w = wd; p.w16 = wd16; p.bias = bd; p.res = sp.res ? sp.res->p : nullptr; p.res_mode = sp.res_mode;
    p.x_st = in.st; p.res_st = sp.res ? sp.res->st : 0;
    p.H = in.H; p.W = in.W; p.cin_log2 = apse_ilog2(cin_p);
    p.KH = KH; p.KW = KW; p.stride = sp.stride; p.pad = sp.pad; p.KWCp = KWCp;
    p.OH = (in.H + 2 * sp.pad - KH) / sp.stride + 1;
    p.OW = (in.W + 2 * sp.pad - KW) / sp.stride + 1;
    if (sp.s2d) { p.OH = in.H; p.OW = in.W; }       // pad 2 above / left, 1 below / right: taps past the map read zeros (range check)
    p.Cout = Cout; p.relu = sp.relu;
    p.steps_total = KH * (KWCp / 32);
    p.splitk = 1;
    p.out_mode = sp.deconv ? 1 : 0;
    // bf16 matrix cores for the bulk GEMMs; decision layers (narrow heads) and the association FC stay exact f32
    p.prec = use_bf16 ? c->cfg.compute_dtype : 0;
    p.cdec = sp.deconv ? Cout / 4 : 0;
    const int out_c = sp.deconv ? Cout / 4 : (sp.y_ld > 0 ? sp.y_ld : Cout);
    const int oh = sp.deconv ? 2 * p.OH : p.OH, ow = sp.deconv ? 2 * p.OW : p.OW;
    const int out_st = sp.out_view ? sp.out_view->st : ((use_bf16 && !sp.out_ptr) ? storage_type(c) : 0);
    if (out_st && (out_c & 7)) return fail(c, APSE_E_INVALID, "16-bit tensors need C % 8 == 0 at " + sp.name);
    Tens o;
    if (sp.out_view) { o = *sp.out_view; o.H = oh; o.W = ow; o.C = out_c; c->t[out_name] = o; }      // a slice of a larger allocation
    else if (sp.out_ptr) { o.p = sp.out_ptr; o.H = oh; o.W = ow; o.C = out_c; }
    else o = make_t(c, out_name, c->cfg.max_batch * sp.items, oh, ow, out_c, out_st);
    p.y_st = o.st;
    if (!o.p) return fail(c, APSE_E_NOMEM, "activation alloc failed at " + sp.name);
    p.y = o.p; p.y_ld = out_c; p.y_coff = 0;
    cs.flops_per_item = sp.s2d ? 2.0 * p.OH * p.OW * (double)Cout * 7 * 7 * 3        // algorithmic: the reference's 7x7x3 taps
                               : 2.0 * p.OH * p.OW * (double)Cout * KH * KW * Cin;
    // tile config / split-K chosen for the full batch; workspace sized for the worst case over 1..max_batch
    const int Mfull = c->cfg.max_batch * sp.items * p.OH * p.OW;
    int sk = 1;
    cs.cfg = apse_conv_pick_cfg(Mfull, Cout, p.steps_total, &sk);
    if (sp.count_kind == 2) {
        // GEMMs over the packed detection list: the tile shape and the K split fix the f32 summation order, so they are
        // chosen HERE, once, from plan constants only (a typical list of APSE_EXPECTED_DETS detections per image of the
        // context's max_batch -- like every other layer's shape; never from the batch of a forward or an earlier frame's
        // count).  Within a context a frame's masks / embeddings are then the same bits whatever ran before it, in whatever
        // batch; contexts with equal configuration (shards, pipeline slots) agree with each other.  The live count only
        // sizes the grid (m_hint).
        const int kd = c->cfg.dets_per_image < APSE_EXPECTED_DETS ? c->cfg.dets_per_image : APSE_EXPECTED_DETS;
        const int rows = kd * c->cfg.max_batch * p.OH * p.OW;
        sk = 1;
        cs.cfg = apse_conv_pick_cfg(rows < Mfull ? rows : Mfull, Cout, p.steps_total, &sk);
    }
    p.splitk = sk;
    if (sk > 1) {
        const size_t need = (size_t)sk * Mfull * Cout;
        if (need > c->ws_floats) c->ws_floats = need;
    }
    // fused Winograd for the named f32 3x3 layers: a plan constant (layer and shape, never the batch of a forward); cs.cfg stays
    // the tiled config the layer would otherwise run and labels its profile slot.  Only maps of at least APSE_WINO_MIN_BLOCKS
    // blocks per image (p3 of a 4K frame: 252): the small-frame configurations keep the direct kernel and its exact results
    // (conv_winograd_f32)
    // The trunk set (winograd_trunk_layer; FPN plans only) is taken when the plan's res4-stride map has at least
    // APSE_WINO_TRUNK_MIN_TILES tiles, with the geometry and the Cin split of winograd_trunk_shape; its slabs share the split-K
    // workspace (these layers run on the caller's stream)
    if (c->f32_winograd && sp.count_kind == 0) {
        ConvParams q = p;
        bool take = false;
        if (winograd_layer(sp.name)) {
            take = sk == 1 && apse_conv_winograd_ok(q, c->cfg.max_batch * sp.items) && apse_conv_winograd_blocks(q) >= APSE_WINO_MIN_BLOCKS;
        } else if (!c->c4 && winograd_trunk_layer(sp.name) &&
                   ((c->PH / 16 + 1) / 2) * ((c->PW / 16 + 1) / 2) >= APSE_WINO_TRUNK_MIN_TILES) {
            q.splitk = 1;
            if (apse_conv_winograd_ok(q, c->cfg.max_batch * sp.items)) {
                winograd_trunk_shape(q);
                take = apse_conv_winograd_ok(q, c->cfg.max_batch * sp.items);
            }
        }
        if (take) {
            p = q;
            p.wu = dupload(c, winograd_filters(rows.data(), Cout, Cin, cin_p));
            if (!p.wu) return fail(c, APSE_E_NOMEM, "weight upload failed at " + sp.name);
            const size_t need = (size_t)p.splitk * Mfull * Cout;
            if (p.splitk > 1 && need > c->ws_floats) c->ws_floats = need;
        }
    }
    if (out) *out = o;
    plan.push_back(st);
    return APSE_OK;
}

// ------------------------------------------------------------------------------------------------
static void layout_results(apse_ctx* c) {
    apse_results_layout& L = c->lay;
    memset(&L, 0, sizeof(L));
    const int B = c->cfg.max_batch, kd = c->cfg.dets_per_image, n = B * kd, E = c->cfg.embed_dim;
    L.n_max = n; L.dets_per_image = kd; L.embed_dim = E; L.max_batch = B;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 15) / 16 * 16; return r; };
    L.total = take(4);
    L.offset = take(4 * (B + 1));
    L.prop_count = take(4 * B);
    L.img = take(4 * n); L.cls = take(4 * n); L.roi = take(4 * n); L.score = take(4 * n);
    L.box_resized = take(16 * n); L.box = take(16 * n); L.valid = take(4 * n); L.rect = take(16 * n);
    L.mass = take(4 * n); L.centroid = take(8 * n);
    L.closest = take((size_t)8 * n * kd);
    L.embedding = take((size_t)4 * n * E);
    L.bytes = o;
}

// Box-inference buffers of both plans: candidates, class lists (wide kernels), kept detections.
static void alloc_box_inference(apse_ctx* c) {
    const apse_config& g = c->cfg;
    const int B = g.max_batch, POST = g.rpn_post_topk, K = g.num_classes, KD = g.dets_per_image;
    c->wide = K > APSE_NARROW_CLASSES;
    if (c->wide) {
        c->cls_list = dalloc<int>(c, (size_t)B * K * POST, false);
        c->cls_cnt = dalloc<int>(c, (size_t)B * K);                 // zero; nms_prepare_list leaves it zero after every forward
    }
    c->cand_boxes = dalloc<float>(c, (size_t)B * POST * K * 4);
    c->cand_scores = dalloc<float>(c, (size_t)B * POST * K);
    c->cand_valid = dalloc<int>(c, (size_t)B * POST * K);
    c->probs = dalloc<float>(c, (size_t)B * POST * (K + 1));
    c->det_boxes = dalloc<float>(c, (size_t)B * KD * 4);
    c->det_scores = dalloc<float>(c, (size_t)B * KD);
    c->det_entry = dalloc<int>(c, (size_t)B * KD);
    c->det_cnt = dalloc<int>(c, (size_t)B);
}

// Proposal and NMS buffers of both plans.  `levels`: RPN levels whose decoded candidates lie side by side (FPN 5, C4 1).
static int alloc_proposals(apse_ctx* c, int levels) {
    const apse_config& g = c->cfg;
    const int B = g.max_batch, PRE = g.rpn_pre_topk, POST = g.rpn_post_topk, K = g.num_classes;
    c->dec_boxes = dalloc<float>(c, (size_t)B * levels * PRE * 4);
    c->dec_scores = dalloc<float>(c, (size_t)B * levels * PRE);
    c->dec_valid = dalloc<int>(c, (size_t)B * levels * PRE);
    c->maxc = dalloc<uint32_t>(c, (size_t)2 * B);
    if (c->c4) c->c4_nms = dalloc<uint8_t>(c, apse_c4_nms_scratch_bytes(B), false);
    const int ncat = K > 8 ? K : 8;                                   // NMS categories per image: 5 RPN levels, K classes
    c->keep_idx = dalloc<int>(c, (size_t)B * ncat * APSE_NMS_SLOT);
    c->keep_cnt = dalloc<int>(c, (size_t)B * ncat);
    c->nms_scratch = dalloc<uint8_t>(c, apse_nms_scratch_bytes(ncat * B));
    c->props = dalloc<float>(c, (size_t)B * POST * 4);
    c->prop_scores = dalloc<float>(c, (size_t)B * POST);
    c->prop_entry = dalloc<int>(c, (size_t)B * POST);
    if (!c->dec_boxes || !c->dec_scores || !c->dec_valid || !c->maxc || (c->c4 && !c->c4_nms) || !c->keep_idx || !c->keep_cnt ||
        !c->nms_scratch || !c->props || !c->prop_scores || !c->prop_entry)
        return fail(c, APSE_E_NOMEM, c->c4 ? "C4 proposal buffers" : "proposal buffers");
    return APSE_OK;
}

// Tail of both plans: mask bit planes, the association head (roi_pool of a feat_C-channel map -> FC -> L2 normalise), the
// split-K workspace and the resize staging.
static int finish_plan(apse_ctx* c, int feat_C) {
    const apse_config& g = c->cfg;
    const int B = g.max_batch, KD = g.dets_per_image, NM = B * KD;
    int rc;
    c->wpr = (g.frame_w + 63) / 64;
    for (int k = 0; k < 2; ++k) c->bits2[k] = dalloc<uint64_t>(c, (size_t)NM * g.frame_h * c->wpr, false);
    c->sums = dalloc<unsigned long long>(c, (size_t)NM * 3);      // cleared by pack_detections in front of every mask tail
    if (!c->bits2[0] || !c->bits2[1]) return fail(c, APSE_E_NOMEM, "mask bit planes alloc");
    // ---- association head: roi_pool(p2) -> FC (RxR valid conv) -> L2 normalise
    const int R = g.assoc_roi;
    Tens ap = make_t(c, "assoc_pooled", NM, R, R, feat_C);
    Tens er;
    {
        ConvSpec sp{"assoc_fc", {"association.fc"}, R, R, 1, 0, 0, R, R};
        c->emb_raw = dalloc<float>(c, (size_t)NM * g.embed_dim);
        sp.items = KD; sp.count_kind = 2; sp.out_ptr = c->emb_raw;
        rc = add_conv(c, c->embedfc, sp, ap, &er);
        if (rc) return rc;
        const ConvParams& fp = c->embedfc[0].c.p;
        // the same filters through the K-sliced form when the shape allows (K = 25600, N = 128 in the reference); APSE_NO_ASSOC_FC
        // (read when the context is built) keeps the split-K convolution + normalise kernels
        if (fp.w && fp.KWCp == R * feat_C && apse_assoc_fc_ok(fp.KH * fp.KWCp, g.embed_dim) && !getenv("APSE_NO_ASSOC_FC")) {
            c->ws_assoc = dalloc<float>(c, (size_t)(fp.KH * fp.KWCp / 128) * NM * g.embed_dim, false);
            if (!c->ws_assoc) return fail(c, APSE_E_NOMEM, "association FC workspace");
        }
    }
    if (c->ws_floats) {
        c->ws = dalloc<float>(c, c->ws_floats, false);
        if (!c->ws) return fail(c, APSE_E_NOMEM, "split-K workspace alloc");
    }
    if (c->lane_on) {
        // the head plans run on the tail lane beside the next frame's trunk, whose res5 reduces use c->ws: a workspace of their own,
        // sized like c->ws (add_conv) from the split-K layers of the three head plans only (run_plan selects it by stream)
        size_t need = 0;
        for (const std::vector<Step>* pl : {&c->boxhead, &c->maskhead, &c->embedfc})
            for (const Step& st : *pl) {
                const ConvParams& q = st.c.p;
                if (st.kind != S_CONV || q.splitk <= 1) continue;
                const size_t n = (size_t)q.splitk * B * st.c.b_mult * q.OH * q.OW * q.Cout;
                if (n > need) need = n;
            }
        if (need) {
            c->ws_lane = dalloc<float>(c, need, false);
            if (!c->ws_lane) return fail(c, APSE_E_NOMEM, "tail lane split-K workspace alloc");
        }
    }
    c->tile_cnt = dalloc<int>(c, 65536);        // zero-initialised; every launch leaves it zero
    c->rs_pitch = (g.image_w * 3 + 15) & ~15;            // row pitch of the intermediate image: dword loads in the vertical pass
    c->rs_tmp = dalloc<uint8_t>(c, (size_t)B * g.frame_h * c->rs_pitch, false);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(c, APSE_E_HIP, std::string("plan build: ") + hipGetErrorString(e));
    return APSE_OK;
}

// One ResNet bottleneck: [shortcut 1x1 when the weights have one], conv1 1x1 (it carries the stride: STRIDE_IN_1X1), conv2 3x3,
// conv3 1x1 + residual + ReLU.  Weights wp.{shortcut, conv1, conv2, conv3}; the steps and their outputs are named
// tp.{shortcut, conv1, conv2, conv3}, the block's output tensor out_name (apse_debug_tensor / apse_export_feature look these up).
static int add_bottleneck(apse_ctx* c, std::vector<Step>& plan, const std::string& wp, const std::string& tp, const Tens& in, int items,
                          int stride, int count_kind, const std::string& out_name, Tens* out) {
    auto spec = [&](const char* part, int k, int s, int relu) {
        ConvSpec sp{tp + part, {wp + part}, k, k, s, k / 2, relu};
        sp.items = items; sp.count_kind = count_kind;
        return sp;
    };
    Tens sc, a, b2;
    const Tens* resp = &in;
    int rc;
    if (getw(c, wp + ".shortcut.weight")) {
        if ((rc = add_conv(c, plan, spec(".shortcut", 1, stride, 0), in, &sc))) return rc;
        resp = &sc;
    }
    if ((rc = add_conv(c, plan, spec(".conv1", 1, stride, 1), in, &a))) return rc;
    if ((rc = add_conv(c, plan, spec(".conv2", 3, 1, 1), a, &b2))) return rc;
    ConvSpec sp3 = spec(".conv3", 1, 1, 1);
    sp3.out_name = out_name; sp3.res = resp; sp3.res_mode = 1;
    return add_conv(c, plan, sp3, b2, out);
}

// 16-bit storage modes, 64 mid channels (res2): conv1 -> conv2 -> conv3 + residual as ONE launch with the two 64-channel
// intermediates in LDS (bottleneck16.hip; same bits as the three launches).  Replaces the last three steps of `plan` (a
// stride-1 bottleneck on `in` that add_bottleneck has just built into `out`) when the block is eligible.  APSE_NO_BNECK_FUSE
// (read when the context is built) keeps the three-kernel form, for the equality test and A/B runs.
static void fuse_bottleneck16(apse_ctx* c, std::vector<Step>& plan, const std::string& name, const Tens& in, const Tens& out) {
    const size_t n = plan.size();
    const ConvParams &q1 = plan[n - 3].c.p, &q2 = plan[n - 2].c.p, &q3 = plan[n - 1].c.p;
    const int st16 = storage_type(c);
    if (!(st16 && q1.stride == 1 && q1.Cout == 64 && out.C == 256 && (in.C == 64 || in.C == 256) && q1.w16 && q2.w16 && q3.w16 &&
          q1.x_st == st16 && q1.y_st == st16 && q2.y_st == st16 && q3.y_st == st16 && q3.res_st == st16 && q2.KWCp == 192 &&
          q1.KWCp == in.C && q3.KWCp == 64 && (size_t)c->cfg.max_batch * in.H * in.W * in.C * 2 < 0xfffffff0ull &&
          !getenv("APSE_NO_BNECK_FUSE")))
        return;
    Step fs;
    fs.kind = S_BNECK;
    fs.c = plan[n - 3].c;
    fs.c.name = name;
    fs.c.flops_per_item = plan[n - 3].c.flops_per_item + plan[n - 2].c.flops_per_item + plan[n - 1].c.flops_per_item;
    fs.p2 = q2; fs.p3 = q3;
    fs.x = in.p; fs.y = out.p; fs.H = in.H; fs.W = in.W; fs.C = in.C; fs.st = st16;
    plan.resize(n - 3);
    plan.push_back(fs);
}

// The max-pool behind the stem as a step of its own (every form but the fused 16-bit stem)
static Tens add_stem_pool(apse_ctx* c, const Tens& cur) {
    Step st; st.kind = S_MAXPOOL; st.x = cur.p; st.H = cur.H; st.W = cur.W; st.C = cur.C;
    Tens o = make_t(c, "stem", c->cfg.max_batch, (cur.H + 2 - 3) / 2 + 1, (cur.W + 2 - 3) / 2 + 1, cur.C, cur.st);
    st.y = o.p; st.c.name = "stem.pool"; st.st = cur.st;
    c->backbone.push_back(st);
    return o;
}

// The mask branch's last two layers in both plans: deconv 2x2 + ReLU, then the 1x1 predictor
static int add_mask_predictor(apse_ctx* c, const Tens& in, Tens* logits) {
    const int KD = c->cfg.dets_per_image;
    Tens md;
    ConvSpec dc{"mask_deconv", {"roi_heads.mask_head.deconv"}, 1, 1, 1, 0, 1};
    dc.deconv = 1; dc.items = KD; dc.count_kind = 2;
    int rc = add_conv(c, c->maskhead, dc, in, &md);
    if (rc) return rc;
    ConvSpec ml{"mask_logits", {"roi_heads.mask_head.predictor"}, 1, 1, 1, 0, 0};
    ml.items = KD; ml.count_kind = 2;
    return add_conv(c, c->maskhead, ml, md, logits);
}

// The fused box predictor of both plans (K + 1 logits, 4 K deltas) on `in`: rows of round_up(5 K + 1, 32)
static int add_box_predictor(apse_ctx* c, const Tens& in) {
    ConvSpec sp{"box_pred", {"roi_heads.box_predictor.cls_score", "roi_heads.box_predictor.bbox_pred"}, 1, 1, 1, 0, 0};
    sp.items = c->cfg.rpn_post_topk; sp.count_kind = 1;
    sp.y_ld = c->pred_ld = apse_roundup(5 * c->cfg.num_classes + 1, 32);
    Tens pr;
    int rc = add_conv(c, c->boxhead, sp, in, &pr);
    if (rc) return rc;
    if (pr.C != c->pred_ld || c->t["box_pred"].st != 0) return fail(c, APSE_E_INVALID, "fused box predictor layout");
    return APSE_OK;
}

// ------------------------------------------------------------------------------------------------ RPN selection plans
void apse_cell_anchors3(int size, float (*base)[4]) {          // DefaultAnchorGenerator.generate_cell_anchors: doubles -> f32
    static const double ratios[3] = {0.5, 1.0, 2.0};
    for (int a = 0; a < 3; ++a) {
        const double area = (double)size * size;
        const double w = sqrt(area / ratios[a]), h = ratios[a] * w;
        base[a][0] = (float)(-w / 2.0); base[a][1] = (float)(-h / 2.0);
        base[a][2] = (float)(w / 2.0); base[a][3] = (float)(h / 2.0);
    }
}

void rpn_levels_desc(const float* const head[5], const int H[5], const int W[5], int head_ld, int pre_topk, RpnLevels* out) {
    static const int sizes[5] = {32, 64, 128, 256, 512};
    static const int strides[5] = {4, 8, 16, 32, 64};
    memset(out, 0, sizeof(*out));
    out->head_ld = head_ld;
    out->pre_topk = pre_topk;
    for (int l = 0; l < 5; ++l) {
        RpnLevel& L = out->lv[l];
        L.head = head[l]; L.H = H[l]; L.W = W[l]; L.stride = strides[l];
        L.n = H[l] * W[l] * 3;
        L.k = L.n < pre_topk ? L.n : pre_topk;
        apse_cell_anchors3(sizes[l], L.base);
    }
}

void rpn_select_plan(const float* const head[5], const int H[5], const int W[5], int head_ld, int pre_topk, RpnSelectPlan* out) {
    rpn_levels_desc(head, H, W, head_ld, pre_topk, &out->levels);
    // top-k tournament plan
    out->stages.clear();
    int slot = 0;
    std::vector<std::vector<int>> cur_slots(5), cur_counts(5);
    std::vector<TopkJob> st0;
    for (int l = 0; l < 5; ++l) {
        const int n = out->levels.lv[l].n;
        for (int beg = 0; beg < n; beg += 4096) {
            TopkJob j; memset(&j, 0, sizeof j);
            j.kind = 0; j.level = l; j.begin = beg; j.count = (n - beg) < 4096 ? (n - beg) : 4096;
            j.dst = slot++; j.dst_count = j.count < pre_topk ? j.count : pre_topk;
            cur_slots[l].push_back(j.dst); cur_counts[l].push_back(j.dst_count);
            st0.push_back(j);
        }
    }
    out->stages.push_back(st0);
    for (;;) {
        std::vector<TopkJob> stn;
        bool any = false;
        for (int l = 0; l < 5; ++l) {
            if (cur_slots[l].size() <= 1) continue;
            any = true;
            std::vector<int> ns, nc;
            for (size_t i = 0; i < cur_slots[l].size(); i += 4) {
                TopkJob j; memset(&j, 0, sizeof j);
                j.kind = 1; j.level = l; int tot = 0;
                for (size_t k = i; k < i + 4 && k < cur_slots[l].size(); ++k) {
                    j.src[j.nsrc] = cur_slots[l][k]; j.src_count[j.nsrc] = cur_counts[l][k]; tot += cur_counts[l][k]; ++j.nsrc;
                }
                j.dst = slot++; j.dst_count = tot < pre_topk ? tot : pre_topk;
                ns.push_back(j.dst); nc.push_back(j.dst_count);
                stn.push_back(j);
            }
            cur_slots[l] = ns; cur_counts[l] = nc;
        }
        if (!any) break;
        out->stages.push_back(stn);
    }
    out->nslots = slot;
    for (int l = 0; l < 5; ++l) out->final_slot[l] = cur_slots[l][0];
}

void c4_rpn_desc(const float* head, int H, int W, int ld, int pre_topk, C4Rpn* Rp) {
    C4Rpn& R = *Rp;
    memset(&R, 0, sizeof R);
    R.head = head; R.H = H; R.W = W; R.ld = ld; R.stride = 16;
    R.n = H * W * 15;
    R.k = R.n < pre_topk ? R.n : pre_topk;
    static const int sizes[5] = {32, 64, 128, 256, 512};
    for (int si = 0; si < 5; ++si) apse_cell_anchors3(sizes[si], R.base + 3 * si);          // sizes outer, ratios inner
}

int build_plan(apse_ctx* c) {
    const apse_config& g = c->cfg;
    const int B = g.max_batch;
    c->PH = apse_roundup(g.image_h, 32);
    c->PW = apse_roundup(g.image_w, 32);
    layout_results(c);
    c->res = dalloc<uint8_t>(c, c->lay.bytes);
    if (!c->res) return fail(c, APSE_E_NOMEM, "results alloc");
    int rc;
    // ---- backbone
    Tens cur;
    bool fused_stem = false;
    if (storage_type(c)) {
        // 16-bit storage modes: space-to-depth(2) input (elementwise.hip, input_store) and the stem as a 4x4 / stride-1 convolution
        // over 16 channels: one 64-element k-step per filter row on the scheduled 16-bit kernel (K = 256 instead of the 448 a
        // 7-pixel x 8-channel run would pad to; the f32-input stem ran on the legacy conditional-load kernel at 428 us per batch 8)
        Tens x0 = make_t(c, "input", B, c->PH / 2, c->PW / 2, 16, storage_type(c));
        ConvSpec sp{"stem.conv1", {"backbone.bottom_up.stem.conv1"}, 4, 4, 1, 2, 1};
        sp.s2d = 1;
        // ... and the max-pool behind it in the same kernel (stem_pool16.hip): the stem output never goes to HBM.
        // APSE_NO_STEM_FUSE (read when the context is built): the two-kernel form, for the equality test and A/B runs.
        if (!getenv("APSE_NO_STEM_FUSE")) {
            Tens pooled = make_t(c, "stem", B, (x0.H + 2 - 3) / 2 + 1, (x0.W + 2 - 3) / 2 + 1, 64, storage_type(c));
            if (!pooled.p) return fail(c, APSE_E_NOMEM, "stem alloc");
            Tens unused;
            sp.out_view = &pooled;
            rc = add_conv(c, c->backbone, sp, x0, &unused);
            if (rc) return rc;
            c->t.erase("stem.conv1");                       // no such tensor in this form
            c->backbone.back().c.pool_y = pooled.p;
            cur = pooled;
            fused_stem = true;
        } else {
            rc = add_conv(c, c->backbone, sp, x0, &cur);
        }
    } else {
        Tens x0 = make_t(c, "input", B, c->PH, c->PW, 4);
        rc = add_conv(c, c->backbone, ConvSpec{"stem.conv1", {"backbone.bottom_up.stem.conv1"}, 7, 7, 2, 3, 1}, x0, &cur);
    }
    if (rc) return rc;
    if (!fused_stem) cur = add_stem_pool(c, cur);
    for (int si = 0; si < 4; ++si) {
        const std::string stage = "res" + std::to_string(si + 2);
        for (int bi = 0; bi < g.blocks[si]; ++bi) {
            const std::string P = "backbone.bottom_up." + stage + "." + std::to_string(bi);
            const int stride = (bi == 0 && si > 0) ? 2 : 1;
            const bool last = (bi == g.blocks[si] - 1);
            Tens out;
            rc = add_bottleneck(c, c->backbone, P, P, cur, 1, stride, 0, last ? stage : P + ".out", &out);
            if (rc) return rc;
            fuse_bottleneck16(c, c->backbone, P + ".fused", cur, out);
            cur = out;
        }
    }
    // ---- FPN (top-down): inner5 = lateral5(res5); p5 = output5(inner5); inner_l = lateral_l(res_l) + up(inner_{l+1})
    // The first lateral is where a trunk joins the tail lane: from here on the plan overwrites maps that the previous forward's
    // heads read (p2..p5, then the RPN buffers); nothing in front of it does.
    c->fpn_step = (int)c->backbone.size();
    Tens inner, pl[5];
    for (int lvl = 5; lvl >= 2; --lvl) {
        char ln[64], on[64], rn[16], in_name[16], pn[8];
        snprintf(ln, sizeof ln, "backbone.fpn_lateral%d", lvl);
        snprintf(on, sizeof on, "backbone.fpn_output%d", lvl);
        snprintf(rn, sizeof rn, "res%d", lvl);
        snprintf(in_name, sizeof in_name, "inner%d", lvl);
        snprintf(pn, sizeof pn, "p%d", lvl);
        Tens ninner;
        ConvSpec lat{ln, {ln}, 1, 1, 1, 0, 0};
        lat.out_name = in_name;
        if (lvl != 5) { lat.res = &inner; lat.res_mode = 2; }
        rc = add_conv(c, c->backbone, lat, c->t[rn], &ninner);
        if (rc) return rc;
        inner = ninner;
        ConvSpec outc{on, {on}, 3, 3, 1, 1, 0};
        outc.out_name = pn;
        rc = add_conv(c, c->backbone, outc, inner, &pl[lvl - 2]);
        if (rc) return rc;
    }
    {
        Step st; st.kind = S_SUBSAMPLE; st.x = pl[3].p; st.H = pl[3].H; st.W = pl[3].W; st.C = 256;
        pl[4] = make_t(c, "p6", B, (pl[3].H - 1) / 2 + 1, (pl[3].W - 1) / 2 + 1, 256, pl[3].st);
        st.y = pl[4].p; st.c.name = "p6"; st.st = pl[3].st;
        c->backbone.push_back(st);
    }
    // ---- RPN head per level: conv3x3+relu, fused 1x1 (3 objectness + 12 deltas) -> ld 16
    static const int strides[5] = {4, 8, 16, 32, 64};
    // The 3x3 convolution runs per level; its outputs are slices of ONE buffer ([level][max_batch][H][W][256]) so that the
    // fused 1x1 head (objectness + deltas, shared weights) is a single launch over all rows of all levels
    // (five launches of 10-20 us, four of them with a handful of blocks, become one).
    size_t rows_total = 0, row_off[6] = {0};
    for (int l = 0; l < 5; ++l) { row_off[l] = rows_total; rows_total += (size_t)B * pl[l].H * pl[l].W; }
    row_off[5] = rows_total;
    const int rpn_st = storage_type(c);
    Tens t_all = make_t(c, "rpn_t_all", 1, 1, (int)rows_total, 256, rpn_st);
    if (!t_all.p) return fail(c, APSE_E_NOMEM, "rpn feature buffer");
    for (int l = 0; l < 5; ++l) {
        char tn[32];
        snprintf(tn, sizeof tn, "rpn_t%d", l + 2);
        Tens view = t_all;
        view.p = reinterpret_cast<float*>(reinterpret_cast<char*>(t_all.p) + row_off[l] * 256 * (rpn_st ? 2 : 4));
        Tens tt;
        ConvSpec sp{tn, {"proposal_generator.rpn_head.conv"}, 3, 3, 1, 1, 1};
        sp.out_view = &view;
        rc = add_conv(c, c->rpnhead, sp, pl[l], &tt);
        if (rc) return rc;
    }
    Tens h_all;
    {
        Tens in_all = t_all;                       // [1][rows_total][256] as one 1 x rows image
        float* hbuf = dalloc<float>(c, rows_total * 16);
        if (!hbuf) return fail(c, APSE_E_NOMEM, "rpn head buffer");
        ConvSpec sp{"rpn_head_all", {"proposal_generator.rpn_head.objectness_logits", "proposal_generator.rpn_head.anchor_deltas"},
                    1, 1, 1, 0, 0};
        sp.y_ld = 16; sp.out_ptr = hbuf;
        rc = add_conv(c, c->rpnhead, sp, in_all, &h_all);
        if (rc) return rc;
        ConvStep& hs = c->rpnhead.back().c;
        hs.fixed_items = 1;                        // all rows of all levels, whatever the batch of this forward
        hs.flops_per_item /= (double)B;            // profile accounting is per image
    }
    {
        const float* heads[5];
        int hH[5], hW[5];
        for (int l = 0; l < 5; ++l) {
            char hn[32];
            snprintf(hn, sizeof hn, "rpn_head%d", l + 2);
            Tens hh = h_all;
            hh.p = h_all.p + row_off[l] * 16;
            hh.H = pl[l].H; hh.W = pl[l].W; hh.C = 16;
            c->t[hn] = hh;
            heads[l] = hh.p; hH[l] = hh.H; hW[l] = hh.W;
        }
        RpnSelectPlan sel;
        rpn_select_plan(heads, hH, hW, 16, g.rpn_pre_topk, &sel);
        c->rl_host = sel.levels;
        c->rl_dev = dalloc<RpnLevels>(c, 1);
        hipMemcpy(c->rl_dev, &c->rl_host, sizeof(RpnLevels), hipMemcpyHostToDevice);
        c->stages = sel.stages;
        c->nslots = sel.nslots;
        for (int l = 0; l < 5; ++l) c->final_slot_host[l] = sel.final_slot[l];
        for (auto& sv : c->stages) c->stage_dev.push_back(dupload(c, sv));
        std::vector<int> fs(c->final_slot_host, c->final_slot_host + 5);
        c->final_slot_dev = dupload(c, fs);
        c->lists = dalloc<uint64_t>(c, (size_t)B * sel.nslots * 1024);
    }
    if ((rc = alloc_proposals(c, 5))) return rc;
    const int POST = g.rpn_post_topk, KD = g.dets_per_image;
    // ---- box head: ROIAlign 7x7 -> fc1 (7x7 valid conv) -> fc2 -> fused predictor (K+1 logits, 4K deltas), ld round_up(5K+1, 32)
    for (int l = 0; l < 4; ++l) { c->fm.p[l] = pl[l].p; c->fm.H[l] = pl[l].H; c->fm.W[l] = pl[l].W; c->fm.scale[l] = 1.0f / (float)strides[l]; }
    c->fm.st = pl[0].st;
    Tens pooled = make_t(c, "box_pooled", B * POST, 7, 7, 256, storage_type(c));
    Tens f1, f2;
    ConvSpec fc1{"box_fc1", {"roi_heads.box_head.fc1"}, 7, 7, 1, 0, 1, 7, 7};
    fc1.items = POST; fc1.count_kind = 1;
    rc = add_conv(c, c->boxhead, fc1, pooled, &f1);
    if (rc) return rc;
    ConvSpec fc2{"box_fc2", {"roi_heads.box_head.fc2"}, 1, 1, 1, 0, 1};
    fc2.items = POST; fc2.count_kind = 1;
    rc = add_conv(c, c->boxhead, fc2, f1, &f2);
    if (rc) return rc;
    if ((rc = add_box_predictor(c, f2))) return rc;
    alloc_box_inference(c);
    // ---- mask head on the packed detection list
    const int NM = B * KD;
    Tens mp = make_t(c, "mask_pooled", NM, 14, 14, 256, storage_type(c));
    Tens m = mp, ml;
    for (int i = 1; i <= 4; ++i) {
        char nm[48], wn[64];
        snprintf(nm, sizeof nm, "mask_fcn%d", i);
        snprintf(wn, sizeof wn, "roi_heads.mask_head.mask_fcn%d", i);
        Tens o;
        ConvSpec sp{nm, {wn}, 3, 3, 1, 1, 1};
        sp.items = KD; sp.count_kind = 2;
        rc = add_conv(c, c->maskhead, sp, m, &o);
        if (rc) return rc;
        m = o;
    }
    if ((rc = add_mask_predictor(c, m, &ml))) return rc;
    return finish_plan(c, 256);
}

// ------------------------------------------------------------------------------------------------ C4 plan (arch 1)
// detectron2 Base-RCNN-C4: ResNet stem + res2..res4 on the UNPADDED image (size_divisibility 0), StandardRPNHead on res4 (15
// anchors per cell), Res5ROIHeads: ROIAlignV2 14x14 on res4 -> res5 (first block stride 2 in its 1x1) -> 7x7 mean -> predictor;
// mask branch: ROIAlignV2 14x14 of the detections -> res5 -> deconv 2x2 + ReLU -> 1x1 predictor (14x14 logits).  f32 only.
static int add_res5(apse_ctx* c, std::vector<Step>& plan, const Tens& in, int items, int count_kind, const std::string& tag, Tens* out) {
    Tens cur = in;
    for (int bi = 0; bi < c->cfg.blocks[3]; ++bi) {
        const std::string T = tag + "." + std::to_string(bi);
        Tens o;
        int rc = add_bottleneck(c, plan, "roi_heads.res5." + std::to_string(bi), T, cur, items, bi == 0 ? 2 : 1, count_kind,
                                T + ".out" + std::to_string(bi), &o);
        if (rc) return rc;
        cur = o;
    }
    *out = cur;
    return APSE_OK;
}

int build_plan_c4(apse_ctx* c) {
    const apse_config& g = c->cfg;
    const int B = g.max_batch;
    c->PH = g.image_h;                    // size_divisibility 0: no padding
    c->PW = g.image_w;
    layout_results(c);
    c->res = dalloc<uint8_t>(c, c->lay.bytes);
    if (!c->res) return fail(c, APSE_E_NOMEM, "results alloc");
    int rc;
    // ---- backbone: stem + max-pool + res2..res4 (keys backbone.stem.*, backbone.res{2,3,4}.N.*)
    Tens cur;
    Tens x0 = make_t(c, "input", B, c->PH, c->PW, 4);
    rc = add_conv(c, c->backbone, ConvSpec{"stem.conv1", {"backbone.stem.conv1"}, 7, 7, 2, 3, 1}, x0, &cur);
    if (rc) return rc;
    cur = add_stem_pool(c, cur);
    for (int si = 0; si < 3; ++si) {
        const std::string stage = "res" + std::to_string(si + 2);
        for (int bi = 0; bi < g.blocks[si]; ++bi) {
            const std::string P = "backbone." + stage + "." + std::to_string(bi);
            const int stride = (bi == 0 && si > 0) ? 2 : 1;
            const bool last = bi == g.blocks[si] - 1;
            Tens out;
            rc = add_bottleneck(c, c->backbone, P, P, cur, 1, stride, 0, last ? stage : P + ".out", &out);
            if (rc) return rc;
            cur = out;
        }
    }
    const Tens res4 = c->t["res4"];
    if (res4.C < 256 || (res4.C & 255)) return fail(c, APSE_E_INVALID, "C4: res4 needs a multiple of 256 channels");
    // ---- RPN head on res4: conv 3x3 + ReLU, then objectness (15) and deltas (60) fused into one 1x1 with an 80-wide row
    {
        Tens t, h;
        rc = add_conv(c, c->rpnhead, ConvSpec{"rpn_conv", {"proposal_generator.rpn_head.conv"}, 3, 3, 1, 1, 1}, res4, &t);
        if (rc) return rc;
        ConvSpec sp{"rpn_head", {"proposal_generator.rpn_head.objectness_logits", "proposal_generator.rpn_head.anchor_deltas"},
                    1, 1, 1, 0, 0};
        sp.y_ld = 80;
        rc = add_conv(c, c->rpnhead, sp, t, &h);
        if (rc) return rc;
        if (c->rpnhead.back().c.p.Cout != 75) return fail(c, APSE_E_INVALID, "C4 RPN head: expected 15 objectness + 60 delta channels");
        c4_rpn_desc(h.p, h.H, h.W, 80, g.rpn_pre_topk, &c->c4r);
    }
    if ((rc = alloc_proposals(c, 1))) return rc;
    const int POST = g.rpn_post_topk, KD = g.dets_per_image;
    // ---- box branch: ROIAlign 14x14 of res4 -> res5 -> mean over 7x7 (box_mean) -> fused predictor
    Tens pooled = make_t(c, "box_pooled", B * POST, 14, 14, res4.C);
    if (!pooled.p) return fail(c, APSE_E_NOMEM, "C4 box features");
    Tens r5;
    rc = add_res5(c, c->c4_res5box, pooled, POST, 1, "box_res5", &r5);
    if (rc) return rc;
    c->t["box_res5"] = r5;
    Tens mean = make_t(c, "box_mean", B * POST, 1, 1, r5.C);
    if ((rc = add_box_predictor(c, mean))) return rc;
    alloc_box_inference(c);
    // ---- mask branch on the packed detection list: ROIAlign 14x14 -> res5 -> deconv + ReLU -> predictor (14 x 14 logits)
    const int NM = B * KD;
    Tens mp = make_t(c, "mask_pooled", NM, 14, 14, res4.C);
    Tens m5, ml;
    rc = add_res5(c, c->maskhead, mp, KD, 2, "mask_res5", &m5);
    if (rc) return rc;
    if ((rc = add_mask_predictor(c, m5, &ml))) return rc;
    if (ml.H != 14 || ml.W != 14) return fail(c, APSE_E_INVALID, "C4 mask logits must be 14 x 14");
    return finish_plan(c, res4.C);
}
