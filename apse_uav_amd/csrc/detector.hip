// libapse_hip.so context: run_plan (the per-forward launch sequence) and the context's C ABI of include/apse_hip.h.
// The plan it runs is built in plan.hip; the stateless operators of the ABI are in ops.hip (detector_ctx.h says which file
// holds what).  Host-side C++ only orchestrates; all arithmetic is in the HIP kernels of this directory.
// One context per device/process rank.  The caller's stream carries every launch, with one exception: a forward enqueued
// while a results copy is pending (a caller that runs ahead) keeps resize, trunk, FPN and the RPN convolutions there and sends
// the rest and its results copy to the context's tail lane (below).  No hidden syncs except apse_read_results.
#include "detector_ctx.h"

#include <math.h>
#include <string.h>

static std::string g_create_error;

int fail(apse_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}
int apse_fail_global(int code, const char* msg) { return fail(nullptr, code, msg); }

// Profiling: the index of a fresh event pair in this forward's half of the pool (the launch records ev_pool[e], ev_pool[e + 1]
// around its kernel), or -1 when profiling is off or the half is used up.  The first pair a forward takes is preceded by the
// calibration pair: two back-to-back records; their elapsed time (the marker overhead a timed kernel also pays) is subtracted
// from every measurement of this forward.
static int take_event_pair(apse_ctx* c, hipStream_t s) {
    if (!c->prof_on) return -1;
    if (c->ev_used == 0) {
        hipEventRecord(c->ev_pool[c->ev_base], s);
        hipEventRecord(c->ev_pool[c->ev_base + 1], s);
        c->ev_used = 2;
    }
    if (c->ev_used + 2 > APSE_EV_HALF) return -1;
    const int e0 = c->ev_base + c->ev_used;
    c->ev_used += 2;
    return e0;
}

// ---- the tail lane (detector_ctx.h)
// The lane carries a forward only when the caller runs ahead: the forward was enqueued while a results copy was pending
// (between apse_read_results_begin and _end), i.e. there is a frame beside whose tail the next trunk can run.  A caller that
// reads each forward before enqueuing the next has nothing to overlap, and several contexts in flight on streams of their own
// already fill the idle capacity: both keep every launch on the caller's stream (measured: DESIGN.md section 6).
static bool lane_active(const apse_ctx* c) { return c->lane_on && !c->prof_on && c->lane_armed; }

// The lane's stream and events, all or nothing: after a failure the context has no lane (c->lane stays null).
static void lane_teardown(apse_ctx* c) {
    hipEvent_t* evs[5] = {&c->fork_ev, &c->follow_ev, &c->tail_ev, &c->bits_ev[0], &c->bits_ev[1]};
    for (hipEvent_t* e : evs) { if (*e) hipEventDestroy(*e); *e = nullptr; }
    if (c->lane) hipStreamDestroy(c->lane);
    c->lane = nullptr;
    c->fork_pending = c->follow_pending = c->tail_live = c->bits_live[0] = c->bits_live[1] = false;
    c->caller_dirty = true;          // a later lane starts behind whatever the caller's stream holds
}

static int lane_create(apse_ctx* c) {
    if (c->lane) return APSE_OK;
    hipEvent_t* evs[5] = {&c->fork_ev, &c->follow_ev, &c->tail_ev, &c->bits_ev[0], &c->bits_ev[1]};
    hipError_t e = hipSuccess;
    for (hipEvent_t* ev : evs) if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    // non-blocking: the legacy default stream (bench.py's headline loop) would serialise against a blocking one
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->lane, hipStreamNonBlocking);
    if (e != hipSuccess) {
        lane_teardown(c);
        return fail(c, APSE_E_HIP, std::string("tail lane: ") + hipGetErrorString(e));
    }
    return APSE_OK;
}

// true when everything recorded under `ev` has finished.  A not-ready answer is no error: it alone is taken off the runtime's
// last-error slot (which PyTorch reads after its own launches); any other error stays there.
static bool event_done(hipEvent_t ev) {
    if (hipEventQuery(ev) == hipSuccess) return true;
    if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();
    return false;
}

// The stream of one ABI entry's lane-owned launches: the lane, made to wait for what the caller's stream holds for it, or the
// caller's stream when the lane is off.  Leaving the scope records tail_ev behind whatever the entry did enqueue, also on an
// error return, so that no later wait refers to an event that was never recorded.
struct LaneScope {
    apse_ctx* c = nullptr; hipStream_t s = nullptr; bool on = false;
    int bits_k = -1;                 // apse_mask_tail: the bit-plane set this entry writes; its event is recorded with tail_ev
    int begin(apse_ctx* c_, hipStream_t caller) {
        c = c_; s = caller;
        if (!lane_active(c)) return APSE_OK;
        int rc = lane_create(c);
        if (rc) return rc;
        if (c->caller_dirty) {
            HIPCHK(c, hipEventRecord(c->fork_ev, caller));
            c->caller_dirty = false; c->fork_pending = true;
        }
        if (c->fork_pending) { HIPCHK(c, hipStreamWaitEvent(c->lane, c->fork_ev, 0)); c->fork_pending = false; }
        if (c->follow_pending) { HIPCHK(c, hipStreamWaitEvent(c->lane, c->follow_ev, 0)); c->follow_pending = false; }
        s = c->lane; on = true;
        return APSE_OK;
    }
    ~LaneScope() {
        if (!on) return;
        if (bits_k >= 0 && hipEventRecord(c->bits_ev[bits_k], c->lane) == hipSuccess) c->bits_live[bits_k] = true;
        if (hipEventRecord(c->tail_ev, c->lane) == hipSuccess) c->tail_live = true;
    }
};

// Entries outside the forward: the caller's stream waits for the lane (for `ev`: tail_ev, or the event of one bit-plane set).
static int lane_join(apse_ctx* c, hipStream_t s, hipEvent_t ev, bool live) {
    if (!c->lane || !live || event_done(ev)) return APSE_OK;
    HIPCHK(c, hipStreamWaitEvent(s, ev, 0));
    ++c->lane_stats[1];
    return APSE_OK;
}
static int lane_join(apse_ctx* c, hipStream_t s) { return lane_join(c, s, c->tail_ev, c->tail_live); }
// ... and when such an entry has put work that reads or writes lane-owned buffers on the caller's stream, the lane's next
// launch follows it
static int lane_follow(apse_ctx* c, hipStream_t s) {
    if (!c->lane) return APSE_OK;
    HIPCHK(c, hipEventRecord(c->follow_ev, s));
    c->follow_pending = true;
    return APSE_OK;
}
// the same for an entry without a stream argument: the host waits until the lane is empty
static int lane_drain(apse_ctx* c) {
    if (!c->lane) return APSE_OK;
    if (c->tail_live && !event_done(c->tail_ev)) ++c->lane_stats[1];
    HIPCHK(c, hipStreamSynchronize(c->lane));
    ++c->lane_stats[3];
    return APSE_OK;
}

// lane_stats[0]: one per forward (a forward starts with apse_backbone) whose tail went to the lane, however many of
// apse_rpn_levels / apse_set_detections it calls
static void count_lane_forward(apse_ctx* c, bool on) {
    if (!on || c->fwd_counted) return;
    ++c->lane_stats[0];
    c->fwd_counted = true;
}

static int run_plan(apse_ctx* c, std::vector<Step>& plan, int batch, hipStream_t s) {
    int* total_dev = reinterpret_cast<int*>(c->res + c->lay.total);
    int* propcnt_dev = reinterpret_cast<int*>(c->res + c->lay.prop_count);
    float* ws = (c->lane && s == c->lane) ? c->ws_lane : c->ws;
    for (size_t si = 0; si < plan.size(); ++si) {
        Step& st = plan[si];
        int rc = APSE_OK;
        if (&plan == &c->backbone && (int)si == c->fpn_step && c->lane && c->tail_live && !event_done(c->tail_ev)) {
            // the FPN and the RPN convolutions overwrite what the previous forward's heads read (p2..p5, rpn_t_all, the RPN
            // logits / deltas): wait for its tail.  stem..res5 write none of these; this also bounds the run-ahead to one frame.
            ++c->lane_stats[2];
            HIPCHK(c, hipStreamWaitEvent(s, c->tail_ev, 0));
        }
        if (st.kind == S_CONV) {
            ConvParams p = st.c.p;
            // next convolution of this plan: its filters are prefetched by this launch
            for (size_t sj = si + 1; sj < plan.size() && sj <= si + 2; ++sj)
                if (plan[sj].kind == S_CONV) {
                    const ConvParams& q = plan[sj].c.p;
                    const size_t elems = q.wu ? (size_t)16 * q.Cout * (1 << q.cin_log2) : (size_t)apse_roundup(q.Cout, 128) * q.KH * q.KWCp;
                    p.next_w = q.w16 ? (const void*)q.w16 : (q.wu ? (const void*)q.wu : (const void*)q.w);
                    const size_t bytes = elems * (q.w16 ? 2 : 4);
                    p.next_w_bytes = bytes > (64u << 20) ? (64u << 20) : (unsigned)bytes;
                    break;
                }
            p.B = st.c.fixed_items > 0 ? st.c.fixed_items : batch * st.c.b_mult;
            p.M = p.B * p.OH * p.OW;
            p.ws = ws;
            // In-launch split-K reduction (last arriver) measured SLOWER here than the separate reduce kernel
            // (f32 132 -> 111 FPS): 64-512 KB of slabs per tile and an agent-scope release (L2 write-back) per
            // block; it stays available through apse_conv_desc.fuse_reduce for small slabs.
            p.tile_cnt = nullptr;
            p.m_count = nullptr; p.m_per_item = p.OH * p.OW; p.m_hint = 0;
            int cfg = st.c.cfg;
            if (st.c.count_kind == 2) {
                p.m_count = total_dev;
                // the previous forward's count sizes the GRID only (blocks are persistent over the live tiles, so any
                // grid computes every tile the same way); tile shape and K split are plan constants (add_conv)
                const int mh = (c->hint_total > 0 ? c->hint_total : 1) * p.m_per_item;
                p.m_hint = mh < p.M ? mh : p.M;
                // 16-bit modes, unsplit layers (round 4): the plan shapes these GEMMs for 8 detections per image; a frame with 40
                // has five times the rows, and 64x64 tiles then run at half the rate of 128x128 ones.  The single-k-group 4-wave
                // tiles (128x128, 64x64, 128x64) add every accumulator's products in the same ascending-k order -- the same bits
                // (tests/test_gpu_ops.py::test_conv2d_16bit_tiles_are_bit_identical) -- so the tile may follow the hinted row count
                // without a frame's results depending on what ran before it.  f32 (two-k-group shapes, split K) keeps the plan's.
                if (p.prec != 0 && p.splitk == 1 && (cfg == 0 || cfg == 1 || cfg == 3)) {
                    int sk_dyn = 1;
                    const int cfg_dyn = apse_conv_pick_cfg(p.m_hint, p.Cout, p.steps_total, &sk_dyn);
                    if (sk_dyn == 1 && (cfg_dyn == 0 || cfg_dyn == 1 || cfg_dyn == 3)) cfg = cfg_dyn;
                }
            }
            else if (st.c.count_kind == 1 && batch == 1) p.m_count = propcnt_dev;
            const int e0 = take_event_pair(c, s);
            const hipEvent_t ev0 = e0 >= 0 ? c->ev_pool[e0] : nullptr, ev1 = e0 >= 0 ? c->ev_pool[e0 + 1] : nullptr;
            if (st.c.pool_y) {
                rc = apse_k_stem_pool16(p.x, p.w16, p.bias, st.c.pool_y, batch, p.H, p.W, p.prec, s, ev0, ev1);
                cfg = APSE_CFG_STEMPOOL;
            } else if (p.wu) {
                // Winograd: profiled in the slot of the tiled config it replaces, with the layer's algorithmic FLOPs
                rc = apse_launch_conv_winograd(p, s, ev0, ev1);
            } else {
                rc = apse_launch_conv(p, cfg, s, ev0, ev1);
                cfg = apse_conv_effective_cfg(p, cfg);                        // profile label of the kernel that actually ran
            }
            if (e0 >= 0) c->pending.push_back({cfg, st.c.flops_per_item, st.c.count_kind, st.c.b_mult, batch, e0, e0 + 1});
        } else if (st.kind == S_BNECK) {
            const int e0 = take_event_pair(c, s);
            const ConvParams& q1 = st.c.p;
            rc = apse_k_bottleneck64_fused16(st.x, st.p3.res, st.y, q1.w16, q1.bias, st.p2.w16, st.p2.bias, st.p3.w16, st.p3.bias, batch,
                                             st.H, st.W, st.C, st.st, s, e0 >= 0 ? c->ev_pool[e0] : nullptr,
                                             e0 >= 0 ? c->ev_pool[e0 + 1] : nullptr);
            if (e0 >= 0) c->pending.push_back({APSE_CFG_BNECK, st.c.flops_per_item, 0, 1, batch, e0, e0 + 1});
        } else if (st.kind == S_MAXPOOL) {
            rc = apse_k_maxpool3x3s2(st.x, st.y, batch, st.H, st.W, st.C, st.st, s);
        } else {
            rc = apse_k_subsample2(st.x, st.y, batch, st.H, st.W, st.C, st.st, s);
        }
        if (rc != APSE_OK) return fail(c, rc, "launch failed at step " + st.c.name);
    }
    return APSE_OK;
}

int fill_camera(UndistortParams& p, int H, int W, const double* m, const double* dist, int ndist, int do_undistort, int do_gamma) {
    memset(&p, 0, sizeof p);
    if (!m || ndist > 14 || ndist < 0 || (ndist > 0 && !dist)) return APSE_E_INVALID;
    for (int i = 0; i < ndist && i < 12; ++i) p.k[i] = dist[i];
    if (ndist > 12 && (dist[12] != 0.0 || (ndist > 13 && dist[13] != 0.0))) return APSE_E_INVALID;   // tilt model not built
    // inverse of the 3x3 camera matrix (double, adjugate / determinant)
    const double a = m[0], b = m[1], c = m[2], dd = m[3], e = m[4], f = m[5], g = m[6], h = m[7], k = m[8];
    const double det = a * (e * k - f * h) - b * (dd * k - f * g) + c * (dd * h - e * g);
    if (det == 0.0) return APSE_E_INVALID;
    const double id = 1.0 / det;
    p.ir[0] = (e * k - f * h) * id; p.ir[1] = (c * h - b * k) * id; p.ir[2] = (b * f - c * e) * id;
    p.ir[3] = (f * g - dd * k) * id; p.ir[4] = (a * k - c * g) * id; p.ir[5] = (c * dd - a * f) * id;
    p.ir[6] = (dd * h - e * g) * id; p.ir[7] = (b * g - a * h) * id; p.ir[8] = (a * e - b * dd) * id;
    p.fx = m[0]; p.fy = m[4]; p.u0 = m[2]; p.v0 = m[5];
    p.H = H; p.W = W; p.do_undistort = do_undistort; p.do_gamma = do_gamma;
    return APSE_OK;
}

// ================================================================================================ C ABI
extern "C" {

#ifndef APSE_SRC_HASH
#define APSE_SRC_HASH "unknown"
#endif
const char* apse_version(void) { return "apse_hip 0.6 (gfx950, f32 / bf16 / f16 MFMA) src " APSE_SRC_HASH; }

int apse_create(const apse_config* cfg, apse_ctx** out) {
    if (!cfg || !out) return fail(nullptr, APSE_E_INVALID, "null argument");
    // callers built against the header before `arch` was appended pass the shorter size: FPN
    // ... and before `tail_lane`: the default (lane on)
    const int old_size = (int)offsetof(apse_config, arch), arch_size = (int)offsetof(apse_config, tail_lane);
    if (cfg->struct_size != (int)sizeof(apse_config) && cfg->struct_size != old_size && cfg->struct_size != arch_size)
        return fail(nullptr, APSE_E_INVALID, "apse_config size mismatch");
    apse_config cf;
    memset(&cf, 0, sizeof cf);
    memcpy(&cf, cfg, (size_t)cfg->struct_size);
    cf.struct_size = (int)sizeof(apse_config);
    cfg = &cf;
    if (cfg->arch != 0 && cfg->arch != 1) return fail(nullptr, APSE_E_INVALID, "arch must be 0 (FPN) or 1 (C4)");
    if (cfg->arch == 1) {
        // C4 limits: the single-level RPN keeps up to 6000 pre-NMS proposals (detectron2's C4 default); f32 only; the res5 stage
        // runs on every box ROI (1000 x 14 x 14 x 1024 f32 = 0.8 GB of pooled features per frame), so the batch is capped where
        // every activation tensor stays below 2^31 bytes
        if (cfg->rpn_pre_topk < 1 || cfg->rpn_pre_topk > APSE_C4_MAX_PRE_TOPK)
            return fail(nullptr, APSE_E_INVALID, "C4 (arch 1): rpn_pre_topk " + std::to_string(cfg->rpn_pre_topk) + " outside 1.." +
                                                 std::to_string(APSE_C4_MAX_PRE_TOPK));
        if (cfg->compute_dtype != 0)
            return fail(nullptr, APSE_E_INVALID, "C4 (arch 1): compute_dtype must be 0 (f32); the 16-bit modes are FPN only");
        if (cfg->max_batch > APSE_C4_MAX_BATCH)
            return fail(nullptr, APSE_E_INVALID, "C4 (arch 1): max_batch " + std::to_string(cfg->max_batch) + " above the limit " +
                                                 std::to_string(APSE_C4_MAX_BATCH));
    }
    const int pre_cap = cfg->arch == 1 ? APSE_C4_MAX_PRE_TOPK : 1000;
    if (cfg->max_batch < 1 || cfg->max_batch > 64 || cfg->rpn_pre_topk > pre_cap || cfg->rpn_post_topk > 1000 ||
        cfg->dets_per_image > 100 || cfg->num_classes < 1 || cfg->num_classes > APSE_MAX_CLASSES || cfg->embed_dim > 256 ||
        cfg->max_batch * cfg->dets_per_image > 1024)
        return fail(nullptr, APSE_E_INVALID, "config out of supported range");
    {
        // fewer than 1 / score_thresh classes of one ROI can score above score_thresh: a bound on the box candidates of an image.
        // detectron2 0.1.2's batched_nms switches to another method (no category offset, unstable sort) from 40000 boxes on; the
        // library restates only the offset form, so a config that could reach the other one is refused.
        const double t = cfg->score_thresh;
        const double per_roi = t > 0.0 ? ceil(1.0 / t) - 1.0 : (double)cfg->num_classes;
        const double bound = (double)cfg->rpn_post_topk * (per_roi < cfg->num_classes ? per_roi : (double)cfg->num_classes);
        if (bound >= 40000.0)
            return fail(nullptr, APSE_E_INVALID,
                        "box candidate bound rpn_post_topk * min(num_classes, ceil(1 / score_thresh) - 1) = " +
                            std::to_string((long long)bound) + " reaches 40000, where detectron2's batched_nms changes method");
    }
    if (cfg->frame_h < 1 || cfg->frame_w < 1 || cfg->frame_h > APSE_MAX_FRAME_H || cfg->frame_w > APSE_MAX_FRAME_W)
        return fail(nullptr, APSE_E_INVALID, "frame size out of supported range (1 <= frame_h <= " + std::to_string(APSE_MAX_FRAME_H) +
                                             ", 1 <= frame_w <= " + std::to_string(APSE_MAX_FRAME_W) + ")");
    if (cfg->compute_dtype < 0 || cfg->compute_dtype > 2 || (cfg->compute_dtype && !cfg->storage16))
        return fail(nullptr, APSE_E_INVALID, "compute_dtype 1 / 2 (bf16 / f16 matrix cores) needs storage16 = 1: the f32-storage variant "
                                             "of the 16-bit modes was removed in round 4 (no BASELINE configuration uses it)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, APSE_E_HIP, "no HIP device visible: the apse_uav hot path has no CPU fallback");
    if (hipSetDevice(cfg->device) != hipSuccess) return fail(nullptr, APSE_E_HIP, "hipSetDevice failed");
    apse_ctx* c = new apse_ctx();
    c->cfg = *cfg;
    c->c4 = cfg->arch == 1;
    {
        const char* e = getenv("APSE_F32_WINOGRAD");
        c->f32_winograd = !(e && atoi(e) == 0);
    }
    {
        // the tail lane: FPN only (the C4 heads read res4, which the next trunk writes early)
        const char* e = getenv("APSE_TAIL_LANE");
        c->lane_on = !c->c4 && cfg->tail_lane >= 0 && !(e && atoi(e) == 0);
    }
    *out = c;
    return APSE_OK;
}

void apse_destroy(apse_ctx* c) {
    if (!c) return;
    hipSetDevice(c->cfg.device);
    if (c->lane) {
        hipStreamSynchronize(c->lane);              // pending tail work reads the buffers freed below
        lane_teardown(c);
    }
    for (void* p : c->allocs) hipFree(p);
    if (c->rf_mask) hipFree(c->rf_mask);
    if (c->mrf_idx) hipFree(c->mrf_idx);
    if (c->read_ev) hipEventDestroy(c->read_ev);
    for (int k = 0; k < 2; ++k) {
        if (c->given_ev[k]) hipEventDestroy(c->given_ev[k]);
        if (c->given_host[k]) hipHostFree(c->given_host[k]);
    }
    delete c;
}

const char* apse_last_error(apse_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int apse_set_weight(apse_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!c || !name || !host || !shape || ndim < 1 || ndim > 4) return fail(c, APSE_E_INVALID, "bad weight argument");
    if (c->finalized) return fail(c, APSE_E_STATE, "weights already finalized");
    HostW w;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { w.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    w.v.assign(host, host + n);
    c->hw[name] = std::move(w);
    return APSE_OK;
}

int apse_finalize_weights(apse_ctx* c) {
    if (!c) return APSE_E_INVALID;
    if (c->finalized) return fail(c, APSE_E_STATE, "already finalized");
    hipSetDevice(c->cfg.device);
    int rc = c->c4 ? build_plan_c4(c) : build_plan(c);
    if (rc) return rc;
    c->hw.clear();
    c->finalized = true;
    return APSE_OK;
}

int apse_set_resize_tables(apse_ctx* c, const int* hb, const int* hc, int hk, const int* vb, const int* vc, int vk) {
    if (!c || !hb || !hc || !vb || !vc) return fail(c, APSE_E_INVALID, "null table");
    const apse_config& g = c->cfg;
    std::vector<int> a(hb, hb + 2 * g.image_w), b(hc, hc + (size_t)hk * g.image_w), d(vb, vb + 2 * g.image_h),
        e(vc, vc + (size_t)vk * g.image_h);
    for (int i = 0; i < g.image_w; ++i)
        if (a[2 * i] < 0 || a[2 * i + 1] > hk || a[2 * i] + a[2 * i + 1] > g.frame_w) return fail(c, APSE_E_INVALID, "bad horizontal bounds");
    for (int i = 0; i < g.image_h; ++i)
        if (d[2 * i] < 0 || d[2 * i + 1] > vk || d[2 * i] + d[2 * i + 1] > g.frame_h) return fail(c, APSE_E_INVALID, "bad vertical bounds");
    c->hb = dupload(c, a); c->hc = dupload(c, b); c->vb = dupload(c, d); c->vc = dupload(c, e);
    c->hk = hk; c->vk = vk;
    c->hcT = nullptr;
    if (hk <= 8) {
        std::vector<int> t((size_t)8 * g.image_w, 0);
        for (int i = 0; i < g.image_w; ++i)
            for (int j = 0; j < a[2 * i + 1] && j < hk; ++j) t[(size_t)j * g.image_w + i] = b[(size_t)i * hk + j];
        c->hcT = dupload(c, t);
    }
    return APSE_OK;
}

#define NEED_READY(c, batch)                                                                     \
    if (!(c) || !(c)->finalized) return fail(c, APSE_E_STATE, "weights not finalized");          \
    if ((batch) < 1 || (batch) > (c)->cfg.max_batch) return fail(c, APSE_E_INVALID, "batch out of range");

int apse_preprocess_frames(apse_ctx* c, const uint8_t* frames, int batch, void* stream) {
    NEED_READY(c, batch);
    if (!c->hb) return fail(c, APSE_E_STATE, "resize tables not set");
    const apse_config& g = c->cfg;
    int rc = apse_k_pil_resize(frames, c->rs_tmp, c->t["input"].p, c->t["input"].st, nullptr, c->hb, c->hc, c->hk, c->vb, c->vc, c->vk, batch,
                               g.frame_h, g.frame_w, g.image_h, g.image_w, c->PH, c->PW, g.pixel_mean, c->cam_on ? &c->cam : nullptr, c->cam_lut, c->cam_map_ok ? c->cam_map : nullptr,
                               c->hcT, c->rs_pitch, nullptr, (hipStream_t)stream);
    return rc ? fail(c, rc, "pil resize launch failed") : APSE_OK;
}

int apse_preprocess_frames_yuv(apse_ctx* c, const uint8_t* frames, int batch, int pitch, int format, int matrix, void* stream) {
    NEED_READY(c, batch);
    if (!c->hb) return fail(c, APSE_E_STATE, "resize tables not set");
    if (!frames) return fail(c, APSE_E_INVALID, "null frames");
    const apse_config& g = c->cfg;
    YuvSource y;
    const char* why = yuv_source_fill(y, g.frame_h, g.frame_w, pitch, format, matrix);
    if (why) return fail(c, APSE_E_INVALID, why);
    if (c->cam_on) {
        // convert, then preprocess_img: the converter writes BGR frames the fused undistort + gamma pass then gathers from (a YUV
        // form of the 2x2 gather would save 25 MB of the ~37 MB this moves per 4K frame, on a path one launch long)
        if (!c->yuv_bgr) {
            hipSetDevice(g.device);
            c->yuv_bgr = dalloc<uint8_t>(c, (size_t)g.max_batch * g.frame_h * g.frame_w * 3 + 16, false);
            if (!c->yuv_bgr) return fail(c, APSE_E_NOMEM, "YUV -> BGR scratch frames alloc");
        }
        int rc = apse_k_yuv_to_bgr(&y, frames, c->yuv_bgr, batch, (hipStream_t)stream);
        if (rc) return fail(c, rc, "yuv_to_bgr launch failed");
        return apse_preprocess_frames(c, c->yuv_bgr, batch, stream);
    }
    int rc = apse_k_pil_resize(frames, c->rs_tmp, c->t["input"].p, c->t["input"].st, nullptr, c->hb, c->hc, c->hk, c->vb, c->vc, c->vk, batch,
                               g.frame_h, g.frame_w, g.image_h, g.image_w, c->PH, c->PW, g.pixel_mean, nullptr, nullptr, nullptr,
                               c->hcT, c->rs_pitch, &y, (hipStream_t)stream);
    return rc ? fail(c, rc, "pil resize (YUV) launch failed: batch of 2 GiB or more?") : APSE_OK;
}

int apse_preprocess_images(apse_ctx* c, const float* images, int batch, void* stream) {
    NEED_READY(c, batch);
    const apse_config& g = c->cfg;
    int rc = apse_k_chw_norm(images, c->t["input"].p, c->t["input"].st, batch, g.image_h, g.image_w, c->PH, c->PW, g.pixel_mean,
                             (hipStream_t)stream);
    return rc ? fail(c, rc, "chw normalise launch failed") : APSE_OK;
}

int apse_backbone(apse_ctx* c, int batch, void* stream) {
    NEED_READY(c, batch);
    c->caller_dirty = true;                         // the lane's next launch follows the maps written here
    c->lane_armed = c->read_pending != nullptr;     // this forward runs ahead of a read: its tail goes to the lane
    c->fwd_since_read = true;
    c->fwd_counted = false;
    return run_plan(c, c->backbone, batch, (hipStream_t)stream);
}

int apse_rpn_levels(apse_ctx* c, int batch, int level_mask, void* stream) {
    NEED_READY(c, batch);
    level_mask &= 31;
    if (!level_mask) return fail(c, APSE_E_INVALID, "empty RPN level mask");
    hipStream_t s = (hipStream_t)stream;
    const apse_config& g = c->cfg;
    if (c->c4 && level_mask != 31) return fail(c, APSE_E_INVALID, "C4 (arch 1) has one RPN level: level_mask must be 31");
    int rc;
    // without an apse_backbone in front (whose first FPN step has joined the lane) the convolutions below would rewrite the RPN
    // maps while the lane's selection of the previous call may still read them: join here
    if (!c->caller_dirty && (rc = lane_join(c, s))) return rc;
    rc = run_plan(c, c->rpnhead, batch, s);
    if (rc) return rc;
    // the fork: selection and everything behind it go to the tail lane, behind the RPN convolutions just enqueued
    c->caller_dirty = true;
    LaneScope ln;
    if ((rc = ln.begin(c, s))) return rc;
    count_lane_forward(c, ln.on);
    s = ln.s;
    if (c->c4) {
        int* propcnt = reinterpret_cast<int*>(c->res + c->lay.prop_count);
        rc = apse_k_c4_rpn(&c->c4r, g.rpn_pre_topk, g.rpn_post_topk, (float)g.image_h, (float)g.image_w, (float)log(1000.0 / 16.0),
                           g.rpn_nms, c->dec_boxes, c->dec_scores, c->dec_valid, c->c4_nms, c->props, c->prop_scores, c->prop_entry,
                           propcnt, batch, s);
        c->box_maxc_clean = false;
        return rc ? fail(c, rc, "C4 rpn selection launch failed") : APSE_OK;
    }
    for (size_t i = 0; i < c->stages.size(); ++i) {
        rc = apse_k_rpn_topk_stage(c->rl_dev, c->stage_dev[i], (int)c->stages[i].size(), c->lists, c->nslots, batch,
                                   i == 0 ? c->maxc : nullptr, s);
        if (rc) return fail(c, rc, "rpn top-k stage launch failed");
    }
    rc = apse_k_rpn_decode(c->rl_dev, g.rpn_pre_topk, c->lists, c->nslots, c->final_slot_dev, (float)g.image_h, (float)g.image_w,
                           (float)log(1000.0 / 16.0), c->dec_boxes, c->dec_scores, c->dec_valid, c->maxc, level_mask, batch, s);
    if (rc) return fail(c, rc, "rpn decode launch failed");
    rc = apse_k_nms_percat(c->dec_boxes, c->dec_scores, c->dec_valid, 5 * g.rpn_pre_topk, g.rpn_pre_topk, 0, c->maxc, g.rpn_nms,
                           c->keep_idx, c->keep_cnt, 5, c->nms_scratch, level_mask, batch, 1, s);
    if (rc) return fail(c, rc, "rpn nms launch failed");
    int* propcnt = reinterpret_cast<int*>(c->res + c->lay.prop_count);
    rc = apse_k_rank_final(c->dec_boxes, c->dec_scores, 5 * g.rpn_pre_topk, c->keep_idx, c->keep_cnt, 5, g.rpn_post_topk, c->props,
                           c->prop_scores, c->prop_entry, propcnt, c->maxc + g.max_batch, batch, s);
    c->box_maxc_clean = true;
    if (rc) return fail(c, rc, "rpn rank launch failed");
    return APSE_OK;
}

int apse_rpn(apse_ctx* c, int batch, void* stream) { return apse_rpn_levels(c, batch, 31, stream); }

static int pack_from_dets(apse_ctx* c, int batch, hipStream_t s) {
    const apse_config& g = c->cfg;
    uint8_t* r = c->res;
    c->sums_dirty = false;                 // pack_detections clears the integer sums of the mask tail
    c->masks_fresh = false;                // a new detection list: the bit planes still hold the previous list's masks
    return apse_k_pack_detections(c->det_boxes, c->det_scores, c->det_entry, c->det_cnt, batch, g.dets_per_image, g.num_classes,
                                  (float*)(r + c->lay.box_resized), (float*)(r + c->lay.score), (int*)(r + c->lay.cls),
                                  (int*)(r + c->lay.img), (int*)(r + c->lay.roi), (int*)(r + c->lay.total),
                                  (int*)(r + c->lay.offset), c->sums, s);
}

int apse_box_head(apse_ctx* c, int batch, void* stream) {
    NEED_READY(c, batch);
    LaneScope ln;
    int rc = ln.begin(c, (hipStream_t)stream);
    if (rc) return rc;
    hipStream_t s = ln.s;
    const apse_config& g = c->cfg;
    int* propcnt = reinterpret_cast<int*>(c->res + c->lay.prop_count);
    const int P = g.rpn_post_topk, K = g.num_classes;
    if (c->c4) {
        const Tens& f = c->t["res4"];
        rc = apse_k_roi_align_c4(f.p, f.H, f.W, f.C, 1.0f / 16.0f, c->props, nullptr, propcnt, nullptr, P, batch * P, 14,
                                 c->t["box_pooled"].p, s);
        if (rc) return fail(c, rc, "C4 roi_align(14) launch failed");
        rc = run_plan(c, c->c4_res5box, batch, s);
        if (rc) return rc;
        const Tens& r5 = c->t["box_res5"];
        rc = apse_k_mean_cells(r5.p, batch * P, r5.H * r5.W, r5.C, c->t["box_mean"].p, s);
        if (rc) return fail(c, rc, "C4 mean launch failed");
    } else {
        rc = apse_k_roi_align(&c->fm, c->props, nullptr, propcnt, nullptr, P, batch * P, 7, c->t["box_pooled"].p,
                              c->t["box_pooled"].st, s);
        if (rc) return fail(c, rc, "roi_align(7) launch failed");
    }
    rc = run_plan(c, c->boxhead, batch, s);
    if (rc) return rc;
    const float wts[4] = {10.f, 10.f, 5.f, 5.f};
    if (!c->box_maxc_clean) hipMemsetAsync(c->maxc + g.max_batch, 0, sizeof(uint32_t) * g.max_batch, s);
    c->box_maxc_clean = false;
    if (c->wide) {
        // 7..80 classes: wave-per-ROI candidates with class-major lists, list-fed per-class NMS, top-dets_per_image by one sort
        rc = apse_k_box_candidates_wide(c->t["box_pred"].p, c->pred_ld, K, c->props, propcnt, P, (float)g.image_h, (float)g.image_w,
                                        g.score_thresh, wts, (float)log(1000.0 / 16.0), c->cand_boxes, c->cand_scores, c->cand_valid,
                                        c->maxc + g.max_batch, c->probs, c->cls_list, c->cls_cnt, batch, s);
        if (rc) return fail(c, rc, "box candidates (wide) launch failed");
        rc = apse_k_nms_lists(c->cand_boxes, c->cand_scores, P * K, c->cls_list, c->cls_cnt, P, c->maxc + g.max_batch, g.box_nms,
                              c->keep_idx, c->keep_cnt, K, c->nms_scratch, batch, s);
        if (rc) return fail(c, rc, "box nms (wide) launch failed");
        rc = apse_k_rank_wide(c->cand_boxes, c->cand_scores, P * K, c->keep_idx, c->keep_cnt, K, g.dets_per_image, c->det_boxes,
                              c->det_scores, c->det_entry, c->det_cnt, batch, s);
        if (rc) return fail(c, rc, "box rank (wide) launch failed");
        rc = pack_from_dets(c, batch, s);
        return rc ? fail(c, rc, "pack launch failed") : APSE_OK;
    }
    rc = apse_k_box_candidates(c->t["box_pred"].p, c->pred_ld, K, c->props, propcnt, P, (float)g.image_h, (float)g.image_w, g.score_thresh,
                               wts, (float)log(1000.0 / 16.0), c->cand_boxes, c->cand_scores, c->cand_valid,
                               c->maxc + g.max_batch, c->probs, batch, s);
    if (rc) return fail(c, rc, "box candidates launch failed");
    rc = apse_k_nms_percat(c->cand_boxes, c->cand_scores, c->cand_valid, P * K, 0, K, c->maxc + g.max_batch, g.box_nms, c->keep_idx,
                           c->keep_cnt, K, c->nms_scratch, 0, batch, 0, s);
    if (rc) return fail(c, rc, "box nms launch failed");
    rc = apse_k_rank_final(c->cand_boxes, c->cand_scores, P * K, c->keep_idx, c->keep_cnt, K, g.dets_per_image, c->det_boxes,
                           c->det_scores, c->det_entry, c->det_cnt, nullptr, batch, s);
    if (rc) return fail(c, rc, "box rank launch failed");
    rc = pack_from_dets(c, batch, s);
    return rc ? fail(c, rc, "pack launch failed") : APSE_OK;
}

int apse_set_detections(apse_ctx* c, const float* boxes, const int* classes, const float* scores, const int* counts, int batch,
                        void* stream) {
    NEED_READY(c, batch);
    LaneScope ln;
    int rc = ln.begin(c, (hipStream_t)stream);
    if (rc) return rc;
    count_lane_forward(c, ln.on);
    hipStream_t s = ln.s;
    const apse_config& g = c->cfg;
    const int KD = g.dets_per_image, K = g.num_classes;
    const size_t nb = (size_t)g.max_batch * KD;
    const size_t bytes = nb * 16 + nb * 4 + nb * 4 + (size_t)g.max_batch * 4;
    const int slot = c->given_k ^= 1;
    if (!c->given_host[slot]) {
        HIPCHK(c, hipHostMalloc((void**)&c->given_host[slot], bytes, hipHostMallocDefault));
        HIPCHK(c, hipEventCreateWithFlags(&c->given_ev[slot], hipEventDisableTiming));
    } else {
        HIPCHK(c, hipEventSynchronize(c->given_ev[slot]));       // the copies of the call before last have left this block
    }
    float* db = (float*)c->given_host[slot];
    float* ds = db + nb * 4;
    int* de = (int*)(ds + nb);
    int* dc = de + nb;
    memset(db, 0, nb * 16 + nb * 4);
    for (size_t i = 0; i < nb; ++i) de[i] = -1;
    for (int b = 0; b < g.max_batch; ++b) dc[b] = 0;
    int o = 0;
    for (int b = 0; b < batch; ++b) {
        if (counts[b] < 0 || counts[b] > KD) return fail(c, APSE_E_INVALID, "too many given detections");
        dc[b] = counts[b];
        for (int k = 0; k < counts[b]; ++k, ++o) {
            memcpy(&db[((size_t)b * KD + k) * 4], boxes + (size_t)o * 4, 16);
            ds[(size_t)b * KD + k] = scores ? scores[o] : 1.0f;
            if (classes[o] < 0 || classes[o] >= K) return fail(c, APSE_E_INVALID, "class out of range");
            de[(size_t)b * KD + k] = k * K + classes[o];      // entry % K = class; entry / K = local index
        }
    }
    const size_t nbb = (size_t)batch * KD;
    HIPCHK(c, hipMemcpyAsync(c->det_boxes, db, nbb * 16, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->det_scores, ds, nbb * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->det_entry, de, nbb * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->det_cnt, dc, (size_t)batch * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(c->given_ev[slot], s));
    rc = pack_from_dets(c, batch, s);
    return rc ? fail(c, rc, "pack launch failed") : APSE_OK;
}

int apse_mask_tail(apse_ctx* c, int batch, void* stream) {
    NEED_READY(c, batch);
    LaneScope ln;
    int rc = ln.begin(c, (hipStream_t)stream);
    if (rc) return rc;
    hipStream_t s = ln.s;
    const apse_config& g = c->cfg;
    uint8_t* r = c->res;
    const int NM = batch * g.dets_per_image;
    int* total = (int*)(r + c->lay.total);
    if (c->c4) {
        const Tens& f = c->t["res4"];
        rc = apse_k_roi_align_c4(f.p, f.H, f.W, f.C, 1.0f / 16.0f, (float*)(r + c->lay.box_resized), (int*)(r + c->lay.img), nullptr,
                                 total, 0, NM, 14, c->t["mask_pooled"].p, s);
    } else {
        rc = apse_k_roi_align(&c->fm, (float*)(r + c->lay.box_resized), (int*)(r + c->lay.img), nullptr, total, 0, NM, 14,
                              c->t["mask_pooled"].p, c->t["mask_pooled"].st, s);
    }
    if (rc) return fail(c, rc, "roi_align(14) launch failed");
    rc = run_plan(c, c->maskhead, batch, s);
    if (rc) return rc;
    PasteParams p;
    p.boxes = (float*)(r + c->lay.box_resized); p.cls = (int*)(r + c->lay.cls); p.total = total;
    p.logits = c->t["mask_logits"].p; p.M = c->t["mask_logits"].H; p.ldc = c->t["mask_logits"].C;
    p.sx = (float)((double)g.frame_w / (double)g.image_w); p.sy = (float)((double)g.frame_h / (double)g.image_h);
    p.out_h = g.frame_h; p.out_w = g.frame_w; p.words_per_row = c->wpr; p.thresh = g.mask_thresh;
    p.boxes_out = (float*)(r + c->lay.box); p.valid = (int*)(r + c->lay.valid); p.rect = (int*)(r + c->lay.rect);
    // Two sets of bit planes, alternating per forward: a caller may enqueue the NEXT forward right behind apse_read_results_begin
    // (nothing in it depends on this one) and still copy this forward's mask windows out afterwards (apse_copy_mask_window reads
    // the set that belongs to the results last read).
    // the integer sums paste_masks adds into are cleared by pack_detections (apse_box_head / apse_set_detections); a caller that
    // repeats apse_mask_tail on one detection list (a timing loop) gets them cleared here, so the call is idempotent
    if (c->sums_dirty) HIPCHK(c, hipMemsetAsync(c->sums, 0, (size_t)g.max_batch * g.dets_per_image * 3 * sizeof(unsigned long long), s));
    c->sums_dirty = true;
    c->bits_cur ^= 1;
    ln.bits_k = c->bits_cur;               // recorded when the entry leaves, also on an error below
    if (!c->read_pending) c->bits_read = c->bits_cur;
    uint64_t* bits = c->bits2[c->bits_cur];
    p.bits = bits; p.sums = c->sums;
    unsigned long long* keys = (unsigned long long*)(r + c->lay.closest);      // raw (distance, index) keys; decoded on the host
    rc = apse_k_mask_paste(&p, NM, keys, g.dets_per_image, s);
    if (rc) return fail(c, rc, "mask paste launch failed");
    c->masks_fresh = true;                 // set bits_cur now holds this detection list's masks (apse_embed with crop features)
    rc = apse_k_closest_points(bits, p.rect, p.valid, c->sums, (int*)(r + c->lay.img), (int*)(r + c->lay.offset), total, NM,
                               g.dets_per_image, g.frame_h, g.frame_w, c->wpr, (int*)(r + c->lay.centroid), (int*)(r + c->lay.mass),
                               keys, c->hint_total, s);
    return rc ? fail(c, rc, "closest points launch failed") : APSE_OK;
}

int apse_embed(apse_ctx* c, int batch, void* stream) {
    NEED_READY(c, batch);
    LaneScope ln;
    int rc = ln.begin(c, (hipStream_t)stream);
    if (rc) return rc;
    hipStream_t s = ln.s;
    const apse_config& g = c->cfg;
    uint8_t* r = c->res;
    const int NM = batch * g.dets_per_image;
    int* total = (int*)(r + c->lay.total);
    if (c->c4) {
        const Tens& f = c->t["res4"];
        rc = apse_k_roi_pool_c4(f.p, f.H, f.W, f.C, (float*)(r + c->lay.box), (int*)(r + c->lay.img), total, NM, g.assoc_roi,
                                g.assoc_scale, (float*)c->t["assoc_pooled"].p, s);
    } else if (c->crop_features) {
        // rcnn_tracker.py:166-180: p2 * the detection's own mask (bilinear to p2's padded size), then roi_align(sampling_ratio 4).
        // The masks are the bit planes and rects the mask tail of THIS forward wrote (set bits_cur, same stream: ordered).
        if (!c->masks_fresh)
            return fail(c, APSE_E_STATE, "apse_embed with crop features needs the masks of these detections: call apse_mask_tail first");
        const Tens& p2 = c->t["p2"];
        rc = apse_k_roi_align_windows(p2.p, p2.st, p2.H, p2.W, (float*)(r + c->lay.box), (int*)(r + c->lay.img), 0, total, NM, nullptr,
                                      c->bits2[c->bits_cur], (int*)(r + c->lay.rect), (int*)(r + c->lay.valid), c->wpr, g.frame_h,
                                      g.frame_w, g.assoc_roi, 4, g.assoc_scale, (float*)c->t["assoc_pooled"].p, 0, s);
    } else {
        const Tens& p2 = c->t["p2"];
        rc = apse_k_roi_pool(p2.p, p2.st, p2.H, p2.W, (float*)(r + c->lay.box), (int*)(r + c->lay.img), total, NM, g.assoc_roi,
                             g.assoc_scale, (float*)c->t["assoc_pooled"].p, 0, 0, s);
    }
    if (rc) return fail(c, rc, c->crop_features && !c->c4 ? "masked roi_align launch failed" : "roi_pool launch failed");
    if (c->ws_assoc) {
        // K-sliced FC + ordered reduction + normalise (roi.hip): the filters of the plan's convolution step, its own two kernels
        const ConvParams& fp = c->embedfc[0].c.p;
        rc = apse_k_assoc_fc((const float*)c->t["assoc_pooled"].p, fp.w, fp.bias, c->ws_assoc, total, NM, fp.KH * fp.KWCp, g.embed_dim,
                             c->emb_raw, (float*)(r + c->lay.embedding), s);
        return rc ? fail(c, rc, "association FC launch failed") : APSE_OK;
    }
    rc = run_plan(c, c->embedfc, batch, s);
    if (rc) return rc;
    rc = apse_k_l2_normalize(c->emb_raw, (float*)(r + c->lay.embedding), g.embed_dim, total, NM, s);
    return rc ? fail(c, rc, "l2 normalise launch failed") : APSE_OK;
}

int apse_forward(apse_ctx* c, int batch, void* stream) {
    int rc;
    if ((rc = apse_backbone(c, batch, stream))) return rc;
    if ((rc = apse_rpn(c, batch, stream))) return rc;
    if ((rc = apse_box_head(c, batch, stream))) return rc;
    if ((rc = apse_mask_tail(c, batch, stream))) return rc;
    return apse_embed(c, batch, stream);
}

int apse_results_describe(apse_ctx* c, apse_results_layout* out) {
    if (!c || !out || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    *out = c->lay;
    return APSE_OK;
}

// The results block goes to the host in two halves so that a caller can put work behind the copy and still get the results
// as soon as the copy has landed: _begin enqueues the D2H and records an event right behind it, _end waits for THAT event
// (not for the stream: kernels enqueued after _begin -- the next frame's resize -- are not waited for).
int apse_read_results_begin(apse_ctx* c, void* host_dst, size_t bytes, void* stream) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    if (bytes < c->lay.bytes) return fail(c, APSE_E_INVALID, "results buffer too small");
    if (!c->read_ev) HIPCHK(c, hipEventCreateWithFlags(&c->read_ev, hipEventDisableTiming));
    // on the lane, behind the tail that fills the block: the next forward's trunk, enqueued on the caller's stream, is not waited for
    LaneScope ln;
    int rc = ln.begin(c, (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(host_dst, c->res, c->lay.bytes, hipMemcpyDeviceToHost, ln.s));
    HIPCHK(c, hipEventRecord(c->read_ev, ln.s));
    c->read_pending = host_dst;
    c->fwd_since_read = false;
    c->bits_read = c->bits_cur;                  // the mask windows that belong to these results
    if (c->prof_on) {                            // this forward's event pairs go to _end; the next forward records into the other half
        c->pending_read.swap(c->pending);
        c->pending.clear();
        c->cal_read = c->ev_used >= 2 ? c->ev_base : -1;
        c->ev_base ^= APSE_EV_HALF;
        c->ev_used = 0;
    }
    return APSE_OK;
}

int apse_read_results_end(apse_ctx* c, void* host_dst) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    if (!c->read_pending || c->read_pending != host_dst) return fail(c, APSE_E_STATE, "apse_read_results_end without a matching _begin");
    HIPCHK(c, hipEventSynchronize(c->read_ev));
    c->read_pending = nullptr;
    if (c->lane && !c->fwd_since_read && !c->prof_on) {
        // The caller has stopped running ahead (no forward was enqueued behind this read): give the lane's stream back.  An idle
        // extra stream is not free for the REST of the process -- the runtime spreads streams over four hardware queues, and one
        // idle non-blocking stream, created in front of them, cost four pipelined contexts 3 % (measured on the parent library
        // too: DESIGN.md section 6).  The next forward that runs ahead creates it again.
        HIPCHK(c, hipStreamSynchronize(c->lane));
        lane_teardown(c);
        ++c->lane_stats[3];
    }
    c->hint_total = *reinterpret_cast<const int*>(reinterpret_cast<const uint8_t*>(host_dst) + c->lay.total);
    {
        // closest-point table: the device leaves (f32 distance bits << 32 | row-major pixel index) keys, all ones = no point;
        // the record the caller sees holds 1-based (x, y) or (-1, -1), entries past the live detections (-1, -1)
        uint8_t* h = reinterpret_cast<uint8_t*>(host_dst) + c->lay.closest;
        const int kd = c->cfg.dets_per_image, W = c->cfg.frame_w;
        int live = c->hint_total < 0 ? 0 : c->hint_total;
        if (live > c->lay.n_max) live = c->lay.n_max;
        for (size_t t = 0; t < (size_t)c->lay.n_max * kd; ++t) {
            unsigned long long k;
            memcpy(&k, h + 8 * t, 8);
            int xy[2] = {-1, -1};
            if (t < (size_t)live * kd && k != ~0ull) {
                const unsigned lin = (unsigned)(k & 0xffffffffu);
                xy[0] = (int)(lin % (unsigned)W) + 1; xy[1] = (int)(lin / (unsigned)W) + 1;
            }
            memcpy(h + 8 * t, xy, 8);
        }
    }
    if (c->prof_on) {
        const uint8_t* h = reinterpret_cast<const uint8_t*>(host_dst);
        const int total = *reinterpret_cast<const int*>(h + c->lay.total);
        const int* pc = reinterpret_cast<const int*>(h + c->lay.prop_count);
        float cal = 0.f;
        if (c->cal_read >= 0 && hipEventElapsedTime(&cal, c->ev_pool[c->cal_read], c->ev_pool[c->cal_read + 1]) != hipSuccess) cal = 0.f;
        for (auto& q : c->pending_read) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->ev_pool[q.e0], c->ev_pool[q.e1]) != hipSuccess) continue;
            ms = ms > cal ? ms - cal : ms;
            double items = q.batch;
            if (q.count_kind == 1) { items = 0; for (int b = 0; b < q.batch; ++b) items += pc[b]; }
            else if (q.count_kind == 2) items = total;
            c->prof[q.cfg][0] += ms; c->prof[q.cfg][1] += q.flops_per_item * items; c->prof[q.cfg][2] += 1;
        }
        c->pending_read.clear();
        c->cal_read = -1;
    }
    return APSE_OK;
}

int apse_read_results(apse_ctx* c, void* host_dst, size_t bytes, void* stream) {
    int rc = apse_read_results_begin(c, host_dst, bytes, stream);
    return rc ? rc : apse_read_results_end(c, host_dst);
}

int apse_profile(apse_ctx* c, int enable) {
    if (!c) return APSE_E_INVALID;
    // the event pairs time single kernels of ONE stream: while profiling is on the lane is off.  Either switch first empties the
    // lane, and the first lane launch after profiling follows what the caller's stream was given meanwhile.
    int rc = lane_drain(c);
    if (rc) return rc;
    c->caller_dirty = true;
    if (enable && c->ev_pool.empty()) {
        c->ev_pool.resize(2 * APSE_EV_HALF);
        for (auto& e : c->ev_pool) if (hipEventCreate(&e) != hipSuccess) return fail(c, APSE_E_HIP, "hipEventCreate");
    }
    c->prof_on = enable != 0;
    c->pending.clear();
    c->pending_read.clear();
    c->cal_read = -1;
    c->ev_used = 0;
    return APSE_OK;
}

int apse_lane_stats(apse_ctx* c, long long* out4) {
    if (!c || !out4) return APSE_E_INVALID;
    memcpy(out4, c->lane_stats, sizeof(c->lane_stats));
    return APSE_OK;
}

int apse_profile_read(apse_ctx* c, double* out42, int reset) {
    if (!c || !out42) return APSE_E_INVALID;
    memcpy(out42, c->prof, sizeof(c->prof));
    if (reset) memset(c->prof, 0, sizeof(c->prof));
    return APSE_OK;
}

int apse_copy_mask_window(apse_ctx* c, int det, int x0, int y0, int x1, int y1, uint64_t* dst, void* stream) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    const apse_config& g = c->cfg;
    if (det < 0 || det >= g.max_batch * g.dets_per_image || x0 < 0 || y0 < 0 || x1 > g.frame_w || y1 > g.frame_h || x1 <= x0 || y1 <= y0)
        return fail(c, APSE_E_INVALID, "bad mask window");
    const int w0 = x0 >> 6, w1 = (x1 + 63) >> 6;
    const uint64_t* src = c->bits2[c->bits_read] + ((size_t)det * g.frame_h + y0) * c->wpr + w0;
    // joins the mask tail that wrote this set only: the next forward's tail (the other set) may still be running
    int rc = lane_join(c, (hipStream_t)stream, c->bits_ev[c->bits_read], c->bits_live[c->bits_read]);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)(w1 - w0) * 8, src, (size_t)c->wpr * 8, (size_t)(w1 - w0) * 8, (size_t)(y1 - y0),
                               hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return lane_follow(c, (hipStream_t)stream);
}

int apse_copy_mask_windows(apse_ctx* c, int n, const int* dets, const int* rects, uint64_t* dst, const long long* dst_off, void* stream) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    const apse_config& g = c->cfg;
    if (n < 0 || n > 100 || (n > 0 && (!dets || !rects || !dst || !dst_off))) return fail(c, APSE_E_INVALID, "bad mask windows");
    long long src[100]; int nw[100], rows[100];
    for (int k = 0; k < n; ++k) {
        const int x0 = rects[k * 4], y0 = rects[k * 4 + 1], x1 = rects[k * 4 + 2], y1 = rects[k * 4 + 3];
        if (dets[k] < 0 || dets[k] >= g.max_batch * g.dets_per_image || x0 < 0 || y0 < 0 || x1 > g.frame_w || y1 > g.frame_h || x1 <= x0 ||
            y1 <= y0 || dst_off[k] < 0)
            return fail(c, APSE_E_INVALID, "bad mask window");
        const int w0 = x0 >> 6, w1 = (x1 + 63) >> 6;
        src[k] = ((long long)dets[k] * g.frame_h + y0) * c->wpr + w0;
        nw[k] = w1 - w0; rows[k] = y1 - y0;
    }
    int rc = lane_join(c, (hipStream_t)stream, c->bits_ev[c->bits_read], c->bits_live[c->bits_read]);
    if (rc) return rc;
    rc = apse_k_copy_mask_windows(c->bits2[c->bits_read], dst, n, src, dst_off, nw, rows, c->wpr, (hipStream_t)stream);
    if (rc) return fail(c, rc, "mask windows launch failed");
    return lane_follow(c, (hipStream_t)stream);
}

int apse_feature_shape(apse_ctx* c, const char* name, int* chw3) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    auto it = c->t.find(name);
    if (it == c->t.end()) return fail(c, APSE_E_MISSING, std::string("no tensor ") + name);
    chw3[0] = it->second.C; chw3[1] = it->second.H; chw3[2] = it->second.W;
    return APSE_OK;
}

int apse_export_feature(apse_ctx* c, const char* name, float* dst, int batch, void* stream) {
    NEED_READY(c, batch);
    auto it = c->t.find(name);
    if (it == c->t.end()) return fail(c, APSE_E_MISSING, std::string("no tensor ") + name);
    const Tens& t = it->second;
    int rc = lane_join(c, (hipStream_t)stream);
    if (rc) return rc;
    rc = apse_k_nhwc_to_nchw(t.p, dst, batch, t.H * t.W, t.C, t.st, (hipStream_t)stream);
    if (rc) return fail(c, rc, "export launch failed");
    return lane_follow(c, (hipStream_t)stream);
}

int apse_roi_features(apse_ctx* c, int image, const float* rois, const uint8_t* masks, int n, int roi_size, float* out, void* stream) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    const apse_config& g = c->cfg;
    if (image < 0 || image >= g.max_batch || n < 0 || roi_size < 1 || roi_size > 32 || (n > 0 && (!rois || !out)))
        return fail(c, APSE_E_INVALID, "bad roi_features arguments");
    if (c->c4) return fail(c, APSE_E_INVALID, "apse_roi_features reads p2: not available under C4 (arch 1)");
    if (n == 0) return APSE_OK;
    hipStream_t s = (hipStream_t)stream;
    const Tens& p2 = c->t["p2"];
    // spatial_scale = feature width / original width (roi_features_generator.py:105; the padded width, like rcnn_tracker.py:165)
    const float scale = (float)p2.W / (float)g.frame_w;
    int rc = lane_join(c, s);          // reads p2 only (written on the caller's stream): nothing for the lane to follow
    if (rc) return rc;
    if (!masks) {
        rc = apse_k_roi_pool(p2.p, p2.st, p2.H, p2.W, rois, nullptr, nullptr, n, roi_size, scale, out, image, 1, s);
        return rc ? fail(c, rc, "roi_pool launch failed") : APSE_OK;
    }
    const size_t need = (size_t)n * p2.H * p2.W;
    if (need > c->rf_mask_floats) {
        HIPCHK(c, hipStreamSynchronize(s));
        if (c->rf_mask) hipFree(c->rf_mask);
        c->rf_mask = nullptr; c->rf_mask_floats = 0;
        if (hipMalloc(reinterpret_cast<void**>(&c->rf_mask), need * sizeof(float)) != hipSuccess) return fail(c, APSE_E_NOMEM, "roi_features scratch");
        c->rf_mask_floats = need;
    }
    rc = apse_k_mask_resize(masks, n, g.frame_h, g.frame_w, p2.H, p2.W, c->rf_mask, s);
    if (rc) return fail(c, rc, "mask resize launch failed");
    rc = apse_k_roi_align_masked(p2.p, p2.st, p2.H, p2.W, image, rois, c->rf_mask, n, roi_size, 4, scale, out, s);
    return rc ? fail(c, rc, "masked roi_align launch failed") : APSE_OK;
}

int apse_set_crop_features(apse_ctx* c, int on) {
    if (!c) return fail(nullptr, APSE_E_INVALID, "null context");
    if (on && c->c4) return fail(c, APSE_E_INVALID, "crop features read p2 (256 channels): not available under C4 (arch 1)");
    c->crop_features = on != 0;
    return APSE_OK;
}

int apse_roi_features_windows(apse_ctx* c, int image, const float* rois, const apse_mots_window* windows, int n, int roi_size,
                              float* out, void* stream) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    const apse_config& g = c->cfg;
    if (image < 0 || image >= g.max_batch || n < 0 || roi_size < 1 || roi_size > 32 || (n > 0 && (!rois || !out || !windows)))
        return fail(c, APSE_E_INVALID, "bad roi_features_windows arguments");
    if (c->c4) return fail(c, APSE_E_INVALID, "apse_roi_features_windows reads p2: not available under C4 (arch 1)");
    if (n == 0) return APSE_OK;
    hipStream_t s = (hipStream_t)stream;
    const Tens& p2 = c->t["p2"];
    const float scale = (float)p2.W / (float)g.frame_w;      // as apse_roi_features
    int rc = lane_join(c, s);          // reads p2 only (written on the caller's stream): nothing for the lane to follow
    if (rc) return rc;
    rc = apse_k_roi_align_windows(p2.p, p2.st, p2.H, p2.W, rois, nullptr, image, nullptr, n, windows, nullptr, nullptr, nullptr, 0,
                                  g.frame_h, g.frame_w, roi_size, 4, scale, out, 1, s);
    return rc ? fail(c, rc, "masked roi_align (windows) launch failed") : APSE_OK;
}

// ROIAlign R x R of n caller-given boxes over p2..p5 of one image: apse_mask_roi_features (R = 14) and apse_box_roi_features (R = 7)
static int pyramid_roi_features(apse_ctx* c, int image, const float* rois, int n, int R, float* out, void* stream, const char* who) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    const apse_config& g = c->cfg;
    if (image < 0 || image >= g.max_batch || n < 0 || n > (1 << 20) || (n > 0 && (!rois || !out)))
        return fail(c, APSE_E_INVALID, std::string("bad ") + who + " arguments (image inside the batch, 0 <= n <= 2^20)");
    if (c->c4) return fail(c, APSE_E_INVALID, std::string("apse_") + who + " pools p2..p5: not available under C4 (arch 1)");
    if (n == 0) return APSE_OK;
    hipStream_t s = (hipStream_t)stream;
    if ((size_t)n + 1 > c->mrf_cap) {
        HIPCHK(c, hipStreamSynchronize(s));
        if (c->mrf_idx) hipFree(c->mrf_idx);
        c->mrf_idx = nullptr; c->mrf_cap = 0;
        if (hipMalloc(reinterpret_cast<void**>(&c->mrf_idx), ((size_t)n + 1) * sizeof(int)) != hipSuccess) return fail(c, APSE_E_NOMEM, "mask_roi_features scratch");
        c->mrf_cap = (size_t)n + 1;
    }
    // the mask branch's own launch (apse_mask_tail) on a list that lives in `image`: the maps are offset to that image, every RoI
    // carries image index 0 and the live count is n.  The kernel strides its blocks over the RoIs, so n has no launch bound.
    FpnMaps fm = c->fm;
    for (int l = 0; l < 4; ++l)
        fm.p[l] = reinterpret_cast<const char*>(fm.p[l]) + (size_t)image * fm.H[l] * fm.W[l] * 256 * (fm.st ? 2 : 4);
    int rc = lane_join(c, s);          // reads p2..p5 only (written on the caller's stream): nothing for the lane to follow
    if (rc) return rc;
    rc = apse_k_mask_roi_index(c->mrf_idx, n, s);
    if (rc) return fail(c, rc, "mask_roi_features index launch failed");
    rc = apse_k_roi_align(&fm, rois, c->mrf_idx, nullptr, c->mrf_idx + n, 0, n, R, out, 0, s);
    return rc ? fail(c, rc, R == 14 ? "roi_align(14) launch failed" : "roi_align(7) launch failed") : APSE_OK;
}

int apse_mask_roi_features(apse_ctx* c, int image, const float* rois, int n, float* out, void* stream) {
    return pyramid_roi_features(c, image, rois, n, 14, out, stream, "mask_roi_features");
}

int apse_box_roi_features(apse_ctx* c, int image, const float* rois, int n, float* out, void* stream) {
    return pyramid_roi_features(c, image, rois, n, 7, out, stream, "box_roi_features");
}

int apse_proposals(apse_ctx* c, int image, float* boxes, int* count, void* stream) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    const apse_config& g = c->cfg;
    if (image < 0 || image >= g.max_batch || !boxes || !count)
        return fail(c, APSE_E_INVALID, "bad proposals arguments (image inside the batch, boxes and count not NULL)");
    hipStream_t s = (hipStream_t)stream;
    int rc = lane_join(c, s);          // the selection of apse_rpn runs on the tail lane
    if (rc) return rc;
    const int* propcnt = reinterpret_cast<const int*>(c->res + c->lay.prop_count);
    HIPCHK(c, hipMemcpyAsync(boxes, c->props + (size_t)image * g.rpn_post_topk * 4, (size_t)g.rpn_post_topk * 4 * sizeof(float),
                             hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(count, propcnt + image, sizeof(int), hipMemcpyDeviceToDevice, s));
    return lane_follow(c, s);
}

int apse_rpn_patches(apse_ctx* c, int image, const int* anchor_idx, int S, float* x, int* slots, float* anchor_boxes, int* levels,
                     void* stream) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    const apse_config& g = c->cfg;
    if (c->c4) return fail(c, APSE_E_INVALID, "apse_rpn_patches reads p2..p6: not available under C4 (arch 1)");
    if (image < 0 || image >= g.max_batch || S < 0 || S > (1 << 20) || (S > 0 && (!anchor_idx || !x || !slots || !anchor_boxes || !levels)))
        return fail(c, APSE_E_INVALID, "bad apse_rpn_patches arguments (image inside the batch, 0 <= S <= 2^20, no NULL pointer)");
    RpnAnchorGrid grid;
    RpnGatherMaps maps;
    int off = 0;
    for (int l = 0; l < 5; ++l) {
        char pn[8];
        snprintf(pn, sizeof pn, "p%d", l + 2);
        const Tens& t = c->t[pn];
        const RpnLevel& lv = c->rl_host.lv[l];
        if (t.st != 0 || !t.p) return fail(c, APSE_E_INVALID, "apse_rpn_patches needs a context that stores f32 maps (compute_dtype 0)");
        if (t.H != lv.H || t.W != lv.W || t.C != 256) return fail(c, APSE_E_STATE, "apse_rpn_patches: FPN maps and RPN levels disagree");
        maps.p[l] = t.p + (size_t)image * t.H * t.W * 256;
        grid.H[l] = lv.H; grid.W[l] = lv.W; grid.stride[l] = lv.stride; grid.off[l] = off;
        off += lv.n;
        memcpy(grid.base[l], lv.base, sizeof lv.base);
    }
    grid.off[5] = off;
    if (S == 0) return APSE_OK;
    hipStream_t s = (hipStream_t)stream;
    int rc = lane_join(c, s);          // reads p2..p6 only (written on the caller's stream): nothing for the lane to follow
    if (rc) return rc;
    rc = apse_k_rpn_gather(&grid, &maps, anchor_idx, S, x, slots, anchor_boxes, levels, s);
    return rc ? fail(c, rc, "apse_rpn_patches: gather launch failed") : APSE_OK;
}

// ---- training-time proposals and the RPN-head refresh (include/apse_hip.h "Training-time proposals")
static int need_fpn_f32(apse_ctx* c, const char* who) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "weights not finalized");
    if (c->c4) return fail(c, APSE_E_INVALID, std::string(who) + " works on the five FPN levels: not available under C4 (arch 1)");
    if (c->cfg.compute_dtype != 0) return fail(c, APSE_E_INVALID, std::string(who) + " needs an f32 context (compute_dtype 0)");
    return APSE_OK;
}

static size_t train_ws_dec_offset(int batch) { return (apse_rpn_train_scratch_bytes(batch) + 15) & ~(size_t)15; }

size_t apse_rpn_train_proposals_workspace_bytes(int batch, int pre_topk) {
    if (batch < 1 || batch > 64 || pre_topk < 1 || pre_topk > APSE_RPN_TRAIN_MAX_PRE_TOPK) return 0;
    // selection scratch, dec_boxes / dec_scores / dec_valid [batch][5 * pre_topk], entry [batch][APSE_RPN_TRAIN_MAX_POST_TOPK]
    return train_ws_dec_offset(batch) + (size_t)batch * 5 * pre_topk * 24 + (size_t)batch * APSE_RPN_TRAIN_MAX_POST_TOPK * 4;
}

int apse_rpn_train_proposals(apse_ctx* c, int batch, int pre_topk, int post_topk, float* boxes, float* scores, int* count, void* ws,
                             size_t ws_bytes, void* stream) {
    int rc = need_fpn_f32(c, "apse_rpn_train_proposals");
    if (rc) return rc;
    if (batch < 1 || batch > c->cfg.max_batch) return fail(c, APSE_E_INVALID, "apse_rpn_train_proposals: batch out of range");
    if (pre_topk < 1 || pre_topk > APSE_RPN_TRAIN_MAX_PRE_TOPK)
        return fail(c, APSE_E_INVALID, "apse_rpn_train_proposals: pre_topk outside 1 .. APSE_RPN_TRAIN_MAX_PRE_TOPK (2048)");
    if (post_topk < 1 || post_topk > APSE_RPN_TRAIN_MAX_POST_TOPK)
        return fail(c, APSE_E_INVALID, "apse_rpn_train_proposals: post_topk outside 1 .. APSE_RPN_TRAIN_MAX_POST_TOPK (2048)");
    if (!boxes || !scores || !count || !ws) return fail(c, APSE_E_INVALID, "apse_rpn_train_proposals: null pointer");
    if (((uintptr_t)ws & 15) || ws_bytes < apse_rpn_train_proposals_workspace_bytes(batch, pre_topk))
        return fail(c, APSE_E_INVALID, "apse_rpn_train_proposals: workspace too small or not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const apse_config& g = c->cfg;
    // the convolutions rewrite the RPN maps that the lane's selection of the last forward may still read
    if ((rc = lane_join(c, s))) return rc;
    if ((rc = run_plan(c, c->rpnhead, batch, s))) return rc;
    RpnLevels L = c->rl_host;
    L.pre_topk = pre_topk;
    for (int l = 0; l < 5; ++l) L.lv[l].k = L.lv[l].n < pre_topk ? L.lv[l].n : pre_topk;
    char* p = reinterpret_cast<char*>(ws) + train_ws_dec_offset(batch);
    float* dec_boxes = reinterpret_cast<float*>(p); p += (size_t)batch * 5 * pre_topk * 16;
    float* dec_scores = reinterpret_cast<float*>(p); p += (size_t)batch * 5 * pre_topk * 4;
    int* dec_valid = reinterpret_cast<int*>(p); p += (size_t)batch * 5 * pre_topk * 4;
    int* entry = reinterpret_cast<int*>(p);
    rc = apse_k_rpn_train_select(&L, post_topk, (float)g.image_h, (float)g.image_w, (float)log(1000.0 / 16.0), g.rpn_nms, 31, nullptr,
                                 dec_boxes, dec_scores, dec_valid, ws, boxes, scores, entry, count, batch, s);
    if (rc) return fail(c, rc, "apse_rpn_train_proposals: selection launch failed");
    return lane_follow(c, s);          // the lane's next selection follows the RPN maps written here
}

int apse_set_rpn_head(apse_ctx* c, const float* conv_w, const float* conv_b, const float* obj_w, const float* obj_b,
                      const float* delta_w, const float* delta_b, void* stream) {
    int rc = need_fpn_f32(c, "apse_set_rpn_head");
    if (rc) return rc;
    if (!conv_w || !conv_b || !obj_w || !obj_b || !delta_w || !delta_b) return fail(c, APSE_E_INVALID, "apse_set_rpn_head: null pointer");
    // the plan's RPN steps: five 3 x 3 convolutions 256 -> 256 (one per level, each with its own copy of the filters) and the
    // fused 1 x 1 head of 3 + 12 rows
    if (c->rpnhead.size() != 6) return fail(c, APSE_E_STATE, "apse_set_rpn_head: unexpected RPN plan");
    for (int i = 0; i < 6; ++i) {
        const ConvParams& q = c->rpnhead[i].c.p;
        const bool ok = c->rpnhead[i].kind == S_CONV && q.w && !q.w16 && q.bias && q.cin_log2 == 8 &&
                        (i < 5 ? (q.KH == 3 && q.KW == 3 && q.Cout == 256 && q.KWCp == 768) : (q.KH == 1 && q.KW == 1 && q.Cout == 15 && q.KWCp == 256));
        if (!ok) return fail(c, APSE_E_STATE, "apse_set_rpn_head: unexpected RPN plan");
    }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = lane_join(c, s))) return rc;
    for (int i = 0; i < 5 && !rc; ++i) {
        const ConvParams& q = c->rpnhead[i].c.p;
        rc = apse_k_pack_oihw(conv_w, 256, 256, 3, 3, 256, q.KWCp, 0, const_cast<float*>(q.w), s);
        if (!rc && q.wu) rc = apse_k_winograd_filters(conv_w, 256, 256, const_cast<float*>(q.wu), s);
        if (!rc && hipMemcpyAsync(const_cast<float*>(q.bias), conv_b, 256 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = APSE_E_HIP;
    }
    const ConvParams& h = c->rpnhead[5].c.p;
    float* hw = const_cast<float*>(h.w);
    float* hb = const_cast<float*>(h.bias);
    if (!rc) rc = apse_k_pack_oihw(obj_w, 3, 256, 1, 1, 256, h.KWCp, 0, hw, s);
    if (!rc) rc = apse_k_pack_oihw(delta_w, 12, 256, 1, 1, 256, h.KWCp, 3, hw, s);
    if (!rc && hipMemcpyAsync(hb, obj_b, 3 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = APSE_E_HIP;
    if (!rc && hipMemcpyAsync(hb + 3, delta_b, 12 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = APSE_E_HIP;
    return rc ? fail(c, rc, "apse_set_rpn_head: launch failed") : APSE_OK;
}

int apse_debug_tensor(apse_ctx* c, const char* name, void* dst, size_t max_bytes, size_t* bytes, void* stream) {
    if (!c || !c->finalized) return fail(c, APSE_E_STATE, "not finalized");
    const apse_config& g = c->cfg;
    const void* src = nullptr;
    size_t n = 0;
    const std::string nm = name;
    const int B = g.max_batch;
    if (nm == "proposals") { src = c->props; n = (size_t)B * g.rpn_post_topk * 16; }
    else if (nm == "proposal_scores") { src = c->prop_scores; n = (size_t)B * g.rpn_post_topk * 4; }
    else if (nm == "proposal_entry") { src = c->prop_entry; n = (size_t)B * g.rpn_post_topk * 4; }
    else if (nm == "rpn_decoded") { src = c->dec_boxes; n = (size_t)B * (c->c4 ? 1 : 5) * g.rpn_pre_topk * 16; }
    else if (nm == "rpn_decoded_scores") { src = c->dec_scores; n = (size_t)B * (c->c4 ? 1 : 5) * g.rpn_pre_topk * 4; }
    else if (nm == "rpn_decoded_valid") { src = c->dec_valid; n = (size_t)B * (c->c4 ? 1 : 5) * g.rpn_pre_topk * 4; }
    else if (nm == "box_probs") { src = c->probs; n = (size_t)B * g.rpn_post_topk * (g.num_classes + 1) * 4; }
    else if (nm == "cand_boxes") { src = c->cand_boxes; n = (size_t)B * g.rpn_post_topk * g.num_classes * 16; }
    else if (nm == "det_boxes") { src = c->det_boxes; n = (size_t)B * g.dets_per_image * 16; }
    else if (nm == "det_scores") { src = c->det_scores; n = (size_t)B * g.dets_per_image * 4; }
    else if (nm == "det_entry") { src = c->det_entry; n = (size_t)B * g.dets_per_image * 4; }
    else if (nm == "det_count") { src = c->det_cnt; n = (size_t)B * 4; }
    else if (nm == "embedding_raw") { src = c->emb_raw; n = (size_t)B * g.dets_per_image * g.embed_dim * 4; }
    else {
        auto it = c->t.find(nm);
        if (it == c->t.end()) return fail(c, APSE_E_MISSING, "no tensor " + nm);
        const Tens& t = it->second;
        int items = B;
        if (nm == "box_pooled" || nm == "box_fc1" || nm == "box_fc2" || nm == "box_pred" || nm == "box_mean" || nm == "box_res5")
            items = B * g.rpn_post_topk;
        else if (nm.rfind("mask_", 0) == 0 || nm.rfind("assoc_", 0) == 0) items = B * g.dets_per_image;
        src = t.p; n = (size_t)items * t.H * t.W * t.C * (t.st ? 2 : 4);
    }
    if (bytes) *bytes = n;
    if (!dst) return APSE_OK;
    if (n > max_bytes) return fail(c, APSE_E_INVALID, "debug buffer too small for " + nm);
    int rc = lane_join(c, (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return lane_follow(c, (hipStream_t)stream);
}

double apse_flops(apse_ctx* c, int batch, double proposals, double detections) {
    if (!c || !c->finalized) return 0.0;
    double f = 0;
    for (auto& s : c->backbone) if (s.kind == S_CONV || s.kind == S_BNECK) f += s.c.flops_per_item * batch;
    for (auto& s : c->rpnhead) f += s.c.flops_per_item * batch;
    for (auto& s : c->c4_res5box) f += s.c.flops_per_item * proposals;
    for (auto& s : c->boxhead) f += s.c.flops_per_item * proposals;
    for (auto& s : c->maskhead) f += s.c.flops_per_item * detections;
    for (auto& s : c->embedfc) f += s.c.flops_per_item * detections;
    return f;
}

int apse_set_camera(apse_ctx* c, const double* m, const double* dist, int ndist, const uint8_t* lut_host, int do_undistort, int do_gamma) {
    if (!c) return APSE_E_INVALID;
    if (lane_drain(c)) return APSE_E_HIP;
    if (!do_undistort && !do_gamma) { c->cam_on = false; return APSE_OK; }
    if (do_gamma && !lut_host) return fail(c, APSE_E_INVALID, "gamma needs a 256-entry LUT");
    UndistortParams p;
    int rc = fill_camera(p, c->cfg.frame_h, c->cfg.frame_w, m, dist, ndist, do_undistort, do_gamma);
    if (rc) return fail(c, rc, "bad camera parameters (3x3 matrix, <= 14 distortion coefficients, tilt terms zero)");
    hipSetDevice(c->cfg.device);
    if (!c->cam_lut) {
        c->cam_lut = dalloc<LabTables>(c, 1);
        if (!c->cam_lut) return fail(c, APSE_E_NOMEM, "camera Lab tables alloc");
    }
    if (lut_host) {
        // the Lab step is integer arithmetic on these tables (preproc_pixel.h); built here once, on the host, in double
        LabTables host;
        lab_tables_build(&host, lut_host);
        HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, hipMemcpy(c->cam_lut, &host, sizeof(LabTables), hipMemcpyHostToDevice));
    }
    // the remap table depends on the camera only: built here once (f64 rational model per pixel), read per frame -- 4 bytes per
    // pixel: the source position relative to the pixel in 1/32 px (preproc_pixel.h).  A camera that displaces a pixel inside the
    // frame by 1024 px or more does not fit; it keeps the per-pixel model (slower, same bytes).
    c->cam_map_ok = false;
    if (do_undistort) {
        if (!c->cam_map) {
            c->cam_map = dalloc<uint32_t>(c, (size_t)c->cfg.frame_h * c->cfg.frame_w + 4, false);
            if (!c->cam_map) return fail(c, APSE_E_NOMEM, "camera map alloc");
        }
        int* ovf = reinterpret_cast<int*>(reinterpret_cast<uint32_t*>(c->cam_map) + (size_t)c->cfg.frame_h * c->cfg.frame_w);
        HIPCHK(c, hipMemset(ovf, 0, sizeof(int)));
        rc = apse_k_undistort_build_map_compact(&p, c->cam_map, ovf, nullptr);
        if (rc) return fail(c, rc, "camera map launch failed");
        int overflow = 0;
        HIPCHK(c, hipMemcpy(&overflow, ovf, sizeof(int), hipMemcpyDeviceToHost));
        c->cam_map_ok = overflow == 0;
    }
    HIPCHK(c, hipDeviceSynchronize());
    c->cam = p;
    c->cam_on = true;
    return APSE_OK;
}

}  // extern "C"
