"""Helpers for the -m gpu parity tests: thin wrappers over the C ABI (apse_uav_amd._lib)."""
import ctypes as C

import numpy as np
import torch

from apse_uav_amd import _lib


# ---------------------------------------------------------------------------------------------- kernel launchers (roi.hip)
class FpnMaps(C.Structure):
    """Mirror of ``struct FpnMaps``.  apse_uav_amd/csrc/apse_kernels.h is the source of truth: four map pointers (p2..p5, each
    [B][H][W][256]), H[4], W[4], scale[4] and the storage type st (0 f32, 1 bf16, 2 f16).  The launcher takes it by HOST pointer."""
    _fields_ = [("p", C.c_void_p * 4), ("H", C.c_int * 4), ("W", C.c_int * 4), ("scale", C.c_float * 4), ("st", C.c_int)]


_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
# argument tables of the ``apse_k_*`` launchers of csrc/roi.hip, in the order apse_kernels.h declares them (exported from
# libapse_hip.so with default visibility; the last argument is the stream)
ROI_KERNEL_SIG = {
    "apse_k_roi_align": ([C.POINTER(FpnMaps), _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp], _i),
    "apse_k_roi_pool": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _i, _i, _vp], _i),
    "apse_k_roi_align_c4": ([_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp], _i),
    "apse_k_roi_pool_c4": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp], _i),
    "apse_k_mean_cells": ([_vp, _i, _i, _i, _vp, _vp], _i),
    "apse_k_mask_resize": ([_vp, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "apse_k_roi_align_masked": ([_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _f, _vp, _vp], _i),
    "apse_k_l2_normalize": ([_vp, _vp, _i, _vp, _i, _vp], _i),
    "apse_assoc_fc_ok": ([_i, _i], C.c_bool),
    "apse_k_assoc_fc": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp], _i),
    "apse_k_sqdist": ([_vp, _vp, _i, _i, _i, _vp, _vp], _i),
}


def roi_kernels():
    """The loaded library with the roi.hip launchers' argument types set."""
    lib = _lib.load()
    for name, (args, ret) in ROI_KERNEL_SIG.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ret
    return lib


# the 16-bit trunk front and the small kernels beside it (csrc/elementwise.hip, stem_pool16.hip, bottleneck16.hip), as
# apse_kernels.h declares them; the fused kernels end with (stream, event before, event after) -- the events may be null
TRUNK_KERNEL_SIG = {
    "apse_k_round16": ([_vp, _vp, C.c_size_t, _i, _vp], _i),
    "apse_k_subsample2": ([_vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "apse_k_nhwc_to_nchw": ([_vp, _vp, _i, _i, _i, _i, _vp], _i),
    "apse_k_stem_pool16": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "apse_k_bottleneck64_fused16": ([_vp] * 9 + [_i] * 5 + [_vp] * 3, _i),
}


def trunk_kernels():
    """The loaded library with the trunk-front launchers' argument types set."""
    lib = _lib.load()
    for name, (args, ret) in TRUNK_KERNEL_SIG.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ret
    return lib


def pack_filter(w_oihw, scale=None):
    """OIHW filter (CPU tensor) -> (apse_conv_pack_weight's layout [Cout_p128][KH][roundup(KW * cin_p, 32)] as a numpy f32 array,
    cin_p = the input channels padded to a power of two >= 4)."""
    lib = _lib.load()
    Cout, Cin, KH, KW = w_oihw.shape
    cin_p = 4
    while cin_p < Cin:
        cin_p *= 2
    d = _lib.ConvDesc()
    d.Cin, d.Cout, d.KH, d.KW = cin_p, Cout, KH, KW
    packed = np.zeros(lib.apse_conv_packed_elems(C.byref(d)), np.float32)
    w = np.ascontiguousarray(w_oihw.numpy(), np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale.numpy(), np.float32)
    _lib.check(lib.apse_conv_pack_weight(C.byref(d), _lib.ptr(w), Cin, _lib.ptr(sc) if sc is not None else None,
                                         _lib.ptr(packed)), None, "pack")
    return packed, cin_p


def pack_filter16(w_oihw, dtype):
    """``pack_filter`` rounded with torch to ``dtype``, on cuda:0 (the filters of the 16-bit kernels)"""
    return torch.from_numpy(pack_filter(w_oihw)[0]).to(dtype).cuda().contiguous()


def fpn_maps(tensors, dims, st, scales=(0.25, 0.125, 0.0625, 0.03125)):
    F = FpnMaps()
    for k in range(4):
        F.p[k] = tensors[k].data_ptr()
        F.H[k], F.W[k] = dims[k]
        F.scale[k] = scales[k]
    F.st = st
    return F


def to_nhwc(x, cpad=None):
    x = x.permute(0, 2, 3, 1).contiguous()
    if cpad and cpad > x.shape[3]:
        x = torch.nn.functional.pad(x, (0, cpad - x.shape[3]))
    return x.contiguous()


def hip_conv2d(x_nchw, w_oihw, bias=None, stride=1, pad=0, relu=False, residual=None, res_mode=0, cfg=-1, splitk=0,
               scale=None, prec=0, fuse=0, x_st=0, res_st=0, y_st=0):
    """x: CPU NCHW f32; returns CPU NCHW f32 computed by apse_conv2d on cuda:0."""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, Cin, H, W = x_nchw.shape
    Cout, _, KH, KW = w_oihw.shape
    packed, cin_p = pack_filter(w_oihw, scale)
    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.Cin = B, H, W, cin_p
    d.Cout, d.KH, d.KW, d.stride, d.pad = Cout, KH, KW, stride, pad
    d.relu, d.res_mode, d.cfg, d.splitk, d.prec, d.fuse_reduce = int(relu), res_mode, cfg, splitk, prec, fuse
    d.x_st, d.res_st, d.y_st = x_st, res_st, y_st
    tdt = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
    bias_p = torch.zeros(((Cout + 127) // 128) * 128)
    if bias is not None:
        bias_p[:Cout] = bias
    xd = to_nhwc(x_nchw, cin_p).to(dev).to(tdt[x_st]).contiguous()
    wd = torch.from_numpy(packed).to(dev)
    bd = bias_p.to(dev)
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    y = torch.full((B, OH, OW, Cout), float("nan"), device=dev, dtype=tdt[y_st])
    rd = None
    if residual is not None:
        rd = to_nhwc(residual).to(dev).to(tdt[res_st]).contiguous()
    ws = torch.empty((64 * B * OH * OW * Cout + 16,), device=dev)
    rc = lib.apse_conv2d(C.byref(d), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(rd), _lib.ptr(y), _lib.ptr(ws),
                         ws.numel() * 4, _lib.stream_ptr())
    assert rc == 0, "apse_conv2d rc=%d" % rc
    torch.cuda.synchronize()
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def storage16_tolerance(ref, prec):
    """Per-element bound on |kernel - reference rounded to the 16-bit type| for a 16-bit STORED output (test_conv2d_16bit_storage):
    the kernel's f32 result differs from the reference's by summation order only; after the 16-bit store the two agree except
    where that tiny difference straddles a rounding boundary (then by one 16-bit ulp).
    + 4e-6: f32 summation-order noise of a unit-variance sum that cancels to |ref| < 1e-3 [round 4: 7 of 7.1 M outputs of the
    K = 512 case sit at 2.3e-6 from the reference with |ref| = 6e-4; the LDS-DMA kernel and the tiled kernel agree on them bit
    for bit]"""
    ulp = 2.0 ** (-7 if prec == 1 else -10)        # one unit in the last place, relative to the binade's lower edge
    return ulp * ref.abs().clamp_min(1e-3) * 1.01 + 4e-6


# ---------------------------------------------------------------------------------------------- apse_conv2d_ex
# fill of y (in its storage type) and of the workspace in front of a launch: NaNs no kernel produces, compared as integers
CONV_FILL = {0: (torch.int32, 0x7fc5a5a5), 1: (torch.int16, 0x7fc5), 2: (torch.int16, 0x7e5a)}
_TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


class ConvExLayer:
    """The device operands of one layer for apse_conv2d_ex, uploaded once: x (CPU NCHW f32, the capacity in items), the packed
    filter, the bias padded to a multiple of 128 entries (entries from Cout on = ``bias_pad``) and the residual.  ``packed`` /
    ``bias_p`` (device tensors) with ``geom`` = (Cout, KH, KW) replace ``w_oihw`` / ``bias`` for a filter packed elsewhere."""

    def __init__(self, x_nchw, w_oihw=None, bias=None, stride=1, pad=0, relu=False, residual=None, res_mode=0, prec=0, x_st=0,
                 res_st=0, y_st=0, packed=None, bias_p=None, geom=None, bias_pad=0.0):
        dev = torch.device("cuda:0")
        self.Bcap, Cin, self.H, self.W = x_nchw.shape
        if packed is None:
            self.Cout, _, self.KH, self.KW = w_oihw.shape
            pk, self.cin_p = pack_filter(w_oihw)
            self.wd = torch.from_numpy(pk).to(dev)
            bp = torch.full((((self.Cout + 127) // 128) * 128,), float(bias_pad))
            bp[:self.Cout] = 0.0 if bias is None else bias
            self.bd = bp.to(dev)
        else:
            (self.Cout, self.KH, self.KW), self.cin_p, self.wd, self.bd = geom, Cin, packed, bias_p
        self.stride, self.pad, self.relu, self.res_mode = stride, pad, relu, res_mode
        self.prec, self.x_st, self.res_st, self.y_st = prec, x_st, res_st, y_st
        self.OH = (self.H + 2 * pad - self.KH) // stride + 1
        self.OW = (self.W + 2 * pad - self.KW) // stride + 1
        self.xd = to_nhwc(x_nchw, self.cin_p).to(dev).to(_TDT[x_st]).contiguous()
        self.rd = None if residual is None else to_nhwc(residual).to(dev).to(_TDT[res_st]).contiguous()

    def run(self, B, cfg=-1, splitk=0, count=None, hint=0, y_ld=0, deconv=0, fuse=0, extra_rows=256, ws_slabs=None):
        """One launch over the first ``B`` items (the capacity of a counted launch).  Returns (rc, y, ws): y as integers of its
        storage type, [output rows + extra_rows][row stride], ws as int32 -- both filled with CONV_FILL in front of the launch."""
        lib = _lib.load()
        dev = self.xd.device
        d = _lib.ConvDesc()
        d.B, d.H, d.W, d.Cin = B, self.H, self.W, self.cin_p
        d.Cout, d.KH, d.KW, d.stride, d.pad = self.Cout, self.KH, self.KW, self.stride, self.pad
        d.relu, d.res_mode, d.cfg, d.splitk, d.prec, d.fuse_reduce = int(self.relu), self.res_mode, cfg, splitk, self.prec, fuse
        d.x_st, d.res_st, d.y_st = self.x_st, self.res_st, self.y_st
        M = B * self.OH * self.OW
        ld = max(self.Cout // 4, 1) if deconv else max(y_ld, self.Cout)
        ydt, ypat = CONV_FILL[self.y_st]
        y = torch.full(((4 * M if deconv else M) + extra_rows, ld), ypat, dtype=ydt, device=dev)
        slabs = ws_slabs if ws_slabs is not None else max(splitk, 1)
        ws = torch.full((slabs * M * self.Cout + 16,), CONV_FILL[0][1], dtype=torch.int32, device=dev)
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32).to(dev)
        rc = lib.apse_conv2d_ex(C.byref(d), _lib.ptr(self.xd), _lib.ptr(self.wd), _lib.ptr(self.bd), _lib.ptr(self.rd), _lib.ptr(y),
                                _lib.ptr(ws), ws.numel() * 4, _lib.ptr(cnt), hint, y_ld, deconv, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, y, ws

    def values(self, y):
        """y of ``run`` as float64 on the CPU (same shape)."""
        return y.view(_TDT[self.y_st]).double().cpu()


def conv_untouched(t, st=0):
    """True when every element of ``t`` (y or ws of ConvExLayer.run) still holds the fill pattern."""
    return bool((t == CONV_FILL[st][1]).all())


def err_stats(a, b):
    a = a.double()
    b = b.double()
    diff = (a - b).abs()
    scale = b.abs().max().clamp_min(1e-30)
    return dict(max_abs=float(diff.max()), rel_to_max=float(diff.max() / scale), nan=int(torch.isnan(a).sum()))


def _live_bytes(model, res):
    """Every live byte a frame produces: the record of image 0 (boxes, scores, classes, centroids, mass, rects,
    closest-point table, embeddings), the raw embeddings, the mask logits and the bit planes of its mask windows."""
    rec = res.record(0)
    parts = [np.ascontiguousarray(rec[k]).tobytes() for k in
             ("boxes", "scores", "classes", "centroids", "mass", "rects", "closest", "embeddings", "packed_index")]
    inst = model.instances_from(res, 0, want_masks=True)
    for m in inst.pred_masks:
        if m.bits is not None:
            parts.append(m.bits.cpu().numpy().tobytes())
    n = len(rec["scores"])
    logits = model.debug_tensor("mask_logits").cpu().numpy().reshape(-1)[: n * 28 * 28 * 4]
    parts.append(logits.tobytes())
    parts.append(model.debug_tensor("embedding_raw").cpu().numpy().reshape(-1)[: n * 128].tobytes())
    return n, b"".join(parts)


def history_independence(tracker, frame_a, image_hw, rng_seed=0):
    """Frame A after forwards that left 0, 8 and 100 detections in the packed list must give the same BYTES: the
    tile shape / K split of the count-limited GEMMs (mask head, deconv, mask logits, association FC) are plan
    constants, the previous count only sizes their grid (csrc/plan.hip add_conv, csrc/detector.hip run_plan)."""
    pr = tracker.predictor
    model = pr.model
    dev = pr._upload([frame_a])
    rng = np.random.RandomState(rng_seed)
    ih, iw = image_hw
    outs = []
    for prev in (0, 8, 100):
        x0 = rng.uniform(0, iw - 60, prev)
        y0 = rng.uniform(0, ih - 60, prev)
        boxes = np.stack([x0, y0, x0 + rng.uniform(8, 56, prev), y0 + rng.uniform(8, 56, prev)], 1).astype(np.float32)
        given = (boxes.reshape(-1, 4), np.zeros(prev, np.int32), np.array([prev], np.int32))
        model.preprocess_frames(dev)
        model.run(1, given)
        assert model.read(1).total == prev                 # the count the next forward sees as its hint
        model.preprocess_frames(dev)
        model.run(1)
        outs.append(_live_bytes(model, model.read(1)))
    return outs



# ---------------------------------------------------------------------------------------------- detection-set analysis
def _iou_matrix(a, b):
    a, b = a.double(), b.double()
    lt = torch.maximum(a[:, None, :2], b[None, :, :2])
    rb = torch.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    aa = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
    ab = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
    return inter / (aa + ab - inter).clamp(min=1e-12)


def _same_matrix(a, b):
    """IoU, except that two boxes whose four coordinates all agree within 1 px count as the same box (1.0): candidates of one
    stage are at least an anchor stride (4 px) apart, and the IoU of slivers -- proposals clipped to a fraction of a pixel at the
    image border -- is sub-pixel noise (0.41 px against 0.71 px wide: IoU 0.57 with every coordinate within 0.3 px)."""
    u = _iou_matrix(a, b)
    d = (a.double()[:, None, :] - b.double()[None, :, :]).abs().amax(dim=2)
    return torch.where(d <= 1.0, torch.ones_like(u), u)


def hip_box_side(model, b=0):
    """Box-branch view of image ``b`` of the last forward: every (proposal, class) candidate and the kept detections,
    in resized-image pixels -- the HIP counterpart of the oracle's ``post["box_det"]``."""
    g = model._cfg_c
    P, K = g.rpn_post_topk, g.num_classes
    res = model.last_results
    n_prop = int(res.prop_count[b])
    allb = model.debug_tensor("cand_boxes").cpu().view(-1, P, K, 4)[b, :n_prop]
    probs = model.debug_tensor("box_probs").cpu().view(-1, P, K + 1)[b, :n_prop]
    lo, hi = res.image_slice(b)
    return dict(all_boxes=allb, probs=probs, boxes=torch.from_numpy(res.box_resized[lo:hi].copy()),
                scores=torch.from_numpy(res.score[lo:hi].copy()), classes=torch.from_numpy(res.cls[lo:hi].astype(np.int64)))


def oracle_box_side(post):
    d = post["box_det"]
    return dict(all_boxes=d["all_boxes"], probs=d["probs"], boxes=d["boxes"], scores=d["scores"], classes=d["classes"])


def _flat_box_side(side):
    """(proposal, class) candidates of the box branch as flat arrays; live = score above the test threshold is applied later."""
    K = side["probs"].shape[1] - 1
    n = side["probs"].shape[0]
    return dict(cand_boxes=side["all_boxes"].reshape(-1, 4), cand_scores=side["probs"][:, :K].reshape(-1),
                cand_cat=torch.arange(K).repeat(n), cand_src=torch.arange(n).repeat_interleave(K),
                boxes=side["boxes"], scores=side["scores"], cats=side["classes"])


def hip_rpn_side(model, b=0):
    """RPN selection view of image ``b``: the pre-NMS candidates (top-k per level, decoded + clipped) and the proposals kept."""
    g = model._cfg_c
    PRE, POST = g.rpn_pre_topk, g.rpn_post_topk
    res = model.last_results
    P = int(res.prop_count[b])
    dec = model.debug_tensor("rpn_decoded").cpu().view(-1, 5 * PRE, 4)[b]
    sc = model.debug_tensor("rpn_decoded_scores").cpu().view(-1, 5 * PRE)[b]
    ok = model.debug_tensor("rpn_decoded_valid", torch.int32).cpu().view(-1, 5 * PRE)[b] != 0
    lvl = torch.arange(5 * PRE) // PRE
    props = model.debug_tensor("proposals").cpu().view(-1, POST, 4)[b, :P]
    psc = model.debug_tensor("proposal_scores").cpu().view(-1, POST)[b, :P]
    pent = model.debug_tensor("proposal_entry", torch.int32).cpu().view(-1, POST)[b, :P].long()
    return dict(cand_boxes=dec[ok], cand_scores=sc[ok], cand_cat=lvl[ok], boxes=props, scores=psc, cats=pent // PRE)


def oracle_rpn_side(post):
    pr = post["proposals"]
    lv = torch.cat([torch.full((t.numel(),), i, dtype=torch.int64) for i, t in enumerate(pr["topk_scores"])])
    sc = torch.cat(pr["topk_scores"])
    ok = pr["valid"]
    return dict(cand_boxes=pr["decoded"][ok], cand_scores=sc[ok], cand_cat=lv[ok], boxes=pr["boxes"], scores=pr["logits"],
                cats=pr["level"])


def explain_detection_sets(A, B, score_thr=0.5, nms_thr=0.5, match_iou=0.9, rank_limit=None):
    """Box-branch form of ``explain_sets`` (sides from hip_box_side / oracle_box_side); ``rank_limit`` = DETECTIONS_PER_IMAGE
    (the top-100 cut of fast_rcnn_inference_single_image: with a full list an item can fall past it inside the score noise)."""
    # noise sample: every candidate pair with p > 0.02 (scores are compared as logits, where the noise does not depend on p: the
    # floor only drops the thousands of background-certain candidates, whose probabilities sit at the clamp)
    return explain_sets(_flat_box_side(A), _flat_box_side(B), score_thr, nms_thr, rank_limit=rank_limit, match_iou=match_iou, noise_floor=0.02)


def explain_sets(A, B, score_thr, nms_thr, rank_limit=None, match_iou=0.9, noise_floor=None, pre_topk=None):
    """Compares what two runs of one selection stage keep (HIP vs oracle, f32 vs 16-bit, ...).

    A side = dict(cand_boxes [n,4], cand_scores [n], cand_cat [n]  -- every candidate the stage ranks (category = class
    for the box branch, pyramid level for the RPN); boxes / scores / cats -- what it keeps after the score threshold
    (``score_thr``, None for the RPN), per-category NMS at ``nms_thr`` and the top-``rank_limit`` cut).
    Returns (report, unexplained).  Kept items are paired by category and IoU >= match_iou.  The numeric noise between
    the runs is MEASURED on the candidates both hold (scores above ``noise_floor`` when given): eps_score = max
    |score_A - score_B| and eps_iou = max |IoU_A(i, j) - IoU_B(i, j)| over candidate pairs with IoU in (0.3, 0.8) --
    in both cases taken over the OTHER candidates: a disputed one does not vouch for itself.  An item only one run
    keeps is *explained* when the other run holds the same candidate and either
      (score) its score there is on the other side of score_thr, within eps_score of the kept one, or
      (nms)   it was suppressed there by a kept item with IoU u > nms_thr while the same pair has IoU <= nms_thr in the
              run that keeps it, and the two IoUs differ by at most eps_iou, or
      (rank)  it falls past the top-``rank_limit`` cut there with a score within eps_score of that run's last kept one, or
      (swap)  it was suppressed there by an item q only that run keeps, and the two runs ORDER p and q differently (greedy NMS
              keeps the better-scored of an overlapping pair) with both score changes within eps_score, or
      (top-k) the other run does not even rank it: its category's candidate list is full (``pre_topk``) and ends within
              eps_score of this item's score (the per-level pre-NMS cut of the RPN).
    Scores are compared in the space the noise is uniform in: the RPN's objectness values are logits already; the box branch's
    are softmax probabilities, whose response to the same logit noise is p (1 - p) -- 0.25 at the 0.5 threshold, 0.09 at 0.9 --
    so they are compared as log(p / (1 - p)) (``score_thr`` given).  Items are paired with ``_same_matrix``.
    "Within eps" means within 1.5 x the 99.9th PERCENTILE of the deviations measured on the other candidates (round 3; rounds
    1-2 used 1.5 x their MAXIMUM, which for bf16 at 4K was a band of 0.35 logits -- wide enough to wave through a real 0.1-0.3
    logit kernel error; 1.5 x the 99.9th percentile of the same ~2 700 samples is ~0.22, and every case reports its z).  Every disputed item also reports where it sits
    in that noise: ``sigma_of_the_others`` (RMS deviation) and ``z`` = its own deviation / sigma.
    Everything else -- including "the other run has no such candidate" -- is returned in ``unexplained``."""
    BAND = 1.5          # x the 99.9th percentile: with ~3 000 samples that percentile is about the third-largest value, itself a noisy
    Q = 0.999           # estimate of the tail (round 3 saw a 5.8-sigma IoU deviation at 1.27 x it among 1 186 same-size pairs)

    def qband(v):
        v = torch.as_tensor(v, dtype=torch.double).reshape(-1)
        return float(torch.quantile(v, Q)) if v.numel() else 0.0

    def rms(v):
        v = torch.as_tensor(v, dtype=torch.double).reshape(-1)
        return float(torch.sqrt((v * v).mean())) if v.numel() else 0.0
    if score_thr is not None:
        def sp(v):
            return torch.logit(torch.as_tensor(v, dtype=torch.double).clamp(1e-7, 1 - 1e-7))
    else:
        def sp(v):
            return torch.as_tensor(v, dtype=torch.double)

    def spf(v):
        return float(sp(v))
    rep = dict(nA=int(A["boxes"].shape[0]), nB=int(B["boxes"].shape[0]))
    fa = A["cand_scores"] > noise_floor if noise_floor is not None else torch.ones_like(A["cand_scores"], dtype=torch.bool)
    ca = (A["cand_boxes"][fa], A["cand_scores"][fa], A["cand_cat"][fa])
    if ca[0].shape[0] > 3000:                       # noise sample: the best-scored candidates are enough
        top = torch.argsort(ca[1], descending=True)[:3000]
        ca = (ca[0][top], ca[1][top], ca[2][top])
    cb = (B["cand_boxes"], B["cand_scores"], B["cand_cat"])
    pair_box = torch.zeros((0, 4))
    pair_ds = torch.zeros((0,))
    sub_box = torch.zeros((0, 4))
    du = torch.zeros((0, 0), dtype=torch.double)
    du_band = torch.zeros((0, 0), dtype=torch.bool)
    eps_s = eps_box = eps_iou = 0.0
    n_pairs = 0
    if ca[0].shape[0] and cb[0].shape[0]:
        best = torch.zeros(ca[0].shape[0], dtype=torch.double)
        arg = torch.zeros(ca[0].shape[0], dtype=torch.long)
        for cat in ca[2].unique().tolist():          # per category: keeps the IoU matrices small
            ia_ = (ca[2] == cat).nonzero()[:, 0]
            ib_ = (cb[2] == cat).nonzero()[:, 0]
            if not ib_.numel():
                continue
            for lo in range(0, ia_.numel(), 1024):
                blk = ia_[lo:lo + 1024]
                m, a = _iou_matrix(ca[0][blk], cb[0][ib_]).max(dim=1)        # noise sample: plain IoU (slivers clipped at the border coincide within 1 px although they are different anchors)
                best[blk], arg[blk] = m, ib_[a]
        ok = best >= match_iou
        n_pairs = int(ok.sum())
        if n_pairs:
            ia = ok.nonzero()[:, 0]
            ib = arg[ia]
            pair_box, pair_ds = ca[0][ia], (sp(ca[1][ia]) - sp(cb[1][ib])).abs()
            eps_s = float(pair_ds.max())
            eps_box = float((ca[0][ia] - cb[0][ib]).abs().max())
            ia, ib = ia[:400], ib[:400]
            sub_box = ca[0][ia]
            ua, ub = _iou_matrix(sub_box, sub_box), _iou_matrix(cb[0][ib], cb[0][ib])
            band = (ua > 0.3) & (ua < 0.8)
            du = (ua - ub).abs() * band
            du_band = band
            if int(band.sum()):
                eps_iou = float(du.max())
    rep.update(cand_pairs=n_pairs, eps_score=eps_s, eps_box_px=eps_box, eps_iou=eps_iou,
               score_noise_q999=qband(pair_ds), score_noise_rms=rms(pair_ds), iou_noise_q999=qband(du[du_band]) if du_band.numel() else 0.0,
               score_noise_largest=[round(float(v), 5) for v in torch.sort(pair_ds, descending=True).values[:8]],
               score_space="logit of the probability" if score_thr is not None else "as given (logits)")
    # pair the kept items
    pairs, onlyA, onlyB = [], [], list(range(rep["nB"]))
    if rep["nA"] and rep["nB"]:
        for i in range(rep["nA"]):
            sel = (B["cats"] == A["cats"][i]).nonzero()[:, 0]
            j = -1
            if sel.numel():
                u = _same_matrix(A["boxes"][i][None], B["boxes"][sel])[0]
                for k in torch.argsort(u, descending=True).tolist():
                    if float(u[k]) < match_iou:
                        break
                    if int(sel[k]) in onlyB:
                        j = int(sel[k])
                        break
            if j >= 0:
                pairs.append((i, j))
                onlyB.remove(j)
            else:
                onlyA.append(i)
    else:
        onlyA = list(range(rep["nA"]))
    rep["matched"] = len(pairs)
    rep["matched_box_max_abs"] = max([float((A["boxes"][i] - B["boxes"][j]).abs().max()) for i, j in pairs] or [0.0])
    rep["matched_score_max_abs"] = max([abs(float(A["scores"][i] - B["scores"][j])) for i, j in pairs] or [0.0])
    rep["only"] = []
    unexplained = []

    def explain(X, Y, i, who, pair_of):
        box, cat, s = X["boxes"][i], int(X["cats"][i]), float(X["scores"][i])
        item = dict(side=who, index=i, score=s, cat=cat, box=[round(float(v), 2) for v in box])
        yb, ys, yc = Y["cand_boxes"], Y["cand_scores"], Y["cand_cat"]
        sel = (yc == cat).nonzero()[:, 0]
        uu = _same_matrix(box[None], yb[sel])[0] if sel.numel() else torch.zeros(0, dtype=torch.double)
        far = _iou_matrix(box[None], pair_box)[0] < 0.5 if pair_box.shape[0] else torch.zeros(0, dtype=torch.bool)
        eps_here = qband(pair_ds[far]) if int(far.sum()) else 0.0       # score noise of the other candidates: 99.9th percentile
        sig_here = rms(pair_ds[far]) if int(far.sum()) else 0.0
        if sel.numel() and float(uu.max()) < match_iou:
            # noisy runs (bf16 moves small boxes by several pixels): the same candidate may fall below match_iou.  Accept one
            # that still overlaps by >= 0.7 AND carries the same score within the measured score noise
            near = (uu >= 0.7) & ((sp(ys[sel]) - spf(s)).abs() <= max(BAND * eps_here, 1e-6))
            if bool(near.any()):
                k2 = int(torch.where(near, uu, torch.zeros_like(uu)).argmax())
                c2 = sel[k2]
                kk = (Y["cats"] == cat).nonzero()[:, 0]
                if kk.numel() and float(_iou_matrix(yb[c2][None], Y["boxes"][kk])[0].max()) >= 0.99:
                    item.update(why="kept in both runs: the same candidate (score within the noise), its box moved to IoU %.3f under the box noise"
                                    % float(uu[k2]), other_score=float(ys[c2]))
                    return item, True
        if not sel.numel() or float(uu.max()) < match_iou:
            item["why"] = "no counterpart candidate in the other run"
            item["best_iou_in_other"] = round(float(uu.max()), 4) if sel.numel() else 0.0
            if pre_topk is not None and int(sel.numel()) >= pre_topk:
                cut = float(ys[sel].min())                       # the other run's list of this category is full and ends here
                item.update(why="pre-NMS top-k cut", other_cut_score=cut, margin_to_cut=round(s - cut, 6),
                            eps_score_of_the_others=round(eps_here, 6))
                return item, (spf(s) - spf(cut)) <= max(BAND * eps_here, 1e-6)
            return item, False
        c = sel[int(uu.argmax())]
        sy = float(ys[c])
        dsy = abs(spf(s) - spf(sy))                          # in the comparison space (logits)
        item.update(other_score=sy, score_diff=round(dsy, 6), eps_score_of_the_others=round(eps_here, 6),
                    sigma_of_the_others=round(sig_here, 6), z=round(dsy / sig_here, 2) if sig_here > 0 else None)
        if score_thr is not None:
            item.update(score_margin_to_thr=round(s - score_thr, 6), other_margin_to_thr=round(sy - score_thr, 6))
            if sy <= score_thr:
                item["why"] = "score threshold"
                return item, dsy <= max(BAND * eps_here, 1e-6)
        # a live candidate in Y that Y does not keep: suppressed by a BETTER-scored kept item of its category (greedy NMS), or
        # past the rank cut
        ksel = ((Y["cats"] == cat) & (Y["scores"] >= sy)).nonzero()[:, 0]
        u_y, j = 0.0, -1
        if ksel.numel():
            uy = _iou_matrix(yb[c][None], Y["boxes"][ksel])[0]
            j = int(ksel[int(uy.argmax())])
            u_y = float(uy.max())
        if u_y <= nms_thr:
            # no better-scored suppressor: look for a kept item that overlaps it and scores (slightly) LOWER in Y's own ranking
            ksel2 = (Y["cats"] == cat).nonzero()[:, 0]
            if ksel2.numel():
                uy2 = _iou_matrix(yb[c][None], Y["boxes"][ksel2])[0]
                if float(uy2.max()) > nms_thr:
                    j = int(ksel2[int(uy2.argmax())])
                    u_y = float(uy2.max())
        if u_y > nms_thr:
            jx = pair_of.get(j)
            item.update(why="nms", iou_in_other=round(u_y, 6), nms_margin_other=round(u_y - nms_thr, 6))
            if jx is None:
                # the suppressor q is itself an item only the other run keeps.  Either the two runs order p and q differently
                # (near-tied scores: greedy NMS keeps whichever ranks first) ...
                qb = Y["boxes"][j]
                xsel = (X["cand_cat"] == cat).nonzero()[:, 0]
                uq = _same_matrix(qb[None], X["cand_boxes"][xsel])[0] if xsel.numel() else torch.zeros(0, dtype=torch.double)
                if xsel.numel() and float(uq.max()) >= match_iou:
                    sq_x = float(X["cand_scores"][xsel[int(uq.argmax())]])
                    sq_y = float(Y["scores"][j])
                    item.update(q_score_here=sq_x, q_score_other=sq_y)
                    if sq_x <= s and sq_y >= sy and dsy <= max(BAND * eps_here, 1e-6) and abs(spf(sq_x) - spf(sq_y)) <= max(BAND * eps_here, 1e-6):
                        item["why"] = "order swap: the runs rank this item and its overlapping rival differently, both score changes inside the noise"
                        return item, True
                # ... or q's presence there is a disagreement of its own: resolved below once every direct case is known
                item["suppressor_only_in_other"] = j
                return item, False
            u_x = float(_iou_matrix(box[None], X["boxes"][jx][None])[0, 0])
            other = _iou_matrix(box[None], sub_box)[0] < match_iou if sub_box.shape[0] else torch.zeros(0, dtype=torch.bool)
            sub = du[other][:, other][du_band[other][:, other]] if int(other.sum()) else torch.zeros(0)
            # IoU noise grows as boxes shrink (the same coordinate noise on a shorter side): where the sample allows (>= 50 pairs),
            # take it from boxes of comparable size only (area within a factor of two of the disputed box's)
            if int(other.sum()):
                ar = (sub_box[:, 2] - sub_box[:, 0]) * (sub_box[:, 3] - sub_box[:, 1])
                a0 = float((box[2] - box[0]) * (box[3] - box[1]))
                near = other & (ar >= 0.5 * a0) & (ar <= 2.0 * a0)
                sub2 = du[near][:, near][du_band[near][:, near]] if int(near.sum()) else torch.zeros(0)
                if sub2.numel() >= 50:
                    sub = sub2
                    item["iou_noise_sample"] = "pairs of boxes with 0.5x..2x this box's area: %d" % int(sub2.numel())
            eps_u = qband(sub)                                                          # IoU noise of the pairs not involving it: 99.9th percentile
            item.update(sigma_iou_of_the_others=round(rms(sub), 6), z_iou=round((u_y - u_x) / rms(sub), 2) if rms(sub) > 0 else None)
            item.update(iou_here=round(u_x, 6), nms_margin_here=round(u_x - nms_thr, 6), iou_diff=round(u_y - u_x, 6),
                        eps_iou_of_the_others=round(eps_u, 6))
            return item, (u_x <= nms_thr and (u_y - u_x) <= max(BAND * eps_u, 1e-6))
        if rank_limit is not None and Y["boxes"].shape[0] >= rank_limit:
            last = float(Y["scores"].min())
            item.update(why="rank cut", other_last_kept_score=last, margin_to_last=round(sy - last, 6))
            return item, (sy <= last + 1e-12 or abs(spf(sy) - spf(last)) <= max(BAND * eps_here, 1e-6)) and dsy <= max(BAND * eps_here, 1e-6)
        item["why"] = "live in the other run, not kept, no suppressor found"
        return item, False

    a_of_b = {j: i for i, j in pairs}
    b_of_a = {i: j for i, j in pairs}
    for i in onlyA:
        item, good = explain(A, B, i, "A", a_of_b)
        item["explained"] = bool(good)
        rep["only"].append(item)
    for j in onlyB:
        item, good = explain(B, A, j, "B", b_of_a)
        item["explained"] = bool(good)
        rep["only"].append(item)
    # NMS cascades: X keeps p, Y suppressed p with q, and q is something only Y keeps.  Had q been suppressed in Y too (as it
    # is in X), p would have survived there: p's disagreement is a consequence of q's, so it stands or falls with it.
    by_key = {(o["side"], o["index"]): o for o in rep["only"]}
    changed = True
    while changed:
        changed = False
        for o in rep["only"]:
            if o["explained"] or "suppressor_only_in_other" not in o:
                continue
            q = by_key.get(("B" if o["side"] == "A" else "A", o["suppressor_only_in_other"]))
            if q is not None and q["explained"]:
                o["explained"] = True
                o["why"] = "nms cascade: suppressed in the other run by an item only that run keeps (whose presence is explained)"
                changed = True
    unexplained = [o for o in rep["only"] if not o["explained"]]
    rep["n_only"] = len(rep["only"])
    rep["n_direct"] = sum(1 for o in rep["only"] if o["explained"] and not o["why"].startswith("nms cascade"))
    rep["n_cascade"] = sum(1 for o in rep["only"] if o["explained"] and o["why"].startswith("nms cascade"))
    return rep, unexplained


def explain_frame(hip_model, post, dump=None, b=0):
    """Both selection stages of one frame, HIP (side A) vs an oracle run (side B).  A box-branch item whose only problem
    is "no counterpart candidate" is traced to its PROPOSAL: if the other run lacks that proposal and the RPN-stage
    analysis explains the proposal's absence (NMS at 0.7 / rank cut inside the measured noise), the item is explained too."""
    hb, ob = hip_box_side(hip_model, b), oracle_box_side(post)
    rep_box, un_box = explain_detection_sets(hb, ob, score_thr=float(hip_model._cfg_c.score_thresh), nms_thr=float(hip_model._cfg_c.box_nms),
                                             rank_limit=int(hip_model._cfg_c.dets_per_image))
    hr, orr = hip_rpn_side(hip_model, b), oracle_rpn_side(post)
    post_topk = int(hip_model._cfg_c.rpn_post_topk)
    rep_rpn, un_rpn = explain_sets(hr, orr, None, float(hip_model._cfg_c.rpn_nms), rank_limit=post_topk,
                                   pre_topk=int(hip_model._cfg_c.rpn_pre_topk))
    res = hip_model.last_results
    lo, hi = res.image_slice(b)
    roi = {"A": torch.from_numpy(res.roi[lo:hi].astype(np.int64)), "B": post["box_det"]["roi_index"]}
    props = {"A": hr["boxes"], "B": orr["boxes"]}
    explained_rpn = {(o["side"], o["index"]) for o in rep_rpn["only"] if o["explained"]}
    still = []

    def fpn_level(b):          # detectron2 assign_boxes_to_levels: floor(4 + log2(sqrt(area) / 224 + 1e-8)), clamped to [2, 5]
        k = 4.0 + float(torch.log2(torch.sqrt((b[2] - b[0]) * (b[3] - b[1])) / 224.0 + 1e-8))
        return k, int(min(max(np.floor(k), 2), 5))

    for item in un_box:
        if item["why"].startswith("no counterpart"):
            side = item["side"]
            other = "B" if side == "A" else "A"
            r = int(roi[side][item["index"]])
            pb = props[side][r]
            item["proposal_index"] = r
            item["proposal_box"] = [round(float(v), 2) for v in pb]
            if (side, r) in explained_rpn:
                item["why"] = "its proposal is absent from the other run; the RPN-stage analysis explains that absence"
                item["explained"] = True
                continue
            # the proposal exists in both runs: does it pool from a different pyramid level there?  (a discrete decision:
            # sqrt(area) / 224 at a power of two)
            uo = _iou_matrix(pb[None], props[other])[0]
            if props[other].shape[0] and float(uo.max()) >= 0.7:
                po = props[other][int(uo.argmax())]
                k_here, l_here = fpn_level(pb)
                k_other, l_other = fpn_level(po)
                item.update(proposal_level_here=l_here, proposal_level_other=l_other, level_k_here=round(k_here, 5), level_k_other=round(k_other, 5))
                if l_here != l_other and abs(k_here - k_other) < 0.05:
                    item["why"] = ("its proposal is pooled from pyramid level %d here and %d there: sqrt(area)/224 sits on a power of two, "
                                   "the box noise decides the floor()" % (l_here, l_other))
                    item["explained"] = True
                    continue
        still.append(item)
    # NMS cascades once more: an item suppressed in the other run by something only that run keeps stands or falls with that
    # suppressor, whose presence may only just have been explained above (through its proposal)
    by_key = {(o["side"], o["index"]): o for o in rep_box["only"]}
    changed = True
    while changed:
        changed = False
        for o in list(still):
            if "suppressor_only_in_other" not in o:
                continue
            q = by_key.get(("B" if o["side"] == "A" else "A", o["suppressor_only_in_other"]))
            if q is not None and q.get("explained"):
                o["explained"] = True
                o["why"] = "nms cascade: suppressed in the other run by an item only that run keeps (whose presence is explained through its proposal)"
                still.remove(o)
                changed = True
    if dump:
        import json
        with open(dump, "w") as f:
            json.dump(dict(box=rep_box, rpn=rep_rpn), f, indent=1)
    rep_rpn = dict(rep_rpn, only=rep_rpn["only"][:6] + ([{"truncated": len(rep_rpn["only"]) - 6}] if len(rep_rpn["only"]) > 6 else []))
    return dict(box=rep_box, rpn=rep_rpn), still + un_rpn
