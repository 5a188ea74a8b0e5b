"""-m gpu: the decision kernels (csrc/select_nms.hip) on injected inputs, at their edges.

apse_rpn_select, apse_box_inference and apse_c4_rpn_select run the launchers of the detector on inputs the test writes.  Every
stage is judged on its own, fed the kernel's own earlier outputs (select_ref.py):

* top-k keys: equal to the stable sort (score descending, ties by index), anchor index and score bits;
* decoded boxes and probabilities: against the float64 form, in units of 2^-23 of the magnitude; allowed is twice what the
  f32 restatement itself is off (the room a device expf gets), at least 4; both figures go to ops_parity.log;
* the nonempty and score flags: exactly the comparison on the kernel's own numbers, and the float64 decision wherever that is
  farther from its threshold than the tolerance (at most 1 % of a case's entries may be that close);
* NMS, rank, truncation, pack: equal to the f32 restatement run on the kernel's own boxes, scores and flags;
* exact-arithmetic inputs (dw = dh = 0): the whole chain equals the restatement bit for bit.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import select_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
WS = [w for _, w in R.FPN_HW]
IMG_H, IMG_W = R.FPN_IMG
PRE = 1000


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "ops_parity.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ calls
def run_rpn(images, post, thr=0.7, mask=31, pre=PRE):
    """images: per image five heads [H*W, ld].  Returns one dict of numpy arrays per image."""
    from apse_uav_amd import _lib
    B = len(images)
    dev = [torch.from_numpy(np.stack([im[l] for im in images])).cuda() for l in range(5)]
    hp = (C.c_void_p * 5)(*[t.data_ptr() for t in dev])
    Hs = (C.c_int * 5)(*[h for h, _ in R.FPN_HW])
    Ws = (C.c_int * 5)(*WS)
    keys = torch.zeros((B, 5, pre), dtype=torch.int64, device="cuda")
    db = torch.zeros((B, 5 * pre, 4), device="cuda")
    ds = torch.zeros((B, 5 * pre), device="cuda")
    dv = torch.zeros((B, 5 * pre), dtype=torch.int32, device="cuda")
    pb = torch.full((B, post, 4), 7.0, device="cuda")
    ps = torch.full((B, post), 7.0, device="cuda")
    pe = torch.full((B, post), 7, dtype=torch.int32, device="cuda")
    pc = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    rc = _lib.load().apse_rpn_select(hp, Hs, Ws, images[0][0].shape[1], B, IMG_H, IMG_W, pre, post, thr, mask, _lib.ptr(keys),
                                     _lib.ptr(db), _lib.ptr(ds), _lib.ptr(dv), _lib.ptr(pb), _lib.ptr(ps), _lib.ptr(pe),
                                     _lib.ptr(pc), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    k, db, ds, dv, pb, ps, pe, pc = [t.cpu().numpy() for t in (keys, db, ds, dv, pb, ps, pe, pc)]
    return [dict(keys=k[b].view(np.uint64), dec_boxes=db[b], dec_scores=ds[b], dec_valid=dv[b], props=pb[b], prop_scores=ps[b],
                 prop_entry=pe[b], count=int(pc[b])) for b in range(B)]


def run_box(pred, K, props, cnt, thresh, thr, dets, wide, img=R.FPN_IMG):
    from apse_uav_amd import _lib
    B, P, ld = pred.shape
    t = lambda shape, dt=torch.float32: torch.full(shape, 7, dtype=dt, device="cuda")
    i32 = torch.int32
    o = dict(probs=t((B * P, K + 1)), cand_boxes=t((B * P * K, 4)), cand_scores=t((B * P * K,)), cand_valid=t((B * P * K,), i32),
             det_boxes=t((B, dets, 4)), det_scores=t((B, dets)), det_entry=t((B, dets), i32), det_cnt=t((B,), i32),
             pk_boxes=t((B * dets, 4)), pk_scores=t((B * dets,)), pk_cls=t((B * dets,), i32), pk_img=t((B * dets,), i32),
             pk_roi=t((B * dets,), i32), pk_total=t((1,), i32), pk_offset=t((B + 1,), i32))
    pd, pr = torch.from_numpy(pred).cuda(), torch.from_numpy(props).cuda()
    cd = torch.tensor(list(cnt), dtype=i32, device="cuda")
    rc = _lib.load().apse_box_inference(_lib.ptr(pd), ld, K, _lib.ptr(pr), _lib.ptr(cd), P, B, img[0], img[1], float(thresh), thr, dets,
                                        int(wide), *[_lib.ptr(v) for v in o.values()], _lib.stream_ptr())
    if rc:
        return rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def run_c4(heads, H, W, img, pre, post, thr):
    from apse_uav_amd import _lib
    B = len(heads)
    hd = torch.from_numpy(np.stack(heads)).cuda()
    db = torch.zeros((B, pre, 4), device="cuda")
    ds = torch.full((B, pre), 7.0, device="cuda")
    dv = torch.full((B, pre), 7, dtype=torch.int32, device="cuda")
    pb = torch.full((B, post, 4), 7.0, device="cuda")
    ps = torch.full((B, post), 7.0, device="cuda")
    pe = torch.full((B, post), 7, dtype=torch.int32, device="cuda")
    pc = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    rc = _lib.load().apse_c4_rpn_select(_lib.ptr(hd), H, W, B, img[0], img[1], pre, post, thr, _lib.ptr(db), _lib.ptr(ds),
                                        _lib.ptr(dv), _lib.ptr(pb), _lib.ptr(ps), _lib.ptr(pe), _lib.ptr(pc), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    db, ds, dv, pb, ps, pe, pc = [t.cpu().numpy() for t in (db, ds, dv, pb, ps, pe, pc)]
    return [dict(dec_boxes=db[b], dec_scores=ds[b], dec_valid=dv[b], props=pb[b], prop_scores=ps[b], prop_entry=pe[b],
                 count=int(pc[b])) for b in range(B)]


# ------------------------------------------------------------------------------------------------ judges
def judge_decode(name, boxes, valid, b32, ok32, b64, mag, margin, exact, worst):
    """Decoded boxes and their nonempty flags of one list, against the restatement (b32, ok32) and the float64 form.  Returns
    how many entries are too close to the empty / nonempty border for float64 to decide."""
    u32, uhip = R.units(b32, b64, mag), R.units(boxes, b64, mag)
    tol = R.tolerance(u32)
    worst["ref"], worst["hip"] = max(worst["ref"], u32), max(worst["hip"], uhip)
    assert uhip <= tol, (name, uhip, tol)
    assert np.array_equal(valid != 0, ((boxes[:, 2] - boxes[:, 0]) > 0) & ((boxes[:, 3] - boxes[:, 1]) > 0)), name
    if exact:                                       # IEEE arithmetic only: the restatement's bits
        assert _same(boxes, b32) and np.array_equal(valid != 0, ok32), name
    near = R.near_empty(margin, tol)
    assert np.array_equal((valid != 0)[~near], (margin > 0)[~near]), name
    return int(near.sum())


def judge_rpn(name, logdir, out, heads, post, thr=0.7, mask=31, exact=False, pre=PRE):
    worst, near, total = dict(ref=0.0, hip=0.0), 0, 0
    for l in range(5):
        logit = np.ascontiguousarray(heads[l][:, :3]).reshape(-1)
        idx = R.stable_topk(logit, pre)
        k = len(idx)
        want = np.full(pre, np.uint64(0xffffffffffffffff))
        want[:k] = R.sort_key(logit[idx], idx)
        assert np.array_equal(out["keys"][l], want), (name, l)
        sl = slice(l * pre, l * pre + k)
        tail = slice(l * pre + k, (l + 1) * pre)
        assert not out["dec_valid"][tail].any() and not _bits(out["dec_scores"][tail]).any(), (name, l)
        if not (mask >> l) & 1:
            assert not out["dec_valid"][sl].any() and not _bits(out["dec_scores"][sl]).any(), (name, l)
            continue
        assert _same(out["dec_scores"][sl], R.canon(logit[idx])), (name, l)
        b32, ok32 = R.rpn_level_decode(heads[l], idx, l, WS[l], IMG_H, IMG_W)
        b64, mag, margin = R.rpn_level_decode(heads[l], idx, l, WS[l], IMG_H, IMG_W, f64=True)
        near += judge_decode("%s/l%d" % (name, l), out["dec_boxes"][sl], out["dec_valid"][sl], b32, ok32, b64, mag, margin, exact,
                             worst)
        total += k
    assert near <= 0.01 * total, (name, near, total)
    _log(logdir, "select/rpn/" + name, dict(decode_units_ref32=worst["ref"], decode_units_hip=worst["hip"], near=near, n=total))
    # NMS, rank and truncation on the kernel's own boxes, scores and flags; categories numbered over the levels present
    kept = R.batched_nms32(out["dec_boxes"], out["dec_scores"], out["dec_valid"], R.level_categories(mask, pre), thr)
    pb, ps, pe, cnt = R.rank32(out["dec_boxes"], out["dec_scores"], kept, post)
    assert out["count"] == cnt, (name, out["count"], cnt)
    assert np.array_equal(out["prop_entry"], pe), name
    assert _same(out["props"], pb) and _same(out["prop_scores"], ps), name
    if exact:
        ref = R.rpn_select(heads, WS, IMG_H, IMG_W, pre, post, thr, mask)
        for k_ in ("dec_boxes", "dec_scores", "props", "prop_scores"):
            assert _same(out[k_], ref[k_]), (name, k_)
        assert np.array_equal(out["dec_valid"] != 0, ref["dec_valid"]) and np.array_equal(out["prop_entry"], ref["prop_entry"])
    return worst


def judge_box(name, logdir, out, pred, K, props, cnt, thresh, thr, dets, wide, exact_scores=False):
    B, P, ld = pred.shape
    worst = dict(pref=0.0, phip=0.0, bref=0.0, bhip=0.0)
    near = live_n = 0
    det = []
    for b in range(B):
        rs, es = slice(b * P, (b + 1) * P), slice(b * P * K, (b + 1) * P * K)
        probs, boxes, cv = out["probs"][rs], out["cand_boxes"][es], out["cand_valid"][es]
        p32, b32, _ = R.box_candidates(pred[b], K, props[b], cnt[b], IMG_H, IMG_W, thresh, wide)
        p64, b64, v64, mag = R.box_candidates(pred[b], K, props[b], cnt[b], IMG_H, IMG_W, thresh, f64=True)
        up, uph = R.units(p32, p64, p64), R.units(probs, p64, p64)
        ub, ubh = R.units(b32, b64, mag), R.units(boxes, b64, mag)
        tp, tb = R.tolerance(up), R.tolerance(ub)
        assert uph <= tp and ubh <= tb, (name, b, uph, tp, ubh, tb)
        for k_, v in (("pref", up), ("phip", uph), ("bref", ub), ("bhip", ubh)):
            worst[k_] = max(worst[k_], v)
        score = probs[:, :K].reshape(-1)
        assert _same(out["cand_scores"][es], score), (name, b)
        live = np.repeat(np.arange(P) < cnt[b], K)
        assert np.array_equal(cv != 0, live & (score > F(thresh))), (name, b)
        if exact_scores:
            assert np.array_equal(cv != 0, v64), (name, b)
        else:
            close = R.near_score(p64[:, :K].reshape(-1), thresh, tp) & live
            assert np.array_equal((cv != 0)[~close], v64[~close]), (name, b)
            near += int(close.sum())
        live_n += int(live.sum())
        ob, os_, oe, n = R.box_nms_rank(boxes, out["cand_scores"][es], cv, K, thr, dets)
        assert out["det_cnt"][b] == n, (name, b, out["det_cnt"][b], n)
        assert np.array_equal(out["det_entry"][b], oe), (name, b)
        assert _same(out["det_boxes"][b], ob) and _same(out["det_scores"][b], os_), (name, b)
        det.append(n)
    assert near <= 0.01 * max(live_n, 1), (name, near, live_n)
    pk = R.pack(out["det_boxes"], out["det_scores"], out["det_entry"], np.asarray(det), K)
    n = pk["total"]
    assert int(out["pk_total"][0]) == n and np.array_equal(out["pk_offset"], pk["offset"]), name
    assert _same(out["pk_boxes"][:n], pk["boxes"]) and _same(out["pk_scores"][:n], pk["scores"]), name
    for k_ in ("cls", "roi", "img"):
        assert np.array_equal(out["pk_" + k_][:n], pk[k_]), (name, k_)
    _log(logdir, "select/box/" + name, dict(prob_units_ref32=worst["pref"], prob_units_hip=worst["phip"],
                                            decode_units_ref32=worst["bref"], decode_units_hip=worst["bhip"], near=near, dets=det))
    return det


def judge_c4(name, logdir, out, head, W, img, pre, post, thr, exact=False):
    logit = np.ascontiguousarray(head[:, :15]).reshape(-1)
    idx = R.stable_topk(logit, pre)                   # exactly k, the lowest indices of a tied run
    k = len(idx)
    assert _same(out["dec_scores"][:k], R.canon(logit[idx])), name
    assert not out["dec_valid"][k:].any() and not _bits(out["dec_scores"][k:]).any(), name
    b32, ok32 = R.c4_decode(head, idx, W, img[0], img[1])
    b64, mag, margin = R.c4_decode(head, idx, W, img[0], img[1], f64=True)
    worst = dict(ref=0.0, hip=0.0)
    near = judge_decode(name, out["dec_boxes"][:k], out["dec_valid"][:k], b32, ok32, b64, mag, margin, exact, worst)
    assert near <= 0.01 * k, (name, near, k)
    _log(logdir, "select/c4/" + name, dict(decode_units_ref32=worst["ref"], decode_units_hip=worst["hip"], near=near, n=k))
    pb, ps, pe, cnt = R.c4_nms(out["dec_boxes"], out["dec_scores"], out["dec_valid"], thr, post)
    assert out["count"] == cnt, (name, out["count"], cnt)
    assert np.array_equal(out["prop_entry"], pe), name
    assert _same(out["props"], pb) and _same(out["prop_scores"], ps), name
    if exact:
        ref = R.c4_select(head, W, img[0], img[1], pre, post, thr)
        assert _same(out["props"], ref["props"]) and np.array_equal(out["prop_entry"], ref["prop_entry"]), name
    return cnt


# ------------------------------------------------------------------------------------------------ FPN selection
@pytest.mark.parametrize("kind,mask,post,exact", [
    ("random", 31, 1000, False), ("random", 31, 50, False), ("random", 16, 1000, False), ("random", 0b00110, 1000, False),
    ("random", 0b10101, 50, False), ("quant16", 31, 1000, False), ("quant16", 0b10101, 1000, True), ("equal", 31, 1000, False),
    ("zeros", 31, 1000, False), ("zeros", 0b00110, 50, True), ("inf", 31, 1000, False), ("random", 31, 1000, True)])
def test_rpn_select(kind, mask, post, exact, logdir):
    heads = R.fpn_heads(21, kind, exact=exact)
    if kind in ("quant16", "zeros", "equal"):         # the ties straddle rank 1000 and a chunk boundary of level 0
        inside, outside, chunks = R.tie_run(heads[0][:, :3].reshape(-1), PRE)
        assert inside >= 1 and outside >= 1 and chunks >= 2
    out = run_rpn([heads], post, mask=mask)[0]
    judge_rpn("%s/m%d/p%d%s" % (kind, mask, post, "/exact" if exact else ""), logdir, out, heads, post, mask=mask, exact=exact)


def test_rpn_select_signed_zeros_tie_by_index(logdir):
    """-0.0 and +0.0 are one score: a level of them comes out in index order."""
    heads = R.fpn_heads(5, "random", exact=True)
    sign = np.random.default_rng(5).random(heads[2][:, :3].shape) < 0.5
    heads[2][:, :3] = np.where(sign, F(-0.0), F(0.0))
    out = run_rpn([heads], 1000)[0]
    _, idx = R.key_parts(out["keys"][2])
    assert np.array_equal(idx, np.arange(PRE))
    assert not _bits(out["dec_scores"][2 * PRE:3 * PRE]).any()          # +0, whatever the logit's sign
    judge_rpn("signed_zero_level", logdir, out, heads, 1000, exact=True)


def test_rpn_select_batch_equals_single_runs(logdir):
    images = [R.fpn_heads(31, "random"), R.fpn_heads(32, "quant16"), R.fpn_heads(33, "zeros")]
    batch = run_rpn(images, 1000)
    for b, heads in enumerate(images):
        single = run_rpn([heads], 1000)[0]
        for k in single:
            assert np.array_equal(np.atleast_1d(batch[b][k]).view(np.uint8), np.atleast_1d(single[k]).view(np.uint8)), (b, k)
        judge_rpn("batch3/%d" % b, logdir, batch[b], heads, 1000)


def test_rpn_select_decode_edges(logdir):
    heads, crafted = R.fpn_edge_heads(3)
    out = run_rpn([heads], 1000)[0]
    judge_rpn("edges", logdir, out, heads, 1000)
    clamped, _ = R.fpn_edge_heads(3, clamp_value=float(R.SCALE_CLAMP))
    ref = run_rpn([clamped], 1000)[0]
    assert _same(out["dec_boxes"], ref["dec_boxes"])              # a size above the clamp decodes as the clamp itself
    for name, (l, e, ok) in crafted.items():
        _, idx = R.key_parts(out["keys"][l])
        pos = l * PRE + int(np.nonzero(idx == e)[0][0])
        b = out["dec_boxes"][pos]
        assert bool(out["dec_valid"][pos]) == ok, name
        if name == "sliver":
            assert b[2] == F(IMG_W) and b[0] == np.nextafter(F(IMG_W), F(0))
        elif name in ("left", "right"):
            assert b[0] == b[2] == (0 if name == "left" else IMG_W)
        elif name in ("top", "bottom"):
            assert b[1] == b[3] == (0 if name == "top" else IMG_H)
        else:
            assert 0 < b[0 if name == "clamp_w" else 1] < IMG_W


def test_rpn_select_invalid_level_and_image(logdir):
    one = R.fpn_all_invalid(R.fpn_heads(3, exact=True), [4])
    dead = R.fpn_all_invalid(R.fpn_heads(4, exact=True), range(5))
    a, d = run_rpn([one, dead], 50)
    judge_rpn("level4_invalid", logdir, a, one, 50, exact=True)
    judge_rpn("image_invalid", logdir, d, dead, 50, exact=True)
    assert not a["dec_valid"][4 * PRE:].any() and a["count"] == 50
    assert d["count"] == 0 and not d["dec_valid"].any() and (d["prop_entry"] == -1).all()
    assert not _bits(d["props"]).any() and not _bits(d["prop_scores"]).any()


def test_rpn_select_numbers_present_levels_consecutively(logdir):
    """Mask 0b10101: level 2 is category 1 of the call.  The head holds a pair whose IoU sits on the threshold only at that
    offset; with level - first level (category 2) the kept set differs."""
    heads, eA, eB = R.mask_flip_heads()
    a = R.rpn_select(heads, WS, IMG_H, IMG_W, PRE, 1000, 0.7, 0b10101, consecutive=True)
    b = R.rpn_select(heads, WS, IMG_H, IMG_W, PRE, 1000, 0.7, 0b10101, consecutive=False)
    assert not np.array_equal(a["prop_entry"], b["prop_entry"])
    out = run_rpn([heads], 1000, mask=0b10101)[0]
    _log(logdir, "select/rpn/mask21_numbering", dict(count=out["count"], consecutive=a["count"], from_first=b["count"],
                                                     equals_from_first=bool(np.array_equal(out["prop_entry"], b["prop_entry"]))))
    judge_rpn("mask21_numbering", logdir, out, heads, 1000, mask=0b10101, exact=True)
    assert np.array_equal(out["prop_entry"], a["prop_entry"])


# ------------------------------------------------------------------------------------------------ box inference
def _dets(K):
    return 64 if K == 127 else 100               # K * dets <= 8192: one block sorts the wide ranking


BOX_GRID = [(P, K, wide, tight) for P in (37, 257, 1000) for (K, wide) in
            [(1, 0), (1, 1), (4, 0), (4, 1), (7, 0), (7, 1), (8, 1), (65, 1), (80, 1), (127, 1)] for tight in (0, 1)]


@pytest.mark.parametrize("P,K,wide,tight", BOX_GRID)
def test_box_inference(P, K, wide, tight, logdir):
    ld = 5 * K + 1 if tight else (5 * K + 1 + 31) // 32 * 32
    pred, props = R.box_inputs(100 + P + K, 3, P, K, ld)
    cnt = (0, 1, P) if tight else (P, P - 1, 1)
    out = run_box(pred, K, props, cnt, 0.05, 0.5, _dets(K), wide)
    judge_box("P%d/K%d/%s/ld%d" % (P, K, "wide" if wide else "narrow", ld), logdir, out, pred, K, props, cnt, 0.05, 0.5, _dets(K), wide)


def test_box_inference_narrow_refused_above_7():
    pred, props = R.box_inputs(1, 1, 37, 8, 64)
    assert run_box(pred, 8, props, (37,), 0.05, 0.5, 100, 0) != 0


@pytest.mark.parametrize("K", [1, 4, 7])
def test_box_inference_narrow_and_wide_agree(K, logdir):
    pred, props = R.box_inputs(7, 2, 257, K, 64)
    n = run_box(pred, K, props, (257, 200), 0.05, 0.5, 100, 0)
    w = run_box(pred, K, props, (257, 200), 0.05, 0.5, 100, 1)
    assert _same(n["cand_boxes"], w["cand_boxes"])                # the same arithmetic
    p64 = np.concatenate([R.softmax64(pred[b][:, :K + 1]) for b in range(2)])
    tol = R.tolerance(max(R.units(np.concatenate([R.softmax32(pred[b][:, :K + 1], wd) for b in range(2)]), p64, p64) for wd in (0, 1)))
    un, uw = R.units(n["probs"], p64, p64), R.units(w["probs"], p64, p64)
    _log(logdir, "select/box/narrow_wide/K%d" % K, dict(narrow=un, wide=uw, tol=tol))
    assert un <= tol and uw <= tol


@pytest.mark.parametrize("wide", [0, 1])
def test_box_inference_score_on_the_threshold(wide, logdir):
    """K = 1 and logits [0, 0]: p = 0.5 exactly.  Not above 0.5; above the float below it."""
    pred, props = R.box_inputs(9, 1, 37, 1, 32)
    pred[:, :, :2] = 0
    pred[:, :, 2:6] = 0
    below = float(np.nextafter(F(0.5), F(0)))
    at = run_box(pred, 1, props, (37,), 0.5, 0.5, 100, wide)
    under = run_box(pred, 1, props, (37,), below, 0.5, 100, wide)
    assert (_bits(at["probs"]) == _bits(F(0.5))).all()
    assert not at["cand_valid"].any() and at["det_cnt"][0] == 0 and at["pk_total"][0] == 0
    assert under["cand_valid"].all() and under["det_cnt"][0] > 0
    judge_box("threshold/at/%d" % wide, logdir, at, pred, 1, props, (37,), 0.5, 0.5, 100, wide, exact_scores=True)
    judge_box("threshold/below/%d" % wide, logdir, under, pred, 1, props, (37,), below, 0.5, 100, wide, exact_scores=True)


@pytest.mark.parametrize("K,wide", [(4, 0), (4, 1), (80, 1)])
def test_box_inference_ties_and_degenerate_boxes(K, wide, logdir):
    """Identical rows on different ROIs tie and go by entry; two identical proposals of zero size have an IoU of 0/0, which
    is not above the threshold: both stay."""
    P, dets = 37, 100
    pred, props = R.box_inputs(13, 1, P, K, 5 * K + 1)
    rows = (3, 9, 20, 30, 31)
    pred[0, rows] = pred[0, 3]
    pred[0, rows, 0] = 6.0                                       # class 0 well above the threshold on all of them
    pred[0, rows, K + 1:K + 5] = 0                               # its box is the proposal itself
    for j, r in enumerate(rows[:3]):
        props[0, r] = [10 + 150 * j, 20, 100 + 150 * j, 90]      # disjoint: none suppresses another
    props[0, 30] = props[0, 31] = [300, 400, 300, 400]           # zero width and height, twice
    out = run_box(pred, K, props, (P,), 0.05, 0.5, dets, wide)
    judge_box("ties/K%d/%d" % (K, wide), logdir, out, pred, K, props, (P,), 0.05, 0.5, dets, wide)
    n = out["det_cnt"][0]
    e = list(out["det_entry"][0][:n])
    pos = [e.index(r * K) for r in rows]                         # all five kept
    assert pos == sorted(pos) and len(set(_bits(out["det_scores"][0][pos]))) == 1
    assert pos[4] == pos[3] + 1


@pytest.mark.parametrize("K,wide,dets", [(4, 0, 100), (4, 0, 5), (4, 1, 5), (80, 1, 100), (80, 1, 5), (8, 1, 100)])
def test_box_inference_truncation_and_one_class(K, wide, dets, logdir):
    """More survivors than dets_per_image; then one class holding every candidate.  K * dets: 8000 (the 8192-key sort) with
    80 classes and 100 detections, 1024 or fewer otherwise."""
    P = 257
    pred, props = R.box_inputs(17, 2, P, K, 5 * K + 1, logit_scale=3.0)
    pred[:, :, K + 1:5 * K + 1] *= 0.2
    out = run_box(pred, K, props, (P, P), 0.05, 0.9, dets, wide)
    judge_box("trunc/K%d/%d/d%d" % (K, wide, dets), logdir, out, pred, K, props, (P, P), 0.05, 0.9, dets, wide)
    for b in range(2):
        boxes, sc, cv = [out[k][b * P * K:(b + 1) * P * K] for k in ("cand_boxes", "cand_scores", "cand_valid")]
        kept = R.batched_nms32(boxes, sc, cv, np.arange(P * K) % K, 0.9)
        assert sum(len(v) for v in kept.values()) > dets and out["det_cnt"][b] == dets
    pred[:, :, :K + 1] = -4.0
    pred[:, :, K // 2] = 6.0
    out = run_box(pred, K, props, (P, P - 1), 0.05, 0.9, dets, wide)
    judge_box("oneclass/K%d/%d/d%d" % (K, wide, dets), logdir, out, pred, K, props, (P, P - 1), 0.05, 0.9, dets, wide)
    assert (out["pk_cls"][:out["pk_total"][0]] == K // 2).all() and out["pk_total"][0] > 0


def test_box_inference_wide_twice_without_clearing(logdir):
    """nms_prepare_list zeroes the class counts for the next call: a second call sees clean counts."""
    K, P = 65, 257
    pred, props = R.box_inputs(19, 3, P, K, 352)
    other, oprops = R.box_inputs(20, 3, P, K, 352)
    first = run_box(pred, K, props, (P, 5, P - 1), 0.05, 0.5, 100, 1)
    run_box(other, K, oprops, (P, P, P), 0.01, 0.5, 100, 1)
    second = run_box(pred, K, props, (P, 5, P - 1), 0.05, 0.5, 100, 1)
    for k in first:
        if not k.startswith("pk_") or k in ("pk_total", "pk_offset"):
            assert np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)), k
    judge_box("wide_twice", logdir, second, pred, K, props, (P, 5, P - 1), 0.05, 0.5, 100, 1)


# ------------------------------------------------------------------------------------------------ C4 selection
C4_MAPS = {"24x23": (24, 23, (384, 368)), "47x84": (47, 84, (750, 1333)), "5x4": (5, 4, (80, 64))}


@pytest.mark.parametrize("m,kind,pre,post,thr,exact", [
    ("24x23", "random", 6000, 1000, 0.7, False), ("24x23", "quant16", 6000, 10, 0.7, False), ("24x23", "quant16", 100, 10, 0.7, True),
    ("47x84", "random", 6000, 1000, 0.7, False), ("47x84", "random", 6000, 1000, 0.95, False), ("47x84", "quant16", 100, 1000, 0.7, False),
    ("47x84", "random", 6000, 10, 0.7, True), ("5x4", "random", 6000, 1000, 0.7, False), ("5x4", "equal", 100, 10, 0.7, True)])
def test_c4_rpn_select(m, kind, pre, post, thr, exact, logdir):
    H, W, img = C4_MAPS[m]
    heads = [R.c4_head(41, H, W, kind, exact=exact), R.c4_head(42, H, W, kind, exact=exact)]          # B = 2
    if kind == "quant16":                             # rank k falls inside a run of equal scores
        inside, outside, _ = R.tie_run(heads[0][:, :15].reshape(-1), pre)
        assert inside >= 1 and outside >= 1
    outs = run_c4(heads, H, W, img, pre, post, thr)
    for b in range(2):
        cnt = judge_c4("%s/%s/pre%d/post%d/thr%g/%d" % (m, kind, pre, post, thr, b), logdir, outs[b], heads[b], W, img, pre, post, thr, exact)
        if m == "47x84" and thr == 0.95:              # more survivors than the scan's 1024 keep slots: it stops at post
            e = np.nonzero(outs[b]["dec_valid"])[0]
            assert len(R.nms_sorted32(outs[b]["dec_boxes"][e], thr)) > 1024 and cnt == post
        if m == "47x84" and post == 10:               # the scan ends chunks before the list does
            assert cnt == 10 and outs[b]["prop_entry"][9] < outs[b]["dec_valid"].sum() - 64
        if m == "5x4":
            assert not outs[b]["dec_valid"][300:].any()
