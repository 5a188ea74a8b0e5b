"""The NumPy reference of the decision kernels (select_ref.py) against the CPU oracle, and the preconditions the GPU tests
(test_gpu_select_ops.py) rely on: what their seeded inputs are meant to contain."""
import numpy as np
import pytest
import torch

import select_ref as R
from oracle import ops
from oracle.detector import DetectorOracle

F = np.float32
WS = [w for _, w in R.FPN_HW]
IMG_H, IMG_W = R.FPN_IMG


def _random_boxes(rng, n):
    anc = np.sort(rng.random((n, 2, 2)) * 500, axis=1).reshape(n, 4)[:, [0, 1, 2, 3]].astype(F)
    anc = np.stack([anc[:, 0], anc[:, 1], anc[:, 2] + 1, anc[:, 3] + 1], 1).astype(F)
    return anc


@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)])
def test_decode_matches_oracle(weights):
    rng = np.random.default_rng(0)
    n = 4000
    anc = _random_boxes(rng, n)
    d = (rng.standard_normal((n, 4)) * (0.5 * np.asarray(weights))).astype(F)
    d[:50, 2] = 30.0 * weights[2]                 # above the clamp
    d[50:100, 0] = 40.0 * weights[0]              # wholly outside
    b32, ok32 = R.decode32(anc, d, weights, 300, 400)
    b64, mag, margin = R.decode64(anc, d, weights, 300, 400)
    want = ops.clip_boxes(ops.apply_deltas(torch.from_numpy(d), torch.from_numpy(anc), weights), 300, 400)
    u32 = R.units(b32, b64, mag)
    assert R.units(want.numpy(), b64, mag) <= R.tolerance(u32)
    flags = ops.nonempty(want).numpy()
    free = ~R.near_empty(margin, R.tolerance(u32))
    assert free.mean() >= 0.99
    assert np.array_equal(flags[free], ok32[free])
    assert not ok32[50:100].any() and ok32[:50].any()


@pytest.mark.parametrize("seed,n,ncat,thr", [(0, 3000, 5, 0.7), (1, 900, 3, 0.5), (2, 1, 1, 0.5)])
def test_batched_nms_matches_oracle(seed, n, ncat, thr):
    rng = np.random.default_rng(seed)
    b, _ = R.decode32(_random_boxes(rng, n), (rng.standard_normal((n, 4)) * 0.3).astype(F), (1, 1, 1, 1), 608, 576)
    s = rng.random(n).astype(F)
    s[::5] = s[0]                                  # exact ties
    valid = rng.random(n) > 0.1
    cat = np.arange(n) % ncat
    kept = R.batched_nms32(b, s, valid, cat, thr)
    _, _, entry, cnt = R.rank32(b, s, kept, 200)
    vi = np.nonzero(valid)[0]
    want = vi[ops.batched_nms(torch.from_numpy(b[vi]), torch.from_numpy(s[vi]), torch.from_numpy(cat[vi]), thr)[:200]]
    assert cnt == len(want) and np.array_equal(entry[:cnt], want)


def _oracle_rpn(heads, mask, pre=1000, post=1000):
    lg, dl = [], []
    for (H, W), h in zip(R.FPN_HW, heads):
        t = torch.from_numpy(h).view(H, W, R.FPN_LD)
        lg.append(t[:, :, :3].permute(2, 0, 1).unsqueeze(0).contiguous())
        dl.append(t[:, :, 3:15].permute(2, 0, 1).unsqueeze(0).contiguous())
    o = DetectorOracle({}, dict(rpn_pre_topk=pre, rpn_post_topk=post, rpn_nms=0.7))
    return o.rpn_select(lg, dl, (IMG_H, IMG_W), [l for l in range(5) if (mask >> l) & 1])


@pytest.mark.parametrize("kind,mask,exact", [("random", 31, False), ("quant16", 31, True), ("random", 0b10101, True),
                                             ("random", 16, True)])
def test_rpn_select_matches_oracle(kind, mask, exact):
    heads = R.fpn_heads(11, kind, exact=exact)
    got = R.rpn_select(heads, WS, IMG_H, IMG_W, 1000, 1000, 0.7, mask)
    want = _oracle_rpn(heads, mask)
    levels = [l for l in range(5) if (mask >> l) & 1]
    for j, l in enumerate(levels):
        sc, idx = R.key_parts(got["keys"][l])
        k = len(want["topk_idx"][j])
        assert np.array_equal(idx[:k], want["topk_idx"][j].numpy())
        assert np.array_equal(sc[:k].view(np.uint32), R.canon(want["topk_scores"][j].numpy()).view(np.uint32))
    sel = np.concatenate([np.arange(l * 1000, l * 1000 + min(1000, 3 * R.FPN_HW[l][0] * R.FPN_HW[l][1])) for l in levels])
    assert np.array_equal(got["dec_valid"][sel], want["valid"].numpy())
    cnt = got["count"]
    assert cnt == want["boxes"].shape[0]
    assert np.array_equal(got["prop_scores"][:cnt].view(np.uint32), R.canon(want["logits"].numpy()).view(np.uint32))
    lvl = np.asarray(levels)[want["level"].numpy()]
    assert np.array_equal(got["prop_entry"][:cnt] // 1000, lvl)
    if exact:
        assert np.array_equal(got["props"][:cnt], want["boxes"].numpy())
    else:
        e = got["prop_entry"][:cnt]
        b64 = np.zeros((5000, 4))
        mag = np.ones((5000, 4))
        for l in levels:
            _, idx = R.key_parts(got["keys"][l])
            k = min(1000, 3 * R.FPN_HW[l][0] * R.FPN_HW[l][1])
            b64[l * 1000:l * 1000 + k], mag[l * 1000:l * 1000 + k], _ = R.rpn_level_decode(heads[l], idx[:k], l, WS[l], IMG_H, IMG_W,
                                                                                           f64=True)
        u32 = R.units(got["dec_boxes"], b64, mag)
        assert R.units(want["boxes"].numpy(), b64[e], mag[e]) <= R.tolerance(u32)


@pytest.mark.parametrize("K,P,wide", [(4, 257, False), (7, 37, True), (80, 257, True)])
def test_box_inference_matches_oracle(K, P, wide):
    pred, props = R.box_inputs(5, 1, P, K, 5 * K + 1)
    pred, props = pred[0], props[0]
    thresh = 0.05
    probs, boxes, valid = R.box_candidates(pred, K, props, P, IMG_H, IMG_W, thresh, wide)
    ob, os_, oe, cnt = R.box_nms_rank(boxes, probs[:, :K].reshape(-1), valid, K, 0.5, 100)
    o = DetectorOracle({}, dict(num_classes=K, score_thresh=thresh, box_nms=0.5, dets_per_image=100))
    want = o.box_inference(torch.from_numpy(pred[:, :K + 1].copy()), torch.from_numpy(pred[:, K + 1:5 * K + 1].copy()),
                           torch.from_numpy(props), (IMG_H, IMG_W))
    p64, b64, v64, mag = R.box_candidates(pred, K, props, P, IMG_H, IMG_W, thresh, f64=True)
    tp = R.tolerance(R.units(probs, p64, p64))
    tb = R.tolerance(R.units(boxes, b64, mag))
    assert R.units(want["probs"].numpy(), p64, p64) <= tp
    assert R.units(want["all_boxes"].numpy().reshape(-1, 4), b64, mag) <= tb
    assert cnt == want["boxes"].shape[0]
    assert np.array_equal(oe[:cnt] % K, want["classes"].numpy()) and np.array_equal(oe[:cnt] // K, want["roi_index"].numpy())
    # the random case leaves few candidates near the score threshold
    assert R.near_score(p64[:, :K].reshape(-1), thresh, tp).mean() <= 0.01
    pk = R.pack(ob[None], os_[None], oe[None], np.asarray([cnt]), K)
    assert pk["total"] == cnt and np.array_equal(pk["cls"], want["classes"].numpy().astype(np.int32))


def test_softmax_forms():
    lg = (np.random.default_rng(2).standard_normal((300, 128)) * 3).astype(F)
    for K1 in (2, 5, 8, 65, 66, 128):
        p64 = R.softmax64(lg[:, :K1])
        for wide in (False, True):
            # exp 2 units, the rounding of logit - max (up to 2^-24 * 16 in the exponent: 8 units), half a unit per addend
            assert R.units(R.softmax32(lg[:, :K1], wide), p64, p64) <= 10.0 + K1 / 2
    assert R.softmax32(np.zeros((1, 2), F), False)[0, 0] == F(0.5) and R.softmax32(np.zeros((1, 2), F), True)[0, 0] == F(0.5)


def test_sort_key_roundtrip_and_order():
    s = np.asarray([np.inf, 3.5, 0.0, -0.0, -1e-30, -2.0, -np.inf], F)
    keys = R.sort_key(s, np.arange(7))
    assert np.array_equal(np.argsort(keys, kind="stable"), np.arange(7))
    sc, idx = R.key_parts(keys)
    assert np.array_equal(idx, np.arange(7)) and np.array_equal(sc.view(np.uint32), R.canon(s).view(np.uint32))
    assert np.array_equal(R.stable_topk(np.asarray([-0.0, 0.0, -0.0, 0.0], F), 4), [0, 1, 2, 3])


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("kind", ["quant16", "zeros", "equal"])
def test_tied_inputs_straddle_rank_and_chunk(kind):
    heads = R.fpn_heads(21, kind)
    logit = heads[0][:, :3].reshape(-1)
    inside, outside, chunks = R.tie_run(logit, 1000)
    assert inside >= 1 and outside >= 1 and chunks >= 2
    if kind == "quant16":
        assert len(np.unique(logit)) == 16
    if kind == "zeros":
        top = logit[R.stable_topk(logit, 1000)]
        z = top[top == 0]
        assert np.signbit(z).any() and (~np.signbit(z)).any()
    c4 = R.c4_head(21, 24, 23, "quant16")[:, :15].reshape(-1)
    for k in (6000, 100):
        inside, outside, _ = R.tie_run(c4, k)
        assert inside >= 1 and outside >= 1


@pytest.mark.parametrize("seed", [0, 11])
def test_random_heads_leave_few_boxes_near_empty(seed):
    heads = R.fpn_heads(seed)
    got = R.rpn_select(heads, WS, IMG_H, IMG_W, 1000, 1000, 0.7)
    near = total = 0
    for l in range(5):
        _, idx = R.key_parts(got["keys"][l])
        k = min(1000, 3 * R.FPN_HW[l][0] * R.FPN_HW[l][1])
        b64, mag, margin = R.rpn_level_decode(heads[l], idx[:k], l, WS[l], IMG_H, IMG_W, f64=True)
        u32 = R.units(got["dec_boxes"][l * 1000:l * 1000 + k], b64, mag)
        near += int(R.near_empty(margin, R.tolerance(u32)).sum())
        total += k
    assert near <= 0.01 * total
    h = R.c4_head(seed, 24, 23)
    r = R.c4_select(h, 23, 384, 368, 6000, 1000, 0.7)
    b64, mag, margin = R.c4_decode(h, r["idx"], 23, 384, 368, f64=True)
    assert R.near_empty(margin, R.tolerance(R.units(r["dec_boxes"], b64, mag))).mean() <= 0.01


def test_crafted_edges_are_what_they_claim():
    heads, crafted = R.fpn_edge_heads(3)
    got = R.rpn_select(heads, WS, IMG_H, IMG_W, 1000, 1000, 0.7)
    for name, (l, e, ok) in crafted.items():
        _, idx = R.key_parts(got["keys"][l])
        pos = l * 1000 + int(np.nonzero(idx == e)[0][0])
        b = got["dec_boxes"][pos]
        assert bool(got["dec_valid"][pos]) == ok, name
        if name == "sliver":
            assert b[2] == F(IMG_W) and b[0] == np.nextafter(F(IMG_W), F(0))
        if name in ("left", "right"):
            assert b[0] == b[2] == (0 if name == "left" else IMG_W)
        if name in ("top", "bottom"):
            assert b[1] == b[3] == (0 if name == "top" else IMG_H)
    same, _ = R.fpn_edge_heads(3, clamp_value=float(R.SCALE_CLAMP))
    ref = R.rpn_select(same, WS, IMG_H, IMG_W, 1000, 1000, 0.7)
    assert np.array_equal(ref["dec_boxes"], got["dec_boxes"])
    l, e, _ = crafted["clamp_w"]
    _, idx = R.key_parts(got["keys"][l])
    b = got["dec_boxes"][l * 1000 + int(np.nonzero(idx == e)[0][0])]
    assert 0 < b[0] < IMG_W                       # the clamped width shows: its left edge is inside the image
    dead = R.rpn_select(R.fpn_all_invalid(R.fpn_heads(3, exact=True), range(5)), WS, IMG_H, IMG_W, 1000, 50, 0.7)
    assert dead["count"] == 0 and not dead["dec_valid"].any() and (dead["prop_entry"] == -1).all() and not dead["props"].any()


def test_level_mask_numbering_matters():
    heads, eA, eB = R.mask_flip_heads()
    a = R.rpn_select(heads, WS, IMG_H, IMG_W, 1000, 1000, 0.7, 0b10101, consecutive=True)
    b = R.rpn_select(heads, WS, IMG_H, IMG_W, 1000, 1000, 0.7, 0b10101, consecutive=False)
    assert not np.array_equal(a["prop_entry"], b["prop_entry"])
    want = _oracle_rpn(heads, 0b10101)
    assert a["count"] == want["boxes"].shape[0] and np.array_equal(a["props"][:a["count"]], want["boxes"].numpy())


def test_c4_inputs_exercise_the_scan():
    h = R.c4_head(0, 47, 84)
    full = R.c4_select(h, 84, 750, 1333, 6000, 1000, 0.95)
    e = np.nonzero(full["dec_valid"])[0]
    assert len(R.nms_sorted32(full["dec_boxes"][e], 0.95)) > 1024          # more survivors than one block of keep slots
    early = R.c4_select(h, 84, 750, 1333, 6000, 10, 0.7)
    assert early["count"] == 10 and early["prop_entry"][9] < full["dec_valid"].sum() - 64      # the scan ends chunks early
    small = R.c4_select(R.c4_head(1, 5, 4), 4, 80, 64, 6000, 1000, 0.7)
    assert len(small["idx"]) == 300 and not small["dec_valid"][300:].any()
