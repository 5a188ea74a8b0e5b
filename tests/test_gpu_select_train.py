"""-m gpu: apse_rpn_select_train, the training-time FPN selection (csrc/select_nms.hip) on injected inputs.

The rules of tests/test_gpu_select_ops.py, stage by stage, at list lengths on both sides of the inference kernels' 1024: the
shapes are select_ref.FPN_HW (p5 has 1026 anchors, p6 270).  The reference is tests/select_train_ref.py.  The clustered heads are
the cases that reach past rank 1024 (tests/test_select_train_ref.py holds them to that): a kernel that cuts a list at 1024 cannot
pass them.  At (1025, 1000) and (2000, 1) no input can reach that far -- one entry per level lies past 1024, and the best
proposal of an image is rank 0 of its level -- so those two pairs check the list lengths and the truncation only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import select_ref as R
import select_train_ref as T
import test_gpu_select_ops as S

pytestmark = pytest.mark.gpu

F = np.float32
WS = S.WS
IMG_H, IMG_W = R.FPN_IMG
FILL = 7
ONES = np.uint64(0xffffffffffffffff)


def run_train(images, pre, post, thr=0.7, mask=31, B=None, null=None, zero_dec=True, outs=None):
    """images: per image five heads [H*W, ld].  Returns (rc, one dict of numpy arrays per image).  The outputs start at FILL
    (the decoded boxes at zero unless zero_dec is off: like apse_rpn_select, the entry leaves the boxes of empty list places
    alone).  null: name of an output passed as NULL.  outs: device tensors of an earlier call to write into again."""
    from apse_uav_amd import _lib
    nb = len(images)
    B = nb if B is None else B
    dev = [torch.from_numpy(np.stack([im[l] for im in images])).cuda() for l in range(5)]
    hp = (C.c_void_p * 5)(*[t.data_ptr() for t in dev])
    Hs = (C.c_int * 5)(*[h for h, _ in R.FPN_HW])
    Ws = (C.c_int * 5)(*WS)
    pa, po = max(min(pre, T.MAX_PRE), 1), max(min(post, T.MAX_POST), 1)           # allocation sizes of a refused call
    if outs is None:
        t = lambda shape, dt=torch.float32, v=FILL: torch.full(shape, v, dtype=dt, device="cuda")
        outs = dict(keys=t((nb, 5, pa), torch.int64), dec_boxes=t((nb, 5 * pa, 4), v=0 if zero_dec else FILL), dec_scores=t((nb, 5 * pa)),
                    dec_valid=t((nb, 5 * pa), torch.int32), props=t((nb, po, 4)), prop_scores=t((nb, po)),
                    prop_entry=t((nb, po), torch.int32), count=t((nb,), torch.int32))
    ptrs = [C.c_void_p(0) if k == null else _lib.ptr(v) for k, v in outs.items()]
    rc = _lib.load().apse_rpn_select_train(hp, Hs, Ws, images[0][0].shape[1], B, IMG_H, IMG_W, pre, post, thr, mask, *ptrs,
                                           _lib.stream_ptr())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    res = [dict(keys=host["keys"][b].view(np.uint64), dec_boxes=host["dec_boxes"][b], dec_scores=host["dec_scores"][b],
                dec_valid=host["dec_valid"][b], props=host["props"][b], prop_scores=host["prop_scores"][b],
                prop_entry=host["prop_entry"][b], count=int(host["count"][b])) for b in range(nb)]
    return rc, res, outs


def _equal_outputs(a, b):
    return all(np.array_equal(np.atleast_1d(a[k]).view(np.uint8), np.atleast_1d(b[k]).view(np.uint8)) for k in a)


def judge_train(name, logdir, out, heads, pre, post, thr=0.7, mask=31, exact=False, near_cap=0.01):
    """judge_rpn of test_gpu_select_ops.py with the long NMS of select_train_ref.py.  near_cap: the share of entries that may lie
    within tolerance of the empty / nonempty border (None: heads the test did not choose, a network's; the count is logged)."""
    worst, near, total = dict(ref=0.0, hip=0.0), 0, 0
    for l in range(5):
        logit = np.ascontiguousarray(heads[l][:, :3]).reshape(-1)
        idx = R.stable_topk(logit, pre)
        k = len(idx)
        want = np.full(pre, ONES)
        want[:k] = R.sort_key(logit[idx], idx)
        assert np.array_equal(out["keys"][l], want), (name, l)
        sl = slice(l * pre, l * pre + k)
        tail = slice(l * pre + k, (l + 1) * pre)
        assert not out["dec_valid"][tail].any() and not S._bits(out["dec_scores"][tail]).any(), (name, l)
        if not (mask >> l) & 1:
            assert not out["dec_valid"][sl].any() and not S._bits(out["dec_scores"][sl]).any(), (name, l)
            continue
        assert S._same(out["dec_scores"][sl], R.canon(logit[idx])), (name, l)
        b32, ok32 = R.rpn_level_decode(heads[l], idx, l, WS[l], IMG_H, IMG_W)
        b64, mag, margin = R.rpn_level_decode(heads[l], idx, l, WS[l], IMG_H, IMG_W, f64=True)
        near += S.judge_decode("%s/l%d" % (name, l), out["dec_boxes"][sl], out["dec_valid"][sl], b32, ok32, b64, mag, margin, exact,
                               worst)
        total += k
    assert near_cap is None or near <= near_cap * total, (name, near, total)
    # NMS, rank and truncation on the kernel's own boxes, scores and flags
    kept = T.batched_nms_long(out["dec_boxes"], out["dec_scores"], out["dec_valid"], R.level_categories(mask, pre), thr)
    pb, ps, pe, cnt = R.rank32(out["dec_boxes"], out["dec_scores"], kept, post)
    deep = T.deep_entries(pe, cnt, pre)
    S._log(logdir, "select_train/" + name, dict(decode_units_ref32=worst["ref"], decode_units_hip=worst["hip"], near=near, n=total,
                                                count=out["count"], rank_1024_up=deep))
    assert out["count"] == cnt, (name, out["count"], cnt)
    assert np.array_equal(out["prop_entry"], pe), name
    assert S._same(out["props"], pb) and S._same(out["prop_scores"], ps), name
    if exact:
        ref = T.rpn_select_train(heads, WS, IMG_H, IMG_W, pre, post, thr, mask)
        for k_ in ("dec_boxes", "dec_scores", "props", "prop_scores"):
            assert S._same(out[k_], ref[k_]), (name, k_)
        assert np.array_equal(out["dec_valid"] != 0, ref["dec_valid"]) and np.array_equal(out["prop_entry"], ref["prop_entry"])
        assert out["count"] == ref["count"]
    return deep


# ------------------------------------------------------------------------------------------------ the old entry's reach
@pytest.mark.parametrize("kind", ["random", "zeros", "inf", "quant16", "equal"])
@pytest.mark.parametrize("pre", [1, 1000])
def test_equals_rpn_select_up_to_1000(kind, pre):
    heads = R.fpn_heads(21, kind)
    old = S.run_rpn([heads], 1000, pre=pre)[0]
    rc, new, _ = run_train([heads], pre, 1000)
    assert rc == 0
    for k in old:
        assert np.array_equal(np.atleast_1d(old[k]).view(np.uint8), np.atleast_1d(new[0][k]).view(np.uint8)), k


# ------------------------------------------------------------------------------------------------ the key lists
@pytest.mark.parametrize("kind", ["random", "zeros", "inf", "quant16", "equal"])
@pytest.mark.parametrize("pre", [1025, 2000, 2048])
def test_topk_lists(kind, pre, logdir):
    heads = R.fpn_heads(21, kind)
    if kind in ("equal", "zeros"):                    # runs of equal scores across rank 1024 and across k
        logits = heads[0][:, :3].reshape(-1)
        for k in (1024, pre):
            inside, outside, _ = R.tie_run(logits, k)
            assert inside >= 1 and outside >= 1
    rc, (out,), _ = run_train([heads], pre, 1000)
    assert rc == 0
    judge_train("lists/%s/pre%d" % (kind, pre), logdir, out, heads, pre, 1000)
    _, idx5 = R.key_parts(out["keys"][3][:min(pre, 1026)])
    if pre == 1025:                                   # p5: 1026 anchors, exactly one left out
        logit = heads[3][:, :3].reshape(-1)
        assert len(set(idx5)) == 1025 and out["keys"][3][1024] != ONES
        assert set(range(1026)) - set(idx5) == {int(np.argsort(-R.canon(logit), kind="stable")[-1])}
    else:                                             # p5 and p6 are short lists: the tail is all ones
        assert sorted(idx5) == list(range(1026)) and (out["keys"][3][1026:] == ONES).all()
    assert (out["keys"][4][:270] != ONES).all() and (out["keys"][4][270:] == ONES).all()


# ------------------------------------------------------------------------------------------------ the whole chain
PAIRS = [(1025, 1000), (2000, 1000), (2048, 2048), (2000, 1)]


@pytest.mark.parametrize("pre,post", PAIRS)
def test_exact_random_heads(pre, post, logdir):
    heads = R.fpn_heads(21, "random", exact=True)
    rc, (out,), _ = run_train([heads], pre, post)
    assert rc == 0
    judge_train("exact/random/%d_%d" % (pre, post), logdir, out, heads, pre, post, exact=True)


@pytest.mark.parametrize("pre,post", PAIRS)
def test_exact_clustered_heads(pre, post, logdir):
    heads = T.clustered_heads(5, 6, 4.0)
    rc, (out,), _ = run_train([heads], pre, post)
    assert rc == 0
    deep = judge_train("exact/clustered/%d_%d" % (pre, post), logdir, out, heads, pre, post, exact=True)
    if (5, 6, 4.0, pre, post) in T.CLUSTERED_LONG:
        assert deep >= 100                            # the first `post` reach past rank 1024


@pytest.mark.parametrize("seed,ncent,width,pre,post", T.CLUSTERED_LONG)
@pytest.mark.parametrize("exact", [True, False])
def test_clustered_long_lists(seed, ncent, width, pre, post, exact, logdir):
    heads = T.clustered_heads(seed, ncent, width, exact=exact)
    rc, (out,), _ = run_train([heads], pre, post)
    assert rc == 0
    deep = judge_train("clustered/s%d_c%d/%d_%d%s" % (seed, ncent, pre, post, "/exact" if exact else ""), logdir, out, heads, pre,
                       post, exact=exact)
    assert deep >= 100 and out["count"] == post
    if exact:                                         # not the result of lists cut at 1024
        cut = T.rpn_select_train(heads, WS, IMG_H, IMG_W, pre, post, 0.7, slot=T.OLD_SLOT)
        assert not np.array_equal(out["prop_entry"], cut["prop_entry"])


@pytest.mark.parametrize("kind,pre,post", [("random", 2000, 1000), ("random", 2048, 2048), ("quant16", 2000, 1000), ("inf", 2048, 50),
                                           ("zeros", 2000, 1000), ("equal", 1025, 1000)])
def test_non_exact_heads(kind, pre, post, logdir):
    heads = R.fpn_heads(23, kind)
    rc, (out,), _ = run_train([heads], pre, post)
    assert rc == 0
    judge_train("f32/%s/%d_%d" % (kind, pre, post), logdir, out, heads, pre, post)


@pytest.mark.parametrize("exact", [True, False])
def test_level_mask(exact, logdir):
    heads = T.clustered_heads(5, 6, 4.0, exact=exact)
    rc, (out,), _ = run_train([heads], 2000, 1000, mask=0b10101)
    assert rc == 0
    judge_train("mask21%s" % ("/exact" if exact else ""), logdir, out, heads, 2000, 1000, mask=0b10101, exact=exact)
    lv = out["prop_entry"][:out["count"]] // 2000
    assert set(lv) <= {0, 2, 4} and out["count"] == 1000


def test_level_mask_numbers_present_levels_consecutively(logdir):
    """select_ref.mask_flip_heads: the kept set depends on level 2 being category 1 of the call."""
    heads, _, _ = R.mask_flip_heads()
    rc, (out,), _ = run_train([heads], 2000, 1000, mask=0b10101)
    assert rc == 0
    judge_train("mask21_numbering", logdir, out, heads, 2000, 1000, mask=0b10101, exact=True)


def test_invalid_levels_and_image(logdir):
    some = R.fpn_all_invalid(T.clustered_heads(5, 6, 4.0), [0, 1, 2])
    dead = R.fpn_all_invalid(R.fpn_heads(4, exact=True), range(5))
    rc, (a, d), _ = run_train([some, dead], 2000, 2048)
    assert rc == 0
    judge_train("levels012_invalid", logdir, a, some, 2000, 2048, exact=True)
    judge_train("image_invalid", logdir, d, dead, 2000, 2048, exact=True)
    assert not a["dec_valid"][:3 * 2000].any() and 0 < a["count"] < 1026 + 270
    assert (a["prop_entry"][a["count"]:] == -1).all() and not S._bits(a["props"][a["count"]:]).any()
    assert d["count"] == 0 and not d["dec_valid"].any() and (d["prop_entry"] == -1).all()
    assert not S._bits(d["props"]).any() and not S._bits(d["prop_scores"]).any()


def test_batch_equals_single_runs_and_repeats(logdir):
    images = [T.clustered_heads(5, 6, 4.0, exact=False), R.fpn_heads(32, "quant16")]
    rc, batch, outs = run_train(images, 2000, 1000)
    assert rc == 0
    for b, heads in enumerate(images):
        rc, (single,), _ = run_train([heads], 2000, 1000)
        assert rc == 0 and _equal_outputs(single, batch[b]), b
        judge_train("batch2/%d" % b, logdir, batch[b], heads, 2000, 1000)
    # into the same buffers, without clearing them: other inputs, then the first again
    rc, _, _ = run_train([R.fpn_heads(33, "zeros"), T.clustered_heads(6, 3, 4.0)], 2000, 1000, outs=outs)
    assert rc == 0
    rc, again, _ = run_train(images, 2000, 1000, outs=outs)
    assert rc == 0
    for b in range(2):
        assert _equal_outputs(again[b], batch[b]), b


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["pre0", "pre2049", "post0", "post2049", "mask0", "null_props", "null_count", "null_dec_valid", "B65"])
def test_refusals_leave_the_outputs_alone(what):
    from apse_uav_amd import _lib
    heads = R.fpn_heads(1, "random")
    kw = dict(pre=1000, post=1000)
    if what.startswith("pre"):
        kw["pre"] = int(what[3:])
    if what.startswith("post"):
        kw["post"] = int(what[4:])
    rc, (out,), _ = run_train([heads], kw["pre"], kw["post"], mask=0 if what == "mask0" else 31, B=65 if what == "B65" else None,
                              null=what[5:] if what.startswith("null_") else None, zero_dec=False)
    assert rc == -1
    assert b"apse_rpn_select_train" in _lib.load().apse_last_error(None)
    assert (out["keys"].view(np.int64) == FILL).all() and out["count"] == FILL
    for k in ("dec_boxes", "dec_scores", "props", "prop_scores"):
        assert (out[k] == F(FILL)).all(), k
    for k in ("dec_valid", "prop_entry"):
        assert (out[k] == FILL).all(), k
