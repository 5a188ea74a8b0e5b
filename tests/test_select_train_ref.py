"""The reference of the training-time FPN selection (select_train_ref.py) against select_ref.py, and what its clustered heads are
meant to contain.  No GPU."""
import numpy as np
import pytest

import select_ref as R
import select_train_ref as T

WS = [w for _, w in R.FPN_HW]
IMG_H, IMG_W = R.FPN_IMG


def _same(a, b):
    for k in a:
        if not np.array_equal(np.atleast_1d(np.asarray(a[k])).view(np.uint8), np.atleast_1d(np.asarray(b[k])).view(np.uint8)):
            return False
    return True


@pytest.mark.parametrize("kind", ["random", "zeros", "inf", "quant16", "equal"])
@pytest.mark.parametrize("pre,post,mask", [(1, 1000, 31), (1000, 1000, 31), (1000, 50, 0b10101)])
def test_equals_select_ref_up_to_1000(kind, pre, post, mask):
    heads = R.fpn_heads(21, kind)
    assert _same(T.rpn_select_train(heads, WS, IMG_H, IMG_W, pre, post, 0.7, mask), R.rpn_select(heads, WS, IMG_H, IMG_W, pre, post, 0.7, mask))


def test_equals_select_ref_on_clustered_heads():
    heads = T.clustered_heads(5)
    assert _same(T.rpn_select_train(heads, WS, IMG_H, IMG_W, 1000, 1000, 0.7), R.rpn_select(heads, WS, IMG_H, IMG_W, 1000, 1000, 0.7))


def test_level_lengths_straddle_the_old_limit():
    n = [3 * h * w for h, w in R.FPN_HW]
    assert n[3] == 1026 and n[4] == 270 and min(n[:3]) > T.MAX_PRE


def test_random_heads_do_not_reach_past_rank_1024():
    """Why the clustered heads exist: on random logits the long lists change nothing."""
    heads = R.fpn_heads(21, "random", exact=True)
    a = T.rpn_select_train(heads, WS, IMG_H, IMG_W, 2000, 1000, 0.7)
    assert T.deep_entries(a["prop_entry"], a["count"], 2000) == 0
    assert _same(a, T.rpn_select_train(heads, WS, IMG_H, IMG_W, 2000, 1000, 0.7, slot=T.OLD_SLOT))


@pytest.mark.parametrize("seed,ncent,width,pre,post", T.CLUSTERED_LONG)
@pytest.mark.parametrize("exact", [True, False])
def test_clustered_heads_exercise_the_long_lists(seed, ncent, width, pre, post, exact):
    """Entries of rank 1024 or above are among the first `post`, and the result differs from the one cut at 1024 boxes per
    level: a kernel that keeps the old list length cannot return it."""
    heads = T.clustered_heads(seed, ncent, width, exact=exact)
    a = T.rpn_select_train(heads, WS, IMG_H, IMG_W, pre, post, 0.7)
    cut = T.rpn_select_train(heads, WS, IMG_H, IMG_W, pre, post, 0.7, slot=T.OLD_SLOT)
    assert a["count"] == post
    assert T.deep_entries(a["prop_entry"], a["count"], pre) >= 100
    assert not np.array_equal(a["prop_entry"], cut["prop_entry"])
    # ... and from the one whose top-k stops at 1024 per level: compared as (level, rank), the numbering being per `pre`
    short = T.rpn_select_train(heads, WS, IMG_H, IMG_W, T.OLD_SLOT, post, 0.7)
    lr = lambda e, p: np.stack([e // p, e % p], 1)
    assert not np.array_equal(lr(a["prop_entry"].astype(np.int64), pre), lr(short["prop_entry"].astype(np.int64), T.OLD_SLOT))


def test_tie_runs_cross_rank_1024_and_k():
    """The "equal" and "zeros" kinds put runs of equal scores across 1024 and across the k of the long lists."""
    for kind in ("equal", "zeros"):
        logits = R.fpn_heads(21, kind)[0][:, :3].reshape(-1)
        for k in (1024, 1025, 2000, 2048):
            inside, outside, _ = R.tie_run(logits, k)
            assert inside >= 1 and outside >= 1, (kind, k)
