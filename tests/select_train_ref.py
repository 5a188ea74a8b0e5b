"""NumPy reference of the training-time FPN selection (csrc/select_nms.hip "training-time FPN selection").

detectron2 0.1.2 runs one find_top_rpn_proposals in training and in test, so the stages are those of select_ref.rpn_select and
this module imports them.  What it restates is batched_nms without select_ref's NMS_SLOT = 1024 cut: a level's list may hold up
to 2048 boxes here.  `slot` puts a cut back in, to show what an implementation that silently keeps the old limit would return.

It also makes the heads that exercise the long path.  With random logits the boxes of a level hardly overlap, nearly all of the
first thousand survive the NMS, and the first `post` merged proposals all come from ranks below 1024: the result equals the one
cut at 1024 and a truncating kernel would pass.  clustered_heads() draws the objectness from a few peaks, so that neighbouring
anchors suppress each other and the merged list reaches far down every level's list.
"""
import numpy as np

from select_ref import (F, FPN_HW, STRIDES, canon, fpn_heads, level_categories, max_coord, nms_sorted32, rank32, rpn_level_decode,
                        sort_key, stable_topk)

MAX_PRE = 2048                                   # APSE_RPN_TRAIN_MAX_PRE_TOPK
MAX_POST = 2048                                  # APSE_RPN_TRAIN_MAX_POST_TOPK
OLD_SLOT = 1024                                  # the list length of the inference kernels


def batched_nms_long(boxes, scores, valid, cat, thr, slot=None):
    """select_ref.batched_nms32 without the slot cut (slot = None), or with a cut of `slot` boxes per category."""
    boxes, scores = np.asarray(boxes, F), canon(scores)
    valid, cat = np.asarray(valid, bool), np.asarray(cat, np.int64)
    m1 = max_coord(boxes, valid) + F(1)
    out = {}
    for c in np.unique(cat[valid]):
        e = np.nonzero(valid & (cat == c))[0]
        e = e[np.argsort(-scores[e], kind="stable")][:slot]
        out[int(c)] = e[nms_sorted32(boxes[e] + F(c) * m1, thr)]
    return out


def rpn_select_train(heads, Ws, img_h, img_w, pre, post, thr, level_mask=31, slot=None):
    """The FPN selection of one image at training limits, f32 restatement: select_ref.rpn_select with the long NMS."""
    keys = np.full((5, pre), np.uint64(0xffffffffffffffff))
    boxes, scores, valid = np.zeros((5 * pre, 4), F), np.zeros(5 * pre, F), np.zeros(5 * pre, bool)
    for l in range(5):
        logit = np.ascontiguousarray(heads[l][:, :3]).reshape(-1)
        idx = stable_topk(logit, pre)
        keys[l, :len(idx)] = sort_key(logit[idx], idx)
        if not (level_mask >> l) & 1:
            continue
        b, ok = rpn_level_decode(heads[l], idx, l, Ws[l], img_h, img_w)
        sl = slice(l * pre, l * pre + len(idx))
        boxes[sl], scores[sl], valid[sl] = b, canon(logit[idx]), ok
    kept = batched_nms_long(boxes, scores, valid, level_categories(level_mask, pre), thr, slot)
    pb, ps, pe, cnt = rank32(boxes, scores, kept, post)
    return dict(keys=keys, dec_boxes=boxes, dec_scores=scores, dec_valid=valid, props=pb, prop_scores=ps, prop_entry=pe, count=cnt)


def deep_entries(prop_entry, count, pre):
    """How many of the first `count` proposals come from rank OLD_SLOT or below it in their level's list."""
    e = np.asarray(prop_entry[:count], np.int64)
    return int(((e % pre) >= OLD_SLOT).sum())


def clustered_heads(seed, ncent=6, width=4.0, exact=True, noise=0.25):
    """fpn_heads(seed, "random", sigma=0.05) with the objectness replaced, per level, by peaks around `ncent` centres drawn
    uniformly over the image: cell (y, x) of a level gets 4 * max over the centres of -distance / (width / stride * 8), the
    distance in cells of that level (so a peak is as wide in pixels on every level), plus noise * N(0, 1) per anchor."""
    heads = fpn_heads(seed, "random", exact=exact, sigma=0.05)
    rng = np.random.default_rng(seed + 7919)
    cen = rng.random((ncent, 2))                                       # (y, x) as fractions of the map
    for l, (H, W) in enumerate(FPN_HW):
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        d = np.stack([np.hypot(y - cy * H, x - cx * W) for cy, cx in cen])
        peak = 4.0 * (-d / (width / STRIDES[l] * 8.0)).max(axis=0)
        obj = peak.reshape(H * W, 1) + noise * rng.standard_normal((H * W, 3))
        heads[l][:, :3] = obj.astype(F)
    return heads


# the clustered cases of tests/test_gpu_select_train.py whose first `post` proposals must reach past rank 1024:
# (seed, centres, width, pre, post).  test_select_train_ref.py holds each of them to that.
CLUSTERED_LONG = [(5, 6, 4.0, 2000, 1000), (5, 6, 4.0, 2048, 2048), (6, 3, 4.0, 2000, 1000), (7, 12, 4.0, 2048, 2048),
                  (8, 40, 4.0, 2000, 1000)]
