"""Plain NumPy reference of the decision kernels (csrc/select_nms.hip): top-k, decode, softmax, NMS, rank, pack.

Two forms of every stage:

* the f32 restatement: every product, sum and division rounded separately in np.float32, in the kernels' operand order
  (rpn_decode, box_candidates, nms_store_sorted, nms_matrix).  Given the same inputs its integer results are what the kernels
  must produce; its float results differ from theirs only where `exp` does;
* the float64 form of decode and softmax: the value both f32 results are judged against.

No torch in the arithmetic.  Shapes: one image at a time.
"""
import math

import numpy as np

F = np.float32
U = 2.0 ** -23                                   # the unit of error: one part in 2^23 of the magnitude
SCALE_CLAMP = F(math.log(1000.0 / 16.0))         # Box2BoxTransform's clamp as the kernels get it: rounded to f32
NMS_SLOT = 1024
SIZES = (32, 64, 128, 256, 512)
STRIDES = (4, 8, 16, 32, 64)
RATIOS = (0.5, 1.0, 2.0)


def canon(x):
    """-0.0 -> +0.0 (the two zeros are one score)."""
    x = np.asarray(x, F)
    return np.where(x == 0, F(0), x)


def stable_topk(scores, k):
    """Indices of the k largest, score descending, ties by ascending index."""
    return np.argsort(-canon(scores), kind="stable")[:k]


def sort_key(score, idx):
    """The u64 list key of apse_rpn_select (include/apse_hip.h) for f32 scores and indices."""
    u = canon(score).view(np.uint32)
    m = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ((~m).astype(np.uint64) << np.uint64(32)) | np.asarray(idx).astype(np.uint64)


def key_parts(keys):
    """(score as f32, index) of u64 list keys."""
    keys = np.asarray(keys, np.uint64)
    m = ~(keys >> np.uint64(32)).astype(np.uint32)
    u = np.where(m & np.uint32(0x80000000), m & np.uint32(0x7fffffff), ~m)
    return u.astype(np.uint32).view(F), (keys & np.uint64(0xffffffff)).astype(np.int64)


def cell_anchors(sizes, ratios=RATIOS):
    """DefaultAnchorGenerator.generate_cell_anchors: sizes outer, ratios inner; doubles, then f32."""
    out = []
    for s in sizes:
        area = float(s) * float(s)
        for r in ratios:
            w = math.sqrt(area / r)
            h = r * w
            out.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    return np.asarray(out, np.float64).astype(F)


def anchors_of(idx, W, stride, base):
    """Anchor boxes (f32) of flat indices e = (y * W + x) * A + a."""
    idx = np.asarray(idx, np.int64)
    A = base.shape[0]
    pix, an = idx // A, idx % A
    y, x = pix // W, pix % W
    sx, sy = (x * stride).astype(F), (y * stride).astype(F)
    b = base[an]
    return np.stack([sx + b[:, 0], sy + b[:, 1], sx + b[:, 2], sy + b[:, 3]], axis=1), pix, an


def _clip(v, hi, dt):
    return np.minimum(np.maximum(v, dt(0)), dt(hi))


def decode32(boxes, deltas, weights, img_h, img_w):
    """apply_deltas + clip + nonempty, each step rounded to f32.  Returns (boxes [n, 4], nonempty [n])."""
    b, d = np.asarray(boxes, F), np.asarray(deltas, F)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cx, cy = b[:, 0] + F(0.5) * w, b[:, 1] + F(0.5) * h
    dx, dy = d[:, 0] / F(weights[0]), d[:, 1] / F(weights[1])
    dw, dh = d[:, 2] / F(weights[2]), d[:, 3] / F(weights[3])
    dw = np.where(dw > SCALE_CLAMP, SCALE_CLAMP, dw)
    dh = np.where(dh > SCALE_CLAMP, SCALE_CLAMP, dh)
    pcx, pcy = dx * w + cx, dy * h + cy
    with np.errstate(over="ignore"):
        pw, ph = np.exp(dw).astype(F) * w, np.exp(dh).astype(F) * h
    x0, y0 = pcx - F(0.5) * pw, pcy - F(0.5) * ph
    x1, y1 = pcx + F(0.5) * pw, pcy + F(0.5) * ph
    x0, x1 = _clip(x0, img_w, F), _clip(x1, img_w, F)
    y0, y1 = _clip(y0, img_h, F), _clip(y1, img_h, F)
    out = np.stack([x0, y0, x1, y1], axis=1).astype(F)
    return out, ((x1 - x0) > 0) & ((y1 - y0) > 0)


def decode64(boxes, deltas, weights, img_h, img_w):
    """The same in float64 from the same f32 inputs.  Returns (clipped boxes [n, 4], magnitude [n, 4], margin [n]): the
    magnitude of a coordinate is |centre| + half the size before the clip, the scale of its f32 rounding error; the margin
    says how far the box is from the nonempty / empty border, in units of that error (positive: nonempty).  A box is nonempty
    when x1 > x0, x1 > 0 and x0 < width before the clip, and the same in y: the margin is the least of the six."""
    b, d = np.asarray(boxes, F).astype(np.float64), np.asarray(deltas, F).astype(np.float64)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cx, cy = b[:, 0] + 0.5 * w, b[:, 1] + 0.5 * h
    dx, dy = d[:, 0] / float(weights[0]), d[:, 1] / float(weights[1])
    dw = np.minimum(d[:, 2] / float(weights[2]), float(SCALE_CLAMP))
    dh = np.minimum(d[:, 3] / float(weights[3]), float(SCALE_CLAMP))
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    raw = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], axis=1)
    hi = np.asarray([img_w, img_h, img_w, img_h], np.float64)
    mx, my = np.abs(pcx) + 0.5 * pw, np.abs(pcy) + 0.5 * ph
    with np.errstate(divide="ignore", invalid="ignore"):
        gx = np.minimum(np.minimum(raw[:, 2] - raw[:, 0], raw[:, 2]), img_w - raw[:, 0]) / (U * mx)
        gy = np.minimum(np.minimum(raw[:, 3] - raw[:, 1], raw[:, 3]), img_h - raw[:, 1]) / (U * my)
    return np.minimum(np.maximum(raw, 0.0), hi), np.stack([mx, my, mx, my], axis=1), np.minimum(gx, gy)


def units(got, ref64, scale):
    """Worst |got - ref| in units of 2^-23 * scale (0 where both are equal, scale 0 included)."""
    err = np.abs(np.asarray(got, np.float64) - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(err == 0, 0.0, err / (U * scale))
    return float(u.max()) if u.size else 0.0


def softmax32(logits, wide):
    """Probabilities [n, K + 1] in f32.  Narrow: the sum runs over the classes in order.  Wide: lane l adds logits l and
    l + 64, then a xor butterfly over the 64 lanes (32, 16, .. 1)."""
    lg = np.asarray(logits, F)
    n, K1 = lg.shape
    mx = lg.max(axis=1, keepdims=True)
    ex = np.exp(lg - mx).astype(F)
    if not wide:
        s = np.zeros(n, F)
        for k in range(K1):
            s = s + ex[:, k]
    else:
        pad = np.zeros((n, 128), F)
        pad[:, :K1] = ex
        lane = pad[:, :64] + pad[:, 64:]
        ids = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[:, ids ^ o]
        s = lane[:, 0]
    return (ex / s[:, None]).astype(F)


def softmax64(logits):
    lg = np.asarray(logits, F).astype(np.float64)
    ex = np.exp(lg - lg.max(axis=1, keepdims=True))
    return ex / ex.sum(axis=1, keepdims=True)


def max_coord(boxes, valid):
    """The running max of batched_nms over the valid boxes (coordinates are >= 0 after the clip; 0 when none is valid)."""
    v = np.asarray(valid, bool)
    return F(np.asarray(boxes, F)[v].max()) if v.any() else F(0)


def nms_sorted32(b, thr, stop=None):
    """Greedy NMS over boxes [n, 4] already in processing order; `iou > thr` suppresses.  Positions kept, in order; stops once
    `stop` are kept."""
    n = b.shape[0]
    x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = (x1 - x0) * (y1 - y0)
    dead = np.zeros(n, bool)
    keep = []
    thr = F(thr)
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        if stop is not None and len(keep) >= stop:
            break
        r = slice(i + 1, n)
        ww = np.maximum(F(0), np.minimum(x1[i], x1[r]) - np.maximum(x0[i], x0[r]))
        hh = np.maximum(F(0), np.minimum(y1[i], y1[r]) - np.maximum(y0[i], y0[r]))
        inter = ww * hh
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (area[i] + area[r] - inter)
        dead[r] |= ovr > thr
    return np.asarray(keep, np.int64)


def batched_nms32(boxes, scores, valid, cat, thr):
    """Per-category NMS of the valid entries: a category's boxes are shifted by cat * (max + 1) in f32 and processed by (score
    descending, entry ascending).  `cat`: category number per entry.  Returns the kept entries of every category, a dict."""
    boxes, scores = np.asarray(boxes, F), canon(scores)
    valid, cat = np.asarray(valid, bool), np.asarray(cat, np.int64)
    m1 = max_coord(boxes, valid) + F(1)
    out = {}
    for c in np.unique(cat[valid]):
        e = np.nonzero(valid & (cat == c))[0]
        e = e[np.argsort(-scores[e], kind="stable")][:NMS_SLOT]
        off = F(c) * m1
        out[int(c)] = e[nms_sorted32(boxes[e] + off, thr)]
    return out


def rank32(boxes, scores, kept, topk):
    """Merge of the kept lists by (score descending, entry ascending), first topk.  Returns (boxes [topk, 4], scores, entry,
    count): zeros and entry -1 past the count."""
    e = np.concatenate([v for v in kept.values()] + [np.zeros(0, np.int64)]).astype(np.int64)
    e = np.sort(e)
    e = e[np.argsort(-canon(np.asarray(scores, F)[e]), kind="stable")][:topk]
    ob, os_, oe = np.zeros((topk, 4), F), np.zeros(topk, F), np.full(topk, -1, np.int32)
    ob[:len(e)], os_[:len(e)], oe[:len(e)] = np.asarray(boxes, F)[e], np.asarray(scores, F)[e], e
    return ob, os_, oe, len(e)


def level_categories(level_mask, pre_topk, consecutive=True):
    """Category number of each of the 5 * pre_topk RPN entries: the rank of the entry's level among the levels present
    (detectron2 numbers the levels it is given), or level - first level."""
    first = min(l for l in range(5) if (level_mask >> l) & 1)
    num = [bin(level_mask & ((1 << l) - 1)).count("1") if consecutive else l - first for l in range(5)]
    return np.repeat(np.asarray(num, np.int64), pre_topk)


def pack(det_boxes, det_scores, det_entry, det_cnt, K):
    """pack_detections on [B][KD] arrays: dict of the packed arrays, total and offsets."""
    B, KD = det_entry.shape
    off = np.concatenate([[0], np.cumsum(det_cnt)]).astype(np.int32)
    sel = [(b, k) for b in range(B) for k in range(int(det_cnt[b]))]
    bi = np.asarray([s[0] for s in sel], np.int64)
    ki = np.asarray([s[1] for s in sel], np.int64)
    e = det_entry[bi, ki].astype(np.int64)
    return dict(boxes=det_boxes[bi, ki].reshape(-1, 4), scores=det_scores[bi, ki], cls=(e % K).astype(np.int32),
                roi=(e // K).astype(np.int32), img=bi.astype(np.int32), total=int(off[-1]), offset=off)


# ------------------------------------------------------------------------------------------------ whole stages, one image
def rpn_level_decode(head, idx, level, W, img_h, img_w, f64=False):
    """Decode of the anchors `idx` of one FPN level from its head [H*W, ld] (objectness 0..2, deltas 3..14)."""
    anc, pix, an = anchors_of(idx, W, STRIDES[level], cell_anchors([SIZES[level]]))
    d = np.stack([head[pix, 3 + 4 * an + j] for j in range(4)], axis=1)
    return (decode64 if f64 else decode32)(anc, d, (1, 1, 1, 1), img_h, img_w)


def rpn_select(heads, Ws, img_h, img_w, pre, post, thr, level_mask=31, consecutive=True):
    """The FPN selection of one image, f32 restatement.  heads[l]: [H*W, ld]."""
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
    kept = batched_nms32(boxes, scores, valid, level_categories(level_mask, pre, consecutive), thr)
    pb, ps, pe, cnt = rank32(boxes, scores, kept, post)
    return dict(keys=keys, dec_boxes=boxes, dec_scores=scores, dec_valid=valid, props=pb, prop_scores=ps, prop_entry=pe, count=cnt)


def c4_decode(head, idx, W, img_h, img_w, f64=False):
    anc, pix, an = anchors_of(idx, W, 16, cell_anchors(SIZES))
    d = np.stack([head[pix, 15 + 4 * an + j] for j in range(4)], axis=1)
    return (decode64 if f64 else decode32)(anc, d, (1, 1, 1, 1), img_h, img_w)


def c4_nms(boxes, scores, valid, thr, post):
    """Long single-category NMS over the decoded list (already in processing order), keep[:post]."""
    e = np.nonzero(np.asarray(valid, bool))[0]
    e = e[nms_sorted32(np.asarray(boxes, F)[e], thr, stop=post)]
    ob, os_, oe = np.zeros((post, 4), F), np.zeros(post, F), np.full(post, -1, np.int32)
    ob[:len(e)], os_[:len(e)], oe[:len(e)] = boxes[e], scores[e], e
    return ob, os_, oe, len(e)


def c4_select(head, W, img_h, img_w, pre, post, thr):
    """The C4 selection of one image.  head: [H*W, 80]."""
    logit = np.ascontiguousarray(head[:, :15]).reshape(-1)
    idx = stable_topk(logit, pre)
    boxes, scores, valid = np.zeros((pre, 4), F), np.zeros(pre, F), np.zeros(pre, bool)
    b, ok = c4_decode(head, idx, W, img_h, img_w)
    boxes[:len(idx)], scores[:len(idx)], valid[:len(idx)] = b, canon(logit[idx]), ok
    pb, ps, pe, cnt = c4_nms(boxes, scores, valid, thr, post)
    return dict(idx=idx, dec_boxes=boxes, dec_scores=scores, dec_valid=valid, props=pb, prop_scores=ps, prop_entry=pe, count=cnt)


BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def box_candidates(pred, K, props, cnt, img_h, img_w, thresh, wide=False, f64=False):
    """Softmax, per-class decode, clip and score filter of one image.  pred [P, ld], props [P, 4].  Returns probs [P, K + 1],
    boxes [P * K, 4], valid [P * K] and, in the float64 form, the coordinate magnitudes."""
    P = props.shape[0]
    probs = softmax64(pred[:, :K + 1]) if f64 else softmax32(pred[:, :K + 1], wide)
    d = np.ascontiguousarray(pred[:, K + 1:5 * K + 1]).reshape(P * K, 4)
    pb = np.repeat(np.asarray(props, F), K, axis=0)
    live = np.repeat(np.arange(P) < cnt, K)
    if f64:
        boxes, mag, _ = decode64(pb, d, BOX_WEIGHTS, img_h, img_w)
        return probs, boxes, live & (probs[:, :K].reshape(-1) > float(F(thresh))), mag
    boxes, _ = decode32(pb, d, BOX_WEIGHTS, img_h, img_w)
    return probs, boxes, live & (probs[:, :K].reshape(-1) > F(thresh))


def box_nms_rank(cand_boxes, cand_scores, cand_valid, K, thr, dets):
    """Per-class NMS and the top `dets` of one image's candidates (entry = roi * K + class)."""
    kept = batched_nms32(cand_boxes, cand_scores, cand_valid, np.arange(len(cand_scores)) % K, thr)
    return rank32(cand_boxes, cand_scores, kept, dets)


# ------------------------------------------------------------------------------------------------ seeded inputs of the tests
# (shared by test_select_ref.py, which checks what they are meant to contain, and test_gpu_select_ops.py)
FPN_HW = ((152, 144), (76, 72), (38, 36), (19, 18), (10, 9))      # a 608 x 576 image
FPN_IMG = (608, 576)
FPN_LD = 16


def _logits(rng, n, kind):
    x = rng.standard_normal(n).astype(F)
    if kind == "quant16":
        return (np.clip(np.round(x * F(3)), -8, 7) / F(4)).astype(F)          # 16 distinct values
    if kind == "equal":
        return np.full(n, F(1.25))
    if kind == "zeros":
        u = rng.random(n)
        z = np.where(rng.random(n) < 0.5, F(-0.0), F(0.0)).astype(F)
        return np.where(u < 0.005, np.abs(x) + F(0.5), np.where(u < 0.6, z, -np.abs(x) - F(0.5))).astype(F)
    if kind == "inf":
        u = rng.random(n)
        return np.where(u < 0.002, F(np.inf), np.where(u < 0.3, F(-np.inf), x)).astype(F)
    return x


def fpn_heads(seed, kind="random", exact=False, sigma=0.3):
    """Five heads [H*W, 16] of one image.  exact: dw = dh = 0 (every decode step is then exact IEEE arithmetic)."""
    rng = np.random.default_rng(seed)
    heads = []
    for (H, W) in FPN_HW:
        h = np.zeros((H * W, FPN_LD), F)
        h[:, :3] = _logits(rng, H * W * 3, kind).reshape(H * W, 3)
        h[:, 3:15] = (rng.standard_normal((H * W, 12)) * sigma).astype(F)
        if exact:
            h[:, 5:15:4] = 0
            h[:, 6:15:4] = 0
        h[:, 15] = F(777.0)                                   # padding column: never read
        heads.append(h)
    return heads


def set_anchor(head, e, A, logit=None, d=None):
    """Writes the logit and / or the four deltas of anchor e of a head with A anchors per cell."""
    pix, an = e // A, e % A
    if logit is not None:
        head[pix, an] = F(logit)
    if d is not None:
        head[pix, A + 4 * an:A + 4 * an + 4] = np.asarray(d, F)


def sliver_dx(anchor, img_w):
    """dx (with dw = 0) for which the decoded x0 is the last f32 below img_w: the box clips to a one-ulp sliver."""
    t = np.nextafter(F(img_w), F(0))
    w = anchor[2] - anchor[0]
    cx = anchor[0] + F(0.5) * w
    dx = F((t + F(0.5) * w - cx) / w)
    cands = [dx]
    lo = hi = dx
    for _ in range(64):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        cands += [lo, hi]
    for c in cands:
        if (c * w + cx) - F(0.5) * w == t:
            return F(c)
    raise AssertionError("no dx gives the sliver for this anchor")


def fpn_edge_heads(seed, clamp_value=10.0):
    """Random exact-arithmetic heads with crafted anchors on top of level 1's list (logits 60 ..): two clamped sizes, four
    boxes wholly outside (left, right, top, bottom) and a one-ulp sliver at the right edge.  Returns (heads, crafted): crafted
    maps a name to (level, anchor, expected nonempty flag)."""
    heads = fpn_heads(seed, "random", exact=True)
    l, (H, W) = 1, FPN_HW[1]
    base = cell_anchors([SIZES[l]])
    crafted = {}
    e0 = ((H // 2) * W + W // 2) * 3
    # the clamped sizes are 62.5 anchors wide: 30 anchors to the right (down) the box's near edge is inside the image
    spec = [("clamp_w", e0 + 1, [30, 0, clamp_value, 0], True), ("clamp_h", e0 + 4, [0, 30, 0, clamp_value], True),
            ("left", e0 + 7, [-100, 0, 0, 0], False), ("right", e0 + 10, [100, 0, 0, 0], False),
            ("top", e0 + 13, [0, -100, 0, 0], False), ("bottom", e0 + 16, [0, 100, 0, 0], False)]
    for i, (name, e, d, ok) in enumerate(spec):
        set_anchor(heads[l], e, 3, 60 + i, d)
        crafted[name] = (l, e, ok)
    e = ((H // 2) * W + W - 2) * 3 + 1                         # a square anchor near the right edge
    anc, _, _ = anchors_of([e], W, STRIDES[l], base)
    set_anchor(heads[l], e, 3, 70, [sliver_dx(anc[0], FPN_IMG[1]), 0, 0, 0])
    crafted["sliver"] = (l, e, True)
    return heads, crafted


def fpn_all_invalid(heads, levels):
    """Every box of the given levels moved wholly to the right of the image."""
    for l in levels:
        heads[l][:, 3:15] = 0
        heads[l][:, 3:15:4] = F(100.0)
    return heads


def iou32(a, b):
    """IoU of box rows a against b in the kernels' f32 steps."""
    ww = np.maximum(F(0), np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]))
    hh = np.maximum(F(0), np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]))
    inter = ww * hh
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)


def mask_flip_heads(seed=1000, thr=0.7, trials=20000):
    """Exact-arithmetic heads for level mask 0b10101 whose kept set differs between consecutive category numbers and
    level - first level: the two best anchors of level 2 (square, neighbouring cells) overlap with an IoU so close to the
    threshold that the f32 rounding of the shifted coordinates decides, found by a seeded search over the second one's dx.
    Level 2 is category 1 of the levels present and category 2 counted from the first level."""
    img_h, img_w = FPN_IMG
    heads = fpn_heads(seed, "random", exact=True)
    l, (H, W) = 2, FPN_HW[2]
    eA = ((H // 2) * W + W // 2) * 3 + 1
    eB = eA + 3
    set_anchor(heads[l], eA, 3, 50, [0, 0, 0, 0])
    set_anchor(heads[l], eB, 3, 49, [0, 0, 0, 0])
    base = rpn_select(heads, [w for _, w in FPN_HW], img_h, img_w, 1000, 1000, thr, 0b10101)
    m1 = max_coord(base["dec_boxes"], base["dec_valid"]) + F(1)
    anc, _, _ = anchors_of([eA, eB], W, STRIDES[l], cell_anchors([SIZES[l]]))
    w = float(anc[0, 2] - anc[0, 0])
    rng = np.random.default_rng(seed)
    shift = w * (1 - thr) / (1 + thr)                             # equal boxes this far apart have an IoU of thr
    dA = np.asarray([rng.uniform(-0.3, 0.0), rng.uniform(-0.2, 0.2), 0, 0], F)
    dxB = (float(dA[0]) + (shift - STRIDES[l]) / w + rng.uniform(-2e-4, 2e-4, trials)).astype(F)
    zeros = np.zeros(trials, F)
    a, _ = decode32(np.repeat(anc[:1], trials, 0), np.repeat(dA[None], trials, 0), (1, 1, 1, 1), img_h, img_w)
    b, _ = decode32(np.repeat(anc[1:], trials, 0), np.stack([dxB, zeros + dA[1], zeros, zeros], 1), (1, 1, 1, 1), img_h, img_w)
    one, two = iou32(a + F(1) * m1, b + F(1) * m1) > F(thr), iou32(a + F(2) * m1, b + F(2) * m1) > F(thr)
    hit = np.nonzero(one != two)[0]
    assert hit.size, "no dx separates the two numberings"
    set_anchor(heads[l], eA, 3, 50, dA)
    set_anchor(heads[l], eB, 3, 49, [dxB[hit[0]], dA[1], 0, 0])
    return heads, eA, eB


def box_inputs(seed, B, P, K, ld, img=FPN_IMG, logit_scale=2.0):
    """pred [B, P, ld] and props [B, P, 4] of a box-inference call."""
    rng = np.random.default_rng(seed)
    pred = np.full((B, P, ld), F(555.0))
    pred[:, :, :K + 1] = (rng.standard_normal((B, P, K + 1)) * logit_scale).astype(F)
    pred[:, :, K + 1:5 * K + 1] = rng.standard_normal((B, P, 4 * K)).astype(F)
    cx, cy = rng.random((B, P)) * img[1], rng.random((B, P)) * img[0]
    w, h = rng.random((B, P)) * 200 + 4, rng.random((B, P)) * 200 + 4
    props = np.stack([np.clip(cx - w / 2, 0, img[1]), np.clip(cy - h / 2, 0, img[0]), np.clip(cx + w / 2, 0, img[1]),
                      np.clip(cy + h / 2, 0, img[0])], axis=2).astype(F)
    return pred, props


def c4_head(seed, H, W, kind="random", exact=False, sigma=0.3):
    rng = np.random.default_rng(seed)
    h = np.zeros((H * W, 80), F)
    h[:, :15] = _logits(rng, H * W * 15, kind).reshape(H * W, 15)
    h[:, 15:75] = (rng.standard_normal((H * W, 60)) * sigma).astype(F)
    if exact:
        h[:, 17:75:4] = 0
        h[:, 18:75:4] = 0
    h[:, 75:] = F(777.0)
    return h


# ------------------------------------------------------------------------------------------------ judging a result
def tolerance(units32):
    """Allowed units of a device result: twice what the f32 restatement itself is off the float64 form, at least 4."""
    return max(4.0, 2.0 * units32)


def near_empty(margin, tol):
    """Entries whose float64 box is within `tol` units (per coordinate, two coordinates) of the nonempty / empty border:
    their flag may go either way in f32."""
    return ~(np.abs(margin) > 2 * tol)


def near_score(p64, thresh, tol):
    return np.abs(p64 - float(F(thresh))) <= tol * U * p64


def tie_run(logits, k, chunk=4096):
    """The run of equal scores around rank k of a level: (selected, unselected, chunks) -- how many of the run are inside
    and outside the top k, and how many chunks of the tournament it touches."""
    s = canon(logits)
    order = np.argsort(-s, kind="stable")
    if k >= len(order):
        return 0, 0, 0
    v = s[order[k - 1]]
    run = np.nonzero(s == v)[0]
    inside = int((s[order[:k]] == v).sum())
    return inside, len(run) - inside, len(np.unique(run // chunk))
