"""torch CPU restatement of RPN-head training (detectron2 0.1.2 / fvcore: DefaultAnchorGenerator, pairwise_iou,
Matcher([0.3, 0.7], [0, -1, 1], allow_low_quality_matches=True), Box2BoxTransform(1, 1, 1, 1).get_deltas, smooth_l1_loss,
RPNOutputs.losses, StandardRPNHead on gathered patches), computed in the dtype of its inputs: the tests run it in float32 (op for op
what csrc/rpn_train.hip computes) and in float64 and judge the HIP result with the arbiter of tests/mask_train_ref.py.
"""
import math

import torch
import torch.nn.functional as F

from mask_train_ref import arbiter  # noqa: F401  (the tests take it from here)

NAMES = ["conv", "objectness_logits", "anchor_deltas"]
SIZES = (32, 64, 128, 256, 512)
STRIDES = (4, 8, 16, 32, 64)
RATIOS = (0.5, 1.0, 2.0)
PATCH = 2304


def param_names():
    return [n + s for n in NAMES for s in (".weight", ".bias")]


def level_shapes(image_h, image_w):
    """(H, W) of p2 .. p6 for a resized image: padded to a multiple of 32, strides 4 .. 32, p6 = p5 subsampled by 2."""
    ph, pw = (image_h + 31) // 32 * 32, (image_w + 31) // 32 * 32
    out = [(ph // s, pw // s) for s in STRIDES[:4]]
    out.append(((out[3][0] - 1) // 2 + 1, (out[3][1] - 1) // 2 + 1))
    return out


# ---- anchors
def cell_anchors(size):
    """generate_cell_anchors: Python doubles, rounded to f32 once."""
    out = []
    area = float(size) ** 2.0
    for ar in RATIOS:
        w = math.sqrt(area / ar)
        h = ar * w
        out.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    return torch.tensor(out, dtype=torch.float32)


def anchors(shapes):
    """f32 [A][4] in (level, y, x, a) order, as the kernels generate them: (float)(x * stride) + base in f32.  -> (boxes, level [A],
    y [A], x [A], slot [A])."""
    boxes, lv, ys, xs, sl = [], [], [], [], []
    for l, (H, W) in enumerate(shapes):
        base = cell_anchors(SIZES[l])
        y, x, a = torch.meshgrid(torch.arange(H), torch.arange(W), torch.arange(3), indexing="ij")
        y, x, a = y.reshape(-1), x.reshape(-1), a.reshape(-1)
        sx, sy = (x * STRIDES[l]).float(), (y * STRIDES[l]).float()
        boxes.append(torch.stack((sx, sy, sx, sy), dim=1) + base[a])
        lv.append(torch.full_like(y, l)); ys.append(y); xs.append(x); sl.append(a)
    return torch.cat(boxes), torch.cat(lv), torch.cat(ys), torch.cat(xs), torch.cat(sl)


# ---- labelling
def pairwise_iou(gt, anc):
    """[G][4], [A][4] -> [G][A]: inter > 0 ? inter / (area_gt + area_anchor - inter) : 0, every operation in the inputs' dtype."""
    area_g = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    area_a = (anc[:, 2] - anc[:, 0]) * (anc[:, 3] - anc[:, 1])
    w = torch.min(gt[:, None, 2], anc[None, :, 2]) - torch.max(gt[:, None, 0], anc[None, :, 0])
    h = torch.min(gt[:, None, 3], anc[None, :, 3]) - torch.max(gt[:, None, 1], anc[None, :, 1])
    inter = w.clamp(min=0) * h.clamp(min=0)
    return torch.where(inter > 0, inter / (area_g[:, None] + area_a[None, :] - inter), torch.zeros(1, dtype=inter.dtype))


def label_anchors(anc, gt, lo=0.3, hi=0.7):
    """-> (labels int64 [A] in {1, 0, -1}, matched_idx int64 [A], matched_iou [A]); ties to the lowest ground-truth index; the
    low-quality rule literally: an anchor whose IoU to a ground truth equals that ground truth's maximum gets label 1."""
    A = anc.shape[0]
    if gt.shape[0] == 0:
        return torch.zeros(A, dtype=torch.int64), torch.zeros(A, dtype=torch.int64), torch.zeros(A, dtype=anc.dtype)
    q = pairwise_iou(gt, anc)
    vals = q.max(dim=0).values
    idx = (q == vals[None, :]).to(torch.int64).argmax(dim=0)            # the first maximum
    labels = torch.zeros(A, dtype=torch.int64)
    labels[vals >= lo] = -1
    labels[vals >= hi] = 1
    best = q.max(dim=1).values
    labels[(q == best[:, None]).any(dim=0)] = 1
    return labels, idx, vals


# ---- losses
def get_deltas(src, tgt):
    """Box2BoxTransform(weights = (1, 1, 1, 1)).get_deltas."""
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tx, ty = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    return torch.stack((1.0 * (tx - sx) / sw, 1.0 * (ty - sy) / sh, 1.0 * torch.log(tw / sw), 1.0 * torch.log(th / sh)), dim=1)


def smooth_l1(x, y, beta):
    """fvcore smooth_l1_loss(reduction="sum")."""
    n = torch.abs(x - y)
    if beta < 1e-5:
        return n.sum()
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum()


def own_columns(logits, deltas, slots):
    """Column slot of logits [S][3] and columns 4 slot .. 4 slot + 3 of deltas [S][12]."""
    r = torch.arange(logits.shape[0])
    s = slots.to(torch.int64)
    return logits[r, s], deltas.reshape(-1, 3, 4)[r, s]


def rpn_losses(logits, deltas, slots, labels, anchor_boxes, gt_boxes, norm, beta=0.0):
    """RPNOutputs.losses on the sampled rows -> (loss_rpn_cls, loss_rpn_loc): sums x 1 / norm."""
    if logits.shape[0] == 0:
        return logits.sum() * 0, deltas.sum() * 0
    x, d = own_columns(logits, deltas, slots)
    y = (labels > 0).to(x.dtype)
    # max(x, 0) - x y + log1p(exp(-|x|)), written so that autograd gives sigmoid(x) - y at x = 0 too
    bce = -(y * F.logsigmoid(x) + (1 - y) * F.logsigmoid(-x)).sum()
    pos = torch.nonzero(labels > 0).squeeze(1)
    loc = smooth_l1(d[pos], get_deltas(anchor_boxes, gt_boxes)[pos], beta)
    return bce * (1.0 / norm), loc * (1.0 / norm)


def rpn_stats(logits, slots, labels):
    """num_pos, num_neg, share of positive rows with logit > 0, share of negative rows with logit < 0."""
    x = logits[torch.arange(logits.shape[0]), slots.to(torch.int64)]
    pos, neg = labels > 0, labels == 0
    npos, nneg = int(pos.sum()), int(neg.sum())
    return (npos, nneg, int((x[pos] > 0).sum()) / npos if npos else 0.0, int((x[neg] < 0).sum()) / nneg if nneg else 0.0)


# ---- the head
def seeded_state(seed):
    g = torch.Generator().manual_seed(seed)
    return {
        "conv.weight": torch.randn(256, 256, 3, 3, generator=g) * (2.0 / PATCH) ** 0.5,
        "conv.bias": torch.randn(256, generator=g) * 0.1,
        "objectness_logits.weight": torch.randn(3, 256, 1, 1, generator=g) * (1.0 / 256) ** 0.5,
        "objectness_logits.bias": torch.randn(3, generator=g) * 0.1,
        "anchor_deltas.weight": torch.randn(12, 256, 1, 1, generator=g) * (1.0 / 256) ** 0.5,
        "anchor_deltas.bias": torch.randn(12, generator=g) * 0.1,
    }


def exact_forward_state(seed):
    """box_train_ref.exact_forward_state for this head: conv weights are 0 or +-1/4 and sparse (about 32 per output), its bias
    multiples of 1/4.  With patches that are multiples of 1/2 (exact_patches) every product and partial sum up to the ReLU is a
    multiple of 1/8 far below 2^24: f32 and f64 see the SAME ReLU mask.  The two 1 x 1 layers are dense and random."""
    g = torch.Generator().manual_seed(seed)
    sd = seeded_state(seed + 1)
    keep = torch.rand(256, 256, 3, 3, generator=g) < 32.0 / PATCH
    sign = (torch.rand(256, 256, 3, 3, generator=g) < 0.5).float() * 2 - 1
    sd["conv.weight"] = keep.float() * sign * 0.25
    sd["conv.bias"] = torch.randint(-2, 3, (256,), generator=g).float() * 0.25
    return sd


def exact_patches(S, seed):
    """Patches [S][2304] that are non-negative multiples of 1/2."""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.round(torch.randn(S, PATCH, generator=g) * 2) / 2)


def head_outputs(x, p):
    """x [S][2304] in (c, kh, kw) order = [S][256][3][3]; p: dict of the 6 parameters -> (logits [S][3], deltas [S][12]): the
    StandardRPNHead layers as convolutions on the 3 x 3 window (no padding: the patch carries it)."""
    t = F.relu(F.conv2d(x.reshape(-1, 256, 3, 3), p["conv.weight"], p["conv.bias"]))
    return (F.conv2d(t, p["objectness_logits.weight"], p["objectness_logits.bias"]).flatten(1),
            F.conv2d(t, p["anchor_deltas.weight"], p["anchor_deltas.bias"]).flatten(1))


def head_step(x, sd, slots, labels, anchor_boxes, gt_boxes, norm, dtype, beta=0.0):
    """(loss_rpn_cls, loss_rpn_loc) and the 6 parameter gradients of their sum, one forward + backward in `dtype`."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    logits, deltas = head_outputs(x.to(dtype), p)
    lc, ll = rpn_losses(logits, deltas, slots, labels, anchor_boxes.to(dtype), gt_boxes.to(dtype), norm, beta)
    (lc + ll).backward()
    return (lc.detach(), ll.detach()), {k: v.grad for k, v in p.items()}


def sample_rows(S, seed, pos_share=0.5):
    """slots, labels (about pos_share positive), anchor boxes on a 1/4-pixel lattice with sides of at least 8 px, and ground truths
    that are the anchor with each coordinate moved by up to 2 px (regression targets of O(0.1), as after matching)."""
    g = torch.Generator().manual_seed(seed)
    slots = torch.randint(0, 3, (S,), generator=g)
    labels = (torch.rand(S, generator=g) < pos_share).to(torch.int64)
    xy = torch.randint(0, 1600, (S, 2), generator=g).float() / 4
    wh = torch.randint(32, 800, (S, 2), generator=g).float() / 4
    anc = torch.cat([xy, xy + wh], dim=1)
    gts = anc + torch.randint(-8, 9, (S, 4), generator=g).float() / 4
    return slots, labels, anc, gts


# ---- hand-made labelling cases on the levels of a 256 x 448 image (shared by the host and the GPU tests)
def hand_cases():
    """name -> ground truths f32 [G][4].
    two_anchor_tie  a 30 x 30 integer box centred between the p2 ratio-1 anchors at x = 100 and x = 104 (y = 100): both have
                    IoU 870 / 1054 with it and no other anchor reaches that
    four_anchor_tie a 24 x 24 box: the four p2 ratio-1 anchors that contain it tie exactly at 576 / 1024, between the two thresholds,
                    so only the low-quality rule makes them positive
    no_overlap      a ground truth that no anchor touches: its maximum is 0 and, literally, every anchor equals it
    larger_than_image, mixed (all of them with two ordinary boxes), none (G = 0)"""
    tie = [87.0, 85.0, 117.0, 115.0]
    tiny = [90.0, 90.0, 114.0, 114.0]
    far = [5000.0, 5000.0, 5010.0, 5010.0]
    big = [-100.0, -100.0, 600.0, 400.0]
    cases = {
        "two_anchor_tie": [tie],
        "four_anchor_tie": [tiny],
        "no_overlap": [far],
        "larger_than_image": [big],
        "mixed": [[40.0, 30.0, 200.0, 170.0], tie, tiny, big, [301.25, 99.5, 352.75, 163.0]],
        "none": [],
    }
    return {k: torch.tensor(v, dtype=torch.float32).reshape(-1, 4) for k, v in cases.items()}
