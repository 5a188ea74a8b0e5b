"""torch CPU restatement of box-head training (detectron2 0.1.2 / fvcore: pairwise_iou, Matcher, ROIHeads._sample_proposals,
subsample_labels, Box2BoxTransform.get_deltas, smooth_l1_loss, FastRCNNOutputs.losses, FastRCNNConvFCHead with two FC layers,
FastRCNNOutputLayers), computed in the dtype of its inputs: the tests run it in float64 and in float32 and judge the HIP result with
the arbiter of tests/mask_train_ref.py.
"""
import torch
import torch.nn.functional as F

from mask_train_ref import arbiter  # noqa: F401  (the tests take it from here)

NAMES = ["box_head.fc1", "box_head.fc2", "box_predictor.cls_score", "box_predictor.bbox_pred"]
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def param_names():
    return [n + s for n in NAMES for s in (".weight", ".bias")]


# ---- matching
def pairwise_iou(boxes1, boxes2):
    """detectron2.structures.pairwise_iou: [N][4], [M][4] -> [N][M]."""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    wh = torch.min(boxes1[:, None, 2:], boxes2[:, 2:]) - torch.max(boxes1[:, None, :2], boxes2[:, :2])
    wh = wh.clamp(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


def match(proposals, gt_boxes, gt_classes, num_classes, thresh=0.5):
    """Matcher([thresh], [0, 1], allow_low_quality_matches=False) on pairwise_iou(gt, proposals) + the class assignment of
    _sample_proposals -> (matched_idx int64 [N], matched_iou [N], labels int64 [N]); ties to the lowest ground-truth index."""
    N = proposals.shape[0]
    if gt_boxes.shape[0] == 0:
        return (torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=proposals.dtype),
                torch.full((N,), num_classes, dtype=torch.int64))
    q = pairwise_iou(gt_boxes, proposals)                      # [G][N]
    vals = q.max(dim=0).values
    idx = (q == vals[None, :]).to(torch.int64).argmax(dim=0)   # the first maximum
    labels = gt_classes.to(torch.int64)[idx].clone()
    labels[vals < thresh] = num_classes
    return idx, vals, labels


def subsample_labels(labels, num_samples, positive_fraction, bg_label, generator=None):
    """detectron2.modeling.sampling.subsample_labels -> (positive indices, negative indices)."""
    positive = torch.nonzero((labels != -1) & (labels != bg_label)).squeeze(1)
    negative = torch.nonzero(labels == bg_label).squeeze(1)
    num_pos = min(positive.numel(), int(num_samples * positive_fraction))
    num_neg = min(negative.numel(), num_samples - num_pos)
    perm1 = torch.randperm(positive.numel(), generator=generator)[:num_pos]
    perm2 = torch.randperm(negative.numel(), generator=generator)[:num_neg]
    return positive[perm1], negative[perm2]


# ---- losses
def get_deltas(src, tgt, weights=WEIGHTS):
    """Box2BoxTransform.get_deltas."""
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tx, ty = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    wx, wy, ww, wh = weights
    return torch.stack((wx * (tx - sx) / sw, wy * (ty - sy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), dim=1)


def smooth_l1(x, y, beta):
    """fvcore smooth_l1_loss(reduction="sum")."""
    if beta < 1e-5:
        return torch.abs(x - y).sum()
    n = torch.abs(x - y)
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum()


def box_losses(logits, deltas, labels, prop_boxes, gt_boxes, beta=0.0, weights=WEIGHTS):
    """FastRCNNOutputs.losses (class-specific regression) -> (loss_cls, loss_box_reg)."""
    n, K = logits.shape[0], logits.shape[1] - 1
    if n == 0:
        return logits.sum() * 0, deltas.sum() * 0
    labels = labels.to(torch.int64)
    loss_cls = F.cross_entropy(logits, labels, reduction="mean")
    fg = torch.nonzero((labels >= 0) & (labels < K)).squeeze(1)
    cols = 4 * labels[fg][:, None] + torch.arange(4)
    target = get_deltas(prop_boxes, gt_boxes, weights)
    loss_box = smooth_l1(deltas[fg[:, None], cols], target[fg], beta) / n
    return loss_cls, loss_box


def box_stats(logits, labels):
    """cls_accuracy, fg_cls_accuracy, false_negative, num_fg, num_bg; argmax ties to the lowest index."""
    n, K = logits.shape[0], logits.shape[1] - 1
    labels = labels.to(torch.int64)
    mx = logits.max(dim=1, keepdim=True).values
    pred = (logits == mx).to(torch.int64).argmax(dim=1)
    fg = (labels >= 0) & (labels < K)
    nfg = int(fg.sum())
    acc = int((pred == labels).sum()) / n
    if nfg == 0:
        return acc, 0.0, 0.0, 0, n
    return acc, int((pred[fg] == labels[fg]).sum()) / nfg, int((pred[fg] == K).sum()) / nfg, nfg, n - nfg


# ---- the head
def seeded_state(K, seed):
    """Weights that keep activations O(1) through the head, biases O(0.1), on the CPU in f32."""
    g = torch.Generator().manual_seed(seed)
    return {
        "box_head.fc1.weight": torch.randn(1024, 12544, generator=g) * (2.0 / 12544) ** 0.5,
        "box_head.fc1.bias": torch.randn(1024, generator=g) * 0.1,
        "box_head.fc2.weight": torch.randn(1024, 1024, generator=g) * (2.0 / 1024) ** 0.5,
        "box_head.fc2.bias": torch.randn(1024, generator=g) * 0.1,
        "box_predictor.cls_score.weight": torch.randn(K + 1, 1024, generator=g) * (1.0 / 1024) ** 0.5,
        "box_predictor.cls_score.bias": torch.randn(K + 1, generator=g) * 0.1,
        "box_predictor.bbox_pred.weight": torch.randn(4 * K, 1024, generator=g) * (1.0 / 1024) ** 0.5,
        "box_predictor.bbox_pred.bias": torch.randn(4 * K, generator=g) * 0.1,
    }


def exact_forward_state(K, seed):
    """The construction of mask_train_ref.exact_forward_state for the box head: fc1 / fc2 weights are 0 or +-1/4 and sparse (about
    32 per row), their biases multiples of 1/4.  With RoI features that are multiples of 1/2 (exact_features) every product and
    partial sum through fc2's ReLU is a multiple of 2^-5 far below 2^24: representable in any order, so f32 and f64 see the SAME
    ReLU masks.  The two predictor layers are dense and random."""
    g = torch.Generator().manual_seed(seed)

    def sparse(shape):
        keep = torch.rand(shape, generator=g) < 32.0 / shape[1]
        sign = (torch.rand(shape, generator=g) < 0.5).float() * 2 - 1
        return keep.float() * sign * 0.25

    sd = seeded_state(K, seed + 1)
    sd["box_head.fc1.weight"] = sparse((1024, 12544))
    sd["box_head.fc1.bias"] = torch.randint(-2, 3, (1024,), generator=g).float() * 0.25
    sd["box_head.fc2.weight"] = sparse((1024, 1024))
    sd["box_head.fc2.bias"] = torch.randint(-2, 3, (1024,), generator=g).float() * 0.25
    return sd


def exact_features(n, seed):
    """RoI features [n][256][7][7] that are non-negative multiples of 1/2."""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.round(torch.randn(n, 256, 7, 7, generator=g) * 2) / 2)


def head_outputs(x, p):
    """x NCHW [n][256][7][7]; p: dict of the 8 parameters -> (logits [n][K + 1], deltas [n][4 K])."""
    h = F.relu(F.linear(torch.flatten(x, start_dim=1), p["box_head.fc1.weight"], p["box_head.fc1.bias"]))
    h = F.relu(F.linear(h, p["box_head.fc2.weight"], p["box_head.fc2.bias"]))
    return (F.linear(h, p["box_predictor.cls_score.weight"], p["box_predictor.cls_score.bias"]),
            F.linear(h, p["box_predictor.bbox_pred.weight"], p["box_predictor.bbox_pred.bias"]))


def head_step(x, sd, labels, prop_boxes, gt_boxes, dtype, beta=0.0):
    """(loss_cls, loss_box_reg) and the 8 parameter gradients of loss_cls + loss_box_reg, one forward + backward in `dtype`."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    logits, deltas = head_outputs(x.to(dtype), p)
    lc, lb = box_losses(logits, deltas, labels, prop_boxes.to(dtype), gt_boxes.to(dtype), beta)
    (lc + lb).backward()
    return (lc.detach(), lb.detach()), {k: v.grad for k, v in p.items()}


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def sample_batch(n, K, seed, fg_share=0.25, related=False):
    """Labels (about fg_share foreground, every class present when n allows), sampled boxes and matched ground truths for n rows:
    f32 boxes on a 1/4-pixel lattice with sides of at least 8 px.  related: every ground truth is its sampled box with each
    coordinate moved by up to 2 px (regression targets of O(1), as after matching); otherwise the two are independent."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.full((n,), K, dtype=torch.int64)
    fg = torch.rand(n, generator=g) < fg_share
    labels[fg] = torch.randint(0, K, (int(fg.sum()),), generator=g)

    def boxes():
        xy = torch.randint(0, 1600, (n, 2), generator=g).float() / 4
        wh = torch.randint(32, 800, (n, 2), generator=g).float() / 4
        return torch.cat([xy, xy + wh], dim=1)
    props = boxes()
    gts = props + torch.randint(-8, 9, (n, 4), generator=g).float() / 4 if related else boxes()
    return labels, props, gts
