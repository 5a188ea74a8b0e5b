"""Host side of RPN-head training: the restatement (tests/rpn_train_ref.py) against the oracle's anchors, against a literal torch
transcription of detectron2's pairwise_iou / Matcher on hand-made cases and against torch's own loss functions; checkpoint merging,
the C4 refusal and the ABI names -- no GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"apse_rpn_train_workspace_bytes", "apse_rpn_anchor_labels", "apse_rpn_patches", "apse_rpn_loss_forward",
               "apse_rpn_loss_backward"}


# ------------------------------------------------------------------------------------------------ anchors
def test_anchors_equal_the_oracle():
    from oracle import ops
    shapes = R.level_shapes(256, 448)
    assert shapes == [(64, 112), (32, 56), (16, 28), (8, 14), (4, 7)]
    boxes, level, y, x, slot = R.anchors(shapes)
    want = torch.cat([ops.grid_anchors(h, w, R.STRIDES[l], R.SIZES[l]) for l, (h, w) in enumerate(shapes)])
    assert boxes.dtype == torch.float32 and np.array_equal(boxes.numpy(), want.numpy())
    for l in range(5):
        assert np.array_equal(R.cell_anchors(R.SIZES[l]).numpy(), ops.cell_anchors(R.SIZES[l]).numpy())
    # the index order: (level, y, x, a)
    i = 3 * (64 * 112) + 3 * (5 * 56 + 7) + 2
    assert (int(level[i]), int(y[i]), int(x[i]), int(slot[i])) == (1, 5, 7, 2)
    assert R.level_shapes(40, 72)[4] == (1, 2)                          # the 1-row p6


# ------------------------------------------------------------------------------------------------ labelling
def d2_pairwise_iou(boxes1, boxes2):
    """detectron2.structures.boxes.pairwise_iou (0.1.2), literally."""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    width_height = torch.min(boxes1[:, None, 2:], boxes2[:, 2:]) - torch.max(boxes1[:, None, :2], boxes2[:, :2])
    width_height.clamp_(min=0)
    inter = width_height.prod(dim=2)
    del width_height
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


def d2_matcher(match_quality_matrix, thresholds=(0.3, 0.7), labels=(0, -1, 1), allow_low_quality_matches=True):
    """detectron2.modeling.matcher.Matcher.__call__ + set_low_quality_matches_ (0.1.2), literally."""
    thresholds = [-float("inf")] + list(thresholds) + [float("inf")]
    if match_quality_matrix.numel() == 0:
        default_matches = match_quality_matrix.new_full((match_quality_matrix.size(1),), 0, dtype=torch.int64)
        default_match_labels = match_quality_matrix.new_full((match_quality_matrix.size(1),), labels[0], dtype=torch.int8)
        return default_matches, default_match_labels
    matched_vals, matches = match_quality_matrix.max(dim=0)
    match_labels = matches.new_full(matches.size(), 1, dtype=torch.int8)
    for (l, low, high) in zip(labels, thresholds[:-1], thresholds[1:]):
        low_high = (matched_vals >= low) & (matched_vals < high)
        match_labels[low_high] = l
    if allow_low_quality_matches:
        highest_quality_foreach_gt, _ = match_quality_matrix.max(dim=1)
        gt_pred_pairs_of_highest_quality = torch.nonzero(match_quality_matrix == highest_quality_foreach_gt[:, None])
        pred_inds_to_update = gt_pred_pairs_of_highest_quality[:, 1]
        match_labels[pred_inds_to_update] = 1
    return matches, match_labels


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_labelling_equals_the_transcription(name):
    gts = R.hand_cases()[name]
    anc = R.anchors(R.level_shapes(256, 448))[0]
    labels, idx, iou = R.label_anchors(anc, gts)
    q = d2_pairwise_iou(gts, anc)
    matches, match_labels = d2_matcher(q)
    assert np.array_equal(labels.numpy(), match_labels.numpy().astype(np.int64))
    if gts.shape[0]:
        assert np.array_equal(iou.numpy(), q.max(dim=0).values.numpy())
        assert np.array_equal(R.pairwise_iou(gts, anc).numpy(), q.numpy())
        # the matched index is AN argmax, and the lowest one
        cols = torch.arange(anc.shape[0])
        assert bool((q[idx, cols] == q.max(dim=0).values).all()) and bool((q[matches, cols] == q[idx, cols]).all())
        assert bool((idx <= matches).all())
    else:
        assert int(labels.abs().max()) == 0 and int(idx.max()) == 0 and float(iou.max()) == 0.0
    if name == "two_anchor_tie":
        best = q[0].max()
        assert float(best) == float(torch.tensor(870.0) / torch.tensor(1054.0))
        tied = torch.nonzero(q[0] == best).squeeze(1)
        assert tied.numel() == 2 and labels[tied].tolist() == [1, 1]
        assert int((labels == 1).sum()) == 2
    if name == "four_anchor_tie":
        assert float(q.max()) == 0.5625 and int((labels == 1).sum()) == 4 and int((q[0] == 0.5625).sum()) == 4
    if name == "no_overlap":
        assert float(q.max()) == 0.0 and bool((labels == 1).all())     # the literal rule: every anchor equals the maximum 0
    if name == "larger_than_image":
        assert int((labels == 1).sum()) >= 1 and int((labels == -1).sum()) >= 1


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("S", [1, 64, 257])
def test_loss_equals_torch(S):
    """The restated loss against F.binary_cross_entropy_with_logits(reduction="sum") plus L1 on torch's own deltas: the float32
    restatement is judged against float64 with torch's float32 result as the yardstick (the arbiter)."""
    g = torch.Generator().manual_seed(S)
    slots, labels, anc, gts = R.sample_rows(S, S + 1)
    logits = torch.randn(S, 3, generator=g) * 3
    deltas = torch.randn(S, 12, generator=g)
    norm = 256

    def torch_own(dt):
        x, d = R.own_columns(logits.to(dt), deltas.to(dt), slots)
        cls = F.binary_cross_entropy_with_logits(x, (labels > 0).to(dt), reduction="sum") / norm
        pos = labels > 0
        loc = F.l1_loss(d[pos], R.get_deltas(anc.to(dt), gts.to(dt))[pos], reduction="sum") / norm
        return torch.stack([cls, loc])
    ours = torch.stack(R.rpn_losses(logits, deltas, slots, labels, anc, gts, norm))
    ours64 = torch.stack(R.rpn_losses(logits.double(), deltas.double(), slots, labels, anc.double(), gts.double(), norm))
    t64, t32 = torch_own(torch.float64), torch_own(torch.float32)
    for j in range(2):
        eh, ef, bound, ok = R.arbiter(ours[j], t64[j], t32[j])
        assert ok, (j, eh, ef, bound)
        assert float(ours64[j]) == pytest.approx(float(t64[j]), rel=1e-13, abs=1e-300)


def test_loss_hand_case():
    logits = torch.tensor([[9.0, 0.0, 9.0], [0.0, 9.0, 9.0]], dtype=torch.float64)
    deltas = torch.full((2, 12), 7.0, dtype=torch.float64)
    deltas[0, 4:8] = torch.tensor([0.5, 0.0, 0.0, -1.0])
    slots, labels = torch.tensor([1, 0]), torch.tensor([1, 0])
    anc = torch.tensor([[0.0, 0.0, 8.0, 4.0], [0.0, 0.0, 1.0, 1.0]], dtype=torch.float64)
    gts = torch.tensor([[2.0, 1.0, 10.0, 5.0], [0.0, 0.0, 1.0, 1.0]], dtype=torch.float64)      # target (0.25, 0.25, 0, 0)
    lc, ll = R.rpn_losses(logits, deltas, slots, labels, anc, gts, 4)
    assert float(lc) == pytest.approx(2 * np.log(2.0) / 4, rel=1e-15)
    assert float(ll) == (0.25 + 0.25 + 0.0 + 1.0) / 4
    assert R.rpn_stats(logits, slots, labels) == (1, 1, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_state_dict_round_trip_and_merge():
    from apse_uav_amd.networks.rpn_head import PREFIX, RPNHead, merge_rpn_head
    from apse_uav_amd.weights import synthetic_detector_state
    det = synthetic_detector_state(0, (1, 1, 1, 1))
    head = RPNHead("cpu")
    head.load_state_dict(det)
    names = R.param_names()
    assert [k for k, _ in head.named_parameters()] == names and len(list(head.parameters())) == 6
    for k, p in head.named_parameters():
        assert p.requires_grad and p.dtype == torch.float32 and torch.equal(p.detach(), det[PREFIX + k]), k
    sd = head.state_dict()
    other = RPNHead("cpu")
    other.load_state_dict(head.state_dict(PREFIX))
    assert all(torch.equal(sd[k], other.state_dict()[k]) for k in names)
    with pytest.raises(RuntimeError):
        RPNHead("cpu").load_state_dict({k: v for k, v in sd.items() if k != "conv.bias"})
    with pytest.raises(RuntimeError):
        RPNHead("cpu").load_state_dict(dict(sd, **{"conv.bias": torch.zeros(3)}))
    changed = {k: v + 1 for k, v in sd.items()}
    merged = merge_rpn_head({"model." + k: v for k, v in det.items()}, changed)
    assert set(merged) == set(det)
    for k, v in det.items():
        if k.startswith(PREFIX):
            assert torch.equal(merged[k], v + 1), k
        else:
            assert merged[k] is v, k
    with pytest.raises(KeyError):
        merge_rpn_head(det, {k: v for k, v in sd.items() if k != "conv.bias"})
    with pytest.raises(KeyError):
        merge_rpn_head(det, dict(sd, stray=torch.zeros(1)))
    # fresh parameters: detectron2's normal(std = 0.01), biases 0
    torch.manual_seed(0)
    fresh = RPNHead("cpu").state_dict()
    assert float(fresh["conv.bias"].abs().max()) == 0.0 and 0.009 < float(fresh["conv.weight"].std()) < 0.011


def test_c4_is_refused():
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks.rpn_head import RPNHead
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    with pytest.raises(NotImplementedError):
        RPNHead.from_cfg(setup_cfg(num_classes=4, arch="C4"))
    assert isinstance(RPNHead.from_cfg(setup_cfg(num_classes=4), "cpu"), RPNHead)
    c4 = TrackRCNN(setup_cfg(num_classes=4, arch="C4"))
    with pytest.raises(NotImplementedError):
        c4.rpn_patches(np.zeros(1, np.int32))
    with pytest.raises(NotImplementedError):
        c4.rpn_anchor_targets(np.zeros((1, 4), np.float32))


def test_new_entries_are_declared_and_exported():
    from apse_uav_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apse_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(apse_[a-z0-9_]+)\s*\(", text))
    assert NEW_ENTRIES <= declared and NEW_ENTRIES <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_ENTRIES)
    # the limits, on the host: 0 outside them
    assert lib.apse_rpn_train_workspace_bytes(28644, 65, 1024) >= 28 * 65 * 4 + 65 * 4
    assert lib.apse_rpn_train_workspace_bytes(0, 0, 1024) >= 1024 * 6 * 8
    assert lib.apse_rpn_train_workspace_bytes(0, 0, 0) > 0
    assert lib.apse_rpn_train_workspace_bytes((1 << 22) + 1, 0, 0) == 0
    assert lib.apse_rpn_train_workspace_bytes(1, 4097, 0) == 0
    assert lib.apse_rpn_train_workspace_bytes(1, 1, (1 << 20) + 1) == 0
