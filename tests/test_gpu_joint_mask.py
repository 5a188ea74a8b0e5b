"""-m gpu: the mask rows of joint training (utils/joint_train.py JointTrainLoader(mask=True), tools/finetune_uav.py --mask) on small
frames with seeded synthetic weights.

* mask=False yields the two tuples of a restatement of the loader as it was before the mask rows existed, bit for bit, and
  mask=True yields the same two tuples and the same state: the mask rows draw nothing;
* the mask rows are the sampled foreground proposals in sampling order: ``mask_roi_features`` of those boxes, their labels, and the
  host path ``mask_targets`` of the matched ground truth's polygons under those boxes, byte for byte;
* annotations without polygons give no mask rows and are counted in ``last_mask_skipped``;
* a saved and restored state repeats the next batch;
* under the three-loss sum the mask head's gradients are those of MaskHead alone on the mask tuple and the RPN / box gradients
  those of the two-head sum, bit for bit; a batch without mask rows has loss_mask == 0 and zero mask gradients."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
DEV = "cuda:0"
K = 4
SEED = 1


@pytest.fixture(scope="module")
def dicts(tmp_path_factory):
    from apse_uav_amd.synthetic import synthetic_dataset
    from apse_uav_amd.utils import COCO_utils
    root = str(tmp_path_factory.mktemp("joint_mask") / "img")
    return COCO_utils.generate_coco_dataset_dictionaries(synthetic_dataset(root, 4, seed=2), root, None, None, False)


@pytest.fixture(scope="module")
def model():
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg(num_classes=K)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 192, 320
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    cfg.APSE.CONTEXT_CACHE = 4
    return TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1), num_classes=K)).model


def _loader(dicts, model, mask, ims=2):
    from apse_uav_amd.utils.joint_train import JointTrainLoader
    return JointTrainLoader(dicts, model, ims, seed=SEED, num_classes=K, mask=mask)


def _no_polygons(dicts, which):
    out = copy.deepcopy(dicts)
    for i in which:
        for a in out[i]["annotations"]:
            a["segmentation"] = []
    return out


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _restated_batch(dicts, model, ims=2):
    """One batch of the loader as it was before it had mask rows: its draws and calls, written out.  -> (rpn, box, per image
    (dictionary, box rows))."""
    from apse_uav_amd.utils.box_train import label_and_sample_proposals
    from apse_uav_amd.utils.joint_train import JointTrainLoader
    from apse_uav_amd.utils.rpn_train import label_and_sample_anchors
    ld = JointTrainLoader(dicts, model, ims, seed=SEED, num_classes=K)
    order = [int(i) for i in ld.rng.permutation(len(dicts))]
    r_items, b_items, per = [], [], []
    for _ in range(ims):
        d = dicts[order.pop(0)]
        boxes, _, classes = ld.prepare_image(d, False)
        gt, cls = ld.ground_truth(boxes, classes, d)
        sel, rl, rm, _ = label_and_sample_anchors(model, gt, 256, 0.5, ld.rpn_generator, (0.3, 0.7))
        patches, slots, anchors, _ = model.rpn_patches(sel)
        props = model.train_proposals(1)[0][0]
        sb, bl, bm, _ = label_and_sample_proposals(props, gt, cls, K, 512, 0.25, ld.box_generator, 0.5)
        r_items.append((patches, slots, rl, anchors, rm))
        b_items.append((model.box_roi_features(sb), bl, sb, bm))
        per.append((d, int(sb.shape[0])))
    rpn = tuple(torch.cat([i[k] for i in r_items]) for k in range(5))
    box = tuple(torch.cat([i[k] for i in b_items]) for k in range(4))
    return rpn, box, per


def test_rpn_and_box_tuples_are_the_same_bits_with_mask_on_and_off(dicts, model):
    want_rpn, want_box, _ = _restated_batch(dicts, model)
    off = _loader(dicts, model, False)
    batch = next(off)
    assert isinstance(batch, tuple) and len(batch) == 2
    assert _equal(batch[0], want_rpn) and _equal(batch[1], want_box)
    on = _loader(dicts, model, True)
    got = next(on)
    assert len(got) == 3 and _equal(got[0], want_rpn) and _equal(got[1], want_box)
    a, b = off.state_dict(), on.state_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    assert _equal(next(off)[1], next(on)[1])                        # and they stay together


def test_mask_rows_are_the_foreground_proposals_with_the_host_targets(dicts, model):
    from apse_uav_amd.utils.COCO_utils import mask_targets
    from apse_uav_amd.utils.joint_train import JointTrainLoader
    ld = _loader(dicts, model, True)
    _, box, mask = next(ld)
    feats, classes, targets = mask
    f = int(feats.shape[0])
    assert tuple(feats.shape) == (f, 14, 14, 256) and feats.dtype == torch.float32 and feats.is_cuda
    assert classes.dtype == torch.int64 and not classes.is_cuda and tuple(classes.shape) == (f,)
    assert tuple(targets.shape) == (f, 28, 28) and targets.dtype == torch.uint8 and targets.is_cuda
    assert sum(ld.last_mask_rows) == f and f > 0 and ld.last_mask_skipped == [0, 0]
    assert ld.last_mask_rows == [fg for fg, _ in ld.last_box_counts]            # every annotation here has a polygon
    # the same images again, by hand: the boxes and labels come from the box tuple, the polygons from the annotations
    helper = JointTrainLoader(dicts, model, 2, seed=SEED, num_classes=K)
    order = [int(i) for i in helper.rng.permutation(len(dicts))]
    row0, m0 = 0, 0
    for i, rows in enumerate(ld.last_box_rows):
        d = dicts[order[i]]
        boxes, polys, _ = helper.prepare_image(d, False)                         # the backbone of this image is current again
        keep = [j for j, a in enumerate(d["annotations"]) if not a.get("iscrowd", 0)]
        gt = torch.from_numpy(np.asarray(boxes, np.float64)[keep].astype(np.float32))
        labels, sb, bm = (t[row0:row0 + rows] for t in box[1:])
        fg = torch.nonzero(labels < K).squeeze(1)
        assert fg.numel() == ld.last_mask_rows[i] and bool((fg == torch.arange(fg.numel(), device=fg.device)).all())
        per_roi = []
        for r in fg.tolist():
            hit = [j for j in range(len(gt)) if torch.equal(gt[j], bm[r].cpu())]
            assert len(hit) == 1, (i, r, hit)
            per_roi.append(polys[keep[hit[0]]])
        n = fg.numel()
        assert torch.equal(feats[m0:m0 + n], model.mask_roi_features(sb[fg]))
        assert torch.equal(classes[m0:m0 + n], labels[fg].cpu().to(torch.int64))
        want = mask_targets(per_roi, sb[fg].cpu().numpy(), model.device)
        assert torch.equal(targets[m0:m0 + n], want)
        assert int(want.sum()) > 0
        row0, m0 = row0 + rows, m0 + n
    assert m0 == f


def test_annotations_without_polygons_give_no_mask_rows(dicts, model):
    helper = _loader(dicts, model, False)
    order = [int(i) for i in helper.rng.permutation(len(dicts))]
    bare = _no_polygons(dicts, [order[0]])                           # the first image of the batch loses its polygons
    full, part = _loader(dicts, model, True), _loader(bare, model, True)
    a, b = next(full), next(part)
    assert _equal(a[0], b[0]) and _equal(a[1], b[1])
    assert part.last_mask_rows == [0, full.last_mask_rows[1]]
    assert part.last_mask_skipped == [full.last_mask_rows[0], 0] and full.last_mask_rows[0] > 0
    cut = full.last_mask_rows[0]
    assert _equal([t[cut:] for t in a[2]], list(b[2]))


def test_a_restored_state_repeats_the_next_batch(dicts, model):
    a = _loader(dicts, model, True)
    next(a)
    sd = a.state_dict()
    want = next(a)
    b = _loader(dicts, model, True)
    b.load_state_dict(sd)
    got = next(b)
    assert all(_equal(x, y) for x, y in zip(want, got))
    assert a.last_mask_rows == b.last_mask_rows and a.last_mask_skipped == b.last_mask_skipped


def _heads(model):
    from apse_uav_amd.networks.box_head import BoxHead
    from apse_uav_amd.networks.mask_head import MaskHead
    from apse_uav_amd.networks.rpn_head import RPNHead
    heads = RPNHead(DEV), BoxHead(K, DEV), MaskHead(K, DEV)
    for h in heads:
        h.load_state_dict(model._state)
    return heads


def _grads(heads, losses):
    import functools
    import operator
    for h in heads:
        h.zero_grad()
    functools.reduce(operator.add, losses.values()).backward()
    torch.cuda.synchronize()
    return [[None if p.grad is None else p.grad.clone() for p in h.parameters()] for h in heads]


def test_three_loss_sum_has_each_head_s_own_gradients(dicts, model):
    from apse_uav_amd.utils.joint_train import box_losses_chunked
    ld = _loader(dicts, model, True)
    rpn_t, box_t, mask_t = next(ld)
    rpn, box, mask = heads = _heads(model)

    def two():
        losses = dict(rpn(*rpn_t, 2))
        losses.update(box_losses_chunked(box, *box_t, ld.last_box_rows))
        return losses
    three = two()
    three.update(mask(*mask_t))
    assert list(three) == ["loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask"]
    assert float(three["loss_mask"].detach()) > 0 and np.isfinite(float(three["loss_mask"].detach()))
    g3 = _grads(heads, three)
    g2 = _grads(heads, two())
    g1 = _grads(heads, mask(*mask_t))
    assert all(g is None for g in g2[2]) and all(g is None for g in g1[0] + g1[1])
    assert _equal(g3[0], g2[0]) and _equal(g3[1], g2[1]) and _equal(g3[2], g1[2])
    assert all(float(g.abs().max()) > 0 for g in g3[2])


def test_a_batch_without_mask_rows_has_zero_loss_and_zero_mask_gradients(dicts, model):
    from apse_uav_amd.utils.joint_train import box_losses_chunked
    ld = _loader(_no_polygons(dicts, range(len(dicts))), model, True)
    rpn_t, box_t, mask_t = next(ld)
    assert ld.last_mask_rows == [0, 0] and tuple(mask_t[0].shape) == (0, 14, 14, 256) and tuple(mask_t[2].shape) == (0, 28, 28)
    assert ld.last_mask_skipped == [fg for fg, _ in ld.last_box_counts]
    rpn, box, mask = heads = _heads(model)
    losses = dict(rpn(*rpn_t, 2))
    losses.update(box_losses_chunked(box, *box_t, ld.last_box_rows))
    losses.update(mask(*mask_t))
    assert float(losses["loss_mask"].detach()) == 0.0
    g = _grads(heads, losses)
    assert all(x is not None and float(x.abs().max()) == 0.0 for x in g[2])
    assert all(x is not None and float(x.abs().max()) > 0 for x in g[0] + g[1])
