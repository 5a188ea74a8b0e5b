"""-m gpu: bitmask ground truth through the loaders and the loops.

6. ``MaskTrainLoader(mask_format="bitmask")`` on the generated dataset with RLE annotations: the targets are tests/bitmask_ref.py
   ``ref_targets`` of the dense masks resized by ``Image.resize(NEAREST)``, on the host-flip path and on the augment path;
   ``JointTrainLoader(mask=True, mask_format="bitmask")``: rpn, box and ``state_dict`` are the bits of ``mask=False`` and the mask
   rows equal the reference.
7. ``tools/finetune_uav.py --synthetic 6 --iters 8 --mask --mask-format bitmask`` and ``tools/finetune_segmentation.py --synthetic
   12 --mots --iters 20``: a finite, falling ``loss_mask``, checkpoints that load into TrackPredictor, ``--resume`` bit for bit."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import bitmask_ref as br                                     # noqa: E402

DEV = "cuda:0"
K = 4
SEED = 1


@pytest.fixture(scope="module")
def rle_dicts(tmp_path_factory):
    """The generated dataset with every polygon (an integer-cornered rectangle) replaced by the RLE of that rectangle."""
    from apse_uav_amd.synthetic import synthetic_dataset
    from apse_uav_amd.utils import COCO_utils, rle
    root = str(tmp_path_factory.mktemp("bitmask_loop") / "img")
    data = json.load(open(synthetic_dataset(root, 4, seed=2)))
    sizes = {im["id"]: (im["height"], im["width"]) for im in data["images"]}
    for ann in data["annotations"]:
        h, w = sizes[ann["image_id"]]
        x, y, bw, bh = (int(v) for v in ann["bbox"])
        m = np.zeros((h, w), np.uint8)
        m[y:y + bh, x:x + bw] = 1
        ann["segmentation"] = {"size": [h, w], "counts": rle.encode(m)["counts"].decode("ascii")}
    path = os.path.join(root, "annotations_rle.json")
    json.dump(data, open(path, "w"))
    with pytest.raises(ValueError, match="RLE"):                         # the parent's refusal, still the default
        COCO_utils.generate_coco_dataset_dictionaries(path, root, None, None, False)
    return COCO_utils.generate_coco_dataset_dictionaries(path, root, None, None, False, mask_format="bitmask")


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


def resized_masks(d, image_hw, flip_before=False, flip_after=False):
    """The annotations' dense masks as detectron2 would hand them to BitMasks: flipped / resized with Pillow's NEAREST."""
    from PIL import Image
    from apse_uav_amd.utils import rle
    out = []
    for a in d["annotations"]:
        m = rle.decode(a["segmentation"]).astype(np.uint8)
        if flip_before:
            m = m[:, ::-1].copy()
        m = np.asarray(Image.fromarray(m).resize((image_hw[1], image_hw[0]), Image.NEAREST))
        out.append(m[:, ::-1] if flip_after else m)
    return out


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("flipped", [False, True])
def test_mask_loader_host_flip_path(rle_dicts, model, flipped):
    from apse_uav_amd.utils import resample
    from apse_uav_amd.utils.COCO_utils import MaskTrainLoader
    ld = MaskTrainLoader(rle_dicts, model, 2, seed=SEED, flip=True, mask_format="bitmask")
    total = 0
    for d in rle_dicts[:3]:
        feats, classes, targets = ld.image_item(d, flipped)
        boxes, src, _ = ld.prepare_image(d, flipped)
        ih, iw = resample.resize_shortest_edge(d["height"], d["width"], 192, 320)
        assert src.image_hw == (ih, iw) and len(src) == len(d["annotations"]) == int(feats.shape[0])
        dense = resized_masks(d, (ih, iw), flip_before=flipped)
        want = br.ref_rows(dense, boxes.astype(np.float32), np.arange(len(dense)), np.float32)
        assert targets.dtype == torch.uint8 and targets.is_cuda and np.array_equal(targets.cpu().numpy(), want)
        total += int(want.sum())
    assert total > 0
    feats, classes, targets = next(ld)                                   # and a batch comes out joined as ever
    assert tuple(targets.shape) == (int(feats.shape[0]), 28, 28) and tuple(classes.shape) == (int(feats.shape[0]),)


@pytest.mark.parametrize("flip", [False, True])
def test_mask_loader_augment_path(rle_dicts, model, flip):
    from apse_uav_amd.utils import resample
    from apse_uav_amd.utils.augment import AugmentParams
    from apse_uav_amd.utils.COCO_utils import MaskTrainLoader
    ld = MaskTrainLoader(rle_dicts, model, 2, seed=SEED, flip=True, augment=True, min_sizes=(160, 192), max_size=320, mask_format="bitmask")
    params = AugmentParams(flip, 1.05, 0.95, 1.02, (0.1, -0.1, 0.05))
    for d, size in zip(rle_dicts[:2], (160, 192)):
        _, _, targets = ld.augmented_item(d, size, params)
        boxes, src, _ = ld.prepare_augmented(d, size, params)
        ih, iw = resample.resize_shortest_edge(d["height"], d["width"], size, 320)
        dense = resized_masks(d, (ih, iw), flip_after=flip)
        want = br.ref_rows(dense, boxes.astype(np.float32), np.arange(len(dense)), np.float32)
        assert np.array_equal(targets.cpu().numpy(), want) and want.sum() > 0


def test_polygon_and_box_only_objects_in_bitmask_mode(rle_dicts, model):
    """A polygon object is transformed like the polygon path's and rasterised at the image size; an object without a
    segmentation gives a zero row."""
    from apse_uav_amd.utils import coco as cocomod
    from apse_uav_amd.utils.COCO_utils import MaskTrainLoader
    d = copy.deepcopy(rle_dicts[0])
    x, y, bw, bh = d["annotations"][0]["bbox"]
    d["annotations"][0]["segmentation"] = [[x, y, x + bw, y, x + bw, y + bh, x, y + bh]]
    if len(d["annotations"]) > 1:
        d["annotations"][1]["segmentation"] = []
    ld = MaskTrainLoader([d], model, 1, seed=SEED, mask_format="bitmask")
    _, _, targets = ld.image_item(d, False)
    boxes, src, _ = ld.prepare_image(d, False)
    bm = src.device_bitmasks(model.device)
    ih, iw = src.image_hw
    dense = cocomod.windows_to_dense(bm.windows, ih, iw)
    win, keep = cocomod.polygons_to_windows([([np.asarray(src.polys[0][0]).reshape(-1, 2)], ih, iw)], model.device)
    assert np.array_equal(dense[0], cocomod.windows_to_dense(win, ih, iw)[0]) and dense[0].any()
    want = br.ref_rows(list(dense), boxes.astype(np.float32), np.arange(len(dense)), np.float32)
    assert np.array_equal(targets.cpu().numpy(), want)
    if len(d["annotations"]) > 1:
        assert bm.has_mask.tolist()[:2] == [True, False] and want[1].sum() == 0


def test_a_polygon_mode_loader_refuses_rle_annotations(rle_dicts, model):
    from apse_uav_amd.utils.COCO_utils import MaskTrainLoader
    with pytest.raises(ValueError, match="bitmask"):
        MaskTrainLoader(rle_dicts, model, 1, seed=SEED).prepare_image(rle_dicts[0])
    with pytest.raises(ValueError, match="mask_format"):
        MaskTrainLoader(rle_dicts, model, 1, seed=SEED, mask_format="rle")


def test_joint_loader_bitmask_rows(rle_dicts, model):
    from apse_uav_amd.utils import resample
    from apse_uav_amd.utils.joint_train import JointTrainLoader
    off = JointTrainLoader(rle_dicts, model, 2, seed=SEED, num_classes=K, mask_format="bitmask")
    on = JointTrainLoader(rle_dicts, model, 2, seed=SEED, num_classes=K, mask=True, mask_format="bitmask")
    a, b = next(off), next(on)
    assert len(a) == 2 and len(b) == 3 and _equal(a[0], b[0]) and _equal(a[1], b[1])
    sa, sb_ = off.state_dict(), on.state_dict()
    assert sorted(sa) == sorted(sb_)
    for k in sa:
        assert torch.equal(sa[k], sb_[k]) if torch.is_tensor(sa[k]) else sa[k] == sb_[k], k
    feats, classes, targets = b[2]
    f = int(feats.shape[0])
    assert f > 0 and sum(on.last_mask_rows) == f and on.last_mask_skipped == [0, 0]
    assert on.last_mask_rows == [fg for fg, _ in on.last_box_counts]
    helper = JointTrainLoader(rle_dicts, model, 2, seed=SEED, num_classes=K, mask_format="bitmask")
    order = [int(i) for i in helper.rng.permutation(len(rle_dicts))]
    row0, m0 = 0, 0
    for i, rows in enumerate(on.last_box_rows):
        d = rle_dicts[order[i]]
        boxes, _, _ = helper.prepare_image(d, False)
        ih, iw = resample.resize_shortest_edge(d["height"], d["width"], 192, 320)
        dense = resized_masks(d, (ih, iw))
        gt = torch.from_numpy(np.asarray(boxes, np.float64).astype(np.float32))
        labels, sb, bm = (t[row0:row0 + rows] for t in b[1][1:])
        fg = torch.nonzero(labels < K).squeeze(1)
        matched = []
        for r in fg.tolist():
            hit = [j for j in range(len(gt)) if torch.equal(gt[j], bm[r].cpu())]
            assert len(hit) == 1, (i, r, hit)
            matched.append(hit[0])
        n = fg.numel()
        want = br.ref_rows(dense, sb[fg].cpu().numpy(), np.array(matched), np.float32)
        assert np.array_equal(targets[m0:m0 + n].cpu().numpy(), want) and want.sum() > 0
        assert torch.equal(feats[m0:m0 + n], model.mask_roi_features(sb[fg]))
        row0, m0 = row0 + rows, m0 + n
    assert m0 == f
    assert _equal(next(off)[1], next(on)[1])                             # and they stay together


# ---------------------------------------------------------------- 7. loops
def _falls(values):
    values = [float(v) for v in values]
    assert all(np.isfinite(v) for v in values), values
    assert np.mean(values[-3:]) < values[0], values


def _same_checkpoint(a, b):
    ca = torch.load(a["checkpoint"], map_location="cpu", weights_only=False)
    cb = torch.load(b["checkpoint"], map_location="cpu", weights_only=False)
    assert ca["iteration"] == cb["iteration"] and sorted(ca["model"]) == sorted(cb["model"])
    for k, v in ca["model"].items():
        assert torch.equal(v, cb["model"][k]), k
    for k, v in a["state"].items():
        assert torch.equal(v, b["state"][k]), k
    return ca


def _loads(state, num_classes=4):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    cfg = setup_cfg(num_classes=num_classes)
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0
    inst = TrackPredictor(cfg, state_dict=state)(SyntheticSequence("dynamic", 270, 480).frame(0))[0]["instances"]
    assert inst.has("pred_masks") and len(inst.pred_masks) == len(inst)


def test_finetune_uav_mask_bitmask_dry_run_and_resume(tmp_path):
    import finetune_uav as tool

    def run(out, *extra):
        return tool.main(["--synthetic", "6", "--iters", "8", "--mask", "--mask-format", "bitmask", "--checkpoint-period", "3",
                          "--warmup-iters", "2", "--out", out] + list(extra))
    a = run(str(tmp_path / "a"))
    assert os.path.exists(os.path.join(str(tmp_path / "a"), "synthetic", "annotations_rle.json"))
    assert len(a["losses"]) == 8 and all(len(row) == 5 for row in a["losses"])
    _falls([row[4] for row in a["losses"]])
    run(str(tmp_path / "b"), "--stop-at", "3")
    b = run(str(tmp_path / "b"), "--resume")
    chk = _same_checkpoint(a, b)
    assert chk["iteration"] == 6 and a["losses"][4:] == b["losses"]
    _loads(chk["model"])


def test_finetune_segmentation_mots_dry_run_and_resume(tmp_path):
    import finetune_segmentation as tool

    def run(out, *extra):
        return tool.main(["--synthetic", "12", "--mots", "--iters", "20", "--checkpoint-period", "5", "--warmup-iters", "5",
                          "--k-folds", "4", "--out", out] + list(extra))
    a = run(str(tmp_path / "a"))
    assert os.path.isdir(os.path.join(str(tmp_path / "a"), "synthetic_mots", "instances_txt"))
    assert len(a["losses"]) == 20
    _falls(a["losses"])
    run(str(tmp_path / "b"), "--stop-at", "10")
    b = run(str(tmp_path / "b"), "--resume")
    chk = _same_checkpoint(a, b)
    assert chk["iteration"] == 15 and a["losses"][11:] == b["losses"]
    _loads(chk["model"])
