"""Host side of mask-head training: dataset dictionaries, the polygon transform, the learning-rate schedule, checkpoint merging,
refused limits and the ABI list -- no GPU needed."""
import bisect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["car", "truck", "bus", "person"]
MAPPING = {3: 0, 8: 1, 6: 2, 1: 3}


@pytest.fixture(scope="module")
def dicts(golden_dir):
    from apse_uav_amd.utils import COCO_utils
    return COCO_utils.generate_coco_dataset_dictionaries(os.path.join(golden_dir, "mask_train_annotations.json"), "/data/img",
                                                         CLASSES, MAPPING, True)


def test_dataset_dictionaries(dicts):
    assert [d["image_id"] for d in dicts] == [7, 9]                   # image 11 holds only a class that is not allowed
    a = dicts[0]
    assert a["file_name"] == os.path.join("/data/img", "a.png") and (a["height"], a["width"]) == (100, 200)
    assert [x["category_id"] for x in a["annotations"]] == [0, 3]     # crowd and "cat" dropped, ids mapped
    assert all(x["iscrowd"] == 0 and x["bbox_mode"] == 1 for x in a["annotations"])
    seg = a["annotations"][1]["segmentation"]
    assert isinstance(seg, list) and len(seg) == 2 and isinstance(seg[0], list)       # the list itself, not a 1-tuple around it
    assert seg[0] == [50.0, 10.0, 70.0, 10.0, 60.0, 60.0]
    assert np.array_equal(a["proposal_boxes"], np.array([[10, 20, 40, 60], [50, 10, 70, 60]], np.float32))      # proposals == boxes
    assert a["proposal_objectness_logits"].shape == (2,)
    assert [x["category_id"] for x in dicts[1]["annotations"]] == [1]


def test_default_mapping_and_no_proposals(golden_dir):
    from apse_uav_amd.utils import COCO_utils
    d = COCO_utils.generate_coco_dataset_dictionaries(os.path.join(golden_dir, "mask_train_annotations.json"), "x", ["cat", "car"],
                                                      None, False)
    assert [[a["category_id"] for a in x["annotations"]] for x in d] == [[0, 1], [1]]      # sorted ids 3, 17 -> 0, 1
    assert "proposal_boxes" not in d[0]


def test_rle_refused(tmp_path, golden_dir):
    import json
    from apse_uav_amd.utils import COCO_utils
    data = json.load(open(os.path.join(golden_dir, "mask_train_annotations.json")))
    data["annotations"][2]["iscrowd"] = 0
    p = tmp_path / "rle.json"
    p.write_text(json.dumps(data))
    with pytest.raises(ValueError, match="RLE"):
        COCO_utils.generate_coco_dataset_dictionaries(str(p), "x", CLASSES, MAPPING)


def test_round_trip_through_coco(dicts):
    from apse_uav_amd.utils import COCO_utils
    from apse_uav_amd.utils.coco import COCO
    ds = COCO_utils.detectron2_dataset_to_coco(dicts, CLASSES)
    gt = COCO.from_dataset(ds, verbose=False)
    assert sorted(gt.getImgIds()) == [7, 9] and sorted(gt.getCatIds()) == [0, 1, 2, 3]
    anns = gt.loadAnns(gt.getAnnIds(imgIds=[7]))
    assert [a["category_id"] for a in anns] == [0, 3] and anns[0]["bbox"] == [10.0, 20.0, 30.0, 40.0]
    assert anns[1]["segmentation"] == dicts[0]["annotations"][1]["segmentation"]
    assert [c["name"] for c in gt.loadCats([0, 3])] == ["car", "person"]


def test_polygon_transform_hand_cases():
    from apse_uav_amd.utils.COCO_utils import crop_and_resize_polygons
    # equal ratios: box 14 x 14 -> ratio 2 for both axes
    q = crop_and_resize_polygons([[10, 20, 24, 20, 17, 34]], [10, 20, 24, 34])
    assert np.array_equal(q[0], np.array([0, 0, 28, 0, 14, 28], np.float64))
    # unequal: 56 wide (ratio 0.5), 7 high (ratio 4)
    q = crop_and_resize_polygons([[4, 1, 60, 1, 60, 8]], [4, 1, 60, 8])
    assert np.array_equal(q[0], np.array([0, 0, 28, 0, 28, 28], np.float64))
    # narrower than 0.1 px: the width ratio is 28 / 0.1, computed in float64
    q = crop_and_resize_polygons([[5.0, 0, 5.05, 0, 5.05, 7]], [5.0, 0, 5.05, 7])
    assert q[0][2] == (5.05 - 5.0) * (28 / 0.1) and q[0][5] == 7 * (28 / 7.0)
    # an odd trailing number is dropped, the input is not modified
    src = [[0.0, 0.0, 2.0, 0.0, 2.0, 2.0, 9.0]]
    q = crop_and_resize_polygons(src, [0, 0, 2, 2])
    assert len(q[0]) == 6 and src[0][2] == 2.0


def test_flip():
    from apse_uav_amd.utils.COCO_utils import flip_annotations
    b, p = flip_annotations([[10, 5, 30, 25]], [[[10, 5, 30, 5, 30, 25]]], 100)
    assert b.tolist() == [[70, 5, 90, 25]] and p[0][0].tolist() == [90, 5, 70, 5, 70, 25]


def test_warmup_multistep_lr():
    from apse_uav_amd.optim import WarmupMultiStepLR
    p = [torch.zeros(1, requires_grad=True)]
    opt = torch.optim.SGD(p, lr=0.02, momentum=0.9)
    sched = WarmupMultiStepLR(opt, [30, 45], 0.1, 0.001, 10)
    ref_opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.02, momentum=0.9)

    def formula(it):
        alpha = it / 10
        warm = 1.0 if it >= 10 else 0.001 * (1 - alpha) + alpha
        return warm * 0.1 ** bisect.bisect_right([30, 45], it)
    ref = torch.optim.lr_scheduler.LambdaLR(ref_opt, formula)
    lrs = []
    for it in range(60):
        lrs.append(opt.param_groups[0]["lr"])
        assert lrs[-1] == pytest.approx(ref_opt.param_groups[0]["lr"], rel=1e-12, abs=0)
        opt.step(); sched.step(); ref_opt.step(); ref.step()
    assert lrs[0] == pytest.approx(0.02 * 0.001)                      # WARMUP_FACTOR at iteration 0
    assert lrs[5] == pytest.approx(0.02 * (0.001 * 0.5 + 0.5))
    assert lrs[9] == pytest.approx(0.02 * (0.001 * 0.1 + 0.9)) and lrs[10] == 0.02     # warm-up ends
    assert lrs[29] == 0.02 and lrs[30] == pytest.approx(0.002) and lrs[44] == pytest.approx(0.002)
    assert lrs[45] == pytest.approx(0.0002) and lrs[59] == pytest.approx(0.0002)
    # state round trip
    sd = sched.state_dict()
    opt2 = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.02, momentum=0.9)
    s2 = WarmupMultiStepLR(opt2, [30, 45], 0.1, 0.001, 10)
    s2.load_state_dict(sd)
    assert s2.last_epoch == 60 and opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
    with pytest.raises(ValueError):
        WarmupMultiStepLR(opt2, [5, 3])


def test_merge_full_mask_rcnn():
    from apse_uav_amd.networks.mask_head import PREFIX, MaskHead, merge_full_mask_rcnn
    head = MaskHead(2, "cpu")
    hs = head.state_dict()
    assert list(hs) == [n + s for n in ("mask_fcn1", "mask_fcn2", "mask_fcn3", "mask_fcn4", "deconv", "predictor")
                        for s in (".weight", ".bias")]
    det = {"backbone.x": torch.ones(1), "model.roi_heads.box_head.fc1.weight": torch.ones(2),
           PREFIX + "deconv.bias": torch.full((256,), 9.0)}
    m = merge_full_mask_rcnn(det, hs)
    assert "roi_heads.box_head.fc1.weight" in m and "backbone.x" in m and len(m) == 2 + 12
    assert torch.equal(m[PREFIX + "deconv.bias"], hs["deconv.bias"])           # the trained head wins
    m2 = merge_full_mask_rcnn(det, head.state_dict(PREFIX))
    assert all(torch.equal(m[k], m2[k]) for k in m)
    with pytest.raises(KeyError):
        merge_full_mask_rcnn(det, {k: v for k, v in hs.items() if k != "predictor.bias"})
    with pytest.raises(KeyError):
        merge_full_mask_rcnn(det, dict(hs, stray=torch.ones(1)))
    # load_state_dict accepts both spellings and checks shapes
    h2 = MaskHead(2, "cpu")
    h2.load_state_dict(m)
    assert all(torch.equal(a, b) for a, b in zip(h2.state_dict().values(), hs.values()))
    with pytest.raises(RuntimeError):
        MaskHead(3, "cpu").load_state_dict(hs)
    assert all(p.requires_grad and p.is_leaf and p.dtype == torch.float32 for p in head.parameters())


def test_limits_refused():
    from apse_uav_amd import _lib
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks import mask_head as mh
    lib = _lib.load()
    assert mh.MAX_ROIS == 1024 and mh.MAX_CLASSES == 80
    assert lib.apse_mask_train_workspace_bytes(mh.MAX_ROIS, 80) > 0
    assert lib.apse_mask_train_workspace_bytes(mh.MAX_ROIS + 1, 4) == 0 and lib.apse_mask_train_workspace_bytes(0, 4) == 0
    assert lib.apse_mask_train_workspace_bytes(4, 81) == 0 and lib.apse_mask_train_workspace_bytes(4, 0) == 0
    one = np.zeros(4, np.float32)
    rc = lib.apse_mask_wgrad(_lib.ptr(one), _lib.ptr(one), mh.MAX_ROIS + 1, 0, _lib.ptr(one), _lib.ptr(one), 16, None)
    assert rc == -1 and b"APSE_MASK_TRAIN_MAX_N" in lib.apse_last_error(None)
    rc = lib.apse_mask_loss_forward(_lib.ptr(one), 81, _lib.ptr(one), _lib.ptr(one), 1, _lib.ptr(one), _lib.ptr(one), 64, None)
    assert rc == -1 and b"APSE_MAX_CLASSES" in lib.apse_last_error(None)
    rc = lib.apse_mask_conv3x3(_lib.ptr(one), _lib.ptr(one), None, 0, 0, _lib.ptr(one), None)
    assert rc == -1
    with pytest.raises(_lib.ApseError):
        mh._workspace(mh.MAX_ROIS + 1, 4, "cpu")
    with pytest.raises(ValueError):
        mh.MaskHead(81)
    with pytest.raises(NotImplementedError):
        mh.MaskHead.from_cfg(setup_cfg(num_classes=4, arch="C4"))
    assert mh.MaskHead.from_cfg(setup_cfg(num_classes=7), "cpu").num_classes == 7


def test_lib_exports_equal_header():
    from apse_uav_amd import _lib
    text = open(os.path.join(ROOT, "include", "apse_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(apse_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.EXPORTS), (sorted(declared - set(_lib.EXPORTS)), sorted(set(_lib.EXPORTS) - declared))
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    mask = {n for n in declared if n.startswith("apse_mask_") and n not in ("apse_mask_tail", "apse_mask_centroid_dense",
                                                                           "apse_mask_closest_dense")}
    assert len(mask) == 12
