"""C4 (Res5ROIHeads) models on a machine without a GPU: apse_create's C4 limits, the C4 config switch, the synthetic C4 state
and its key names through the model-zoo converter, and the C4 anchors.  The GPU side is tests/test_gpu_c4.py."""
import ctypes as C
import math
import pickle

import pytest
import torch

from apse_uav_amd import _lib
from apse_uav_amd.config import get_cfg, is_c4, setup_cfg
from apse_uav_amd.networks.track_rcnn import c4_res4_size
from apse_uav_amd.weights import (blocks_from_state, convert_model_zoo_pickle, is_c4_state, load_detector_file,
                                  synthetic_c4_state)


def _config(arch=1, pre=6000, dtype=0, batch=1):
    cfg = _lib.ConfigArch()
    cfg.struct_size = C.sizeof(_lib.ConfigArch)
    cfg.max_batch, cfg.frame_h, cfg.frame_w, cfg.num_classes, cfg.dets_per_image = batch, 270, 480, 4, 100
    cfg.image_h, cfg.image_w = 252, 448
    cfg.score_thresh = 0.5
    cfg.rpn_pre_topk, cfg.rpn_post_topk = pre, 1000
    cfg.assoc_roi, cfg.embed_dim = 10, 128
    cfg.compute_dtype, cfg.storage16 = dtype, 1 if dtype else 0
    cfg.arch = arch
    return cfg


def _create(cfg):
    lib = _lib.load()
    ctx = C.c_void_p()
    rc = lib.apse_create(C.byref(cfg), C.byref(ctx))
    assert not ctx.value
    return rc, lib.apse_last_error(None).decode()


no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="checks the refusal path of a machine without a GPU")


@no_gpu
@pytest.mark.parametrize("pre,batch", [(6000, 1), (1000, 1), (6000, 2)])
def test_c4_create_accepts_its_limits(pre, batch):
    rc, msg = _create(_config(pre=pre, batch=batch))
    assert rc == -2 and "no HIP device visible" in msg, (rc, msg)


@pytest.mark.parametrize("kw,words", [(dict(pre=6001), ("rpn_pre_topk", "6000")),
                                      (dict(dtype=1), ("compute_dtype", "f32")),
                                      (dict(dtype=2), ("compute_dtype", "f32")),
                                      (dict(batch=3), ("max_batch", "2"))])
def test_c4_create_refuses_outside_its_limits(kw, words):
    rc, msg = _create(_config(**kw))
    assert rc == -1 and "C4" in msg and all(w in msg for w in words), (kw, rc, msg)


def test_fpn_limits_unchanged():
    rc, msg = _create(_config(arch=0, pre=1001))
    assert rc == -1 and "out of supported range" in msg, (rc, msg)
    rc, msg = _create(_config(arch=2))
    assert rc == -1 and "arch" in msg


@no_gpu
def test_old_struct_size_means_fpn():
    cfg = _config(arch=1, pre=6000)
    cfg.struct_size = C.sizeof(_lib.Config)          # the layout before `arch`: FPN, so 6000 is refused
    rc, msg = _create(cfg)
    assert rc == -1 and "out of supported range" in msg, (rc, msg)
    cfg.rpn_pre_topk = 1000
    rc, msg = _create(cfg)
    assert rc == -2 and "no HIP device visible" in msg, (rc, msg)


def _check_c4_geometry(cfg):
    m = cfg.MODEL
    assert is_c4(cfg)
    assert tuple(m.RPN.IN_FEATURES) == ("res4",) and tuple(m.ROI_HEADS.IN_FEATURES) == ("res4",)
    assert tuple(m.RESNETS.OUT_FEATURES) == ("res4",)
    assert tuple(tuple(s) for s in m.ANCHOR_GENERATOR.SIZES) == ((32, 64, 128, 256, 512),)
    assert tuple(tuple(r) for r in m.ANCHOR_GENERATOR.ASPECT_RATIOS) == ((0.5, 1.0, 2.0),)
    assert m.RPN.PRE_NMS_TOPK_TEST == 6000 and m.RPN.POST_NMS_TOPK_TEST == 1000
    assert m.ROI_BOX_HEAD.POOLER_RESOLUTION == 14 and m.ROI_MASK_HEAD.POOLER_RESOLUTION == 14
    assert m.ROI_MASK_HEAD.NUM_CONV == 0


def test_setup_cfg_c4():
    cfg = setup_cfg(arch="C4")
    _check_c4_geometry(cfg)
    assert cfg.MODEL.ROI_HEADS.NUM_CLASSES == 4 and cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST == 0.5


def test_get_cfg_unchanged_and_fpn():
    cfg = get_cfg()
    assert not is_c4(cfg)
    assert cfg.MODEL.RPN.PRE_NMS_TOPK_TEST == 1000 and cfg.MODEL.ROI_MASK_HEAD.NUM_CONV == 4
    assert tuple(cfg.MODEL.RPN.IN_FEATURES) == ("p2", "p3", "p4", "p5", "p6")
    assert setup_cfg() == setup_cfg(arch="FPN")


def test_c4_yaml_gives_c4_config(tmp_path):
    base = tmp_path / "Base-RCNN-C4.yaml"
    base.write_text("MODEL:\n  META_ARCHITECTURE: GeneralizedRCNN\n  RPN:\n    PRE_NMS_TOPK_TEST: 6000\n"
                    "  ROI_HEADS:\n    NAME: Res5ROIHeads\n")
    child = tmp_path / "mask_rcnn_R_50_C4_3x.yaml"
    child.write_text("_BASE_: Base-RCNN-C4.yaml\nMODEL:\n  MASK_ON: True\n  RESNETS:\n    DEPTH: 50\n")
    cfg = get_cfg()
    cfg.merge_from_file(str(child))
    _check_c4_geometry(cfg)
    assert cfg.MODEL.RESNETS.DEPTH == 50
    # a YAML value wins over the C4 default
    child.write_text("_BASE_: Base-RCNN-C4.yaml\nMODEL:\n  RPN:\n    POST_NMS_TOPK_TEST: 300\n")
    cfg = get_cfg()
    cfg.merge_from_file(str(child))
    assert is_c4(cfg) and cfg.MODEL.RPN.POST_NMS_TOPK_TEST == 300 and cfg.MODEL.ROI_MASK_HEAD.NUM_CONV == 0


def test_synthetic_c4_state_keys_and_shapes():
    sd = synthetic_c4_state(0, (1, 2, 1, 2), num_classes=4)
    assert is_c4_state(sd)
    assert not any(k.startswith("backbone.bottom_up") or "fpn" in k for k in sd)
    shapes = {
        "backbone.stem.conv1.weight": (64, 3, 7, 7),
        "backbone.res2.0.shortcut.weight": (256, 64, 1, 1),
        "backbone.res3.1.conv2.weight": (128, 128, 3, 3),
        "backbone.res4.0.conv3.norm.running_var": (1024,),
        "roi_heads.res5.0.shortcut.weight": (2048, 1024, 1, 1),
        "roi_heads.res5.0.conv1.weight": (512, 1024, 1, 1),
        "roi_heads.res5.1.conv3.weight": (2048, 512, 1, 1),
        "proposal_generator.rpn_head.conv.weight": (1024, 1024, 3, 3),
        "proposal_generator.rpn_head.objectness_logits.weight": (15, 1024, 1, 1),
        "proposal_generator.rpn_head.anchor_deltas.weight": (60, 1024, 1, 1),
        "roi_heads.box_predictor.cls_score.weight": (5, 2048),
        "roi_heads.box_predictor.bbox_pred.weight": (16, 2048),
        "roi_heads.mask_head.deconv.weight": (2048, 256, 2, 2),
        "roi_heads.mask_head.predictor.weight": (4, 256, 1, 1),
    }
    for k, shp in shapes.items():
        assert tuple(sd[k].shape) == shp, k
    assert "roi_heads.mask_head.mask_fcn1.weight" not in sd and "roi_heads.box_head.fc1.weight" not in sd


@pytest.mark.parametrize("blocks", [(3, 4, 6, 3), (3, 4, 23, 3)])
def test_c4_block_counts(blocks):
    # block counting reads key names only: a state with the shapes' names but tiny tensors is enough
    sd = {}
    sd["backbone.stem.conv1.weight"] = torch.zeros(1)
    for si, n in enumerate(blocks):
        for bi in range(n):
            pre = ("backbone.res%d.%d" % (si + 2, bi)) if si < 3 else "roi_heads.res5.%d" % bi
            sd[pre + ".conv1.weight"] = torch.zeros(1)
    assert blocks_from_state(sd) == blocks


def test_c4_state_through_model_zoo_converter(tmp_path):
    sd = synthetic_c4_state(3, (1, 1, 1, 1), num_classes=80)
    pkl = tmp_path / "model_final_c4.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "Detectron2 Model Zoo"}, f, protocol=2)
    dst = tmp_path / "c4.pth"
    convert_model_zoo_pickle(str(pkl), str(dst))
    back = load_detector_file(str(dst))
    assert set(back) == set(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert blocks_from_state(back) == (1, 1, 1, 1) and is_c4_state(back)


def test_c4_anchors_match_detectron2_formula():
    from c4_ref import c4_grid_anchors
    got = c4_grid_anchors(2, 3)
    assert got.shape == (2 * 3 * 15, 4)
    exp = []
    for y in range(2):
        for x in range(3):
            for size in (32, 64, 128, 256, 512):           # size-major cell order
                for ratio in (0.5, 1.0, 2.0):
                    w = math.sqrt(size * size / ratio)
                    h = ratio * w
                    exp.append([x * 16 - w / 2, y * 16 - h / 2, x * 16 + w / 2, y * 16 + h / 2])
    assert torch.allclose(got, torch.tensor(exp, dtype=torch.float32), atol=1e-4, rtol=0)


def test_c4_res4_geometry():
    assert c4_res4_size(750, 1333) == (47, 84)
    assert c4_res4_size(252, 448) == (16, 28)
    assert c4_res4_size(403, 1333) == (26, 84)


def test_c4_refused_where_fpn_only():
    from apse_uav_amd.engines.roi_features_generator import RoiFeaturesGenerator
    from apse_uav_amd.engines.selective_predictor import SelectivePredictor
    cfg = setup_cfg(arch="C4", device="cpu")
    with pytest.raises(NotImplementedError):
        SelectivePredictor(cfg)
    with pytest.raises(NotImplementedError):
        RoiFeaturesGenerator(cfg)


def test_c4_non_default_anchors_refused():
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    cfg = setup_cfg(arch="C4", device="cpu")
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = ((64, 128, 256),)
    with pytest.raises(ValueError, match="anchors"):
        TrackRCNN(cfg)
