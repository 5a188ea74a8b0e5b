"""Class-count limits of apse_create on a machine without a GPU (1..80 classes, the 40000-candidate guard) and the model-zoo
pickle converter.  The GPU side of the wide box inference is tests/test_gpu_many_classes.py."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from apse_uav_amd import _lib
from apse_uav_amd.weights import convert_model_zoo_pickle, load_detector_file


def _config(num_classes, score_thresh=0.05, post_topk=1000):
    cfg = _lib.Config()
    cfg.struct_size = C.sizeof(_lib.Config)
    cfg.max_batch, cfg.frame_h, cfg.frame_w, cfg.num_classes, cfg.dets_per_image = 1, 270, 480, num_classes, 100
    cfg.image_h, cfg.image_w = 252, 448
    cfg.score_thresh = score_thresh
    cfg.rpn_pre_topk, cfg.rpn_post_topk = 1000, post_topk
    cfg.assoc_roi, cfg.embed_dim = 10, 128
    return cfg


def _create(cfg):
    lib = _lib.load()
    ctx = C.c_void_p()
    rc = lib.apse_create(C.byref(cfg), C.byref(ctx))
    assert not ctx.value
    return rc, lib.apse_last_error(None).decode()


no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="checks the refusal path of a machine without a GPU")


@no_gpu
@pytest.mark.parametrize("k", [1, 4, 6, 7, 32, 80])
def test_create_accepts_up_to_80_classes(k):
    rc, msg = _create(_config(k))
    assert rc == -2 and "no HIP device visible" in msg, (k, rc, msg)


@pytest.mark.parametrize("k", [0, 81, 1000])
def test_create_refuses_class_counts_out_of_range(k):
    rc, msg = _create(_config(k))
    assert rc == -1 and "out of supported range" in msg, (k, rc, msg)


@pytest.mark.parametrize("k,thr,post", [(80, 0.01, 1000), (80, 0.0, 1000), (50, 0.02, 1000), (40, 0.0, 1000)])
def test_create_refuses_configs_that_reach_the_batched_nms_switch(k, thr, post):
    # rpn_post_topk * min(K, ceil(1 / thr) - 1) >= 40000: detectron2's batched_nms would take its other method
    rc, msg = _create(_config(k, thr, post))
    assert rc == -1 and "40000" in msg and "ceil(1 / score_thresh)" in msg, (k, thr, rc, msg)


@no_gpu
@pytest.mark.parametrize("k,thr,post", [(80, 0.05, 1000), (80, 0.0251, 1000), (80, 0.01, 400), (39, 0.0, 1000), (6, 0.0, 1000)])
def test_create_accepts_configs_below_the_batched_nms_switch(k, thr, post):
    # COCO's 0.05: 1000 x 19 = 19000 candidates at most; 0.0251: 39 classes of a ROI at most
    rc, msg = _create(_config(k, thr, post))
    assert rc == -2 and "no HIP device visible" in msg, (k, thr, rc, msg)


def _zoo_like_state():
    rng = np.random.default_rng(5)
    return {"backbone.bottom_up.stem.conv1.weight": rng.standard_normal((64, 3, 7, 7)).astype(np.float32),
            "backbone.bottom_up.stem.conv1.norm.running_mean": rng.standard_normal(64).astype(np.float32),
            "roi_heads.box_predictor.cls_score.weight": rng.standard_normal((81, 1024)).astype(np.float32),
            "roi_heads.box_predictor.bbox_pred.bias": rng.standard_normal(320).astype(np.float32),
            "roi_heads.mask_head.predictor.weight": rng.standard_normal((80, 256, 1, 1)).astype(np.float32)}


@pytest.mark.parametrize("protocol", [2, pickle.HIGHEST_PROTOCOL])
def test_model_zoo_pickle_converts(tmp_path, protocol):
    src, dst = tmp_path / "model_final_f10217.pkl", tmp_path / "model_final_f10217.pth"
    model = _zoo_like_state()
    with open(src, "wb") as f:
        pickle.dump({"model": model, "__author__": "Detectron2 Model Zoo"}, f, protocol=protocol)
    convert_model_zoo_pickle(str(src), str(dst))
    sd = load_detector_file(str(dst))
    assert set(sd) == set(model)
    for k, v in model.items():
        assert sd[k].dtype == torch.float32 and torch.equal(sd[k], torch.from_numpy(v)), k


class _Payload:
    def __init__(self, path):
        self.path = path

    def __reduce__(self):
        return (os.system, ("touch " + self.path,))


def test_model_zoo_converter_refuses_other_globals(tmp_path):
    marker = tmp_path / "ran"
    src = tmp_path / "evil.pkl"
    with open(src, "wb") as f:
        pickle.dump({"model": {"w": np.zeros(3, np.float32)}, "x": _Payload(str(marker))}, f)
    with pytest.raises(pickle.UnpicklingError) as ei:
        convert_model_zoo_pickle(str(src), str(tmp_path / "out.pth"))
    assert "system" in str(ei.value)
    assert not marker.exists()
    assert not (tmp_path / "out.pth").exists()
