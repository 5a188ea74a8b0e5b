"""Frame-size limits of apse_create on a machine without a GPU, and the host resize tables at widths that are not a
multiple of 4 (the sizes of tests/test_gpu_frame_sizes.py).  The GPU side of the same sizes is that file's."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from apse_uav_amd import _lib
from apse_uav_amd.utils import resample

SIZES = [(375, 1242), (721, 1283), (1080, 1918), (217, 389)]

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="checks the refusal path of a machine without a GPU")


def _config(h, w):
    cfg = _lib.Config()
    cfg.struct_size = C.sizeof(_lib.Config)
    cfg.max_batch, cfg.frame_h, cfg.frame_w, cfg.num_classes, cfg.dets_per_image = 1, h, w, 4, 100
    cfg.image_h, cfg.image_w = resample.resize_shortest_edge(h, w, 800, 1333) if h > 0 and w > 0 else (800, 1333)
    cfg.rpn_pre_topk = cfg.rpn_post_topk = 1000
    cfg.assoc_roi, cfg.embed_dim = 10, 128
    return cfg


def _create(cfg):
    lib = _lib.load()
    ctx = C.c_void_p()
    rc = lib.apse_create(C.byref(cfg), C.byref(ctx))
    assert not ctx.value
    return rc, lib.apse_last_error(None).decode()


@pytest.mark.parametrize("hw", SIZES)
def test_create_passes_the_config_check(hw):
    # the config is in range: creation gets as far as looking for a device
    rc, msg = _create(_config(*hw))
    assert rc == -2 and "no HIP device visible" in msg, (rc, msg)


@pytest.mark.parametrize("hw", [(375, 0), (-1, 1242), (0, 1242), (375, -4), (375, 49153), (32769, 1242)])
def test_create_refuses_frame_sizes_out_of_range(hw):
    rc, msg = _create(_config(*hw))
    assert rc == -1 and "frame size" in msg, (rc, msg)


def test_create_accepts_the_bounds():
    for hw in [(1, 49152), (32768, 1), (2, 49151)]:
        rc, msg = _create(_config(*hw))
        assert rc == -2 and "no HIP device visible" in msg, (hw, rc, msg)


@pytest.mark.parametrize("hw", SIZES)
def test_resize_reference_equals_pillow(hw):
    h, w = hw
    oh, ow = resample.resize_shortest_edge(h, w, 800, 1333)
    img = np.random.default_rng(h * 7 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
    got = resample.resize_reference_numpy(img, oh, ow)
    assert got.shape == want.shape and np.array_equal(got, want)
