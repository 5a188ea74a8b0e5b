"""-m gpu: the f32 plan's trunk Winograd layers (plan.hip, winograd_trunk_layer): the bottlenecks' conv2, fpn_output4 and rpn_t4 of
a plan whose res4-stride map has at least 1000 Winograd tiles.

* one forward of a 270 x 480 frame at the default 800 / 1333 resize (750 x 1333: the map sizes of a 4K frame), once with
  APSE_F32_WINOGRAD=1 and once with 0: res2 .. res5 and p2 .. p6 agree within 4e-6 of the map's largest value, the gate the p2 / p3
  layers were admitted under (numerics);
* below the size rule -- a 375 x 1242 frame at the default resize (546 tiles), a 270 x 480 frame at 600 / 1000 (576) -- the trunk
  keeps the direct kernels: res2 .. res5 of the two contexts are the same bits.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BLOCKS = (1, 1, 1, 1)
TRUNK = ("res2", "res3", "res4", "res5")
MAPS = TRUNK + ("p2", "p3", "p4", "p5", "p6")
BAR = 4e-6


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "winograd.log"), "a") as f:
        f.write("trunk/" + name + " " + json.dumps(obj) + "\n")


@pytest.fixture(scope="module")
def sd():
    from apse_uav_amd.weights import synthetic_detector_state
    return synthetic_detector_state(0, BLOCKS)


def _maps(sd, frame_hw, resize, winograd):
    """res2 .. p6 (device layout, host tensors) of frame 0 of the dynamic sequence in a fresh context."""
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_association_state
    cfg = setup_cfg()
    if resize:
        cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = resize
    old = os.environ.get("APSE_F32_WINOGRAD")
    os.environ["APSE_F32_WINOGRAD"] = "1" if winograd else "0"     # read once, when the context is created
    try:
        tr = RcnnTracker(cfg, frame_hw, synthetic_association_state(1), detector_state=sd)
        tr.predictor.predict_batch([SyntheticSequence("dynamic", *frame_hw).frame(0)], want_masks=False)
    finally:
        if old is None:
            os.environ.pop("APSE_F32_WINOGRAD")
        else:
            os.environ["APSE_F32_WINOGRAD"] = old
    torch.cuda.synchronize()
    return {k: tr.predictor.model.debug_tensor(k).cpu() for k in MAPS}


def test_trunk_winograd_vs_direct_at_4k_map_sizes(sd, logdir):
    wino = _maps(sd, (270, 480), None, True)
    direct = _maps(sd, (270, 480), None, False)
    assert direct["res4"].numel() == 48 * 84 * 1024, direct["res4"].numel()
    err = {k: float((wino[k].double() - direct[k].double()).abs().max() / direct[k].double().abs().max()) for k in MAPS}
    _log(logdir, "vs_direct", err)
    print(err)
    assert all(np.isfinite(v) for v in err.values())
    assert max(err[k] for k in TRUNK) > 0, "the trunk of the Winograd context ran the direct kernels"
    for k in MAPS:
        assert err[k] <= BAR, (k, err)


@pytest.mark.parametrize("frame_hw,resize", [((375, 1242), None), ((270, 480), (600, 1000))], ids=["kitti_default", "600_1000"])
def test_size_rule_keeps_the_direct_trunk(sd, frame_hw, resize):
    wino = _maps(sd, frame_hw, resize, True)
    direct = _maps(sd, frame_hw, resize, False)
    for k in TRUNK:
        assert torch.equal(wino[k].view(torch.int32), direct[k].view(torch.int32)), k
