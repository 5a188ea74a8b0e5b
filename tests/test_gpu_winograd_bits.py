"""-m gpu: the fused f32 Winograd layers give the bits they gave before the k loop of conv_winograd_f32 was re-scheduled.

For the frame sizes and batches of test_gpu_winograd.py (resize 600 / 1000, BLOCKS = (1, 1, 1, 1), seeded frames and weights) the
sha256 of `debug_tensor` of p2, p3, rpn_t2, rpn_t3 equals tests/golden/winograd_layer_sha256.json, which
tools/record_winograd_hashes.py recorded with the library of the commit before the re-schedule (APSE_HIP_LIB).  The kernels
involved are deterministic and the re-schedule keeps every accumulator's order of products, so there is no tolerance.  inner2 /
inner3 (the layers' inputs, produced by kernels this change does not touch) are hashed too: when they differ the mismatch is
upstream of the Winograd kernel, and the message says so.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BLOCKS = (1, 1, 1, 1)
CASES = [((270, 480), 1), ((375, 1242), 2), ((721, 1283), 4)]
INPUTS = ("inner2", "inner3")
OUTPUTS = ("p2", "p3", "rpn_t2", "rpn_t3")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "winograd_layer_sha256.json")


def case_key(frame_hw, batch):
    return "%dx%d_batch%d" % (frame_hw[0], frame_hw[1], batch)


def layer_hashes(frame_hw, batch):
    """sha256 of the debug tensors of one seeded batch through a fresh f32 context with the Winograd plan."""
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_association_state, synthetic_detector_state
    cfg = setup_cfg()
    cfg.INPUT.MIN_SIZE_TEST = 600              # p2 / p3 of >= 128 Winograd blocks per image: the plan takes the Winograd kernel
    cfg.INPUT.MAX_SIZE_TEST = 1000
    cfg.APSE.MAX_BATCH = batch
    old = os.environ.get("APSE_F32_WINOGRAD")
    os.environ["APSE_F32_WINOGRAD"] = "1"      # read once, when the context is created
    try:
        tr = RcnnTracker(cfg, frame_hw, synthetic_association_state(1), detector_state=synthetic_detector_state(0, BLOCKS))
        seq = SyntheticSequence("dynamic", *frame_hw)
        tr.predictor.predict_batch([seq.frame(t) for t in range(batch)], want_masks=False)
    finally:
        if old is None:
            os.environ.pop("APSE_F32_WINOGRAD")
        else:
            os.environ["APSE_F32_WINOGRAD"] = old
    torch.cuda.synchronize()
    model = tr.predictor.model
    out = {}
    for name in INPUTS + OUTPUTS:
        t = model.debug_tensor(name).cpu().contiguous()
        out[name] = hashlib.sha256(t.numpy().view(np.uint8).tobytes()).hexdigest()
    return out


@pytest.mark.parametrize("frame_hw,batch", CASES)
def test_winograd_layers_keep_their_bits(frame_hw, batch):
    golden = json.load(open(GOLDEN))["cases"][case_key(frame_hw, batch)]
    got = layer_hashes(frame_hw, batch)
    print(case_key(frame_hw, batch), json.dumps(got))
    for name in INPUTS:
        assert got[name] == golden[name], "%s differs: the mismatch is upstream of conv_winograd_f32" % name
    for name in OUTPUTS:
        assert got[name] == golden[name], "%s differs from the recorded bits of conv_winograd_f32" % name
