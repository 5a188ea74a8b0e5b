"""-m gpu: the fused f32 Winograd F(2x2,3x3) layers (conv_winograd.hip): fpn_output2 / fpn_output3 / rpn_t2 / rpn_t3.

* each layer's output against a float64 direct convolution of the SAME input tensor (read back from the context), next to
  the error of the direct kernel (a context created with APSE_F32_WINOGRAD=0) on that input: odd H / W, batch 1, 2 and 4;
* the same frame gives the same bits alone, in a batch of 4, before and after other frames, and in a second context.
Frames are resized to 600 / 1000 (not the 256 / 448 of the other small-frame tests): below 128 blocks per image the plan keeps
the direct kernel.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BLOCKS = (1, 1, 1, 1)
LAYERS = (  # (output tensor, input tensor, weight name, relu)
    ("p2", "inner2", "backbone.fpn_output2", False),
    ("p3", "inner3", "backbone.fpn_output3", False),
    ("rpn_t2", "p2", "proposal_generator.rpn_head.conv", True),
    ("rpn_t3", "p3", "proposal_generator.rpn_head.conv", True),
)
# Winograd's error over the direct kernel's on the same inputs (CPU emulation of the kernel's order: 1.8 .. 2.1x vs torch's
# f32 convolution, profiles/r05w_numerics.txt; on MI355X Winograd measured below the direct kernel)
MAX_RATIO = 2.5


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "winograd.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _tracker(sd, frame, max_batch, winograd):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.weights import synthetic_association_state
    cfg = setup_cfg()
    cfg.INPUT.MIN_SIZE_TEST = 600              # p2 / p3 of >= 128 Winograd blocks per image: the plan takes the Winograd kernel
    cfg.INPUT.MAX_SIZE_TEST = 1000
    cfg.APSE.MAX_BATCH = max_batch
    old = os.environ.get("APSE_F32_WINOGRAD")
    os.environ["APSE_F32_WINOGRAD"] = "1" if winograd else "0"     # read once, when the context is created
    try:
        tr = RcnnTracker(cfg, frame, synthetic_association_state(1), detector_state=sd)
        tr.predictor.predict_batch([np.zeros((frame[0], frame[1], 3), np.uint8)], want_masks=False)   # builds the context
    finally:
        if old is None:
            os.environ.pop("APSE_F32_WINOGRAD")
        else:
            os.environ["APSE_F32_WINOGRAD"] = old
    return tr


def _layer_tensors(tr, frames):
    model = tr.predictor.model
    _, feats = tr.predictor.predict_batch(frames, want_masks=False)
    torch.cuda.synchronize()
    out = {"hw": {k: tuple(feats[k].shape[-2:]) for k in ("p2", "p3")}}
    for oname, iname, _, _ in LAYERS:
        for nm in (oname, iname):
            if nm not in out:
                out[nm] = model.debug_tensor(nm).cpu()
    return out


def _errors(sd, tens, n):
    """per layer: max |y - y64| / max |y64| over the first n images; y64 from the float64 direct convolution of the input"""
    res = {}
    for oname, iname, wname, relu in LAYERS:
        H, W = tens["hw"]["p" + oname[-1]]
        x = tens[iname][: n * H * W * 256].view(n, H, W, 256).permute(0, 3, 1, 2).double()
        y = tens[oname][: n * H * W * 256].view(n, H, W, 256).permute(0, 3, 1, 2).double()
        ref = F.conv2d(x, sd[wname + ".weight"].double(), sd[wname + ".bias"].double(), padding=1)
        if relu:
            ref = F.relu(ref)
        res[oname] = float((y - ref).abs().max() / ref.abs().max())
    return res


@pytest.fixture(scope="module")
def sd():
    from apse_uav_amd.weights import synthetic_detector_state
    return synthetic_detector_state(0, BLOCKS)


@pytest.mark.parametrize("frame_hw,batch", [((270, 480), 1), ((375, 1242), 2), ((721, 1283), 4)])
def test_winograd_layers_vs_float64(sd, logdir, frame_hw, batch):
    from apse_uav_amd.synthetic import SyntheticSequence
    seq = SyntheticSequence("dynamic", *frame_hw)
    frames = [seq.frame(t) for t in range(batch)]
    errs = {}
    for wino in (True, False):
        tr = _tracker(sd, frame_hw, batch, wino)
        errs[wino] = _errors(sd, _layer_tensors(tr, frames), batch)
        del tr
    _log(logdir, "layers_vs_f64", dict(frame=frame_hw, batch=batch, winograd=errs[True], direct=errs[False]))
    for k in errs[True]:
        assert errs[True][k] < 5e-6, (k, errs[True][k])
        assert errs[True][k] <= MAX_RATIO * max(errs[False][k], 1e-7), (k, errs[True][k], errs[False][k])


def test_winograd_same_bits_in_any_batch_and_context(sd, logdir):
    from apse_uav_amd.synthetic import SyntheticSequence
    frame_hw = (270, 480)
    seq = SyntheticSequence("dynamic", *frame_hw)
    f = [seq.frame(t) for t in range(5)]
    tr = _tracker(sd, frame_hw, 4, True)
    alone = _layer_tensors(tr, [f[0]])
    alone.pop("hw")
    n1 = {k: v.numel() // 4 for k, v in alone.items()}
    first = {k: v[: n1[k]] for k, v in alone.items()}
    for frames, slot in (([f[1], f[2], f[0], f[3]], 2), ([f[4], f[0]], 1)):
        got = _layer_tensors(tr, frames)
        for k in first:
            assert torch.equal(got[k][slot * n1[k]:(slot + 1) * n1[k]], first[k]), (k, slot)
    again = _layer_tensors(tr, [f[0]])
    other = _layer_tensors(_tracker(sd, frame_hw, 4, True), [f[0]])
    for k in first:
        assert torch.equal(again[k][: n1[k]], first[k]), k
        assert torch.equal(other[k][: n1[k]], first[k]), k
    _log(logdir, "bits", dict(ok=True, tensors=sorted(first)))
