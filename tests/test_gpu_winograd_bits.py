"""-m gpu: the fused f32 Winograd layers give the bits they gave before the k loop of conv_winograd_f32 was re-scheduled.

For the frame sizes and batches of test_gpu_winograd.py (resize 600 / 1000, BLOCKS = (1, 1, 1, 1), seeded frames and weights) the
sha256 of `debug_tensor` of p2, p3, rpn_t2, rpn_t3 equals tests/golden/winograd_layer_sha256.json, which
tools/record_winograd_hashes.py recorded with the library of the commit before the re-schedule (APSE_HIP_LIB).  The kernels
involved are deterministic and the re-schedule keeps every accumulator's order of products, so there is no tolerance.  inner2 /
inner3 (the layers' inputs, produced by kernels this change does not touch) are hashed too: when they differ the mismatch is
upstream of the Winograd kernel, and the message says so.

test_plans_keep_their_bits pins every plan variant the same way (PLAN_CASES; the file's "plans" section, recorded with the library
of the commit before the host code was split into plan.hip / detector.hip / ops.hip, whose apse_version() is stored as
"plans_recorded_with"): a change that only moves host code launches the same kernels with the same arguments, so the results
block and the debug tensors of one detecting forward and one forward on given boxes keep their bytes.
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


# ---------------------------------------------------------------------------------------------- every plan variant
# name -> frame, batch, arch, dtype, classes, (min, max) test size or None for the config's own, environment read when the context
# is built, and the maps hashed on top of PLAN_TENSORS
PLAN_CASES = {
    "fpn_f32": dict(frame=(721, 1283), batch=4, arch="FPN", dtype="f32", classes=4, size=(600, 1000), env={},
                    maps=("rpn_t2", "rpn_head2", "rpn_head3", "rpn_head4", "rpn_head5", "rpn_head6", "p6")),
    "fpn_f32_80cls": dict(frame=(375, 1242), batch=2, arch="FPN", dtype="f32", classes=80, size=None, env={},
                          maps=("box_probs", "cand_boxes")),
    "fpn_bf16": dict(frame=(375, 1242), batch=2, arch="FPN", dtype="bf16", classes=4, size=None, env={},
                     maps=("stem", "res2", "p2")),
    "fpn_f16_unfused": dict(frame=(270, 480), batch=1, arch="FPN", dtype="f16", classes=4, size=None,
                            env={"APSE_NO_STEM_FUSE": "1", "APSE_NO_BNECK_FUSE": "1", "APSE_NO_ASSOC_FC": "1"},
                            maps=("stem.conv1", "res2")),
    "c4_f32": dict(frame=(375, 1242), batch=1, arch="C4", dtype="f32", classes=4, size=None, env={},
                   maps=("res4", "box_res5", "box_mean")),
}
PLAN_TENSORS = ("box_pred", "det_boxes", "mask_logits", "embedding_raw")
# Left out of the pin by name: what two recordings with one library did not reproduce ("pass/name").  Nothing: both recordings
# of the parent library gave the same hash for every entry of every configuration.
PLAN_NOT_DETERMINISTIC = ()
PLAN_MUST_KEEP = ("results", "mask_logits")      # of both passes of every configuration: the pin cannot be emptied


def plan_hashes(name):
    """{"detect/<x>", "given/<x>": sha256} for x = the raw results block and the debug tensors of configuration `name`: a fresh
    context with seeded weights, one detecting forward on seeded frames, then one forward on 8 fixed given boxes per image."""
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import resample
    from apse_uav_amd.weights import synthetic_association_state, synthetic_c4_state, synthetic_detector_state
    c = PLAN_CASES[name]
    frame_hw, batch, k = c["frame"], c["batch"], c["classes"]
    cfg = setup_cfg(num_classes=k, arch=c["arch"])
    if c["size"]:
        cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = c["size"]
    cfg.APSE.MAX_BATCH = batch
    cfg.APSE.DTYPE = c["dtype"]
    cfg.APSE.STORAGE16 = c["dtype"] != "f32"
    if c["arch"] == "C4":
        sd, asd = synthetic_c4_state(0, BLOCKS), synthetic_association_state(1, depth=1024)
    else:
        sd, asd = synthetic_detector_state(0, BLOCKS, num_classes=k), synthetic_association_state(1)
    seq = SyntheticSequence("dynamic", *frame_hw)
    ih, iw = resample.resize_shortest_edge(frame_hw[0], frame_hw[1], cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    i = np.arange(8, dtype=np.float32)
    x0, y0 = (0.05 + 0.1 * i) * iw, (0.1 + 0.08 * i) * ih
    boxes = np.stack([x0, y0, np.minimum(x0 + 24 + 12 * i, iw - 1), np.minimum(y0 + 20 + 10 * i, ih - 1)], 1).astype(np.float32)
    given = (np.tile(boxes, (batch, 1)), np.tile(np.arange(8, dtype=np.int32) % k, batch), np.full(batch, 8, np.int32))
    out = {}
    env = dict(c["env"], APSE_F32_WINOGRAD="1")          # read when the context is built, which may be as late as the first forward
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        tr = RcnnTracker(cfg, frame_hw, asd, detector_state=sd)
        pr = tr.predictor
        model = pr.model
        dev = pr._upload([seq.frame(t) for t in range(batch)])
        for tag, g in (("detect", None), ("given", given)):
            model.preprocess_frames(dev)
            model.run(batch, g)
            res = model.read(batch)
            out[tag + "/results"] = hashlib.sha256(res.raw).hexdigest()
            out[tag + "/total"] = int(res.total)             # not a hash: tells a reader what the forward found
            for t in PLAN_TENSORS + c["maps"]:
                data = model.debug_tensor(t, dtype=torch.uint8).cpu().contiguous()
                out[tag + "/" + t] = hashlib.sha256(data.numpy().tobytes()).hexdigest()
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n)
            else:
                os.environ[n] = v
    return out


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_plans_keep_their_bits(name):
    golden = json.load(open(GOLDEN))["plans"][name]
    got = plan_hashes(name)
    print(name, json.dumps(got))
    keys = [k for k in sorted(golden) if k not in PLAN_NOT_DETERMINISTIC]
    for tag in ("detect", "given"):
        for must in PLAN_MUST_KEEP:
            assert tag + "/" + must in keys, "%s/%s must stay in the pin" % (tag, must)
    assert sorted(got) == sorted(golden), "the recorded entries of %s are not the ones the test computes" % name
    differ = [k for k in keys if got[k] != golden[k]]
    assert not differ, "%s: differs from the recorded bits of the parent library: %s" % (name, differ)
