"""-m gpu: tools/finetune_uav.py --mask, the dry run on generated data: three heads under one optimiser, the segm columns in
results.txt, a checkpoint whose mask head moved and that loads into TrackPredictor, and ``--resume`` bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
NAME = "R_50_FPN_UAV"


def _run(out, *extra):
    import finetune_uav as ft
    return ft.main(["--synthetic", "6", "--iters", "12", "--checkpoint-period", "4", "--mask", "--out", out] + list(extra))


def test_finetune_uav_mask_dry_run_and_resume(tmp_path):
    import finetune_uav as tool
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.networks.mask_head import PREFIX, MaskHead
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_detector_state
    a_dir = str(tmp_path / "a")
    a = _run(a_dir)
    # five finite losses per iteration, loss_mask last
    assert len(a["losses"]) == 12 and all(len(row) == 5 and all(np.isfinite(v) for v in row) for row in a["losses"])
    assert all(row[4] > 0 for row in a["losses"])                   # every generated annotation has a polygon
    # results.txt: the extended header, and 12 + 2 + 12 numbers per scored line
    lines = open(os.path.join(a_dir, "results.txt")).read().splitlines()
    assert lines[0] + "\n" == tool.results_header(True)
    head = lines[0].split()
    assert head[:1] == ["AP"] and head[12:14] == ["prop_AR@100", "prop_AR@1000"] and head[14] == "segm_AP" and len(head) == 26
    assert len(lines) == 3                                           # checkpoints at 4 and 8
    for line in lines[1:]:
        cols = line.split("\t")[1:]
        cols[-1] = cols[-1].split(" ")[0]                            # " Best precision!" / " Best recall!"
        assert len(cols) == 26 and all(np.isfinite(float(c)) for c in cols), line
    assert all(len(res) == 26 for _, res in a["tests"]) and len(a["before"]) == 26 and len(a["after"]) == 26
    # the three heads of _last moved, the trunk did not
    for suffix in ("_last", "_bestAP", "_bestAR"):
        assert os.path.exists(os.path.join(a_dir, NAME + suffix + ".pth")), suffix
    chk = torch.load(a["checkpoint"], map_location="cpu", weights_only=False)
    assert chk["iteration"] == 8
    start = synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)
    for name in MaskHead.names:
        assert not torch.equal(chk["model"][PREFIX + name], start[PREFIX + name]), name
    for k in ("proposal_generator.rpn_head.conv.weight", "roi_heads.box_head.fc1.weight"):
        assert not torch.equal(chk["model"][k], start[k]), k
    assert torch.equal(chk["model"]["backbone.bottom_up.stem.conv1.weight"], start["backbone.bottom_up.stem.conv1.weight"])
    assert sorted(chk["model"]) == sorted(start)
    assert len(a["state"]) == 14 + 12
    # the checkpoint loads into TrackPredictor and runs a frame, masks included
    cfg = setup_cfg(num_classes=4)
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0
    inst = TrackPredictor(cfg, state_dict=chk["model"])(SyntheticSequence("dynamic", 270, 480).frame(0))[0]["instances"]
    assert len(inst) > 0 and inst.has("pred_masks") and len(inst.pred_masks) == len(inst)
    # the summary's predictor holds the final heads (push: none undoes another)
    final = a["predictor"].model._state
    for k, v in a["state"].items():
        assert torch.equal(final[k], v), k
    # interrupted at 8, resumed to 12: the same checkpoint bytes, results.txt and final weights
    b_dir = str(tmp_path / "b")
    _run(b_dir, "--stop-at", "8")
    b = _run(b_dir, "--resume")
    ca = torch.load(a["checkpoint"], map_location="cpu", weights_only=False)
    cb = torch.load(b["checkpoint"], map_location="cpu", weights_only=False)
    assert sorted(ca["model"]) == sorted(cb["model"])
    for k, v in ca["model"].items():
        assert torch.equal(v, cb["model"][k]), k
    assert open(os.path.join(a_dir, "results.txt")).read() == open(os.path.join(b_dir, "results.txt")).read()
    assert a["losses"][9:] == b["losses"]
    for k, v in a["state"].items():
        assert torch.equal(v, b["state"][k]), k
