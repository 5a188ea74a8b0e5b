"""Box-head fine-tuning beyond one step: the 20-step trajectory against torch CPU in float64 and float32, proposal labelling and
sampling through the device path, and tools/finetune_box_head.py (checkpoints, resume, results file, another class count)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import box_train_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
DEV = "cuda:0"


def _log(logdir, name, obj):
    print(name, json.dumps(obj))
    with open(os.path.join(logdir, "box_train.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


# ------------------------------------------------------------------------------------------------ trajectory
def test_trajectory_against_torch(logdir):
    """20 steps of apse_uav_amd.optim.SGD (lr 0.02, momentum 0.9) on one fixed batch (K = 4, n = 256, seeded features, about a
    quarter foreground) from detectron2's seeded initialisation: HIP against the torch CPU restatement in float64 and float32;
    the arbiter rule with factor 4 on both losses at every step, and both losses fall in all three runs."""
    from apse_uav_amd import optim
    from apse_uav_amd.networks import box_head as bh
    K, n, steps = 4, 256, 20
    g = torch.Generator().manual_seed(9)
    x = torch.relu(torch.randn(n, 256, 7, 7, generator=g))
    labels, props, gts = R.sample_batch(n, K, 10, related=True)
    torch.manual_seed(5)
    sd = {k: v.cpu() for k, v in bh.BoxHead(K, DEV).state_dict().items()}
    curves = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        p = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.SGD(list(p.values()), lr=0.02, momentum=0.9)
        xx, pp, gg = x.to(dt), props.to(dt), gts.to(dt)
        out = []
        for _ in range(steps + 1):
            opt.zero_grad()
            lc, lb = R.box_losses(*R.head_outputs(xx, p), labels, pp, gg)
            (lc + lb).backward()
            out.append((float(lc), float(lb)))
            opt.step()
        curves[name] = out
    head = bh.BoxHead(K, DEV)
    head.load_state_dict(sd)
    opt = optim.SGD(list(head.parameters()), lr=0.02, momentum=0.9)
    xd = R.nhwc(x).to(DEV)
    out = []
    for _ in range(steps + 1):
        opt.zero_grad()
        losses = head(xd, labels, props, gts)
        (losses["loss_cls"] + losses["loss_box_reg"]).backward()
        out.append((float(losses["loss_cls"].detach().double()), float(losses["loss_box_reg"].detach().double())))
        opt.step()
    curves["hip"] = out
    rows = []
    for i in range(steps + 1):
        row = {"step": i}
        for j, nm in enumerate(("loss_cls", "loss_box_reg")):
            t = [torch.tensor([curves[k][i][j]], dtype=torch.float64) for k in ("hip", "f64", "f32")]
            eh, ef, bound, ok = R.arbiter(t[0], t[1], t[2], factor=4.0)
            row[nm] = {"hip": curves["hip"][i][j], "f32": curves["f32"][i][j], "f64": curves["f64"][i][j], "err_hip": eh,
                       "err_f32": ef, "bound": bound, "ok": ok}
        rows.append(row)
    _log(logdir, "trajectory", rows)
    for k in ("hip", "f32", "f64"):
        for j in (0, 1):
            assert curves[k][steps][j] < curves[k][0][j], (k, j, curves[k][0], curves[k][steps])
    bad = [r for r in rows if not (r["loss_cls"]["ok"] and r["loss_box_reg"]["ok"])]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ sampler
def test_sampler_through_the_device_path():
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import box_train as bt
    from apse_uav_amd.weights import synthetic_detector_state
    K = 4
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    model = TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1))).model
    frames = torch.from_numpy(SyntheticSequence("dynamic", 360, 640).frame(0)[None]).cuda()
    props = model.rpn_proposals(frames=frames)[0]
    P = props.shape[0]
    assert P >= 11
    # three ground truths: proposals 0, 5 and 10 grown by a pixel on every side, so that some proposals are foreground
    gts = (props[[0, 5, 10]] + torch.tensor([-1.0, -1.0, 1.0, 1.0], device=DEV)).contiguous()
    cls = torch.tensor([2, 0, 3])
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    boxes, labels, matched, (nfg, nbg) = bt.label_and_sample_proposals(props, gts, cls, K, generator=gen)
    torch.cuda.synchronize()
    boxes, labels, matched, gc, pc = boxes.cpu(), labels.cpu().long(), matched.cpu(), gts.cpu(), props.cpu()
    # the 512 / 128 rule on the restatement's labels of the candidates (proposals, then the ground truths)
    cand = torch.cat([pc, gc])
    _, _, cand_lab = R.match(cand, gc, cls, K)
    cfg_n, cbg_n = int((cand_lab != K).sum()), int((cand_lab == K).sum())
    assert cfg_n >= 3
    assert nfg == min(cfg_n, 128) and nbg == min(cbg_n, 512 - nfg) and boxes.shape[0] == nfg + nbg
    assert bool((labels[:nfg] != K).all()) and bool((labels[nfg:] == K).all())            # foreground rows first
    # every ground-truth box is among the candidates: with at most 128 foreground candidates all of them are drawn
    if cfg_n <= 128:
        for b in gc:
            assert bool((boxes[:nfg] == b).all(dim=1).any())
    # every sampled row is a candidate, none twice unless the candidates repeat a box
    assert all(bool((cand == b).all(dim=1).any()) for b in boxes)
    q = R.pairwise_iou(gc, boxes)                                  # [3][n]
    for r in range(nfg):
        j = int((gc == matched[r]).all(dim=1).nonzero()[0])
        assert float(q[j, r]) >= 0.5 and float(q[j, r]) == float(q[:, r].max()) and int(labels[r]) == int(cls[j])
    assert float(q[:, nfg:].max()) < 0.5 if nbg else True
    # the same generator seed draws the same rows; without ground truth everything is background
    gen.manual_seed(3)
    again = bt.label_and_sample_proposals(props, gts, cls, K, generator=gen)
    assert torch.equal(again[0].cpu(), boxes) and torch.equal(again[1].cpu().long(), labels)
    b0, l0, m0, (f0, g0) = bt.label_and_sample_proposals(props, torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64), K, generator=gen)
    assert f0 == 0 and g0 == min(P, 512) and bool((l0 == K).all()) and float(m0.abs().max()) == 0.0
    feats = model.box_roi_features(boxes)
    assert tuple(feats.shape) == (nfg + nbg, 7, 7, 256) and bool(torch.isfinite(feats).all())


def test_loader_device_path_and_state(tmp_path):
    """BoxTrainLoader down the augmented path (two sizes, flip, colour chain): batch shapes, the 512 / 128 rule per image, foreground
    rows that overlap their matched boxes, and a state_dict that makes a second loader repeat the next batch bit for bit."""
    from eval_detector import synthetic_dataset
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.utils import COCO_utils
    from apse_uav_amd.utils.box_train import BoxTrainLoader
    from apse_uav_amd.weights import synthetic_detector_state
    K = 4
    ann = synthetic_dataset(str(tmp_path / "img"), 4, seed=2)
    dicts = COCO_utils.generate_coco_dataset_dictionaries(ann, str(tmp_path / "img"), None, None, False)
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    model = TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1), num_classes=K)).model

    def make():
        return BoxTrainLoader(dicts, model, 2, seed=1, flip=True, augment=True, min_sizes=(224, 256), max_size=448)
    a = make()
    feats, labels, boxes, matched = next(a)
    n = feats.shape[0]
    assert tuple(feats.shape) == (n, 7, 7, 256) and tuple(labels.shape) == (n,) and tuple(boxes.shape) == (n, 4) == tuple(matched.shape)
    assert labels.dtype == torch.int32 and int(labels.min()) >= 0 and int(labels.max()) <= K and bool(torch.isfinite(feats).all())
    assert len(a.last_counts) == 2 and sum(f + b for f, b in a.last_counts) == n
    assert all(1 <= f <= 128 and f + b <= 512 for f, b in a.last_counts)              # the ground truths themselves are foreground
    fg = (labels != K).cpu()
    iou = R.pairwise_iou(boxes.cpu()[fg], matched.cpu()[fg]).diagonal()
    assert int(fg.sum()) == sum(f for f, _ in a.last_counts) and float(iou.min()) >= 0.5
    sd = a.state_dict()
    want = next(a)
    b = make()
    b.load_state_dict(sd)
    got = next(b)
    assert all(torch.equal(x, y) for x, y in zip(want, got)) and a.last_counts == b.last_counts
    with pytest.raises(ValueError):
        BoxTrainLoader(dicts, model, 3)                                               # 3 x 512 RoIs exceed one step


# ------------------------------------------------------------------------------------------------ loop
def _run(out, *extra):
    import finetune_box_head as ft
    return ft.main(["--synthetic", "6", "--iters", "12", "--checkpoint-period", "4", "--out", out] + list(extra))


def test_finetune_loop(tmp_path, logdir):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    a_dir = str(tmp_path / "a")
    a = _run(a_dir)
    name = "R_50_FPN_UAV_BOX"
    for suffix in ("_last", "_bestAP", "_bestAR"):
        assert os.path.exists(os.path.join(a_dir, name + suffix + ".pth")), suffix
    chk = torch.load(a["checkpoint"], map_location="cpu", weights_only=False)
    for key in ("model", "iteration", "optimizer", "scheduler", "kfold_split", "best_precision", "best_recall", "k_folds",
                "training_results", "loader"):
        assert key in chk, key
    assert chk["iteration"] == 8
    lines = open(os.path.join(a_dir, "results.txt")).read().splitlines()
    assert lines[0].split() == ["AP", "AP_05", "AP0.75", "AP_s", "AP_m", "AP_l", "AR_1", "AR_10", "AR_100", "AR_s", "AR_m", "AR_l"]
    assert len(a["losses"]) == 12 and all(np.isfinite(v) for pair in a["losses"] for v in pair)
    _log(logdir, "loop", {"losses": a["losses"], "tests": a["tests"]})
    # _last loads into TrackPredictor and detects
    cfg = setup_cfg(num_classes=4)
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0
    pr = TrackPredictor(cfg, state_dict=chk["model"])
    inst = pr(SyntheticSequence("dynamic", 270, 480).frame(0))[0]["instances"]
    assert len(inst) > 0
    # interrupted at 8, resumed: the same bytes in _last and the same final weights, bitwise
    b_dir = str(tmp_path / "b")
    _run(b_dir, "--stop-at", "8")
    b = _run(b_dir, "--resume")
    assert open(a["checkpoint"], "rb").read() == open(b["checkpoint"], "rb").read()
    for k, v in a["state"].items():
        assert torch.equal(v, b["state"][k]), k


def test_finetune_other_class_count(tmp_path):
    """--classes with three names on the 4-class synthetic checkpoint: fresh predictor layers of 4 and 12 rows, fc1 / fc2 from the
    checkpoint."""
    import finetune_box_head as ft
    from apse_uav_amd.weights import synthetic_detector_state
    base = ["--synthetic", "6", "--classes", "c0", "c1", "c2", "--checkpoint-period", "4"]
    start = ft.main(base + ["--iters", "0", "--out", str(tmp_path / "s")])
    det = synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)
    assert start["num_classes"] == 3
    for nm in ("box_head.fc1", "box_head.fc2"):
        for s in (".weight", ".bias"):
            assert torch.equal(start["state"][nm + s], det["roi_heads." + nm + s]), nm + s
    assert tuple(start["state"]["box_predictor.cls_score.weight"].shape) == (4, 1024)
    assert tuple(start["state"]["box_predictor.bbox_pred.weight"].shape) == (12, 1024)
    assert not torch.equal(start["state"]["box_predictor.cls_score.weight"], det["roi_heads.box_predictor.cls_score.weight"][:4])
    run = ft.main(base + ["--iters", "5", "--out", str(tmp_path / "r")])
    chk = torch.load(run["checkpoint"], map_location="cpu", weights_only=False)
    assert tuple(chk["model"]["roi_heads.box_predictor.cls_score.weight"].shape) == (4, 1024)
    assert tuple(chk["model"]["roi_heads.box_predictor.bbox_pred.weight"].shape) == (12, 1024)
    assert tuple(chk["model"]["roi_heads.mask_head.predictor.weight"].shape)[0] == 3
    assert not torch.equal(chk["model"]["roi_heads.box_head.fc2.weight"], det["roi_heads.box_head.fc2.weight"])      # it trained
