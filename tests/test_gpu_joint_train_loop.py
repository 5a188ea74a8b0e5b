"""-m gpu: joint RPN / box-head fine-tuning (utils/joint_train.py, tools/finetune_uav.py): three steps are deterministic in all
14 parameters, the loader's proposals follow the RPN head from step to step, the chunked box loss over 2048 rows has the
gradients of the loss over all rows, the tool's dry run with checkpoints and resume, and BoxTrainLoader's default path."""
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
K = 4


def _log(logdir, name, obj):
    print(name, json.dumps(obj))
    with open(os.path.join(logdir, "joint_train.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _dataset(tmp_path, n=4, seed=2):
    from eval_detector import synthetic_dataset
    from apse_uav_amd.utils import COCO_utils
    ann = synthetic_dataset(str(tmp_path / "img"), n, seed=seed)
    return COCO_utils.generate_coco_dataset_dictionaries(ann, str(tmp_path / "img"), None, None, False)


def _model(state=None):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    cfg.APSE.CONTEXT_CACHE = 4
    return TrackPredictor(cfg, state_dict=state if state is not None else synthetic_detector_state(0, (1, 1, 1, 1), num_classes=K)).model


def _heads(model):
    from apse_uav_amd.networks.box_head import BoxHead
    from apse_uav_amd.networks.rpn_head import RPNHead
    rpn, box = RPNHead(DEV), BoxHead(K, DEV)
    rpn.load_state_dict(model._state)
    box.load_state_dict(model._state)
    return rpn, box


def _steps(dicts, n, ims_per_batch=2):
    """n joint steps from the synthetic detector: (the 14 parameters on the host, the model, the loader, the heads)."""
    from apse_uav_amd import optim
    from apse_uav_amd.utils.joint_train import JointTrainLoader, box_losses_chunked
    model = _model()
    rpn, box = _heads(model)
    opt = optim.SGD(list(rpn.parameters()) + list(box.parameters()), lr=0.01, momentum=0.9)
    loader = JointTrainLoader(dicts, model, ims_per_batch, seed=1, num_classes=K)
    for _ in range(n):
        r, b = next(loader)
        losses = dict(rpn(*r, ims_per_batch))
        losses.update(box_losses_chunked(box, *b, loader.last_box_rows))
        opt.zero_grad()
        sum(losses.values()).backward()
        opt.step()
        model.set_rpn_head(rpn)
    params = {**{"rpn." + k: v.cpu() for k, v in rpn.state_dict().items()}, **{"box." + k: v.cpu() for k, v in box.state_dict().items()}}
    return params, model, loader, (rpn, box)


def test_three_steps_are_deterministic_and_proposals_follow_the_head(tmp_path):
    from apse_uav_amd.networks.rpn_head import merge_rpn_head
    from apse_uav_amd.weights import synthetic_detector_state
    dicts = _dataset(tmp_path)
    a, model, loader, (rpn, _) = _steps(dicts, 3)
    b, _, _, _ = _steps(dicts, 3)
    assert len(a) == 14
    start = synthetic_detector_state(0, (1, 1, 1, 1), num_classes=K)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    moved = [k for k in a if not torch.equal(a[k], start[("proposal_generator.rpn_head." if k.startswith("rpn.") else "roi_heads.") + k[4:]])]
    assert len(moved) == 14, moved                     # every tensor trained
    assert model.contexts_built <= len({(d["height"], d["width"]) for d in dicts})        # the refresh rebuilt nothing
    # the proposals the loader draws for the next image are those of a fresh model with the merged head
    sd = loader.state_dict()
    next(loader)
    got = loader.last_proposals[0]
    fresh = _model(merge_rpn_head(start, rpn.state_dict()))
    from apse_uav_amd.utils.joint_train import JointTrainLoader
    other = JointTrainLoader(dicts, fresh, 2, seed=1, num_classes=K)
    other.load_state_dict(sd)
    next(other)
    want = other.last_proposals[0]
    assert got.shape[0] > 0 and torch.equal(got.cpu(), want.cpu())
    # ... and not those of the head the run started from
    old = JointTrainLoader(dicts, _model(), 2, seed=1, num_classes=K)
    old.load_state_dict(sd)
    next(old)
    assert not (old.last_proposals[0].shape == got.shape and torch.equal(old.last_proposals[0].cpu(), got.cpu()))


def test_loader_batch_and_state(tmp_path):
    from apse_uav_amd.utils.joint_train import JointTrainLoader
    dicts = _dataset(tmp_path)
    model = _model()

    def make():
        return JointTrainLoader(dicts, model, 2, seed=1, flip=True, augment=True, min_sizes=(224, 256), max_size=448, num_classes=K)
    a = make()
    rpn, box = next(a)
    n, m = rpn[0].shape[0], box[0].shape[0]
    assert tuple(rpn[0].shape) == (n, 2304) and all(t.shape[0] == n for t in rpn) and n <= 512
    assert tuple(box[0].shape) == (m, 7, 7, 256) and all(t.shape[0] == m for t in box) and sum(a.last_box_rows) == m
    assert all(p + q <= 256 for p, q in a.last_rpn_counts) and all(1 <= f <= 128 and f + g <= 512 for f, g in a.last_box_counts)
    sd = a.state_dict()
    assert "rpn_generator" in sd and "box_generator" in sd
    want = next(a)
    b = make()
    b.load_state_dict(sd)
    got = next(b)
    for x, y in zip(want[0] + want[1], got[0] + got[1]):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        JointTrainLoader(dicts, model, 5)              # 5 x 256 RPN rows exceed one step


def test_chunk_rule_against_the_loss_over_all_rows(logdir):
    """Four images of 512 box rows each: two chunks of 1024.  The gradients that the weighted chunk losses accumulate in the
    eight box tensors against torch on the CPU taking all 2048 rows at once, in float64 and float32: the arbiter rule of
    tests/mask_train_ref.py with its factor 2."""
    from apse_uav_amd.networks import box_head as bh
    from apse_uav_amd.utils.joint_train import box_chunks, box_losses_chunked
    n, rows = 2048, [512] * 4
    assert box_chunks(rows) == [(0, 1024), (1024, 2048)] and box_chunks([512, 300, 512, 100]) == [(0, 812), (812, 1424)]
    assert box_chunks([1024, 1, 1023]) == [(0, 1024), (1024, 2048)] and box_chunks([]) == []
    g = torch.Generator().manual_seed(12)
    x = torch.relu(torch.randn(n, 256, 7, 7, generator=g))
    labels, props, gts = R.sample_batch(n, K, 13, related=True)
    sd = R.seeded_state(K, 14)
    (lc64, lb64), g64 = R.head_step(x, sd, labels, props, gts, torch.float64)
    (lc32, lb32), g32 = R.head_step(x, sd, labels, props, gts, torch.float32)
    head = bh.BoxHead(K, DEV)
    head.load_state_dict(sd)
    xd = R.nhwc(x).to(DEV)
    losses = box_losses_chunked(head, xd, labels, props, gts, rows)
    (losses["loss_cls"] + losses["loss_box_reg"]).backward()
    torch.cuda.synchronize()
    out = {}
    for name, hip, f64, f32 in [("loss_cls", losses["loss_cls"], lc64, lc32), ("loss_box_reg", losses["loss_box_reg"], lb64, lb32)] + \
            [(k, p.grad, g64[k], g32[k]) for k, p in head.named_parameters()]:
        eh, ef, bound, ok = R.arbiter(hip, f64, f32, factor=2.0)
        out[name] = {"err_hip": eh, "err_f32": ef, "bound": bound, "ok": ok}
    _log(logdir, "chunk rule n=2048", out)
    assert len(out) == 10 and all(v["ok"] for v in out.values()), out
    with pytest.raises(ValueError):
        box_chunks([1025])


# ------------------------------------------------------------------------------------------------ the tool
def _run(out, *extra):
    import finetune_uav as ft
    return ft.main(["--synthetic", "6", "--iters", "12", "--checkpoint-period", "4", "--out", out] + list(extra))


def test_finetune_uav_dry_run_and_resume(tmp_path, logdir):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    a_dir = str(tmp_path / "a")
    a = _run(a_dir)
    name = "R_50_FPN_UAV"
    for suffix in ("_last", "_bestAP", "_bestAR"):
        assert os.path.exists(os.path.join(a_dir, name + suffix + ".pth")), suffix
    chk = torch.load(a["checkpoint"], map_location="cpu", weights_only=False)
    for key in ("model", "iteration", "optimizer", "scheduler", "kfold_split", "best_precision", "best_recall", "k_folds",
                "training_results", "loader"):
        assert key in chk, key
    assert chk["iteration"] == 8
    lines = open(os.path.join(a_dir, "results.txt")).read().splitlines()
    assert lines[0].split()[:1] == ["AP"] and lines[0].split()[-2:] == ["prop_AR@100", "prop_AR@1000"]
    assert len(a["losses"]) == 12 and all(np.isfinite(v) for row in a["losses"] for v in row) and len(a["losses"][0]) == 4
    _log(logdir, "loop", {"losses": a["losses"], "tests": a["tests"]})
    # both heads of _last differ from the start, and it loads into TrackPredictor and detects
    from apse_uav_amd.weights import synthetic_detector_state
    start = synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)
    for k in ("proposal_generator.rpn_head.conv.weight", "roi_heads.box_head.fc1.weight"):
        assert not torch.equal(chk["model"][k], start[k]), k
    assert torch.equal(chk["model"]["backbone.bottom_up.stem.conv1.weight"], start["backbone.bottom_up.stem.conv1.weight"])
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


def test_ims_per_batch_above_four_is_refused(tmp_path):
    import finetune_uav as ft
    with pytest.raises(SystemExit):
        ft.main(["--synthetic", "6", "--iters", "1", "--ims-per-batch", "5", "--out", str(tmp_path / "x")])


# ------------------------------------------------------------------------------------------------ the box loader
def test_box_loader_default_path_is_the_inference_selection(tmp_path):
    """Without train_topk BoxTrainLoader samples from proposals_after_backbone, as before: its batches equal, bit for bit, those
    of a restatement of that path (the loader's own draws, the inference proposals, label_and_sample_proposals, ROIAlign 7).
    With train_topk = (1000, 1000) the training selection returns the same proposals, so the batches are the same again; with
    (2000, 1000) the proposals come from apse_rpn_train_proposals."""
    from apse_uav_amd.utils import box_train as bt
    dicts = _dataset(tmp_path)
    model = _model()
    a = bt.BoxTrainLoader(dicts, model, 2, seed=1, num_classes=K)
    assert a.train_topk is None
    want = next(a)
    # the restatement: the same image order and generator, the proposals asked from the model directly
    b = bt.BoxTrainLoader(dicts, model, 2, seed=1, num_classes=K)
    rows = []
    for _ in range(2):
        if not b._order:
            b._order = [int(i) for i in b.rng.permutation(len(dicts))]
        d = dicts[b._order.pop(0)]
        boxes, _, classes = b.prepare_image(d, False)
        keep = [i for i, an in enumerate(d["annotations"]) if not an.get("iscrowd", 0)]
        gt = torch.from_numpy(np.asarray(boxes, np.float64)[keep].astype(np.float32)).reshape(-1, 4).to(model.device)
        cls = torch.as_tensor(classes)[keep].to(model.device, torch.int32)
        props = model.proposals_after_backbone(1)[0]
        sb, labels, matched, _ = bt.label_and_sample_proposals(props, gt, cls, K, 512, 0.25, b.generator, 0.5)
        rows.append((model.box_roi_features(sb), labels, sb, matched))
    for k in range(4):
        assert torch.equal(want[k], torch.cat([r[k] for r in rows])), k
    same = next(bt.BoxTrainLoader(dicts, model, 2, seed=1, num_classes=K, train_topk=(1000, 1000)))
    for k in range(4):
        assert torch.equal(want[k], same[k]), k
    c = bt.BoxTrainLoader(dicts, model, 2, seed=1, num_classes=K, train_topk=(2000, 1000))
    assert c.train_topk == (2000, 1000)
    got = next(c)
    assert tuple(got[0].shape[1:]) == (7, 7, 256) and bool(torch.isfinite(got[0]).all())
