"""RPN-head fine-tuning beyond one step: anchor labelling and sampling through the device path, the loader, proposal recall, and
tools/finetune_rpn.py (the dry run in a child process, checkpoints, resume, results file, the pushed weights in the detector)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_train_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEV = "cuda:0"
NAME = "R_50_FPN_UAV_RPN"


def _log(logdir, name, obj):
    print(name, json.dumps(obj))
    with open(os.path.join(logdir, "rpn_train.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _model():
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg(num_classes=4)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    return TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)).model


# ------------------------------------------------------------------------------------------------ sampler, loader, recall
def test_sampler_loader_and_recall(tmp_path):
    """label_and_sample_anchors on a context's own anchors (the 256 / 128 rule, positives first, matched boxes that are the argmax),
    RpnTrainLoader down the augmented path with a state_dict that makes a second loader repeat the next batch bit for bit, and
    proposal_recall: 1.0 against ground truths that ARE proposals, 2 / 3 when a third box is one that nothing overlaps, 1 / 3 when
    only the best-scored proposal counts."""
    from eval_detector import synthetic_dataset
    from apse_uav_amd.utils import COCO_utils
    from apse_uav_amd.utils import rpn_train as rt
    model = _model()
    ann = synthetic_dataset(str(tmp_path / "img"), 4, seed=2)
    dicts = COCO_utils.generate_coco_dataset_dictionaries(ann, str(tmp_path / "img"), None, None, False)
    # --- sampling on the first image's context
    loader = rt.RpnTrainLoader(dicts, model, 2, seed=1)
    boxes, _, _ = loader.prepare_image(dicts[0])
    gt = torch.from_numpy(boxes.astype(np.float32))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    sel, lab, matched, (npos, nneg) = rt.label_and_sample_anchors(model, gt, generator=gen)
    torch.cuda.synchronize()
    shapes = model.rpn_level_shapes()
    anc = R.anchors(shapes)[0]
    labels, idx, _ = R.label_anchors(anc, gt)
    cpos, cneg = int((labels == 1).sum()), int((labels == 0).sum())
    assert cpos >= 1 and npos == min(cpos, 128) and nneg == min(cneg, 256 - npos) and sel.numel() == npos + nneg
    assert lab.dtype == torch.int32 and lab.cpu().tolist() == [1] * npos + [0] * nneg
    sel_c = sel.cpu()
    assert sel_c.unique().numel() == sel_c.numel()
    assert bool((labels[sel_c[:npos]] == 1).all()) and bool((labels[sel_c[npos:]] == 0).all())
    assert torch.equal(matched.cpu(), gt[idx[sel_c]])
    gen.manual_seed(3)
    again = rt.label_and_sample_anchors(model, gt, generator=gen)
    assert torch.equal(again[0], sel) and torch.equal(again[2], matched)
    s0, l0, m0, (p0, n0) = rt.label_and_sample_anchors(model, torch.zeros(0, 4), generator=gen)
    assert p0 == 0 and n0 == 256 and int(l0.abs().max()) == 0 and float(m0.abs().max()) == 0.0
    patches, slots, aboxes, levels = model.rpn_patches(sel)
    assert tuple(patches.shape) == (npos + nneg, 2304) and torch.equal(aboxes.cpu(), anc[sel_c])
    # --- the loader down the augmented path
    def make():
        return rt.RpnTrainLoader(dicts, model, 2, seed=1, flip=True, augment=True, min_sizes=(224, 256), max_size=448)
    a = make()
    batch = next(a)
    n = batch[0].shape[0]
    assert [tuple(t.shape) for t in batch] == [(n, 2304), (n,), (n,), (n, 4), (n, 4)]
    assert len(a.last_counts) == 2 and sum(p + q for p, q in a.last_counts) == n
    assert all(1 <= p <= 128 and p + q == 256 for p, q in a.last_counts)
    pos = (batch[2] == 1).cpu()
    assert int(pos.sum()) == sum(p for p, _ in a.last_counts) and int(batch[1].min()) >= 0 and int(batch[1].max()) <= 2
    sd = a.state_dict()
    want = next(a)
    b = make()
    b.load_state_dict(sd)
    got = next(b)
    assert all(torch.equal(x, y) for x, y in zip(want, got)) and a.last_counts == b.last_counts
    with pytest.raises(ValueError):
        rt.RpnTrainLoader(dicts, model, 5)                                            # 5 x 256 rows exceed one step
    # --- recall
    from PIL import Image
    d = dicts[0]
    frame = np.asarray(Image.open(d["file_name"]).convert("RGB"))[:, :, ::-1].copy()
    props = model.rpn_proposals(frames=torch.from_numpy(frame[None]).cuda())[0].cpu()
    assert props.shape[0] >= 3
    from apse_uav_amd.utils import resample
    ih, iw = resample.resize_shortest_edge(d["height"], d["width"], model.cfg.INPUT.MIN_SIZE_TEST, model.cfg.INPUT.MAX_SIZE_TEST)
    sx, sy = d["width"] / iw, d["height"] / ih

    def as_dict(bx):
        anns = [{"bbox": [float(x0 * sx), float(y0 * sy), float((x1 - x0) * sx), float((y1 - y0) * sy)], "iscrowd": 0}
                for x0, y0, x1, y1 in bx]
        return dict(d, annotations=anns)
    hit = rt.proposal_recall(model, [as_dict(props[:3].tolist())], 0.5, (100, 1000))
    assert hit == {100: 1.0, 1000: 1.0}
    # two of three found; with a limit of 1 only the best-scored proposal counts (the second box is a proposal far from the first)
    far = int(torch.nonzero(R.pairwise_iou(props[:1], props)[0] < 0.3)[0])
    mixed = rt.proposal_recall(model, [as_dict([props[0].tolist(), props[far].tolist(), [-900.0, -900.0, -890.0, -890.0]])], 0.5,
                               (1, 100))
    assert mixed[100] == pytest.approx(2 / 3) and mixed[1] == pytest.approx(1 / 3)
    assert rt.proposal_recall(model, [dict(d, annotations=[])]) is None


# ------------------------------------------------------------------------------------------------ loop
ARGS = ["--synthetic", "6", "--iters", "12", "--checkpoint-period", "4"]


def _run(out, *extra):
    import finetune_rpn as ft
    return ft.main(ARGS + ["--out", out] + list(extra))


def test_finetune_loop(tmp_path, logdir):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.networks.rpn_head import PREFIX, RPNHead
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_detector_state
    # the dry run end to end, as a user starts it
    a_dir = str(tmp_path / "a")
    child = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "finetune_rpn.py")] + ARGS + ["--out", a_dir],
                           capture_output=True, text=True, cwd=str(tmp_path))
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert child.stdout.count("loss_rpn_cls") == 12
    for suffix in ("_last", "_bestAR"):
        assert os.path.exists(os.path.join(a_dir, NAME + suffix + ".pth")), suffix
    a_last = os.path.join(a_dir, NAME + "_last.pth")
    chk = torch.load(a_last, map_location="cpu", weights_only=False)
    for key in ("model", "iteration", "optimizer", "scheduler", "kfold_split", "best_recall", "k_folds", "training_results", "loader"):
        assert key in chk, key
    assert chk["iteration"] == 8
    lines = open(os.path.join(a_dir, "results.txt")).read().splitlines()
    assert lines[0].split() == ["AR@100", "AR@1000"] and len(lines) == 3
    for line in lines[1:]:
        r100, r1000 = (float(v) for v in line.replace(" Best recall!", "").split("\t")[1:3])
        assert 0.0 <= r100 <= r1000 <= 1.0
    # it trained: the RPN head moved, nothing else did
    det = synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)
    assert set(chk["model"]) == set(det)
    for k, v in det.items():
        assert torch.equal(chk["model"][k], v) != k.startswith(PREFIX), k
    # interrupted after the checkpoint of iteration 4 and resumed: the resumed run executes iterations 5 .. 11 and writes the
    # checkpoint of iteration 8 itself, from restored weights, momentum, scheduler, loader order and sampling generator.  Its bytes
    # are those of the uninterrupted run's _last
    b_dir = str(tmp_path / "b")
    stopped = _run(b_dir, "--stop-at", "4")
    assert len(stopped["losses"]) == 5
    b_last = os.path.join(b_dir, NAME + "_last.pth")
    at4 = torch.load(b_last, map_location="cpu", weights_only=False)
    assert at4["iteration"] == 4
    b = _run(b_dir, "--resume")
    assert torch.load(b_last, map_location="cpu", weights_only=False)["iteration"] == 8
    assert open(a_last, "rb").read() == open(b_last, "rb").read()
    # the resumed run moved on from the state it restored
    assert not torch.equal(at4["model"][PREFIX + "conv.weight"], chk["model"][PREFIX + "conv.weight"])
    assert len(b["losses"]) == 7 and all(np.isfinite(v) for pair in b["losses"] for v in pair)
    _log(logdir, "rpn loop", {"results": lines, "losses_5_to_11": b["losses"], "after": b["recall_after"]})
    # _last loads into TrackPredictor and detects
    cfg = setup_cfg(num_classes=4)
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0
    pr = TrackPredictor(cfg, state_dict=chk["model"])
    frame = SyntheticSequence("dynamic", 270, 480).frame(0)
    assert len(pr(frame)[0]["instances"]) > 0
    # after push_into the running detector's rpn_head tensors are RPNHead.predict's values (tests/test_gpu_rpn_train.py pins the
    # order; here the trained weights are what the detector computes with)
    pred = b["predictor"]
    model = pred.model
    head = RPNHead(DEV)
    head.load_state_dict(b["state"])
    for k, v in head.state_dict(PREFIX).items():
        assert torch.equal(model._state[k], v.cpu()), k
    model.inference_frames(torch.from_numpy(frame[None]).cuda())
    torch.cuda.synchronize()
    shapes = model.rpn_level_shapes()
    anc, level, ys, xs, slot = R.anchors(shapes)
    g = torch.Generator().manual_seed(12)
    idx, off = [], 0
    for (H, W) in shapes:
        idx.append(off + torch.randperm(3 * H * W, generator=g)[:24])
        off += 3 * H * W
    idx = torch.cat(idx)
    taps = [model.debug_tensor("rpn_head%d" % (l + 2)).reshape(shapes[l][0], shapes[l][1], 16).cpu() for l in range(5)]
    cols = [F.unfold(model.export_feature("p%d" % (l + 2), 1).cpu(), 3, padding=1)[0] for l in range(5)]
    logits, deltas = head.predict(model.rpn_patches(idx.to(DEV))[0])
    got = R.own_columns(logits.cpu(), deltas.cpu(), slot[idx])
    tap_l = torch.stack([taps[int(level[i])][int(ys[i]), int(xs[i]), int(slot[i])] for i in idx])
    tap_d = torch.stack([taps[int(level[i])][int(ys[i]), int(xs[i]), 3 + 4 * int(slot[i]):7 + 4 * int(slot[i])] for i in idx])
    x32 = torch.stack([cols[int(level[i])][:, int(ys[i]) * shapes[int(level[i])][1] + int(xs[i])] for i in idx])
    p64 = R.own_columns(*R.head_outputs(x32.double(), {k: v.cpu().double() for k, v in head.state_dict().items()}), slot[idx])
    for j, tap in enumerate((tap_l, tap_d)):
        eh, ef, bound, ok = R.arbiter(got[j], p64[j], tap)
        assert ok, (j, eh, ef, bound)
