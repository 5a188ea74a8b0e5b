"""Host side of utils/finetune.py: the bookkeeping of the shared fine-tune loop (results file, best checkpoints, resume) under a
stub task -- one tiny CPU tensor as the head, a scripted score -- no GPU needed."""
import argparse
import json
import os
import types

import pytest
import torch

from apse_uav_amd.networks.head_base import TrainableHead
from apse_uav_amd.utils import finetune as ft

NAME = "STUB"


class StubHead(TrainableHead):
    prefix = "roi_heads.stub."
    names = ["w.weight"]
    noun = "stub-head"

    def __init__(self):
        super().__init__({"w.weight": (3,)}, "cpu")

    def _init_tensor(self, name, t):
        torch.nn.init.normal_(t, std=1.0)


class StubLoader:
    """Batch n is a function of n alone; the state is n."""

    def __init__(self):
        self.n = 0

    def __next__(self):
        self.n += 1
        return (torch.arange(3, dtype=torch.float32) + self.n,)

    def state_dict(self):
        return {"n": self.n}

    def load_state_dict(self, sd):
        self.n = sd["n"]


class StubTask(ft.Task):
    what = "stub"
    coco_ground_truth = False

    def __init__(self, script, **settings):
        self.script = script                  # {batches served so far: the scores do_test returns} (absent: None)
        self.pushes = 0
        for k, v in settings.items():
            assert hasattr(ft.Task, k), k
            setattr(self, k, v)

    def num_classes(self, args, detector, dicts):
        return 4

    def build_heads(self, args, cfg, detector, K):
        self.heads = [StubHead()]
        return detector

    def merged_state(self, detector):
        return StubHead.merge_into(detector, self.heads[0].state_dict())

    def optimizer(self, args, params):
        return torch.optim.SGD(params, lr=args.lr, momentum=args.momentum)

    def predictor(self, cfg, state):
        return types.SimpleNamespace(model=None, state=state)

    def make_loader(self, args, dicts, model, K, sizes):
        assert sizes == {"min_sizes": None, "max_size": None}
        self.loader = StubLoader()
        return self.loader

    def losses(self, batch, loader, args):
        return {"loss_a": (self.heads[0]._params["w.weight"] * batch[0]).sum(), "loss_b": (self.heads[0]._params["w.weight"] ** 2).sum()}

    def push(self, pred):
        self.pushes += 1

    def do_test(self, pred, dicts, coco_gt):
        assert coco_gt is None and len(dicts) >= 1
        return self.script.get(self.loader.n)


def scores(n, **at):
    out = [0.0] * n
    for k, v in at.items():
        out[int(k[1:])] = v
    return out


def run(tmp_path, sub, task, *extra):
    ann = str(tmp_path / "annotations.json")
    if not os.path.exists(ann):
        images = [dict(id=i + 1, file_name="%d.png" % i, height=8, width=8) for i in range(6)]
        anns = [dict(id=i + 1, image_id=i + 1, category_id=i % 4, bbox=[1, 1, 4, 4], area=16, iscrowd=0, segmentation=[[1, 1, 5, 1, 5, 5]])
                for i in range(6)]
        with open(ann, "w") as fh:
            json.dump(dict(images=images, annotations=anns, categories=[dict(id=c, name="c%d" % c) for c in range(4)]), fh)
    ap = argparse.ArgumentParser()
    ft.add_common_arguments(ap, NAME)
    out = str(tmp_path / sub)
    os.makedirs(out, exist_ok=True)
    args = ap.parse_args(["--annotations", ann, "--images", str(tmp_path), "--out", out, "--iters", "11", "--checkpoint-period", "2",
                          "--warmup-iters", "4"] + list(extra))
    return ft.run(task, args, {"backbone.x": torch.ones(2)}), out


def load(out, suffix):
    return torch.load(os.path.join(out, NAME + suffix + ".pth"), map_location="cpu", weights_only=False)


# checkpoints at iterations 2, 4, 6, 8, 10 = after 3, 5, 7, 9, 11 batches; (precision, recall) scripted, nothing scored at 2
def script(n, p, r):
    return {0: scores(n, **{"i%d" % r: 0.05}), 5: scores(n, **{"i%d" % p: 0.5, "i%d" % r: 0.2}), 7: scores(n, **{"i%d" % p: 0.4, "i%d" % r: 0.3}),
            9: scores(n, **{"i%d" % p: 0.6, "i%d" % r: 0.3}), 11: scores(n, **{"i%d" % p: 0.1, "i%d" % r: 0.1})}


@pytest.mark.parametrize("n,p,r", [(12, 0, 8), (2, None, 0), (14, 0, 12)])
def test_results_file_marks(tmp_path, n, p, r):
    task = StubTask(script(n, 1 if p is None else p, r), precision_index=p, recall_index=r, header="\t\thead\n",
                    summary_keys=("before", "after"))
    summary, out = run(tmp_path, "a", task)
    lines = open(os.path.join(out, "results.txt")).read().splitlines()
    assert lines[0] == "\t\thead" and len(lines) == 5                       # nothing scored at iteration 2: no line
    marks = [line.split("\t")[-1].partition(" ")[2] for line in lines[1:]]
    if p is None:                                                           # column 1 is an ordinary number here
        assert marks == ["Best recall!", "Best recall!", "", ""]
    else:
        assert marks == ["Best precision! Best recall!", "Best recall!", "Best precision!", ""]
    assert [line.split(":")[0] for line in lines[1:]] == ["4/11", "6/11", "8/11", "10/11"]
    assert lines[1].split("\t")[1:] == ["%.3f" % v for v in task.script[5]][:-1] + ["%.3f" % task.script[5][-1] + " " + marks[0]]
    assert [it for it, _ in summary["tests"]] == [4, 6, 8, 10] and len(summary["losses"]) == 11 and len(summary["losses"][0]) == 2
    assert summary["before"] == task.script[0] and summary["after"] == task.script[11] and summary["num_classes"] == 4
    assert "predictor" not in summary and task.pushes == 5 + 1
    chk = load(out, "_last")
    keys = ["model", "optimizer", "scheduler", "iteration", "kfold_split", "k_folds", "best_precision", "best_recall",
            "training_results", "loader"]
    assert list(chk) == [k for k in keys if p is not None or k != "best_precision"]
    assert chk["iteration"] == 10 and chk["best_recall"] == 0.3 and chk["loader"] == {"n": 11}
    assert chk["training_results"] == open(os.path.join(out, "results.txt")).read()
    assert set(chk["model"]) == {"backbone.x", "roi_heads.stub.w.weight"}
    assert torch.equal(chk["model"]["roi_heads.stub.w.weight"], summary["state"]["w.weight"])
    assert os.path.exists(os.path.join(out, NAME + "_bestAP.pth")) == (p is not None)
    assert load(out, "_bestAR")["iteration"] == 8                           # 0.3 again at 8: equal to the best counts
    if p is not None:
        assert chk["best_precision"] == 0.6 and load(out, "_bestAP")["iteration"] == 8


@pytest.mark.parametrize("needs_score", [False, True])
def test_best_checkpoint_rules(tmp_path, needs_score):
    task = StubTask(script(12, 0, 8), best_needs_score=needs_score)
    _, out = run(tmp_path, "a", task, "--stop-at", "2")
    # nothing scored at iteration 2: the majority rule writes both files all the same, the mask tool's rule neither
    want = {NAME + "_last.pth"} | (set() if needs_score else {NAME + "_bestAP.pth", NAME + "_bestAR.pth"})
    assert {f for f in os.listdir(out) if f.endswith(".pth")} == want
    task = StubTask(script(12, 0, 8), best_needs_score=needs_score)
    _, out = run(tmp_path, "b", task, "--stop-at", "6")
    # 4: both best; 6: the recall only
    assert load(out, "_last")["iteration"] == 6 and load(out, "_bestAP")["iteration"] == 4 and load(out, "_bestAR")["iteration"] == 6
    assert {f for f in os.listdir(out) if f.endswith(".pth")} == {NAME + s + ".pth" for s in ("_last", "_bestAP", "_bestAR")}


def test_stop_and_resume_repeats_the_straight_run(tmp_path):
    a, a_out = run(tmp_path, "a", StubTask(script(12, 0, 8)))
    stopped, b_out = run(tmp_path, "b", StubTask(script(12, 0, 8)), "--stop-at", "4")
    assert len(stopped["losses"]) == 5 and load(b_out, "_last")["iteration"] == 4
    b, _ = run(tmp_path, "b", StubTask(script(12, 0, 8)), "--resume")
    assert b["ap_before"] is None and len(b["losses"]) == 6 and b["losses"] == a["losses"][5:]
    assert open(os.path.join(a_out, NAME + "_last.pth"), "rb").read() == open(os.path.join(b_out, NAME + "_last.pth"), "rb").read()
    assert open(os.path.join(a_out, "results.txt")).read() == open(os.path.join(b_out, "results.txt")).read()
    assert torch.equal(a["state"]["w.weight"], b["state"]["w.weight"])


def test_resume_takes_the_checkpoints_detector_where_the_task_says(tmp_path):
    _, out = run(tmp_path, "a", StubTask({}), "--stop-at", "2")
    chk = load(out, "_last")
    chk["model"]["backbone.x"] = torch.full((2,), 7.0)
    torch.save(chk, os.path.join(out, NAME + "_last.pth"))
    for takes, want in ((True, 7.0), (False, 1.0)):
        task = StubTask({}, resume_takes_detector=takes)
        run(tmp_path, "a", task, "--resume", "--stop-at", "4")
        assert float(load(out, "_last")["model"]["backbone.x"][0]) == want
        chk["model"]["backbone.x"] = torch.full((2,), 7.0)
        torch.save(chk, os.path.join(out, NAME + "_last.pth"))


def test_checkpoint_without_loader_state(tmp_path):
    _, out = run(tmp_path, "a", StubTask({}), "--stop-at", "2")
    chk = load(out, "_last")
    del chk["loader"]
    torch.save(chk, os.path.join(out, NAME + "_last.pth"))
    with pytest.raises(KeyError):
        run(tmp_path, "a", StubTask({}), "--resume")
    task = StubTask({}, loader_state_optional=True)
    summary, _ = run(tmp_path, "a", task, "--resume", "--stop-at", "4")
    assert len(summary["losses"]) == 2 and task.loader.n == 2               # the loader started over


def test_holdout_split_and_adapt_detector():
    train, test = ft.holdout_split(10, 4, 0)
    assert sorted(train + test) == list(range(10)) and len(test) == 2 and train == sorted(train)
    assert ft.holdout_split(10, 4, 0) == (train, test) and len(ft.holdout_split(3, 1000, 0)[1]) == 1
    det = {ft.CLS_SCORE: torch.zeros(5, 8), ft.MASK_PREDICTOR + "weight": torch.ones(4, 6, 1, 1), ft.MASK_PREDICTOR + "bias": torch.ones(4)}
    same, changed = ft.adapt_detector(det, 4)
    assert same is det and not changed
    torch.manual_seed(3)
    out, changed = ft.adapt_detector(det, 2)
    torch.manual_seed(3)
    assert changed and torch.equal(out[ft.MASK_PREDICTOR + "weight"], torch.nn.init.normal_(torch.zeros(2, 6, 1, 1), std=0.001))
    assert out[ft.MASK_PREDICTOR + "bias"].tolist() == [0.0, 0.0] and det[ft.MASK_PREDICTOR + "bias"].shape == (4,)
