"""GPU tests (-m gpu): the MOTS kernels (csrc/mots.hip) against numpy, the online id map against the host writers, tools/mots_eval.py
against the reference's stdout (tests/golden/mots_golden.json), and online == offline == numpy scoring behind RcnnTracker."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import mots_ref
from apse_uav_amd import _lib
from apse_uav_amd.structures.instances import Instances
from apse_uav_amd.structures.window_mask import MaskList
from apse_uav_amd.utils import mots_evaluation as writers
from apse_uav_amd.utils import mots_eval as me
from apse_uav_amd.utils import mots_metrics as mm
from apse_uav_amd.utils import rle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "mots")
with open(os.path.join(ROOT, "tests", "golden", "mots_golden.json")) as _fh:
    GOLDEN = json.load(_fh)
SIZES = [(37, 131), (375, 1242), (2160, 3840)]


def windows_host(windows):
    """uint8 [n, 32] device -> [(rect, wpr, area, bits pointer)]."""
    raw = windows.cpu().numpy()
    out = []
    for row in raw:
        w = _lib.MotsWindow.from_buffer_copy(row.tobytes())
        out.append((tuple(w.rect), w.words_per_row, w.area, w.bits))
    return out


def window_dense(w, pool, H, W):
    """A window (pointing into ``pool``) -> dense bool [H, W]."""
    rect, wpr, _, ptr = w
    x0, y0, x1, y1 = rect
    off = (ptr - pool.data_ptr()) // 8
    rows = y1 - y0
    words = pool[off:off + rows * wpr].cpu().numpy().view(np.uint64).reshape(rows, wpr)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(rows, wpr * 64)
    out = np.zeros((H, W), bool)
    base = (x0 >> 6) << 6
    out[y0:y1, x0:x1] = bits[:, x0 - base:x1 - base]
    return out


def random_idmap(g, H, W, n):
    img = np.zeros((H, W), np.uint16)
    vals = g.choice(np.arange(1, 65536), size=n, replace=False)
    for v in vals:
        x0, y0 = int(g.integers(0, W)), int(g.integers(0, H))
        x1, y1 = min(W, x0 + int(g.integers(1, max(2, W // 3)))), min(H, y0 + int(g.integers(1, max(2, H // 3))))
        img[y0:y1, x0:x1] = np.where(g.random((y1 - y0, x1 - x0)) < 0.7, v, img[y0:y1, x0:x1])
    img[int(g.integers(0, H)), int(g.integers(0, W))] = 65535                 # a 1-pixel mask, the largest value
    return img


@pytest.mark.parametrize("hw", SIZES)
def test_split_idmap_equals_unique(hw):
    H, W = hw
    g = np.random.default_rng(H)
    for n in (0, 1, 12, 40):
        img = random_idmap(g, H, W, n) if n else np.zeros((H, W), np.uint16)
        if n == 1:
            img[:] = 0
            img[:, :] = 777                                                 # a whole-frame window
        t = torch.from_numpy(img).to(DEV)
        values, windows, pool = me.split_idmap(t)
        want = [int(v) for v in np.unique(img) if v != 0]
        assert values == want
        for v, w in zip(values, windows_host(windows)):
            d = window_dense(w, pool, H, W)
            assert np.array_equal(d, img == v), v
            ys, xs = np.nonzero(img == v)
            assert w[0] == (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
            assert w[2] == len(xs)
    # too small a pool is reported, and the retry sizes it exactly
    img = random_idmap(g, H, W, 8)
    values, windows, pool = me.split_idmap(torch.from_numpy(img).to(DEV), pool_words=1)
    assert values == [int(v) for v in np.unique(img) if v != 0]


@pytest.mark.parametrize("hw", SIZES)
def test_rle_to_bits_equals_decode(hw):
    H, W = hw
    g = np.random.default_rng(W)
    masks = [np.zeros((H, W), bool)]                                        # empty
    one = np.zeros((H, W), bool)
    one[H - 1, W - 1] = True
    masks += [one, np.ones((H, W), bool)]                                   # 1 pixel, whole frame
    for _ in range(6):
        m = np.zeros((H, W), bool)
        x0, y0 = int(g.integers(0, W)), int(g.integers(0, H))
        m[y0:min(H, y0 + int(g.integers(1, H))), x0:min(W, x0 + int(g.integers(1, W)))] = True
        m &= g.random((H, W)) < 0.8
        masks.append(m)
    items = [rle.string_to_counts(rle.encode(m)["counts"]) for m in masks]
    windows, keep = me.rle_masks(items, H, W, DEV)
    pool = keep[0]
    for m, w, counts in zip(masks, windows_host(windows), items):
        if not m.any():
            assert w[0] == (0, 0, 0, 0)
            continue
        assert np.array_equal(window_dense(w, pool, H, W), rle.decode({"size": [H, W], "counts": counts}).astype(bool))


@pytest.mark.parametrize("hw", SIZES)
def test_overlaps_equal_numpy(hw):
    H, W = hw
    g = np.random.default_rng(H + W)
    img_a = random_idmap(g, H, W, 10)
    img_b = random_idmap(g, H, W, 10)
    va, wa, pa = me.split_idmap(torch.from_numpy(img_a).to(DEV))
    vb, wb, pb = me.split_idmap(torch.from_numpy(img_b).to(DEV))
    empty_counts = [H * W]
    we, ke = me.rle_masks([empty_counts], H, W, DEV)                       # an empty mask among the windows
    windows = torch.cat([wa, wb, we])
    dense = [img_a == v for v in va] + [img_b == v for v in vb] + [np.zeros((H, W), bool)]
    n = len(dense)
    pairs = [(i, j) for i in range(n) for j in range(n)]
    union = list(range(len(va), len(va) + 3))
    pairs += [(i, -1) for i in range(n)]
    res = me.overlaps(windows, pairs, union)
    U = np.logical_or.reduce([dense[k] for k in union])
    for (i, j), row in zip(pairs, res):
        b = U if j < 0 else dense[j]
        assert row[0] == int((dense[i] & b).sum()) and row[1] == int(dense[i].sum()), (i, j)
        assert row[2] == (-1 if j < 0 else int(dense[j].sum()))
    res0 = me.overlaps(windows, [(0, -1)], [])                              # no ignore region: the empty region
    assert res0[0, 0] == 0
    assert np.array_equal(me.overlaps(windows, pairs, union), res)         # run to run


def _instances(g, H, W, n, classes=None, scores=None, ids=None):
    inst = Instances((H, W))
    rects, masks = [], []
    for k in range(n):
        x0, y0 = int(g.integers(0, W - 1)), int(g.integers(0, H - 1))
        x1, y1 = min(W, x0 + int(g.integers(1, max(2, W // 2)))), min(H, y0 + int(g.integers(1, max(2, H // 2))))
        win = g.random((y1 - y0, x1 - x0)) < 0.75
        masks.append(writers._repack(win, (x0, y0, x1, y1), (H, W), DEV))
    inst.pred_classes = torch.as_tensor(classes if classes is not None else g.choice([0, 1, 2, 7], size=n))
    sc = scores if scores is not None else g.random(n).astype(np.float32)
    inst.scores = list(torch.as_tensor(np.asarray(sc, np.float32)))
    inst.ids = list(ids) if ids is not None else list(range(1, n + 1))
    inst.pred_masks = MaskList(masks)
    return inst


def _host_idmap(inst, size):
    clone = Instances(size)
    clone.pred_classes, clone.scores, clone.ids = inst.pred_classes, list(inst.scores), list(inst.ids)
    clone.pred_masks = MaskList(inst.pred_masks)
    writers.crop_overlapping_masks(clone)
    return writers.result_image_from_objects(clone, size)


@pytest.mark.parametrize("hw", SIZES)
def test_render_idmap_equals_host_writers(hw):
    H, W = hw
    g = np.random.default_rng(7 + H)
    for n in (0, 1, 8, 30):
        inst = _instances(g, H, W, n)
        if n >= 8:
            sc = [float(s) for s in inst.scores]
            sc[3] = sc[1] = sc[5]                                          # ties: the highest index keeps the pixel
            inst.scores = list(torch.as_tensor(np.asarray(sc, np.float32)))
        got = me.render_idmap(inst, (H, W)).cpu().numpy()
        assert np.array_equal(got, _host_idmap(inst, (H, W))), n
    # a truck (class 7) over a car keeps its pixels and writes 0 there; a car cropped to nothing writes nothing
    inst = _instances(g, H, W, 3, classes=[2, 7, 2], scores=[0.5, 0.9, 0.3], ids=[4, 5, 6])
    m0 = inst.pred_masks[0]
    x0, y0, x1, y1 = m0.rect
    full = np.ones((y1 - y0, x1 - x0), bool)
    inst.pred_masks[0] = writers._repack(full, m0.rect, (H, W), DEV)
    inst.pred_masks[1] = writers._repack(full, m0.rect, (H, W), DEV)       # the truck covers the car entirely
    inst.pred_masks[2] = writers._repack(full[:1, :1], (x0, y0, x0 + 1, y0 + 1), (H, W), DEV)
    got = me.render_idmap(inst, (H, W)).cpu().numpy()
    assert np.array_equal(got, _host_idmap(inst, (H, W)))
    assert not (got == 1004).any() and not (got == 1006).any()


def test_render_idmap_refuses_values_above_u16_like_the_host():
    H, W = 40, 70
    g = np.random.default_rng(1)
    inst = _instances(g, H, W, 2, classes=[2, 0], ids=[64536, 3])
    with pytest.raises(OverflowError) as host:
        _host_idmap(inst, (H, W))
    with pytest.raises(OverflowError) as dev:
        me.render_idmap(inst, (H, W))
    assert str(dev.value) == str(host.value)


@pytest.mark.parametrize("run", GOLDEN["runs"], ids=[r["name"] for r in GOLDEN["runs"]])
def test_tool_stdout_equals_reference(run):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mots_eval.py"), run["results"], run["gt"], run["seqmap"]],
                       cwd=FIX, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout == run["stdout"]


@pytest.mark.parametrize("run", GOLDEN["runs"], ids=[r["name"] for r in GOLDEN["runs"]])
def test_evaluate_mots_fields_equal_golden(run):
    cwd = os.getcwd()
    os.chdir(FIX)
    try:
        got = me.evaluate_mots(run["results"], run["gt"], run["seqmap"], out=None)
    finally:
        os.chdir(cwd)
    for cls in (1, 2):
        per_seq, total = got[cls]
        want = run["classes"][str(cls)]
        for seq, r in list(per_seq.items()) + [("all", total)]:
            w = want["all"] if seq == "all" else want["per_seq"][seq]
            for k, v in r.as_dict().items():
                assert type(v) is type(w[k]) or (isinstance(v, float) and isinstance(w[k], float)), (seq, k)
                assert v == w[k] or (v != v and w[k] != w[k]), (cls, seq, k, v, w[k])


def test_txt_overlap_refusal_on_device():
    with pytest.raises(AssertionError) as e:
        me.load_txt_masks(os.path.join(FIX, "bad", "overlap.txt"), DEV)
    assert str(e.value) == GOLDEN["errors"]["overlap.txt"]
    with pytest.raises(AssertionError) as e:
        me.load_txt_masks(os.path.join(FIX, "bad", "duplicate.txt"), DEV)
    assert str(e.value) == GOLDEN["errors"]["duplicate.txt"]


# ---------------------------------------------------------------- behind the tracker
def _tracker(hw):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.weights import UAV4K_R101_CLS_BIAS, synthetic_association_state, synthetic_detector_state
    sd = synthetic_detector_state(0, cls_bias=UAV4K_R101_CLS_BIAS)
    return RcnnTracker(setup_cfg(), hw, synthetic_association_state(1), detector_state=sd)


def _ground_truth(maps, H, W):
    """A ground truth that differs from the tracker: shifted masks, one object missing in every third frame, ignore pieces."""
    gt = {}
    for f, img in maps.items():
        g = np.roll(img, (2, 3), axis=(0, 1)).astype(np.uint16)
        vals = [v for v in np.unique(g) if v != 0]
        if vals and f % 3 == 2:
            g[g == vals[0]] = 0
        g[: H // 10, : W // 12] = 10000
        g[H - H // 10:, W - W // 12:] = 10001
        gt[f] = g
    return gt


def _track_sequence(hw, frames, evaluator, seq, out_dir):
    from apse_uav_amd.synthetic import SyntheticSequence
    tracker = _tracker(hw)
    src = SyntheticSequence("dynamic", *hw)
    evaluator.begin_sequence(seq) if evaluator is not None else None
    maps, count = {}, 0
    for t in range(frames):
        objs = tracker.next_frame(src.frame(t))
        f = tracker.frame_count - 1
        count += len(objs)
        dev_map = me.render_idmap(objs, hw).cpu().numpy()
        if evaluator is not None:
            evaluator.add_frame(f, objs, hw)
        writers.crop_overlapping_masks(objs)                                # the reference's writer path
        img = writers.result_image_from_objects(objs, hw)
        assert np.array_equal(dev_map, img), f
        maps[f] = img
        if out_dir:
            os.makedirs(os.path.join(out_dir, seq), exist_ok=True)
            Image.fromarray(img).save(os.path.join(out_dir, seq, "%06d.png" % f))
    if evaluator is not None:
        evaluator.end_sequence()
    return maps, count


def _as_dicts(results):
    return {cls: ({s: r.as_dict() for s, r in per.items()}, tot.as_dict()) for cls, (per, tot) in results.items()}


@pytest.mark.parametrize("hw,frames", [((375, 1242), 8), ((2160, 3840), 5)])
def test_online_equals_offline_equals_numpy(hw, frames, tmp_path, logdir):
    H, W = hw
    res_dir, gt_dir = str(tmp_path / "res"), str(tmp_path / "gt")
    maps, count = _track_sequence(hw, frames, None, "0000", res_dir)
    gt = _ground_truth(maps, H, W)
    for f, img in gt.items():
        os.makedirs(os.path.join(gt_dir, "0000"), exist_ok=True)
        Image.fromarray(img).save(os.path.join(gt_dir, "0000", "%06d.png" % f))
    seqmap = str(tmp_path / "s.seqmap")
    with open(seqmap, "w") as fh:
        fh.write("0000 empty 000000 %06d\n" % (frames - 1))
    online = []
    for _ in range(2):                                                      # two runs: bit-identical
        ev = me.MotsEvaluator(gt_dir, seqmap, DEV)
        _track_sequence(hw, frames, ev, "0000", "")
        online.append(_as_dicts(ev.finish()))
    offline = _as_dicts(me.evaluate_mots(res_dir, gt_dir, seqmap, out=None))
    seqs, max_frames = mm.load_seqmap(seqmap, out=None)
    tabs = mots_ref.tables(mots_ref.load_sequences(gt_dir, seqs), mots_ref.load_sequences(res_dir, seqs))
    ref = _as_dicts({cls: mm.evaluate_class(tabs, max_frames, cls, out=None) for cls in (1, 2)})
    assert repr(online[0]) == repr(online[1])
    assert repr(online[0]) == repr(offline)
    assert repr(offline) == repr(ref)
    with open(os.path.join(logdir, "mots_eval.log"), "a") as fh:
        fh.write("tracker %s: %d objects over %d frames; cars all %s\n" % (hw, count, frames, offline[1][1]))
    if hw == (2160, 3840):
        assert count > 0
