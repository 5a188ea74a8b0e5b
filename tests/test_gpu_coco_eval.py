"""GPU tests (-m gpu): COCO box and mask AP (csrc/coco_eval.hip, utils/coco.py, utils/coco_eval.py) against the literal
restatement tests/coco_ref.py -- hand cases, seeded random datasets for 'bbox' and 'segm' with default and custom Params, polygon
rasterisation at three image sizes, a dataset at COCO val's list sizes (multi-tile score sorts, 130 ground truths and 150
detections in one group), the sort against numpy's, the online evaluator behind TrackPredictor against the product's own JSON
path, tools/coco_eval.py's stdout, reproducibility and the limits of the C ABI."""
import copy
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import coco_ref
from apse_uav_amd import _lib
from apse_uav_amd.utils import coco as cocomod
from apse_uav_amd.utils import coco_eval as ce
from apse_uav_amd.utils import rle
from test_coco_eval_host import HAND, dataset, det, square

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def product(gt_dataset, results, iou_type, params=None):
    gt = cocomod.COCO.from_dataset(copy.deepcopy(gt_dataset), verbose=False)
    dt = gt.loadRes(copy.deepcopy(results))
    ev = ce.COCOeval(gt, dt, iou_type)
    if params is not None:
        params(ev.params)
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev


def assert_same(ev, ref, capsys=None):
    for k in ("precision", "recall", "scores"):
        assert ev.eval[k].shape == ref.eval[k].shape, k
        assert np.array_equal(ev.eval[k], ref.eval[k]), k
    assert np.array_equal(ev.stats, ref.stats)
    got, want = ev.evalImgs, ref.evalImgs
    assert len(got) == len(want)
    for e, r in zip(got, want):
        assert (e is None) == (r is None)
        if e is None:
            continue
        for k in ("image_id", "category_id", "maxDet", "dtIds", "gtIds", "dtScores"):
            assert e[k] == r[k], k
        assert list(e["aRng"]) == list(r["aRng"])
        for k in ("dtMatches", "gtMatches", "gtIgnore", "dtIgnore"):
            assert np.array_equal(np.asarray(e[k]), np.asarray(r[k])), (k, e[k], r[k])
            assert np.asarray(e[k]).dtype == np.asarray(r[k]).dtype or k == "gtIgnore", (k, np.asarray(e[k]).dtype)
    for key, r in ref.ious.items():
        g = ev.ious[key]
        assert (len(g) == 0) == (len(r) == 0)
        if len(r):
            assert np.array_equal(g, r)


# ---------------------------------------------------------------- 1. hand cases
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name, capsys):
    gts, dts, want = HAND[name]
    ev = product(dataset(gts), dts, "bbox")
    for i, v in want.items():
        assert ev.stats[i] == pytest.approx(v, abs=1e-12), (name, i, ev.stats)
    assert_same(ev, coco_ref.run(dataset(gts), dts, "bbox"))


def test_hand_case_f_segm_and_polygon_gt():
    gts = [dict(bbox=[10, 10, 20, 20], area=400, segmentation=[[10, 10, 30, 10, 30, 30, 10, 30]])]
    dts = [det([100, 100, 40, 40], .9, segmentation=square(100, 100, 30)), det([10, 10, 20, 20], .8, segmentation=square(10, 10, 20))]
    ds = dataset(gts, h=200, w=200)
    ev = product(ds, dts, "segm")
    assert ev.stats[3] == pytest.approx(1, abs=1e-12)
    assert_same(ev, coco_ref.run(ds, dts, "segm"))


def test_ground_truth_id_zero_never_matches():
    ds = dataset([dict(bbox=[0, 0, 50, 50], id=0), dict(bbox=[100, 100, 50, 50], id=5)])
    dts = [det([0, 0, 50, 50], .9), det([100, 100, 50, 50], .8)]
    ev = product(ds, dts, "bbox")
    ref = coco_ref.run(ds, dts, "bbox")
    assert_same(ev, ref)
    e = ev.evalImgs[0]
    assert e["dtMatches"][0, 0] == 0 and e["dtMatches"][0, 1] == 5     # matched to id 0: counted as a false positive
    assert ev.stats[1] < 1


# ---------------------------------------------------------------- 2. random datasets
def random_set(seed, segm):
    g = np.random.default_rng(seed)
    img_ids = [5, 2, 9, 11, 3, 8, 14]
    sizes = {i: (int(g.integers(40, 90)), int(g.integers(50, 120))) for i in img_ids}
    cats = [1, 3, 7]
    images = [dict(id=i, height=sizes[i][0], width=sizes[i][1]) for i in img_ids]
    anns, res = [], []
    aid = 0

    def box(H, W):
        half = g.random() < .5
        x, y = g.integers(0, W - 4), g.integers(0, H - 4)
        w, h = g.integers(2, max(3, W - x)), g.integers(2, max(3, H - y))
        b = [float(x), float(y), float(w), float(h)]
        return [v + .5 for v in b[:2]] + b[2:] if half else b

    for i in img_ids:
        H, W = sizes[i]
        if i == 14:                                       # an image with detections only
            pass
        else:
            for c in cats:
                for _ in range(int(g.integers(0, 5))):
                    b = box(H, W)
                    crowd = int(g.random() < .12)
                    a = dict(id=aid, image_id=i, category_id=c, bbox=b, iscrowd=crowd,
                             area=float(b[2] * b[3]) if g.random() < .6 else float(g.integers(1, 3000)))
                    aid += 1
                    x0, y0, x1, y1 = b[0], b[1], b[0] + b[2], b[1] + b[3]
                    if crowd:
                        m = np.zeros((H, W), np.uint8)
                        m[int(y0):int(np.ceil(y1)), int(x0):int(np.ceil(x1))] = g.random((int(np.ceil(y1)) - int(y0),
                                                                                           int(np.ceil(x1)) - int(x0))) < .7
                        a["segmentation"] = dict(size=[H, W], counts=rle.counts_from_mask(m) or [H * W])
                    else:
                        jit = lambda: float(g.random() * 3 - 1.5)
                        poly = [x0 + jit(), y0 + jit(), x1 + jit(), y0 + jit(), x1 + jit(), y1 + jit(), x0 + jit(), y1 + jit()]
                        if g.random() < .3:                # a second part
                            poly2 = list(np.asarray(poly) * .5)
                            a["segmentation"] = [poly, poly2]
                        else:
                            a["segmentation"] = [poly]
                    anns.append(a)
        if i == 3:                                        # an image with ground truths only
            continue
        gts_i = [a for a in anns if a["image_id"] == i]
        n_det = int(g.integers(0, 14)) + (110 if i == 9 else 0)      # more than the custom maxDets (50) in one group
        for k in range(n_det):
            c = cats[int(g.integers(0, 3))] if i != 9 or k < 10 else 3
            if gts_i and g.random() < .6:
                src = gts_i[int(g.integers(0, len(gts_i)))]
                b = [float(v + g.integers(-2, 3) * .5) for v in src["bbox"]]
                b[2], b[3] = max(b[2], 1.0), max(b[3], 1.0)
                c = src["category_id"] if g.random() < .8 else c
            else:
                b = box(H, W)
            r = dict(image_id=i, category_id=c, bbox=b, score=float(int(g.integers(1, 20)) * .05))
            if segm:
                m = np.zeros((H, W), np.uint8)
                x0, y0 = int(b[0]), int(b[1])
                m[y0:y0 + int(b[3]), x0:x0 + int(b[2])] = 1
                if g.random() < .5:
                    m &= (g.random((H, W)) < .8).astype(np.uint8)
                e = rle.encode(m)
                e["counts"] = e["counts"].decode()
                r["segmentation"] = e
            res.append(r)
    ds = dict(images=images, annotations=anns, categories=[dict(id=c, name=str(c)) for c in cats])
    return ds, res


def custom(p):
    p.imgIds = [2, 9, 11, 14, 3]
    p.catIds = [3, 7]
    p.maxDets = [1, 5, 50]
    p.areaRng = [[0, 1e10], [0, 400], [400, 1600], [1600, 1e10]]


@pytest.mark.parametrize("iou_type", ["bbox", "segm"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_datasets_equal_reference(iou_type, seed, capsys):
    ds, res = random_set(seed, iou_type == "segm")
    for params in (None, custom):
        ev = product(ds, res, iou_type, params)
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith(" Average")]
        ref = coco_ref.run(ds, res, iou_type, params)
        assert_same(ev, ref)
        assert lines == ref.lines


def test_two_runs_identical():
    ds, res = random_set(7, True)
    a = product(ds, res, "segm")
    b = product(ds, res, "segm")
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(a.eval[k], b.eval[k])


# ---------------------------------------------------------------- 3. polygons
def random_polys(g, H, W, n):
    out = []
    for k in range(n):
        parts = []
        for _ in range(1 if k % 3 else int(g.integers(2, 4))):
            nv = int(g.integers(3, 12))
            cx, cy = g.uniform(-.1 * W, 1.1 * W), g.uniform(-.1 * H, 1.1 * H)
            r = g.uniform(1, .6 * max(H, W))
            pts = np.stack([cx + r * g.uniform(-1, 1, nv), cy + r * g.uniform(-1, 1, nv)], 1)
            if k % 4 == 1:
                pts = np.round(pts)                      # integer vertices
            if k % 5 == 2:
                pts = np.concatenate([pts, pts[:2]])     # duplicate vertices
            parts.append([float(v) for v in pts.reshape(-1)])
        out.append(parts)
    out.append([[g.uniform(0, W / 2), g.uniform(0, H / 2), g.uniform(1, W / 2), g.uniform(1, H / 2)]])      # the box form
    out.append([[1.0, 1.0, 3.0, 2.0], [W - 5.5, H - 4.25, 9.0, 9.0]])
    out.append([[0.0, 0.0, 0.5, 0.3, 0.2, 0.9]])          # sub-pixel
    return out


@pytest.mark.parametrize("hw", [(37, 131), (480, 640), (2160, 3840)])
def test_polygons_equal_frpoly_merge(hw):
    H, W = hw
    g = np.random.default_rng(H)
    polys = random_polys(g, H, W, 4 if H > 1000 else 24)
    windows, sizes, keep = cocomod.segm_to_windows([(p, H, W) for p in polys], DEV)
    got = cocomod.windows_to_dense(windows, H, W)
    for k, p in enumerate(polys):
        want = coco_ref.decode(coco_ref.merge(coco_ref.frPyObjects(p, H, W)))
        assert np.array_equal(got[k], want), (k, int(got[k].sum()), int(want.sum()))


# ---------------------------------------------------------------- 4. online evaluator behind TrackPredictor
def test_online_evaluator_equals_json_path(tmp_path):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_detector_state
    H, W = 270, 480
    cfg = setup_cfg(score_thresh=0.05)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 256, 448
    pred = TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1)))
    seq = SyntheticSequence("dynamic", H, W)
    g = np.random.default_rng(11)
    images, anns = [], []
    for i in range(4):
        images.append(dict(id=100 + i, height=H, width=W))
        for _ in range(6):
            x, y = float(g.integers(0, W - 60)), float(g.integers(0, H - 40))
            w, h = float(g.integers(8, 60)), float(g.integers(8, 40))
            anns.append(dict(id=len(anns) + 1, image_id=100 + i, category_id=int(g.integers(0, 4)), bbox=[x, y, w, h], area=w * h,
                             iscrowd=0, segmentation=[[x, y, x + w, y, x + w, y + h, x, y + h]]))
    gt = cocomod.COCO.from_dataset(dict(images=images, annotations=anns, categories=[dict(id=c, name=str(c)) for c in range(4)]),
                                   verbose=False)
    online = ce.CocoEvaluator(gt)
    results = []
    n = 0
    for i in range(4):
        inst = pred(seq.frame(i))[0]["instances"]
        n += len(inst)
        online.add(100 + i, inst)
        results += ce.instances_to_coco_json(inst, 100 + i)
    assert n > 0
    path = tmp_path / "results.json"
    path.write_text(json.dumps(results))
    for iou_type in ("bbox", "segm"):
        a = online.evaluate(iou_type)
        b = ce.COCOeval(gt, gt.loadRes(str(path)), iou_type)
        b.evaluate()
        b.accumulate()
        b.summarize()
        for k in ("precision", "recall", "scores"):
            assert np.array_equal(a.eval[k], b.eval[k]), (iou_type, k)
        assert np.array_equal(a.stats, b.stats)


# ---------------------------------------------------------------- 5. tools/coco_eval.py
def test_tool_stdout(tmp_path):
    ds, res = random_set(3, True)
    gt_path, res_path = tmp_path / "gt.json", tmp_path / "res.json"
    gt_path.write_text(json.dumps(ds))
    res_path.write_text(json.dumps(res))
    for iou_type in ("bbox", "segm"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "coco_eval.py"), str(gt_path), str(res_path), "--iou-type",
                              iou_type], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert out.returncode == 0, out.stderr
        ref = coco_ref.run(ds, res, iou_type)
        want = ["loading annotations into memory...", "Done (t=X)", "creating index...", "index created!",
                "Loading and preparing results...", "DONE (t=X)", "creating index...", "index created!",
                "Running per image evaluation...", "Evaluate annotation type *%s*" % iou_type, "DONE (t=X).",
                "Accumulating evaluation results...", "DONE (t=X)."] + ref.lines
        got = [re.sub(r"\(t=\d+\.\d\ds\)", "(t=X)", l) for l in out.stdout.splitlines()]
        assert got == want


# ---------------------------------------------------------------- 7. limits
def test_limits_refused():
    lib = _lib.load()
    st = _lib.stream_ptr()
    z = C.c_void_p(0)

    def refused(rc):
        assert rc == -1
        assert lib.apse_last_error(None).decode().startswith("apse_coco_")

    refused(lib.apse_coco_box_iou(z, z, z, -1, 0, 0, z, z, z, z, st))
    refused(lib.apse_coco_box_iou(z, z, z, 1, 4097, 1, z, z, z, z, st))
    refused(lib.apse_coco_box_iou(z, z, z, 1, 1, 4097, z, z, z, z, st))
    refused(lib.apse_coco_box_iou(z, z, z, (1 << 24) + 1, 1, 1, z, z, z, z, st))
    rng = np.zeros(64, np.float64)
    for A, T, md, mg in ((0, 10, 1, 1), (17, 10, 1, 1), (4, 0, 1, 1), (4, 65, 1, 1), (4, 10, 4097, 1), (4, 10, 1, 4097)):
        refused(lib.apse_coco_match(z, z, z, 1, md, mg, z, z, z, 0, z, z, z, 0, _lib.ptr(rng), A, _lib.ptr(rng), T, z, z, z, z, st))
    ws = torch.empty(lib.apse_coco_accumulate_workspace_bytes(10), dtype=torch.uint8, device=DEV)
    for T, R, K, A, M, mx, nk, wsb in ((65, 101, 1, 4, 3, 1, 1, ws.numel()), (10, 1025, 1, 4, 3, 1, 1, ws.numel()),
                                       (10, 101, 1025, 4, 3, 1, 1, ws.numel()), (10, 101, 1, 17, 3, 1, 1, ws.numel()),
                                       (10, 101, 1, 4, 17, 1, 1, ws.numel()), (10, 101, 1, 4, 3, (1 << 24) + 1, 1, ws.numel()),
                                       (10, 101, 1, 4, 3, 10, 100, ws.numel()), (10, 101, 1, 4, 3, 10, 10, ws.numel() - 1)):
        refused(lib.apse_coco_accumulate(z, z, z, 0, z, 0, z, z, z, nk, mx, z, T, R, K, A, M, z, z, z, _lib.ptr(ws), wsb, st))
    hw = np.array([0, 10], np.int32)
    refused(lib.apse_coco_poly_to_bits(z, z, 0, z, 1, z, _lib.ptr(hw), z, 0, z, z, z, st))
    hw = np.array([32769, 10], np.int32)
    refused(lib.apse_coco_poly_to_bits(z, z, 0, z, 1, z, _lib.ptr(hw), z, 0, z, z, z, st))
    refused(lib.apse_coco_poly_to_bits(z, z, 0, z, (1 << 20) + 1, z, _lib.ptr(hw), z, 0, z, z, z, st))
    refused(lib.apse_coco_poly_to_bits(z, z, 0, z, 0, z, _lib.ptr(hw), z, (1 << 26) + 1, z, z, z, st))


# ---------------------------------------------------------------- sizes of COCO val: multi-tile sorts, G > 64, D > maxDets
def large_set(seed):
    """400 images: category 1 with 0-19 detections per image (about 3800 in its maxDet-100 list: four 1024-key tiles, the last
    partial) on a 0.05 score grid, so ties cross the tiles; category 2 on one image with 130 ground truths (lanes own up to three)
    and 150 detections (a cut at maxDets 100 under default Params)."""
    g = np.random.default_rng(seed)
    H, W = 200, 300
    img_ids = [int(v) for v in g.permutation(np.arange(1000, 1400))]
    images = [dict(id=i, height=H, width=W) for i in img_ids]
    anns, res = [], []

    def rbox():
        w, h = float(g.integers(4, 60)), float(g.integers(4, 60))
        return [float(g.integers(0, W - int(w))) + .5 * int(g.integers(0, 2)), float(g.integers(0, H - int(h))), w, h]

    for i in img_ids:
        gts = []
        for _ in range(int(g.integers(1, 3))):
            b = rbox()
            anns.append(dict(id=len(anns) + 1, image_id=i, category_id=1, bbox=b, iscrowd=int(g.random() < .03),
                             area=b[2] * b[3] if g.random() < .8 else float(g.integers(1, 4000))))
            gts.append(b)
        for _ in range(int(g.integers(0, 20))):
            b = [v + .5 * int(g.integers(-2, 3)) for v in gts[int(g.integers(0, len(gts)))]] if g.random() < .5 else rbox()
            b[2], b[3] = max(b[2], 1.0), max(b[3], 1.0)
            res.append(dict(image_id=i, category_id=1, bbox=b, score=float(int(g.integers(1, 20)) * .05)))
    big = img_ids[7]
    grid = [[float(20 * c + 5), float(18 * r + 10), 15.0, 14.0] for r in range(10) for c in range(13)]
    for k, b in enumerate(grid):
        anns.append(dict(id=len(anns) + 1, image_id=big, category_id=2, bbox=b, iscrowd=int(k % 37 == 5),
                         area=b[2] * b[3] if k % 5 else 2000.0))
    for k in range(150):
        b = list(grid[int(g.integers(0, len(grid)))])
        b[0] += .5 * int(g.integers(-3, 4))
        b[1] += .5 * int(g.integers(-3, 4))
        res.append(dict(image_id=big, category_id=2, bbox=b, score=float(int(g.integers(1, 20)) * .05)))
    ds = dict(images=images, annotations=anns, categories=[dict(id=1, name="a"), dict(id=2, name="b")])
    return ds, res


def test_large_lists_equal_reference(capsys):
    ds, res = large_set(4)
    n1 = sum(1 for r in res if r["category_id"] == 1)
    assert n1 > 3 * 1024 and n1 % 1024                   # several sort tiles, the last one partial
    ev = product(ds, res, "bbox")
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith(" Average")]
    ref = coco_ref.run(ds, res, "bbox")
    big = [e for e in ref.evalImgs if e is not None and e["category_id"] == 2][0]
    assert len(big["gtIds"]) == 130 and len(big["dtIds"]) == 100       # lanes own several ground truths; the cut at 100
    assert_same(ev, ref)
    assert lines == ref.lines


def test_sort_lists_equal_numpy_argsort():
    lib = _lib.load()
    g = np.random.default_rng(1)
    coarse = np.round(g.random(100000) * 40) / 40 - .25      # 41 values, negatives and zeros among them
    coarse[g.integers(0, 100000, 300)] = -0.0
    coarse[g.integers(0, 100000, 300)] = 0.0
    fine = g.standard_normal(10000)                          # every byte of the key differs: no pass skipped
    f32 = g.random(10000).astype(np.float32).astype(np.float64)
    f32[:5] = np.nan
    score = np.concatenate([coarse, fine, f32])
    lists = [g.permutation(100000), np.zeros(0, np.int64), np.array([100007]), 100000 + g.permutation(10000)[:3000],
             110000 + g.permutation(10000)[:2049], 110000 + g.permutation(10000)[:1024]]
    lists[5][3] = 110000                                     # NaN scores sort last, in list order
    lists[5][700] = 110001
    seg_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    seg_idx = np.concatenate(lists).astype(np.int32)
    n = int(seg_off[-1])
    ws = torch.empty(lib.apse_coco_accumulate_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    out = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    t_score = torch.from_numpy(score).to(DEV)
    t_off, t_idx = torch.from_numpy(seg_off).to(DEV), torch.from_numpy(seg_idx).to(DEV)
    _lib.check(lib.apse_coco_sort_lists(_lib.ptr(t_score), _lib.ptr(t_off), len(lists), _lib.ptr(t_idx), n,
                                        max(len(l) for l in lists), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               None, "apse_coco_sort_lists")
    got = out.cpu().numpy()
    for s, l in enumerate(lists):
        want = l[np.argsort(-score[l], kind="mergesort")]
        assert np.array_equal(got[seg_off[s]:seg_off[s + 1]], want), s


def test_polygon_rectangle_through_kernel():
    H, W = 30, 40
    rects = [(10, 10, 20, 20), (3, 5, 17, 9), (0, 0, 7, 4), (2, 1, 3, 2), (0, 0, 40, 30)]
    polys = [[[x0, y0, x1, y0, x1, y1, x0, y1]] for x0, y0, x1, y1 in rects]
    windows, _, keep = cocomod.segm_to_windows([(p, H, W) for p in polys], DEV)
    got = cocomod.windows_to_dense(windows, H, W)
    for k, (x0, y0, x1, y1) in enumerate(rects):
        want = np.zeros((H, W), bool)
        want[y0:y1, x0:x1] = True
        assert np.array_equal(got[k], want), rects[k]


def test_mask_sizes_of_one_image_must_agree():
    ds = dataset([dict(bbox=[10, 10, 20, 20], segmentation=[[10, 10, 30, 10, 30, 30, 10, 30]])], h=200, w=200)
    dts = [det([10, 10, 20, 20], .9, segmentation=square(10, 10, 20, h=100, w=100))]
    gt = cocomod.COCO.from_dataset(ds, verbose=False)
    ev = ce.COCOeval(gt, gt.loadRes(dts), "segm")
    with pytest.raises(ValueError, match="differ in size"):
        ev.evaluate()


def test_accumulate_refuses_other_params():
    ds, res = random_set(5, False)
    gt = cocomod.COCO.from_dataset(copy.deepcopy(ds), verbose=False)
    ev = ce.COCOeval(gt, gt.loadRes(copy.deepcopy(res)), "bbox")
    ev.evaluate()
    ev.params.iouThrs = np.linspace(.5, .95, 11)             # edited in place after evaluate()
    with pytest.raises(ValueError):
        ev.accumulate()
    ev.params.iouThrs = np.linspace(.5, .95, 10)
    ev.params.catIds = list(ev.params.catIds) + [99]
    with pytest.raises(ValueError):
        ev.accumulate()
    ev.params.catIds = ev.params.catIds[:-1]
    ev.accumulate()
    assert ev.eval["precision"].shape == (10, 101, 3, 4, 3)


def test_more_limits_refused():
    lib = _lib.load()
    st = _lib.stream_ptr()
    z = C.c_void_p(0)

    def refused(rc):
        assert rc == -1
        assert lib.apse_last_error(None).decode().startswith("apse_coco_")

    rng = np.zeros(64, np.float64)
    refused(lib.apse_coco_match(z, z, z, (1 << 24) + 1, 1, 1, z, z, z, 0, z, z, z, 0, _lib.ptr(rng), 4, _lib.ptr(rng), 10, z, z, z,
                                z, st))
    hw = np.array([10, 10], np.int32)
    refused(lib.apse_coco_poly_to_bits(z, z, (1 << 22) + 1, z, 1, z, _lib.ptr(hw), z, 0, z, z, z, st))
    ws = torch.empty(lib.apse_coco_accumulate_workspace_bytes(10), dtype=torch.uint8, device=DEV)
    for n_seg, nk, mx, wsb in ((1024 * 16 + 1, 1, 1, ws.numel()), (1, 1, (1 << 24) + 1, ws.numel()), (2, 11, 5, ws.numel()),
                               (1, 10, 10, ws.numel() - 1), (-1, 0, 0, ws.numel())):
        refused(lib.apse_coco_sort_lists(z, z, n_seg, z, nk, mx, z, _lib.ptr(ws), wsb, st))
