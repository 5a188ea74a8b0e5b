#!/usr/bin/env python3
"""Generate the MOTS evaluation golden (build container only): python tests/golden/make_mots_golden.py

Writes small synthetic KITTI MOTS sequences under tests/golden/mots/ -- ground truth and tracker results, as per-sequence PNG
id-map folders and as RLE .txt files -- then scores them with the reference's own mots_tools (mots_eval/eval.py run_eval,
mots_eval/MOTS_metrics.py, mots_common/io.py) and records its result objects, its captured stdout and the error messages of
its loader checks in tests/golden/mots_golden.json.

pycocotools is not installed, so a numpy ``pycocotools.mask`` (encode, decode, area, merge, iou with the crowd flag) is
registered for the import only, as make_golden.py does for cv2.  The golden therefore pins the reference's metric logic and
its IO; its mask arithmetic rests on the shim, which restates pycocotools' published semantics and whose encode is pinned
against the line the reference quotes (tests/test_mots_rle.py MOTS_EXAMPLE).

Sequences (frames 30 x 150, so windows cross the 64-pixel word columns):
  0000  cars and pedestrians; id switches and fragments, one at the last frame; trajectories tracked in exactly 1 of 5 and 4
        of 5 frames (MT / PT / ML at 0.2 and 0.8); ignore regions in two pieces, one tracker mask inside them by more than
        half of its area (each piece alone less), one by less; a class-3 tracker object; tracker frames after the last
        ground-truth frame and after the seqmap's last frame
  0001  ground truth only: the results are an empty .txt file
  0002  cars only in the ground truth (pedestrians: -inf), pedestrian false positives
Every id is >= 1000 (class = value // 1000).  Runs: PNG vs PNG, TXT vs TXT, PNG results vs TXT ground truth, a run with no
true positive (MOTSP inf) and a cars-only seqmap (pedestrians -inf over all sequences).
"""
import contextlib
import glob
import importlib
import io
import json
import os
import shutil
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_TOOLS = "/root/reference/dcnn/mots_tools"
OUT = os.path.join(HERE, "mots")
H, W = 30, 150
sys.path.insert(0, ROOT)

from apse_uav_amd.utils import rle  # noqa: E402


# ---------------------------------------------------------------- numpy pycocotools.mask
def _dec(r):
    h, w = r["size"]
    if h * w == 0:
        return np.zeros((h, w), np.uint8)
    return rle.decode(r).astype(bool)


def _encode(mask):
    m = np.asarray(mask)
    if m.ndim == 3:
        return [_encode(m[:, :, k]) for k in range(m.shape[2])]
    return rle.encode(m)


def _area(r):
    if isinstance(r, list):
        return np.array([_area(x) for x in r], dtype=np.uint32)
    return np.uint32(_dec(r).sum())


def _merge(rs, intersect=False):
    if len(rs) == 0:
        return {"size": [0, 0], "counts": b""}
    acc = _dec(rs[0]).copy()
    for r in rs[1:]:
        acc = (acc & _dec(r)) if intersect else (acc | _dec(r))
    return rle.encode(acc)


def _iou(dt, gt, iscrowd):
    out = np.zeros((len(dt), len(gt)), np.float64)
    for d, a in enumerate(dt):
        for g, b in enumerate(gt):
            ma, mb = _dec(a), _dec(b)
            if ma.size == 0 or mb.size == 0:
                continue                                  # an empty region's box overlaps nothing
            if ma.shape != mb.shape:
                raise ValueError("shim: sizes differ")
            i = int((ma & mb).sum())
            if i == 0:
                continue
            u = int(ma.sum()) if iscrowd[g] else int((ma | mb).sum())
            out[d, g] = float(i) / float(u)
    return out


def install_shim():
    pkg = types.ModuleType("pycocotools")
    mod = types.ModuleType("pycocotools.mask")
    mod.encode, mod.decode, mod.area, mod.merge, mod.iou = _encode, _dec, _area, _merge, _iou
    pkg.mask = mod
    sys.modules["pycocotools"] = pkg
    sys.modules["pycocotools.mask"] = mod


# ---------------------------------------------------------------- synthetic sequences
def rect(img, v, x0, y0, x1, y1):
    img[y0:y1, x0:x1] = v


def seq0000():
    gt, res = {}, {}
    for f in range(10):
        g = np.zeros((H, W), np.uint16)
        rect(g, 1001, 50 + f, 2, 80 + f, 12)                     # car A
        if f <= 4:
            rect(g, 1002, 100, 2, 141, 12)                       # car B: 5 frames
        else:
            rect(g, 1003, 99, 1, 140, 13)                        # car C: 5 frames
        rect(g, 2001, 10, 15, 22, 29)                            # pedestrian D
        if 3 <= f <= 7:
            rect(g, 2002, 30, 15, 43, 29)                        # pedestrian E
        if 2 <= f <= 6:
            rect(g, 10000, 60, 18, 70, 24)                       # ignore region, two pieces
            rect(g, 10001, 80, 18, 90, 24)
        g[12 + f % 3, 55 + f] = 1001                             # a stray pixel of A below its box
        gt[f] = g
    a_ids = {0: 1001, 1: 1001, 2: 1001, 3: 1001, 5: 1001, 6: 1001, 7: 1001, 8: 1007, 9: 1001}
    for f in range(13):
        r = np.zeros((H, W), np.uint16)
        if f in a_ids:
            rect(r, a_ids[f], 51 + f, 2, 80 + f - (f % 4), 12)   # IoU above 0.5, a different one per frame
        if f == 2:
            rect(r, 1002, 101, 3, 141, 12)                       # B tracked in 1 of 5 frames
        if 5 <= f <= 8:
            rect(r, 1003, 99, 2, 139 - f, 13)                    # C tracked in 4 of 5 frames
        if f <= 9:
            rect(r, 2005, 10, 16 + f % 2, 22, 29)                # D tracked throughout
        if 3 <= f <= 7:
            rect(r, 2006, 30, 15, 35, 29)                        # E: IoU below 0.5, a false positive
        if 2 <= f <= 6:
            rect(r, 1020, 62, 18, 88, 21)                        # inside the ignore pieces by 48 / 78: ignored
            rect(r, 1021, 64, 21, 100, 24)                       # by 48 / 108: a false positive
        rect(r, 3001, 140, 20, 150, 28)                          # a class the evaluation does not score
        if f >= 10:
            rect(r, 1001, 5, 2, 30, 10)                          # after the last ground-truth frame (12: after the seqmap's)
        res[f] = r
    return gt, res, 11


def seq0001():
    gt = {}
    for f in range(4):
        g = np.zeros((H, W), np.uint16)
        rect(g, 1001, 3 + 2 * f, 3, 40 + 2 * f, 20)
        rect(g, 2001, 90, 5, 100, 28)
        gt[f] = g
    return gt, None, 3


def seq0002():
    gt, res = {}, {}
    for f in range(5):
        g = np.zeros((H, W), np.uint16)
        rect(g, 1005, 60, 4, 130, 26)
        gt[f] = g
        r = np.zeros((H, W), np.uint16)
        rect(r, 1002, 61, 4, 130, 26)
        if f in (1, 2):
            rect(r, 2003, 5, 5, 15, 25)
        res[f] = r
    return gt, res, 4


def nomatch(res):
    """Every tracker mask cut to its top-left quarter: no IoU above 0.5."""
    out = {}
    for f, r in res.items():
        o = np.zeros_like(r)
        for v in np.unique(r):
            if v == 0:
                continue
            ys, xs = np.nonzero(r == v)
            y0, x0 = ys.min(), xs.min()
            y1, x1 = y0 + (ys.max() - y0 + 2) // 2, x0 + (xs.max() - x0 + 2) // 2
            o[y0:y1, x0:x1] = np.where(r[y0:y1, x0:x1] == v, v, o[y0:y1, x0:x1])
        out[f] = o
    return out


def write_png_seq(folder, frames):
    os.makedirs(folder, exist_ok=True)
    for f, img in frames.items():
        Image.fromarray(img).save(os.path.join(folder, "%06d.png" % f))


def write_txt_seq(path, frames):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        for f in sorted(frames):
            img = frames[f]
            for v in np.unique(img):
                if v == 0 or int(v) // 1000 not in (1, 2, 10):         # load_txt refuses other classes
                    continue
                s = rle.encode(img == v)["counts"].decode("ascii")
                fh.write("%d %d %d %d %d %s\n" % (f, int(v), int(v) // 1000, H, W, s))


def write_fixtures():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    seqs = {"0000": seq0000(), "0001": seq0001(), "0002": seq0002()}
    for name, (gt, res, last) in seqs.items():
        write_png_seq(os.path.join(OUT, "gt_png", name), gt)
        write_txt_seq(os.path.join(OUT, "gt_txt", name + ".txt"), gt)
        for kind in ("res_png", "res_txt", "res_nomatch"):
            os.makedirs(os.path.join(OUT, kind), exist_ok=True)
        if res is None:
            for kind in ("res_png", "res_txt", "res_nomatch"):
                open(os.path.join(OUT, kind, name + ".txt"), "w").close()
            continue
        write_png_seq(os.path.join(OUT, "res_png", name), res)
        write_txt_seq(os.path.join(OUT, "res_txt", name + ".txt"), res)
        write_png_seq(os.path.join(OUT, "res_nomatch", name), nomatch(res))
    with open(os.path.join(OUT, "all.seqmap"), "w") as fh:
        for name, (_, _, last) in seqs.items():
            fh.write("%s empty 000000 %06d\n" % (name, last))
    with open(os.path.join(OUT, "cars_only.seqmap"), "w") as fh:
        fh.write("0002 empty 000000 %06d\n" % seqs["0002"][2])
    # loader refusals
    bad = os.path.join(OUT, "bad")
    os.makedirs(bad, exist_ok=True)
    m1, m2, m3 = np.zeros((H, W), bool), np.zeros((H, W), bool), np.zeros((H, W), bool)
    m1[2:10, 5:70], m2[8:20, 60:90], m3[20:25, 100:120] = True, True, True
    enc = lambda m: rle.encode(m)["counts"].decode("ascii")
    lines = {
        "overlap.txt": ["0 1001 1 %d %d %s" % (H, W, enc(m3)), "1 1001 1 %d %d %s" % (H, W, enc(m1)),
                        "1 2001 2 %d %d %s" % (H, W, enc(m3)), "1 2002 2 %d %d %s" % (H, W, enc(m2))],
        "duplicate.txt": ["0 1001 1 %d %d %s" % (H, W, enc(m1)), "0 1001 1 %d %d %s" % (H, W, enc(m3))],
        "class.txt": ["0 1001 1 %d %d %s" % (H, W, enc(m1)), "0 3001 3 %d %d %s" % (H, W, enc(m3))],
    }
    for fname, ls in lines.items():
        with open(os.path.join(bad, fname), "w") as fh:
            fh.write("\n".join(ls) + "\n")
    os.makedirs(os.path.join(bad, "badname"), exist_ok=True)
    Image.fromarray(seqs["0002"][0][0]).save(os.path.join(bad, "badname", "0.png"))


RUNS = [("png", "res_png", "gt_png", "all.seqmap"), ("txt", "res_txt", "gt_txt", "all.seqmap"),
        ("mixed", "res_png", "gt_txt", "all.seqmap"), ("nomatch", "res_nomatch", "gt_png", "all.seqmap"),
        ("cars_only", "res_png", "gt_png", "cars_only.seqmap")]


def _plain(v):
    if isinstance(v, (np.floating, float)):
        return float(v)
    if isinstance(v, (np.integer, int)):
        return int(v)
    return v


def main():
    write_fixtures()
    install_shim()
    sys.path.insert(0, REF_TOOLS)
    mask_mod = sys.modules["pycocotools.mask"]
    example = "52 1005 1 375 1242 WSV:2d;1O10000O10000O1O100O100O1O100O1000000000000000O100O102N5K00O1O1N2O110OO2O001O1NTga3"
    _, _, _, h, w, s = example.split(" ")
    assert mask_mod.encode(np.asfortranarray(_dec({"size": [int(h), int(w)], "counts": s}).astype(np.uint8)))["counts"] \
        == s.encode()
    metrics = importlib.import_module("mots_eval.MOTS_metrics")
    ev = importlib.import_module("mots_eval.eval")
    mio = importlib.import_module("mots_common.io")
    recorded = []

    def recording(*a, **k):
        out = metrics.compute_MOTS_metrics(*a, **k)
        recorded.append(out)
        return out

    ev.compute_MOTS_metrics = recording
    golden = {"frame_size": [H, W], "runs": [], "errors": {}}
    cwd = os.getcwd()
    os.chdir(OUT)                      # relative paths, as a user would type them: they show in no output
    try:
        for name, res, gt, seqmap in RUNS:
            recorded.clear()
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                ev.run_eval(res, gt, seqmap)
            classes = {}
            for cls, (per_seq, total) in zip((1, 2), recorded):
                classes[str(cls)] = {"all": {k: _plain(v) for k, v in sorted(total.__dict__.items())},
                                     "per_seq": {s: {k: _plain(v) for k, v in sorted(r.__dict__.items())}
                                                 for s, r in per_seq.items()},
                                     "kitti_summary": metrics.create_summary_KITTI_style(total)}
            golden["runs"].append({"name": name, "results": res, "gt": gt, "seqmap": seqmap, "stdout": buf.getvalue(),
                                   "classes": classes})
        for fname in ("overlap.txt", "duplicate.txt", "class.txt"):
            try:
                mio.load_txt(os.path.join("bad", fname))
                raise SystemExit("expected a refusal: " + fname)
            except AssertionError as e:
                golden["errors"][fname] = str(e)
        try:
            mio.load_images_for_folder(os.path.join("bad", "badname"))
            raise SystemExit("expected a refusal: badname")
        except AssertionError as e:
            golden["errors"]["badname"] = str(e)
    finally:
        os.chdir(cwd)
    with open(os.path.join(HERE, "mots_golden.json"), "w") as fh:
        json.dump(golden, fh, indent=1, sort_keys=True)
    print("wrote", os.path.join(HERE, "mots_golden.json"), len(glob.glob(os.path.join(OUT, "**", "*"), recursive=True)),
          "fixture files")


if __name__ == "__main__":
    main()
