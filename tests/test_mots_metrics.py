"""CPU tests (no GPU): the CLEAR-MOTS accumulator of utils/mots_metrics.py against the golden of the reference's own
mots_eval (tests/golden/make_mots_golden.py), the loader refusals, and the MOTS C ABI's argument checks."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import mots_ref
from apse_uav_amd.utils import mots_metrics as mm

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = os.path.join(GOLDEN_DIR, "mots")
with open(os.path.join(GOLDEN_DIR, "mots_golden.json")) as _fh:
    GOLDEN = json.load(_fh)
RUNS = {r["name"]: r for r in GOLDEN["runs"]}


def same(a, b):
    """Equal value and type class: floats bit for bit (inf included), ints, strings."""
    if isinstance(b, float):
        return isinstance(a, float) and (a == b or (math.isnan(a) and math.isnan(b))) and \
            math.copysign(1.0, a) == math.copysign(1.0, b)
    return type(a) == type(b) and a == b


def run_host(run):
    seqs, max_frames = mm.load_seqmap(os.path.join(FIX, run["seqmap"]), out=None)
    gt = mots_ref.load_sequences(os.path.join(FIX, run["gt"]), seqs)
    res = mots_ref.load_sequences(os.path.join(FIX, run["results"]), seqs)
    tabs = mots_ref.tables(gt, res)
    lines, out = [], {}
    for cls in (1, 2):
        lines.append([])
        out[cls] = mm.evaluate_class(tabs, max_frames, cls, out=lines[-1].append)
    return out, lines


@pytest.mark.parametrize("name", sorted(RUNS))
def test_accumulator_reproduces_golden(name):
    run = RUNS[name]
    out, lines = run_host(run)
    for cls in (1, 2):
        want = run["classes"][str(cls)]
        per_seq, total = out[cls]
        assert list(per_seq) == list(want["per_seq"])
        for seq, r in list(per_seq.items()) + [("all", total)]:
            w = want["all"] if seq == "all" else want["per_seq"][seq]
            got = r.as_dict()
            assert sorted(got) == sorted(w)
            for k in w:
                assert same(got[k], w[k]), (name, cls, seq, k, got[k], w[k])
        assert mm.kitti_summary(total) == want["kitti_summary"]
    # the summary tables are the reference's stdout, line for line
    body = run["stdout"].split("Evaluate class: Cars\n")[1]
    cars, peds = body.split("Evaluate class: Pedestrians\n")
    assert "\n".join(lines[0]) + "\n" == cars
    assert "\n".join(lines[1]) + "\n" == peds


def test_golden_covers_the_edge_cases():
    png = RUNS["png"]["classes"]
    assert png["2"]["per_seq"]["0002"]["sMOTSA"] == -math.inf
    assert RUNS["cars_only"]["classes"]["2"]["all"]["MOTSA"] == -math.inf
    assert RUNS["nomatch"]["classes"]["1"]["all"]["MOTSP"] == math.inf
    c0 = png["1"]["per_seq"]["0000"]
    assert c0["id_switches"] == 2 and c0["fragments"] == 3 and c0["n_itr"] > 0
    assert c0["PT"] == 2 / 3.0                                 # tracked in exactly 1 of 5 and 4 of 5 frames


def test_pair_rules():
    assert mm.pair_iou(0, 0, 0) == 0.0 and mm.crowd_overlap(0, 0) == 0.0
    assert mm.pair_iou(3, 4, 5) == 3 / 6.0
    assert mm.crowd_overlap(3, 4) == 0.75


def test_trajectory_thresholds():
    def one(assigned):
        tab = {f: mm.FrameTable([1], [7], [10], [1] if a >= 0 else [], [a] if a >= 0 else [], [10] if a >= 0 else [],
                                [[10]] if a >= 0 else np.zeros((1, 0)), [0] if a >= 0 else [])
               for f, a in enumerate(assigned)}
        return mm.evaluate_sequence("s", tab, len(assigned) - 1, 1)
    r = one([5, -1, -1, -1, -1])
    assert (r.MT, r.PT, r.ML) == (0, 1, 0)                     # 0.2: partly tracked
    r = one([5, 5, 5, 5, -1])
    assert (r.MT, r.PT, r.ML) == (0, 1, 0)                     # 0.8: partly tracked
    r = one([5, 6, -1, 6, 5])
    assert r.id_switches == 2 and r.fragments == 2


@pytest.mark.parametrize("fname", ["overlap.txt", "duplicate.txt", "class.txt"])
def test_txt_refusals(fname):
    with pytest.raises(AssertionError) as e:
        mots_ref.load_txt(os.path.join(FIX, "bad", fname))
    assert str(e.value) == GOLDEN["errors"][fname]


def test_png_name_refusal():
    with pytest.raises(AssertionError) as e:
        mots_ref.load_folder(os.path.join(FIX, "bad", "badname"))
    assert str(e.value) == GOLDEN["errors"]["badname"]


def test_evaluator_refusals_and_limits_without_gpu():
    from apse_uav_amd.utils import mots_eval as me
    with pytest.raises(AssertionError) as e:
        me.parse_txt(os.path.join(FIX, "bad", "duplicate.txt"))
    assert str(e.value) == GOLDEN["errors"]["duplicate.txt"]
    with pytest.raises(AssertionError) as e:
        me.parse_txt(os.path.join(FIX, "bad", "class.txt"))
    assert str(e.value) == GOLDEN["errors"]["class.txt"]
    with pytest.raises(AssertionError) as e:
        me.png_frames(os.path.join(FIX, "bad", "badname"))
    assert str(e.value) == GOLDEN["errors"]["badname"]
    with pytest.raises(OverflowError):
        me.check_idmap_values([(1, 64536, True)])             # 1000 * 1 + 64536 > 65535, as numpy refuses it
    me.check_idmap_values([(1, 64535, True)])
    me.check_idmap_values([(1, 70000, False)])                 # an empty window is never written
    me.check_idmap_values([(None, 70000, True)])               # nor an object of a class MOTS does not score


def test_rle_window_geometry():
    from apse_uav_amd.utils import mots_eval as me
    from apse_uav_amd.utils import rle
    g = np.random.default_rng(3)
    for _ in range(20):
        h, w = int(g.integers(1, 40)), int(g.integers(1, 200))
        m = np.zeros((h, w), bool)
        if g.random() < 0.9:
            y0, x0 = int(g.integers(0, h)), int(g.integers(0, w))
            m[y0:int(g.integers(y0, h)) + 1, x0:int(g.integers(x0, w)) + 1] = g.random() < 0.5
        counts = rle.counts_from_mask(m)
        rect, area = me.rle_rect(counts, h)
        assert area == int(m.sum())
        if area:
            ys, xs = np.nonzero(m)
            assert rect == (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)
        else:
            assert rect == (0, 0, 0, 0)


def test_abi_refuses_bad_arguments_without_gpu():
    from apse_uav_amd import _lib
    lib = _lib.load()
    assert lib.apse_mots_split_workspace_bytes() >= 5 * 65536 * 4
    dummy = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any launch
    info = C.c_void_p(0x2000)
    assert lib.apse_mots_split_idmap(None, 4, 4, 8, dummy, 16, dummy, dummy, info, dummy, 1 << 22, None) == -1
    assert lib.apse_mots_split_idmap(dummy, 0, 4, 8, dummy, 16, dummy, dummy, info, dummy, 1 << 22, None) == -1
    assert lib.apse_mots_split_idmap(dummy, 4, 49153, 8, dummy, 16, dummy, dummy, info, dummy, 1 << 22, None) == -1
    assert lib.apse_mots_split_idmap(dummy, 4, 4, 1025, dummy, 16, dummy, dummy, info, dummy, 1 << 22, None) == -1
    assert lib.apse_mots_split_idmap(dummy, 4, 4, 8, dummy, 16, dummy, dummy, info, dummy, 16, None) == -1
    assert lib.apse_mots_rle_to_bits(dummy, dummy, 1025, 4, 4, dummy, None) == -1
    assert lib.apse_mots_rle_to_bits(None, dummy, 1, 4, 4, dummy, None) == -1
    assert lib.apse_mots_rle_to_bits(None, None, 0, 4, 4, None, None) == 0          # nothing to do
    assert lib.apse_mots_overlaps(dummy, 2, dummy, 65537, None, 0, dummy, None) == -1
    assert lib.apse_mots_overlaps(dummy, 2, dummy, 1, None, 1, dummy, None) == -1
    assert lib.apse_mots_overlaps(dummy, 2, dummy, 1, dummy, 1025, dummy, None) == -1
    assert lib.apse_mots_overlaps(None, 0, None, 0, None, 0, None, None) == 0
    vals = (C.c_int * 2)(1001, 65536)
    assert lib.apse_mots_render_idmap(dummy, vals, 2, 4, 4, dummy, None) == -1      # a value above 65535
    vals = (C.c_int * 2)(1001, -1)
    assert lib.apse_mots_render_idmap(dummy, vals, 2, 4, 4, dummy, None) == -1
    assert lib.apse_mots_render_idmap(dummy, vals, 1025, 4, 4, dummy, None) == -1
    assert lib.apse_mots_render_idmap(dummy, None, 1, 4, 4, dummy, None) == -1
