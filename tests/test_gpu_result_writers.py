"""GPU tests (-m gpu): the result writers on the device path (utils/rle_device.py behind utils/mots_evaluation.py and
utils/coco_eval.py, tools/mots_images_to_txt.py, tools/track_mots.py --txt) against the host writers, which the same functions
run when they are given the masks' CPU copies."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from apse_uav_amd import _lib
from apse_uav_amd.structures.instances import Boxes, Instances
from apse_uav_amd.structures.window_mask import MaskList, WindowMask
from apse_uav_amd.utils import coco_eval as ce
from apse_uav_amd.utils import mots_eval as me
from apse_uav_amd.utils import mots_evaluation as writers
from apse_uav_amd.utils import rle, rle_device

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "mots")
H, W = 12, 200


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _instances(items, size=(H, W), classes=None, ids=None, device=DEV):
    """items: [(bool window or None, rect, score)] -> Instances with WindowMasks on ``device``."""
    inst = Instances(size)
    masks = []
    for win, rect, _ in items:
        if win is None:
            masks.append(WindowMask(None, rect, size, (-1, -1), 0))
        else:
            masks.append(writers._repack(np.asarray(win, bool), rect, size, device))
    n = len(items)
    inst.pred_classes = torch.as_tensor(classes if classes is not None else [0] * n, dtype=torch.int64)
    inst.scores = list(torch.as_tensor(np.asarray([s for _, _, s in items], np.float32)))
    inst.ids = list(ids) if ids is not None else list(range(1, n + 1))
    inst.pred_masks = MaskList(masks)
    return inst


def _cpu_copy(inst):
    clone = Instances(inst.image_size)
    clone.pred_classes, clone.scores, clone.ids = inst.pred_classes, list(inst.scores), list(inst.ids)
    clone.pred_masks = MaskList(m.to("cpu") for m in inst.pred_masks)
    return clone


def _same_mask(a, b):
    assert a.rect == b.rect and a.mass == b.mass
    assert np.array_equal(a.window().cpu().numpy(), b.window().cpu().numpy())
    for u, v in zip(a.centroid, b.centroid):
        assert u == v or (math.isnan(u) and math.isnan(v))


def _crop_cases():
    g = np.random.default_rng(11)
    full = lambda r: np.ones((r[3] - r[1], r[2] - r[0]), bool)                      # noqa: E731
    cases = []
    a, b, c = (10, 0, 90, 12), (60, 2, 140, 10), (70, 0, 80, 12)
    cases.append([(full(a), a, 0.9), (full(b), b, 0.7), (full(c), c, 0.5)])         # three-way overlap, c eaten entirely
    cases.append([(full(a), a, 0.7), (full(b), b, 0.7), (full(c), c, 0.7)])         # all tied: the highest index keeps
    cases.append([(full(a), a, 0.5), (full(b), b, 0.9)])
    left, right = np.zeros((12, 80), bool), np.zeros((8, 80), bool)
    left[:, :40] = True
    right[:, 60:] = True
    cases.append([(left, a, 0.5), (right, b, 0.9)])                                 # rects intersect, no shared pixel
    cases.append([(full((0, 0, 30, 5)), (0, 0, 30, 5), 0.9), (full((150, 6, 200, 12)), (150, 6, 200, 12), 0.5)])   # disjoint
    cases.append([(None, (0, 0, 0, 0), 0.9), (None, (5, 1, 60, 9), 0.5), (None, (0, 0, 0, 0), 0.5)])   # all empty
    for n in (2, 3, 4, 5, 6):                                                       # random, scores with ties
        for _ in range(4):
            items = []
            for k in range(n):
                x0, y0 = int(g.integers(0, W - 1)), int(g.integers(0, H - 1))
                x1, y1 = min(W, x0 + int(g.integers(1, 130))), min(H, y0 + int(g.integers(1, H)))
                win = g.random((y1 - y0, x1 - x0)) < 0.8
                items.append((win if (n + k) % 5 else None, (x0, y0, x1, y1), float(g.choice([0.5, 0.7, 0.9]))))
            cases.append(items)
    return cases


@pytest.mark.parametrize("case", range(len(_crop_cases())))
def test_crop_overlaps_equals_host_pair_loop(case):
    items = _crop_cases()[case]
    inst = _instances(items)
    host = _cpu_copy(inst)
    writers.crop_overlapping_masks(host)                     # CPU WindowMasks: the pair loop with _repack
    before = [m.bits.clone() if m.bits is not None else None for m in inst.pred_masks]
    got = rle_device.crop_overlaps(inst)
    assert len(got) == len(items)
    for k, (a, b) in enumerate(zip(got, host.pred_masks)):
        _same_mask(a, b)
        assert a.bits is None or a.bits.device.type == "cuda"
    for m, b in zip(inst.pred_masks, before):                # the inputs keep their bits
        assert b is None or torch.equal(m.bits, b)
    again = rle_device.crop_overlaps(inst)
    for a, b in zip(got, again):                             # run to run
        assert (a.bits is None and b.bits is None) or torch.equal(a.bits, b.bits)
    writers.crop_overlapping_masks(inst)                     # the writer takes the device path for these masks
    for a, b in zip(inst.pred_masks, host.pred_masks):
        _same_mask(a, b)
    if case == 0:
        assert got[2].mass == 0 and math.isnan(got[2].centroid[0])


def test_crop_overlaps_invalid_arguments():
    lib = _lib.load()
    inst = _instances([(np.ones((3, 3), bool), (1, 1, 4, 4), 0.5)])
    arr = (_lib.MotsObject * 1)()
    arr[0].rect[:] = [1, 1, 4, 4]
    arr[0].words_per_row = 1
    arr[0].bits = inst.pred_masks[0].bits.data_ptr()
    dev_arr = torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).to(DEV)
    pool = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    stats = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    st = _lib.stream_ptr()

    def call(a=arr, d=dev_arr, n=1, h=H, w=W, p=pool, o=off, s=stats):
        return lib.apse_mots_crop_overlaps(_lib.ptr(d), a, n, h, w, _lib.ptr(p), 8, _lib.ptr(o), _lib.ptr(s), st)

    assert call(n=rle_device.MAX_OBJECTS + 1) == -1 and call(n=-1) == -1
    assert call(h=0) == -1 and call(w=49153) == -1
    assert call(a=None) == -1 and call(d=None) == -1 and call(p=None) == -1 and call(o=None) == -1 and call(s=None) == -1
    bad = (_lib.MotsObject * 1)()
    bad[0].rect[:] = [198, 1, 201, 4]                        # leaves the frame
    bad[0].words_per_row = 1
    assert call(a=bad) == -1
    arr[0].words_per_row = 0                                 # too few words for the rect
    assert call() == -1
    arr[0].words_per_row = 1
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (pool.cpu() == -7).all() and (stats.cpu() == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [9, 9, 9 * 3, 9 * 3]


def test_crop_null_bits_object_between_live_ones_writes_nothing():
    """The C entry with guard words around every pool region: an object with NULL bits and a non-empty rect, placed between two
    live ones and pointed at the middle of their words, stores nothing; the live regions hold exactly their cropped words."""
    lib = _lib.load()
    g = np.random.default_rng(4)
    ra, rn, rb = (10, 0, 150, 12), (0, 0, 200, 12), (60, 2, 190, 10)
    wa, wb = g.random((12, 140)) < 0.8, g.random((8, 130)) < 0.8
    inst = _instances([(wa, ra, 0.9), (wb, rb, 0.5)])
    ma, mb = inst.pred_masks
    guard, fill = 5, -7
    wpr_a, wpr_b = ma.bits.shape[1], mb.bits.shape[1]
    off_a = guard
    off_b = off_a + 12 * wpr_a + guard
    total = off_b + 8 * wpr_b + guard
    arr = (_lib.MotsObject * 3)()
    for k, (rect, wpr, score, bits) in enumerate(((ra, wpr_a, 1.0, ma.bits), (rn, 4, 2.0, None), (rb, wpr_b, 0.0, mb.bits))):
        arr[k].rect[:] = list(rect)
        arr[k].words_per_row = wpr
        arr[k].score = score                                 # the NULL-bits object has the highest score and covers both
        arr[k].bits = bits.data_ptr() if bits is not None else None
    dev_arr = torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).to(DEV)
    pool = torch.full((total,), fill, dtype=torch.int64, device=DEV)
    off = torch.tensor([off_a, off_a + 3, off_b], dtype=torch.int64, device=DEV)   # the middle one points into a's words
    stats = torch.full((3, 4), fill, dtype=torch.int64, device=DEV)
    host = _cpu_copy(inst)
    writers.crop_overlapping_masks(host)
    for _ in range(2):
        pool.fill_(fill)
        assert lib.apse_mots_crop_overlaps(_lib.ptr(dev_arr), arr, 3, H, W, _lib.ptr(pool), total, _lib.ptr(off),
                                           _lib.ptr(stats), _lib.stream_ptr()) == 0
        got = pool.cpu()
        for lo, hi in ((0, off_a), (off_a + 12 * wpr_a, off_b), (off_b + 8 * wpr_b, total)):
            assert (got[lo:hi] == fill).all()
        for m, o, rows, wpr in ((host.pred_masks[0], off_a, 12, wpr_a), (host.pred_masks[1], off_b, 8, wpr_b)):
            assert torch.equal(got[o:o + rows * wpr].view(rows, wpr), m.bits)
        st = stats.cpu().tolist()
        assert st[1] == [0, 0, 0, 0]
        assert st[0][:2] == [int(wa.sum()), host.pred_masks[0].mass] and st[2][:2] == [int(wb.sum()), host.pred_masks[1].mass]


def _writer_instances(g, n, size):
    h, w = size
    items = []
    for k in range(n):
        x0, y0 = int(g.integers(0, w - 2)), int(g.integers(0, h - 2))
        x1, y1 = min(w, x0 + int(g.integers(1, 150))), min(h, y0 + int(g.integers(1, 60)))
        win = None if k % 6 == 4 else g.random((y1 - y0, x1 - x0)) < 0.8
        items.append((win, (x0, y0, x1, y1) if k % 12 != 4 else (0, 0, 0, 0), float(g.random())))
    inst = _instances(items, size, classes=[(0, 2, 1, 7)[k % 4] for k in range(n)], ids=list(range(3, n + 3)))
    xy = g.random((n, 2)) * 10
    inst.pred_boxes = Boxes(torch.from_numpy(np.concatenate([xy, xy + 1 + g.random((n, 2)) * 9], 1).astype(np.float32)))
    inst.scores = torch.stack(list(inst.scores)) if n else torch.zeros(0)
    return inst


@pytest.mark.parametrize("size", [(H, W), (375, 1242)])
def test_writers_equal_their_host_path(size):
    g = np.random.default_rng(size[0])
    for n in (0, 1, 9):
        inst = _writer_instances(g, n, size)
        host = _cpu_copy(inst)
        host.pred_boxes, host.scores = inst.pred_boxes, inst.scores
        lines = writers.file_lines_from_instances(inst, 5, size)
        assert lines == writers.file_lines_from_instances(host, 5, size)
        assert lines.count("\n") == sum(1 for k in range(n) if k % 4 in (0, 1))        # classes 1 and 7 are skipped
        assert ce.instances_to_coco_json(inst, 42) == ce.instances_to_coco_json(host, 42)
    empty = _instances([(None, (0, 0, 0, 0), 0.5), (None, (2, 2, 30, 9), 0.7)], size, classes=[0, 2])   # all-empty windows
    empty.pred_boxes = Boxes(torch.zeros((2, 4)))
    empty.scores = torch.stack(list(empty.scores))
    host = _cpu_copy(empty)
    host.pred_boxes, host.scores = empty.pred_boxes, empty.scores
    assert writers.file_lines_from_instances(empty, 0, size) == writers.file_lines_from_instances(host, 0, size)
    assert ce.instances_to_coco_json(empty, 1) == ce.instances_to_coco_json(host, 1)
    only_skipped = _instances([(np.ones((2, 2), bool), (1, 1, 3, 3), 0.5)], size, classes=[1])
    assert writers.file_lines_from_instances(only_skipped, 0, size) == ""


def test_images_to_txt_equals_golden(tmp_path):
    tool = _tool("mots_images_to_txt")
    out = str(tmp_path / "txt")
    tool.main(["mots_images_to_txt.py", os.path.join(FIX, "gt_png"), out, os.path.join(FIX, "all.seqmap")])
    for seq, lines in (("0000", 45), ("0001", 8), ("0002", 5)):
        with open(os.path.join(out, seq + ".txt"), "rb") as fh:
            got = fh.read()
        with open(os.path.join(FIX, "gt_txt", seq + ".txt"), "rb") as fh:
            assert got == fh.read(), seq
        assert got.count(b"\n") == lines


def test_track_mots_txt_lines_redraw_to_the_cropped_windows(tmp_path):
    tool = _tool("track_mots")
    size = (40, 300)
    g = np.random.default_rng(21)
    frames = []
    for t in range(3):
        items = []
        for k in range(5):
            x0, y0 = int(g.integers(0, 200)), int(g.integers(0, 20))
            x1, y1 = x0 + int(g.integers(20, 100)), y0 + int(g.integers(5, 20))
            items.append((g.random((y1 - y0, x1 - x0)) < 0.9, (x0, y0, x1, y1), float(g.choice([0.5, 0.7, 0.9]))))
        frames.append(_instances(items, size, classes=[0, 2, 0, 1, 2], ids=[1, 2, 3, 4, 5]))
    path = str(tmp_path / "0000.txt")
    with open(path, "w") as fh:
        for t, inst in enumerate(frames):
            before = [m.bits.clone() for m in inst.pred_masks]
            fh.write(tool.frame_txt_lines(inst, t, size))
            assert all(torch.equal(m.bits, b) for m, b in zip(inst.pred_masks, before))   # the tracker's masks are kept
    parsed, err = me._parse_txt(path)
    assert err is None and sorted(parsed) == [0, 1, 2]
    for t, inst in enumerate(frames):
        cropped = rle_device.crop_overlaps(inst)
        scored = [k for k in range(5) if k != 3]
        objs = parsed[t]
        assert [(o[0], o[1]) for o in objs] == [((2, 1)[int(inst.pred_classes[k]) == 2],
                                                 (2, 1)[int(inst.pred_classes[k]) == 2] * 1000 + inst.ids[k]) for k in scored]
        assert all((o[2], o[3]) == size for o in objs)
        windows, keep = me.rle_masks([o[4] for o in objs], size[0], size[1], DEV)   # apse_mots_rle_to_bits
        raw = windows.cpu().numpy()
        for row, k in zip(raw, scored):
            wn = _lib.MotsWindow.from_buffer_copy(row.tobytes())
            x0, y0, x1, y1 = wn.rect
            redrawn = np.zeros(size, bool)
            if x1 > x0:
                off = (wn.bits - keep[0].data_ptr()) // 8
                words = keep[0][off:off + (y1 - y0) * wn.words_per_row].cpu().numpy().view(np.uint64)
                bits = ((words.reshape(y1 - y0, -1)[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1))
                base = (x0 >> 6) << 6
                redrawn[y0:y1, x0:x1] = bits.astype(bool).reshape(y1 - y0, -1)[:, x0 - base:x1 - base]
            assert np.array_equal(redrawn, cropped[k].dense().cpu().numpy()), (t, k)
