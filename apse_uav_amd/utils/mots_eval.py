"""MOTS evaluation on the GPU -- counterpart of the reference's mots_tools/mots_eval/eval.py (and mots_common/io.py).

The mask arithmetic runs in HIP (csrc/mots.hip) on bit windows in the WindowMask layout; the CLEAR-MOTS bookkeeping is the
host restatement in utils/mots_metrics.py, fed one FrameTable of exact integer counts per frame.

 * ``evaluate_mots(results_dir, gt_dir, seqmap_path)``  offline, as eval.py: per-sequence PNG id-map folders or RLE .txt files
   on either side.  PNG id maps go to the device and are split into one window per value (``apse_mots_split_idmap``); RLE
   runs are parsed on the host (rle.string_to_counts) and drawn into windows on the device (``apse_mots_rle_to_bits``).
 * ``MotsEvaluator(gt_dir, seqmap_path)``  online: ``begin_sequence(seq)`` uploads the ground truth of one sequence once,
   ``add_frame(frame_idx, objects)`` takes ``RcnnTracker.next_frame``'s objects and keeps their masks on the device: id map
   (``apse_mots_render_idmap``), split, overlaps; only the values present and the counts come back.  ``finish()`` scores.
 * ``render_idmap(objects, image_size)``  the device id map of result_image_from_objects(crop_overlapping_masks(objects)).

Limits: ids maps are u16, frames as in include/apse_hip.h, at most APSE_MOTS_MAX_OBJECTS (1024) objects per frame and side;
all masks of one frame share one size (a mismatch raises ValueError; pycocotools would score such a pair -1).
"""
import ctypes as C
import glob
import os
from collections import OrderedDict

import numpy as np
import torch
from PIL import Image

from .. import _lib
from ..structures import device_windows as dw
from ..structures.device_windows import MAX_OBJECTS, MAX_PAIRS          # noqa: F401  (tests and coco.py read them here)
from ..structures.window_mask import WindowMask
from . import mots_metrics as mm
from . import rle
from .mots_evaluation import _mots_class

_ws_cache = {}


def _workspace(dev):
    key = str(dev)
    if key not in _ws_cache:
        _ws_cache[key] = torch.empty(_lib.load().apse_mots_split_workspace_bytes(), dtype=torch.uint8, device=dev)
    return _ws_cache[key]


class FrameMasks:
    """One frame of one side on the device: ``windows`` uint8 [n, sizeof(apse_mots_window)], host ``classes``, ``tracks``
    and the buffers the windows point into (kept alive here)."""
    __slots__ = ("windows", "classes", "tracks", "size", "keep")

    def __init__(self, windows, classes, tracks, size, keep):
        self.windows, self.classes, self.tracks, self.size, self.keep = windows, list(classes), list(tracks), size, keep

    def __len__(self):
        return len(self.classes)


# ---------------------------------------------------------------- kernels
def split_idmap(idmap, max_values=MAX_OBJECTS, pool_words=None):
    """u16 id map [H, W] on the device -> (values [n] host ints, windows uint8 [n, 32] device, pool).  Raises ValueError when
    the map holds more than ``max_values`` distinct non-zero values."""
    lib = _lib.load()
    dev = idmap.device
    H, W = idmap.shape
    idmap = idmap.contiguous()
    values = torch.empty(max_values, dtype=torch.int32, device=dev)
    windows = torch.empty((max_values, dw.STRUCT_BYTES), dtype=torch.uint8, device=dev)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    ws = _workspace(dev)
    words = pool_words if pool_words is not None else H * dw.words_per_row((0, 0, W, H))
    for _ in range(2):
        pool = torch.empty(max(int(words), 1), dtype=torch.int64, device=dev)
        _lib.check(lib.apse_mots_split_idmap(_lib.ptr(idmap), H, W, max_values, _lib.ptr(pool), pool.numel(), _lib.ptr(values),
                                             _lib.ptr(windows), _lib.ptr(info), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   None, "apse_mots_split_idmap")
        n, need, ok = (int(v) for v in info.cpu())
        if n > max_values:
            raise ValueError("id map holds %d values, more than %d" % (n, max_values))
        if ok:
            return values[:n].cpu().tolist(), windows[:n], pool
        words = need                                     # the first guess was short: exact size now
    raise RuntimeError("apse_mots_split_idmap: pool sizing did not converge")


def rle_rect(counts, h):
    """Exact bounding box (x0, y0, x1, y1) and area of column-major runs over an h-row image; (0, 0, 0, 0) when empty."""
    x0 = y0 = 1 << 62
    x1 = y1 = -1
    area = pos = 0
    for j, c in enumerate(counts):
        c = int(c)
        if j & 1 and c > 0:
            area += c
            s, e = pos, pos + c - 1
            cs, ce = s // h, e // h
            x0, x1 = min(x0, cs), max(x1, ce)
            if cs == ce:
                y0, y1 = min(y0, s % h), max(y1, e % h)
            else:                                        # the run wraps past the bottom of a column: every row
                y0, y1 = 0, h - 1
        pos += c
    if area == 0:
        return (0, 0, 0, 0), 0
    return (x0, y0, x1 + 1, y1 + 1), area


def rle_masks(items, h, w, dev):
    """[(counts list)] over an h x w image -> windows uint8 [n, 32] on the device (and the buffers they point into)."""
    lib = _lib.load()
    n = len(items)
    if n > MAX_OBJECTS:
        raise ValueError("%d masks in one frame, more than %d" % (n, MAX_OBJECTS))
    rects, ends, offs = [], [], [0]
    for counts in items:
        if sum(int(c) for c in counts) != h * w:
            raise ValueError("run lengths do not cover the %d x %d image" % (h, w))
        r, _ = rle_rect(counts, h)
        rects.append(r)
        e = np.cumsum(np.asarray(counts, np.int64))
        ends.append(e)
        offs.append(offs[-1] + len(e))
    arr, pool = dw.pooled_windows(rects, dev)
    windows = dw.upload(arr, dev)
    ends_t = torch.from_numpy(np.concatenate(ends).astype(np.int32) if n else np.zeros(1, np.int32)).to(dev)
    offs_t = torch.from_numpy(np.asarray(offs, np.int32)).to(dev)
    _lib.check(lib.apse_mots_rle_to_bits(_lib.ptr(ends_t), _lib.ptr(offs_t), n, h, w, _lib.ptr(windows), _lib.stream_ptr()),
               None, "apse_mots_rle_to_bits")
    return windows, (pool, ends_t, offs_t)


def overlaps(windows, pairs, union_idx=()):
    """windows uint8 [n, 32] (device), pairs [(a, b)] (b = -1: the union of ``union_idx``) -> int64 [P, 3] host array of
    |a & b|, |a|, |b| (-1 for the union)."""
    lib = _lib.load()
    P = len(pairs)
    if P == 0:
        return np.zeros((0, 3), np.int64)
    if P > MAX_PAIRS:
        raise ValueError("%d pairs in one frame, more than %d" % (P, MAX_PAIRS))
    dev = windows.device
    pr = torch.from_numpy(np.asarray(pairs, np.int32).reshape(P, 2)).to(dev)
    un = torch.from_numpy(np.asarray(list(union_idx) or [0], np.int32)).to(dev)
    out = torch.empty((P, 3), dtype=torch.int32, device=dev)
    _lib.check(lib.apse_mots_overlaps(_lib.ptr(windows), windows.shape[0], _lib.ptr(pr), P, _lib.ptr(un), len(union_idx),
                                      _lib.ptr(out), _lib.stream_ptr()), None, "apse_mots_overlaps")
    return out.cpu().numpy().astype(np.int64)


def check_idmap_values(items):
    """items: [(mots class or None, id, window non-empty)].  The host writer stores class * 1000 + id into a u16 image for every
    object of a scored class whose window is not empty, and numpy refuses a value outside u16 there: the same error here."""
    for cls, oid, nonempty in items:
        if cls is None or not nonempty:
            continue
        v = cls * 1000 + int(oid)
        if v < 0 or v > 65535:
            raise OverflowError("Python integer %d out of bounds for uint16" % v)


def _object_structs(objects, image_size, dev):
    """ObjectInstances -> (apse_mots_object array on the device, host values, buffers to keep alive)."""
    n = len(objects)
    if n > MAX_OBJECTS:
        raise ValueError("%d objects in one frame, more than %d" % (n, MAX_OBJECTS))
    H, W = image_size
    classes = [_mots_class(int(objects.pred_classes[k])) for k in range(n)]
    ids = [int(objects.ids[k]) for k in range(n)]
    scores = [float(objects.scores[k]) for k in range(n)]
    rects, wprs, ptrs, *keep = dw.masks_words([objects.pred_masks[k] for k in range(n)], (H, W), dev)
    items = [(classes[k], ids[k], rects[k][2] > rects[k][0] and rects[k][3] > rects[k][1]) for k in range(n)]
    check_idmap_values(items)
    values = [classes[k] * 1000 + ids[k] if classes[k] is not None and items[k][2] else 0 for k in range(n)]
    rank = dw.score_ranks(scores)
    arr = dw.fill_objects(rects, wprs, ptrs, [rank[v] for v in scores])
    return dw.upload(arr, dev), values, keep


def render_idmap(objects, image_size, device=None, out=None):
    """Device u16 [H, W] id map of ``objects`` (ObjectInstances), byte-identical to
    result_image_from_objects(crop_overlapping_masks(objects), image_size); the objects are not changed."""
    lib = _lib.load()
    dev = dw.default_device(device)
    H, W = (int(v) for v in image_size)
    objs, values, keep = _object_structs(objects, (H, W), dev)
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint16, device=dev)
    vals = (C.c_int * max(len(values), 1))(*values)
    _lib.check(lib.apse_mots_render_idmap(_lib.ptr(objs), vals, len(values), H, W, _lib.ptr(out), _lib.stream_ptr()), None,
               "apse_mots_render_idmap")
    out._mots_keep = (objs, keep)                        # the launch reads them: alive until the tensor is
    return out


# ---------------------------------------------------------------- loading (mots_common/io.py)
def png_frames(folder):
    """{frame index: path} of a folder of id-map PNGs (the reference's file-name check)."""
    out = OrderedDict()
    for path in sorted(glob.glob(os.path.join(folder, "*.png"))):
        base = os.path.basename(path)
        assert len(base) == 10, "Expect filenames to have format 000000.png, 000001.png, ..."
        out[int(base.split(".")[0])] = path
    return out


def _parse_txt(path):
    """Lines of a MOTS .txt file -> ({frame: [(class, track, h, w, counts, line, frame field)]}, first refusal or None).  The
    track id and class checks of load_txt run here, in file order, and parsing stops at the first line they refuse."""
    frames = OrderedDict()
    seen = {}
    with open(path, "r") as fh:
        for ln, line in enumerate(fh):
            fields = line.strip().split(" ")
            frame = int(fields[0])
            frames.setdefault(frame, [])
            ids = seen.setdefault(frame, set())
            if int(fields[1]) in ids:
                return frames, "Multiple objects with track id " + fields[1] + " in frame " + fields[0]
            ids.add(int(fields[1]))
            cls = int(fields[2])
            if not (cls == 1 or cls == 2 or cls == 10):
                return frames, "Unknown object class " + fields[2]
            frames[frame].append((cls, int(fields[1]), int(fields[3]), int(fields[4]), rle.string_to_counts(fields[5]), ln,
                                  fields[0]))
    return frames, None


def parse_txt(path):
    """The host checks of load_txt (AssertionError with the reference's message): {frame: [objects]}."""
    frames, err = _parse_txt(path)
    if err is not None:
        raise AssertionError(err)
    return frames


def load_txt_masks(path, dev):
    """load_txt on the device: {frame: FrameMasks}.  The reference refuses a line whose mask meets an earlier mask of its
    frame; every such line precedes the first line the host checks refuse, so the overlap refusal wins when both occur."""
    frames, err = _parse_txt(path)
    out = OrderedDict()
    first_bad = None
    for frame, objs in frames.items():
        fm = _txt_frame(objs, dev)
        out[frame] = fm
        n = len(objs)
        pairs = [(i, j) for j in range(n) for i in range(j)]
        for p0 in range(0, len(pairs), MAX_PAIRS):
            chunk = pairs[p0:p0 + MAX_PAIRS]
            for (i, j), row in zip(chunk, overlaps(fm.windows, chunk)):
                if row[0] > 0 and (first_bad is None or objs[j][5] < first_bad[0]):
                    first_bad = (objs[j][5], objs[j][6])
    if first_bad is not None:
        raise AssertionError("Objects with overlapping masks in frame " + first_bad[1])
    if err is not None:
        raise AssertionError(err)
    return out


def _txt_frame(objs, dev):
    sizes = {(o[2], o[3]) for o in objs}
    if len(sizes) > 1:
        raise ValueError("masks of different sizes in one frame: %s" % sorted(sizes))
    h, w = sizes.pop() if sizes else (0, 0)
    if not objs:
        return FrameMasks(dw.no_windows(dev), [], [], None, None)
    windows, keep = rle_masks([o[4] for o in objs], h, w, dev)
    return FrameMasks(windows, [o[0] for o in objs], [o[1] for o in objs], (h, w), keep)


def png_frame(path, dev):
    img = np.array(Image.open(path))
    if img.dtype != np.uint16:
        img = img.astype(np.uint16)
    t = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    values, windows, pool = split_idmap(t)
    return FrameMasks(windows, [v // 1000 for v in values], values, tuple(img.shape), (pool, t))


def load_sequence(path, seq, dev):
    """{frame: FrameMasks} of one sequence: a folder of PNGs or a .txt file (load_sequences' order of preference)."""
    folder, txt = os.path.join(path, seq), os.path.join(path, seq + ".txt")
    if os.path.isdir(folder):
        return OrderedDict((f, png_frame(p, dev)) for f, p in png_frames(folder).items())
    if os.path.exists(txt):
        return load_txt_masks(txt, dev)
    raise AssertionError("Can't find data in directory " + path)


# ---------------------------------------------------------------- scoring
def frame_table(gt, tr, ignore_class=mm.IGNORE_CLASS):
    """FrameMasks x 2 (either may be None) -> mm.FrameTable: one overlaps launch for every same-class pair and every tracker
    mask against the union of the ignore regions."""
    g_cls = gt.classes if gt is not None else []
    t_cls = tr.classes if tr is not None else []
    if gt is not None and tr is not None and len(gt) and len(tr) and gt.size != tr.size:
        raise ValueError("ground truth %s and results %s differ in size" % (gt.size, tr.size))
    G, T = len(g_cls), len(t_cls)
    inter = np.zeros((G, T), np.int64)
    g_area, t_area, ign = [0] * G, [0] * T, [0] * T
    if G == 0 and T == 0:
        return mm.FrameTable([], [], [], [], [], [], inter, [])
    if G and T:
        windows = torch.cat([gt.windows, tr.windows])
    else:
        windows = gt.windows if G else tr.windows
    t0 = G if G else 0
    ignore = [k for k in range(G) if g_cls[k] == ignore_class]
    pairs = [(k, k) for k in range(G)] + [(t0 + j, t0 + j) for j in range(T)]               # areas
    pairs += [(k, t0 + j) for k in range(G) for j in range(T) if g_cls[k] == t_cls[j] and g_cls[k] != ignore_class]
    pairs += [(t0 + j, -1) for j in range(T)]
    res = overlaps(windows, pairs, ignore)
    for k in range(G):
        g_area[k] = int(res[k, 1])
    for j in range(T):
        t_area[j] = int(res[G + j, 1])
    p = G + T
    for k in range(G):
        for j in range(T):
            if g_cls[k] == t_cls[j] and g_cls[k] != ignore_class:
                inter[k, j] = res[p, 0]
                p += 1
    for j in range(T):
        ign[j] = int(res[p + j, 0])
    return mm.FrameTable(g_cls, gt.tracks if gt is not None else [], g_area, t_cls, tr.tracks if tr is not None else [],
                         t_area, inter, ign)


def _score(tables, max_frames, out):
    results = OrderedDict()
    for cls in (1, 2):
        if out is not None:
            out("Evaluate class: " + mm.CLASS_NAMES[cls])
        results[cls] = mm.evaluate_class(tables, max_frames, cls, out=out)
    return results


def evaluate_mots(results_dir, gt_dir, seqmap_path, out=print, device=None):
    """eval.py's run_eval on the GPU: {1: (per-sequence, all), 2: (...)} of utils/mots_metrics.MOTSResults (1 cars, 2
    pedestrians).  ``out`` receives the lines eval.py prints (None: silent)."""
    dev = dw.default_device(device)
    say = out if out is not None else (lambda s: None)
    seqs, max_frames = mm.load_seqmap(seqmap_path, out=out)
    say("Loading ground truth...")
    gt = OrderedDict()
    for seq in seqs:
        say("Loading sequence " + seq)
        gt[seq] = load_sequence(gt_dir, seq, dev)
    say("Loading results...")
    res = OrderedDict()
    for seq in seqs:
        say("Loading sequence " + seq)
        res[seq] = load_sequence(results_dir, seq, dev)
    say("Compute KITTI tracking eval with simplified matching and MOTSA")
    tables = OrderedDict()
    for seq in gt:
        gf, rf = gt[seq], res.get(seq, {})
        tables[seq] = {f: frame_table(gf.get(f), rf.get(f)) for f in sorted(set(gf) | set(rf))}
    return _score(tables, max_frames, out)


class MotsEvaluator:
    """Online scoring of a tracker against KITTI MOTS ground truth (PNG folders or .txt files under ``gt_dir``)."""

    def __init__(self, gt_dir, seqmap_path, device=None):
        self.gt_dir = gt_dir
        self.device = dw.default_device(device)
        self.seqs, self.max_frames = mm.load_seqmap(seqmap_path, out=None)
        self.tables = OrderedDict()
        self._seq = None
        self._gt = None

    def begin_sequence(self, seq):
        if seq not in self.max_frames:
            raise KeyError("sequence %s is not in the seqmap" % seq)
        self._seq = seq
        self._gt = load_sequence(self.gt_dir, seq, self.device)
        self.tables[seq] = {}

    def frame_masks(self, objects, image_size=None):
        """The tracker side of one frame on the device: render -> split."""
        size = tuple(image_size) if image_size is not None else tuple(objects.image_size)
        idmap = render_idmap(objects, size, self.device)
        words = _pool_bound(objects, size)
        values, windows, pool = split_idmap(idmap, pool_words=words)
        return FrameMasks(windows, [v // 1000 for v in values], values, size, (pool, idmap))

    def add_frame(self, frame_idx, objects, image_size=None):
        if self._seq is None:
            raise RuntimeError("begin_sequence first")
        tr = self.frame_masks(objects, image_size)
        self.tables[self._seq][int(frame_idx)] = frame_table(self._gt.get(int(frame_idx)), tr)

    def finish(self, out=None):
        """Scores every sequence begun so far, in seqmap order: {1: (per-sequence, all), 2: (...)}.  Ground-truth frames the
        tracker never reported count as frames without tracker objects.  ``out`` receives the summary lines."""
        self.end_sequence()
        tables = OrderedDict((seq, self.tables[seq]) for seq in self.seqs if seq in self.tables)
        return _score(tables, self.max_frames, out)

    def end_sequence(self):
        """Fills in the ground-truth frames the tracker never reported and releases the sequence's device memory."""
        if self._seq is None:
            return
        tabs = self.tables[self._seq]
        for f, fm in self._gt.items():
            if f not in tabs:
                tabs[f] = frame_table(fm, None)
        self._seq, self._gt = None, None


def _pool_bound(objects, image_size):
    """Words the split of the rendered id map can need: per value, the bounding rect of its objects' windows."""
    H, W = image_size
    boxes = {}
    for k in range(len(objects)):
        cls = _mots_class(int(objects.pred_classes[k]))
        m = objects.pred_masks[k]
        rect = m.rect if isinstance(m, WindowMask) else (0, 0, W, H)
        if cls is None or rect[2] <= rect[0] or rect[3] <= rect[1]:
            continue
        v = cls * 1000 + int(objects.ids[k])
        b = boxes.get(v)
        boxes[v] = rect if b is None else (min(b[0], rect[0]), min(b[1], rect[1]), max(b[2], rect[2]), max(b[3], rect[3]))
    return sum((r[3] - r[1]) * dw.words_per_row(r) for r in boxes.values())
