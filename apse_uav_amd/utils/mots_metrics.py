"""CLEAR-MOTS bookkeeping of the KITTI MOTS evaluation (mots_tools/mots_eval/MOTS_metrics.py), restated over overlap tables.

The reference walks its masks through pycocotools for every (ground truth, tracker) pair.  Here the mask arithmetic is done
beforehand (on the GPU by utils/mots_eval.py, in numpy by tests/mots_ref.py) and reaches this module as one :class:`FrameTable`
per frame: exact integer intersections and areas.  Everything below is a pure function of those tables, so it runs without a
GPU and gives the reference's numbers bit for bit:

 * IoU is ``i / (|a| + |b| - i)`` and the ignore ("crowd") overlap ``i / |a|``, each a float64 division of exact integers as
   pycocotools' ``(double)i / (double)u``, and 0 when ``i == 0`` (which covers disjoint boxes, empty masks and the empty
   region that merging no ignore masks gives);
 * ``total_cost`` and the per-frame MODSP sums are accumulated in the reference's loop order (frames, then ground truth rows,
   then tracker columns);
 * the per-sequence result objects are summed attribute by attribute before precision, recall and CLEAR-MOT are derived,
   with the reference's ``-inf`` / ``inf`` / ``"n/a"`` cases and the MT / PT / ML thresholds (> 0.8, < 0.2, else partly).
"""
import math
from collections import OrderedDict

import numpy as np

IGNORE_CLASS = 10
CLASS_NAMES = {1: "Cars", 2: "Pedestrians"}

# (column title, attribute) of print_summary, in the reference's order
SUMMARY_COLUMNS = (("sMOTSA", "sMOTSA"), ("MOTSA", "MOTSA"), ("MOTSP", "MOTSP"), ("MOTSAL", "MOTSAL"), ("MODSA", "MODSA"),
                   ("MODSP", "MODSP"), ("Recall", "recall"), ("Prec", "precision"), ("F1", "F1"), ("FAR", "FAR"),
                   ("MT", "MT"), ("PT", "PT"), ("ML", "ML"), ("TP", "tp"), ("FP", "fp"), ("FN", "fn"),
                   ("IDS", "id_switches"), ("Frag", "fragments"), ("GT Obj", "n_gt"), ("GT Trk", "n_gt_trajectories"),
                   ("TR Obj", "n_tr"), ("TR Trk", "n_tr_trajectories"), ("Ig TR Tck", "n_itr"))

_FIELDS = ("n_gt_trajectories", "n_tr_trajectories", "total_num_frames", "n_gt", "n_tr", "n_itr", "tp", "fp", "fn", "MOTSA",
           "sMOTSA", "MOTSP", "MOTSAL", "MODSA", "MODSP", "recall", "precision", "F1", "FAR", "total_cost", "fragments",
           "id_switches", "MT", "PT", "ML")


class MOTSResults:
    """The reference's result object: the same attribute names, all starting at integer 0."""

    def __init__(self):
        for k in _FIELDS:
            setattr(self, k, 0)

    def as_dict(self):
        return OrderedDict((k, getattr(self, k)) for k in sorted(_FIELDS))


class FrameTable:
    """One frame of one sequence, both sides, as exact integers.

    gt_class, gt_track:  [G] ground-truth objects in file order (the ignore class included)
    tr_class, tr_track:  [T] tracker objects in file order
    gt_area, tr_area:    [G], [T] pixel counts
    inter:               [G, T] |gt & tr| (only pairs of one class other than the ignore class are read)
    ignore_inter:        [T] |tr & union of the frame's ignore-class ground truth| (0 when there is none)
    """
    __slots__ = ("gt_class", "gt_track", "gt_area", "tr_class", "tr_track", "tr_area", "inter", "ignore_inter")

    def __init__(self, gt_class, gt_track, gt_area, tr_class, tr_track, tr_area, inter, ignore_inter):
        self.gt_class, self.gt_track, self.gt_area = list(gt_class), list(gt_track), [int(a) for a in gt_area]
        self.tr_class, self.tr_track, self.tr_area = list(tr_class), list(tr_track), [int(a) for a in tr_area]
        self.inter = np.asarray(inter, dtype=np.int64).reshape(len(self.gt_class), len(self.tr_class))
        self.ignore_inter = [int(v) for v in ignore_inter]


# Both return numpy float64, the element type of pycocotools' iou matrix: the sums built from them (total_cost, MODSP) then
# have the reference's types too, which shows in create_summary_KITTI_style (only a Python float prints as %f there).
def pair_iou(inter, area_a, area_b):
    """pycocotools iou without the crowd flag, from exact counts."""
    if inter == 0:
        return np.float64(0.0)
    return np.float64(float(inter) / float(area_a + area_b - inter))


def crowd_overlap(inter, area_a):
    """pycocotools iou with the crowd flag on the second mask: the share of ``a`` inside it."""
    if inter == 0:
        return np.float64(0.0)
    return np.float64(float(inter) / float(area_a))


def _trajectory_stats(assigned):
    """(tracked frames, id switches, fragments) of one ground-truth trajectory: ``assigned`` holds the matched tracker id per
    frame the object is present in, or -1."""
    tracked = 1 if assigned[0] >= 0 else 0
    last = assigned[0]
    switches = frags = 0
    n = len(assigned)
    for k in range(1, n):
        cur, prev = assigned[k], assigned[k - 1]
        if cur != -1 and last != -1 and cur != last:
            switches += 1
        if k < n - 1 and cur != -1 and last != -1 and prev != cur and assigned[k + 1] != -1:
            frags += 1
        if cur != -1:
            tracked += 1
            last = cur
    # the reference looks once more at the last step after its loop (a final change of id counts as a fragment again)
    if n > 1 and assigned[n - 2] != assigned[n - 1] and last != -1 and assigned[n - 1] != -1:
        frags += 1
    return tracked, switches, frags


def evaluate_sequence(seq_name, frames, max_frame, class_id, ignore_class=IGNORE_CLASS):
    """compute_MOTS_metrics_per_sequence over ``frames`` {frame index: FrameTable} (a missing frame has no objects)."""
    res = MOTSResults()
    res.total_num_frames = max_frame + 1
    trajectories = OrderedDict()           # gt track id -> matched tracker id per frame of presence
    gt_ids, tr_ids = set(), set()
    for f in range(max_frame + 1):
        tab = frames.get(f)
        if tab is None:
            g_rows, t_cols = [], []
        else:
            g_rows = [k for k, c in enumerate(tab.gt_class) if c == class_id and c != ignore_class]
            t_cols = [k for k, c in enumerate(tab.tr_class) if c == class_id]
        for k in g_rows:
            gt_ids.add(tab.gt_track[k])
        for k in t_cols:
            tr_ids.add(tab.tr_track[k])
        res.n_gt += len(g_rows)
        res.n_tr += len(t_cols)
        matched = [False] * len(t_cols)
        frame_cost = 0
        tp = 0
        for k in g_rows:
            trajectories.setdefault(tab.gt_track[k], []).append(-1)
        for k in g_rows:
            for j, col in enumerate(t_cols):
                c = pair_iou(int(tab.inter[k, col]), tab.gt_area[k], tab.tr_area[col])
                if c > 0.5:
                    matched[j] = True
                    res.total_cost += c
                    frame_cost += c
                    trajectories[tab.gt_track[k]][-1] = tab.tr_track[col]
                    tp += 1
        ignored = sum(1 for j, col in enumerate(t_cols)
                      if crowd_overlap(tab.ignore_inter[col], tab.tr_area[col]) > 0.5 and not matched[j])
        fn = len(g_rows) - tp
        fp = len(t_cols) - tp - ignored
        res.tp += tp
        res.fn += fn
        res.fp += fp
        res.n_itr += ignored
        # the reference's sanity checks
        if tp < 0:
            raise NameError("Something went wrong! TP is negative")
        if fn < 0:
            raise NameError("Something went wrong! FN is negative")
        if fp < 0:
            raise NameError("Something went wrong! FP is negative")
        if tp + fn != len(g_rows):
            raise NameError("Something went wrong! nGroundtruth is not TP+FN")
        if tp + fp + ignored != len(t_cols):
            raise NameError("Something went wrong! nTracker is not TP+FP")
        res.MODSP += frame_cost / float(tp) if tp else 1
    assert len(trajectories) == len(gt_ids)
    res.n_gt_trajectories = len(gt_ids)
    res.n_tr_trajectories = len(tr_ids)
    for assigned in trajectories.values():
        if all(a == -1 for a in assigned):
            res.ML += 1
            continue
        tracked, switches, frags = _trajectory_stats(assigned)
        res.id_switches += switches
        res.fragments += frags
        ratio = tracked / float(len(assigned))
        if ratio > 0.8:
            res.MT += 1
        elif ratio < 0.2:
            res.ML += 1
        else:
            res.PT += 1
    return res


def derive(res):
    """compute_prec_rec_clearmot: precision, recall and CLEAR-MOT from the counts, in place."""
    if res.fp + res.tp == 0 or res.tp + res.fn == 0:
        res.recall, res.precision = 0., 0.
    else:
        res.recall = res.tp / float(res.tp + res.fn)
        res.precision = res.tp / float(res.fp + res.tp)
    res.F1 = 0. if res.recall + res.precision == 0 else \
        2. * (res.precision * res.recall) / (res.precision + res.recall)
    res.FAR = "n/a" if res.total_num_frames == 0 else res.fp / float(res.total_num_frames)
    if res.n_gt == 0:
        res.MOTSA = res.MODSA = res.sMOTSA = -float("inf")
        res.MOTSAL = -float("inf")
    else:
        n_gt = float(res.n_gt)
        res.MOTSA = 1 - (res.fn + res.fp + res.id_switches) / n_gt
        res.MODSA = 1 - (res.fn + res.fp) / n_gt
        res.sMOTSA = (res.total_cost - res.fp - res.id_switches) / n_gt
        log_ids = res.id_switches if res.id_switches == 0 else math.log10(res.id_switches)
        res.MOTSAL = 1 - (res.fn + res.fp + log_ids) / n_gt
    res.MOTSP = float("inf") if res.tp == 0 else res.total_cost / float(res.tp)
    res.MODSP = "n/a" if res.total_num_frames == 0 else res.MODSP / float(res.total_num_frames)
    n_traj = res.n_gt_trajectories
    if n_traj == 0:
        res.MT = res.PT = res.ML = 0.
    else:
        res.MT, res.PT, res.ML = res.MT / float(n_traj), res.PT / float(n_traj), res.ML / float(n_traj)
    return res


def evaluate_class(tables, max_frames, class_id, ignore_class=IGNORE_CLASS, out=print):
    """compute_MOTS_metrics: {seq: {frame: FrameTable}} -> (per-sequence results, results for all sequences).  Prints the
    summary table through ``out`` (None: silent)."""
    per_seq = OrderedDict()
    for seq, frames in tables.items():
        per_seq[seq] = evaluate_sequence(seq, frames, max_frames[seq], class_id, ignore_class)
    total = MOTSResults()
    for k in _FIELDS:
        setattr(total, k, sum(getattr(r, k) for r in per_seq.values()))
    for r in per_seq.values():
        derive(r)
    derive(total)
    if out is not None:
        for line in summary_lines(list(tables.keys()), per_seq, total):
            out(line)
    return per_seq, total


def _cell(v):
    return "%.1f" % (v * 100.0) if isinstance(v, float) else str(v)


def summary_lines(seq_names, per_seq, total):
    """The lines of the reference's print_summary."""
    names = [t for t, _ in SUMMARY_COLUMNS]
    fmt = "{:>4}" + "".join("{:>%d}" % (max(len(t), 4) + 2) for t in names)
    lines = [fmt.format("", *names), fmt.format("all", *[_cell(getattr(total, a)) for _, a in SUMMARY_COLUMNS])]
    for seq in seq_names:
        lines.append(fmt.format(seq, *[_cell(getattr(per_seq[seq], a)) for _, a in SUMMARY_COLUMNS]))
    return lines


def format_entry(key, val, width=(70, 10)):
    """print_entry: a key padded to 70 columns, then an int, a float (%f) or anything else right-aligned in 10."""
    if type(val) == int:
        tail = "%*d" % (width[1], val)
    elif type(val) == float:
        tail = "%*f" % (width[1], val)
    else:
        tail = ("%s" % val).rjust(width[1])
    return key.ljust(width[0]) + tail


def kitti_summary(res):
    """create_summary_KITTI_style."""
    rows = [("Multiple Object Tracking Segmentation Accuracy (sMOTSA)", "sMOTSA"),
            ("Multiple Object Tracking Accuracy (MOTSA)", "MOTSA"), ("Multiple Object Tracking Precision (MOTSP)", "MOTSP"),
            ("Multiple Object Tracking Accuracy (MOTSAL)", "MOTSAL"), ("Multiple Object Detection Accuracy (MODSA)", "MODSA"),
            ("Multiple Object Detection Precision (MODSP)", "MODSP"), None,
            ("Recall", "recall"), ("Precision", "precision"), ("F1", "F1"), ("False Alarm Rate", "FAR"), None,
            ("Mostly Tracked", "MT"), ("Partly Tracked", "PT"), ("Mostly Lost", "ML"), None,
            ("True Positives", "tp"), ("False Positives", "fp"), ("False Negatives", "fn"), ("Missed Targets", "fn"),
            ("ID-switches", "id_switches"), ("Fragmentations", "fragments"), None,
            ("Ground Truth Objects (Total)", "n_gt"), ("Ground Truth Trajectories", "n_gt_trajectories"), None,
            ("Tracker Objects (Total)", "n_tr"), ("Ignored Tracker Objects", "n_itr"),
            ("Tracker Trajectories", "n_tr_trajectories")]
    s = "tracking evaluation summary".center(80, "=") + "\n"
    for r in rows:
        s += "\n" if r is None else format_entry(r[0], getattr(res, r[1])) + "\n"
    return s + "=" * 80


def load_seqmap(path, out=print):
    """mots_common.io.load_seqmap: ([seq names "%04d"], {seq: last frame index})."""
    if out is not None:
        out("Loading seqmap...")
    seqs, max_frames = [], {}
    with open(path, "r") as fh:
        for line in fh:
            fields = line.split(" ")
            seq = "%04d" % int(fields[0])
            seqs.append(seq)
            max_frames[seq] = int(fields[3])
    return seqs, max_frames
