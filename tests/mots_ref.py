"""numpy restatement of the MOTS evaluation's inputs: the loaders of mots_common/io.py (PNG id maps, RLE .txt files, with the
.txt checks) on dense masks, and the per-frame overlap tables (utils/mots_metrics.FrameTable) the GPU computes."""
import glob
import os

import numpy as np
from PIL import Image

from apse_uav_amd.utils import mots_metrics as mm
from apse_uav_amd.utils import rle


def load_image(path, id_divisor=1000):
    img = np.array(Image.open(path))
    return [(int(v) // id_divisor, int(v), img == v) for v in np.unique(img) if v != 0]


def load_folder(path):
    out = {}
    for fname in sorted(glob.glob(os.path.join(path, "*.png"))):
        base = os.path.basename(fname)
        assert len(base) == 10, "Expect filenames to have format 000000.png, 000001.png, ..."
        out[int(base.split(".")[0])] = load_image(fname)
    return out


def load_txt(path):
    out, ids, union = {}, {}, {}
    with open(path) as fh:
        for line in fh:
            fields = line.strip().split(" ")
            f, tid, cls = int(fields[0]), int(fields[1]), int(fields[2])
            out.setdefault(f, [])
            seen = ids.setdefault(f, set())
            assert tid not in seen, "Multiple objects with track id " + fields[1] + " in frame " + fields[0]
            seen.add(tid)
            assert cls in (1, 2, 10), "Unknown object class " + fields[2]
            m = rle.decode({"size": [int(fields[3]), int(fields[4])], "counts": fields[5]}).astype(bool)
            if f in union:
                assert not (union[f] & m).any(), "Objects with overlapping masks in frame " + fields[0]
                union[f] = union[f] | m
            else:
                union[f] = m
            out[f].append((cls, tid, m))
    return out


def load_sequences(path, seqs):
    out = {}
    for seq in seqs:
        folder, txt = os.path.join(path, seq), os.path.join(path, seq + ".txt")
        if os.path.isdir(folder):
            out[seq] = load_folder(folder)
        elif os.path.exists(txt):
            out[seq] = load_txt(txt)
        else:
            raise AssertionError("Can't find data in directory " + path)
    return out


def frame_table(gt_objs, tr_objs, ignore_class=mm.IGNORE_CLASS):
    ign = [m for c, _, m in gt_objs if c == ignore_class]
    union = np.logical_or.reduce(ign) if ign else None
    inter = np.array([[int((g & t).sum()) for _, _, t in tr_objs] for _, _, g in gt_objs], np.int64)
    return mm.FrameTable([c for c, _, _ in gt_objs], [t for _, t, _ in gt_objs], [int(m.sum()) for _, _, m in gt_objs],
                         [c for c, _, _ in tr_objs], [t for _, t, _ in tr_objs], [int(m.sum()) for _, _, m in tr_objs],
                         inter.reshape(len(gt_objs), len(tr_objs)),
                         [int((union & t).sum()) if union is not None else 0 for _, _, t in tr_objs])


def tables(gt, res):
    """{seq: {frame: objects}} x 2 -> {seq: {frame: FrameTable}} over the frames either side has."""
    out = {}
    for seq, gframes in gt.items():
        rframes = res.get(seq, {})
        out[seq] = {f: frame_table(gframes.get(f, []), rframes.get(f, [])) for f in sorted(set(gframes) | set(rframes))}
    return out
