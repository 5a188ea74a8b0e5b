#!/usr/bin/env python
"""Time ``apse_bitmask_targets`` (mask targets from bitmask ground truth) on a 1333 x 750 image: 128 and 512 RoIs at a typical
box size (about 60 px) and a large one (about 1000 px wide).  Beside it, for context, ``apse_coco_mask_targets`` on rectangle
polygons of the same boxes -- the polygon path does different work (it rasterises 28 x 28 cells, whatever the box size), so there
is no bar between the two.

  python tools/bitmask_targets_time.py [--reps 50]

Per case: the median and the minimum of ``--reps`` launches timed one by one with device events, after warm-up launches; the
inputs stay in cache between launches, as they do in the training loop, where the windows were written just before.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apse_uav_amd.utils import rle                                             # noqa: E402
from apse_uav_amd.utils.COCO_utils import (DeviceBitmasks, DevicePolygons, bitmask_targets_device,     # noqa: E402
                                            mask_targets_device)

H, W = 750, 1333
N_OBJ = 16


def case(n, box_w, box_h, seed, device):
    """N_OBJ rectangle objects of about box_w x box_h and n proposals jittered around them."""
    rng = np.random.default_rng(seed)
    rects = []
    for _ in range(N_OBJ):
        bw, bh = int(box_w * rng.uniform(0.8, 1.2)), int(box_h * rng.uniform(0.8, 1.2))
        bw, bh = min(bw, W - 2), min(bh, H - 2)
        x0, y0 = int(rng.integers(0, W - bw)), int(rng.integers(0, H - bh))
        rects.append((x0, y0, x0 + bw, y0 + bh))
    segs = []
    for x0, y0, x1, y1 in rects:
        m = np.zeros((H, W), np.uint8)
        m[y0:y1, x0:x1] = 1
        segs.append(rle.encode(m))
    polys = [[[x0, y0, x1, y0, x1, y1, x0, y1]] for x0, y0, x1, y1 in rects]
    matched = rng.integers(0, N_OBJ, n).astype(np.int32)
    r = np.array(rects, np.float64)[matched]
    ext = np.stack([r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]] * 2, 1)
    rois = (r + rng.uniform(-0.15, 0.15, (n, 4)) * ext).astype(np.float32)
    rois[:, [0, 2]] = np.clip(rois[:, [0, 2]], 0, W)
    rois[:, [1, 3]] = np.clip(rois[:, [1, 3]], 0, H)
    return (DeviceBitmasks(segs, (H, W), device), DevicePolygons(polys, device), torch.from_numpy(rois).to(device),
            torch.from_numpy(matched).to(device))


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    rows = []
    print("image %d x %d, %d objects; microseconds per launch (median / min of %d)" % (W, H, N_OBJ, args.reps))
    print("%-22s %6s %26s %26s" % ("boxes", "RoIs", "apse_bitmask_targets", "apse_coco_mask_targets"))
    for label, bw, bh in (("typical (60 x 60)", 60, 60), ("large (1000 x 560)", 1000, 560)):
        for n in (128, 512):
            bm, poly, rois, matched = case(n, bw, bh, 7, args.device)
            out = torch.empty((n, 28, 28), dtype=torch.uint8, device=args.device)
            bit = timed(lambda: bitmask_targets_device(bm, rois, matched, out=out), args.reps)
            pol = timed(lambda: mask_targets_device(poly, rois, matched, out=out), args.reps)
            rows.append((label, n, bit, pol))
            print("%-22s %6d %16.1f / %7.1f %16.1f / %7.1f" % (label, n, 1e3 * bit[0], 1e3 * bit[1], 1e3 * pol[0], 1e3 * pol[1]))
    return rows


if __name__ == "__main__":
    main()
