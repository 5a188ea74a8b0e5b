#!/usr/bin/env python3
"""Per-frame cost of the 'mask_iou' association's GPU part: utils/mask_utils.masks_iou_matrix on one GPU.

    python tools/mask_iou_time.py [--size 2160x3840] [--pairs 8x8,100x100] [--reps 200] [--warmup 20]

Builds N detection and O object masks as seeded random windows of a 4K car's size (about 300 x 110 pixels: 5-6 words x 110 rows)
anywhere in the frame and times masks_iou_matrix(detections, objects) ``--reps`` times after ``--warmup`` untimed calls.  Per
shape it prints one JSON line with the medians of
  call_ms    HIP events around the whole call: struct and pair upload, the launch, the D2H copy of 3 N O ints and the f32 division
  kernel_ms  HIP events around the apse_mots_shift_overlaps launch alone, everything already on the device
  wall_ms    host clock around the call (it ends in the D2H copy's synchronise)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_masks(g, n, H, W, dev):
    from apse_uav_amd.utils.mots_evaluation import _repack
    out = []
    for _ in range(n):
        w, h = int(g.integers(260, 340)), int(g.integers(90, 130))
        x0, y0 = int(g.integers(0, W - w)), int(g.integers(0, H - h))
        out.append(_repack(g.random((h, w)) < 0.85, (x0, y0, x0 + w, y0 + h), (H, W), dev))
    return out


def median_ms(events):
    return float(np.median([a.elapsed_time(b) for a, b in events]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="2160x3840")
    ap.add_argument("--pairs", default="8x8,100x100")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("mask_iou_time.py: no GPU visible (a time needs the device)")
    from apse_uav_amd import _lib
    from apse_uav_amd.utils import mask_utils
    H, W = [int(v) for v in args.size.split("x")]
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for shape in args.pairs.split(","):
        N, O = [int(v) for v in shape.split("x")]
        g = np.random.default_rng(N * 1000 + O)
        det, obj = make_masks(g, N, H, W, dev), make_masks(g, O, H, W, dev)
        for _ in range(args.warmup):
            iou = mask_utils.masks_iou_matrix(det, obj)
        call, wall = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            mask_utils.masks_iou_matrix(det, obj)
            e1.record()
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            call.append((e0, e1))
        # the launch alone: the same windows and pairs, resident on the device
        windows, keep = mask_utils.frame_windows(det + obj, (H, W), dev)
        quads = [(n, N + o, int(obj[o].centroid[0] - det[n].centroid[0]), int(obj[o].centroid[1] - det[n].centroid[1]))
                 for n in range(N) for o in range(O)]
        kernel = []
        for p0 in range(0, len(quads), mask_utils.MAX_PAIRS):
            q = torch.from_numpy(np.asarray(quads[p0:p0 + mask_utils.MAX_PAIRS], np.int32)).to(dev)
            out = torch.empty((q.shape[0], 3), dtype=torch.int32, device=dev)
            ev = []
            for r in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(lib.apse_mots_shift_overlaps(_lib.ptr(windows), windows.shape[0], _lib.ptr(q), q.shape[0], H, W,
                                                        _lib.ptr(out), _lib.stream_ptr()), None, "apse_mots_shift_overlaps")
                e1.record()
                if r >= args.warmup:
                    ev.append((e0, e1))
            torch.cuda.synchronize()
            kernel.append(median_ms(ev))
        del keep
        print(json.dumps(dict(size=[H, W], detections=N, objects=O, pairs=N * O, reps=args.reps,
                              call_ms=round(median_ms(call), 4), kernel_ms=round(sum(kernel), 4),
                              wall_ms=round(float(np.median(wall)), 4), mean_iou=round(float(iou.mean()), 4))))


if __name__ == "__main__":
    main()
