#!/usr/bin/env python3
"""Time of the result writers per frame, the dense host path against the device path, on one GPU.

    python tools/rle_encode_time.py [--reps 20] [--host-reps 5] [--warmup 3]

Cases: 8 objects of about 250 x 110 px at 2160 x 3840, 10 objects of about 100 x 200 px at 375 x 1242, and one whole-frame mask
at 2160 x 3840; seeded blobs as WindowMasks on the GPU.  For each case and each of file_lines_from_instances and
instances_to_coco_json it prints one JSON line with the median wall time of a call (the stream synchronised before and after)
 * host_ms    with utils/rle_device.device_of answering None, which sends the same masks through the writers' dense host code
              (window -> host -> dense frame -> rle.encode per object): the only path before the device encoder existed
 * device_ms  the path the writers take now (apse_mots_bits_to_rle + apse_mots_rle_pack, one copy of the bytes)
and checks that both give the same output.  The box and GPU are named on the first line.
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def blob(g, rows, cols):
    yy, xx = np.mgrid[0:rows, 0:cols]
    inside = ((yy - (rows - 1) / 2) / (rows / 2)) ** 2 + ((xx - (cols - 1) / 2) / (cols / 2)) ** 2 <= 1.0
    return inside & (g.random((rows, cols)) < 0.97)


def make_instances(g, n, size, rows, cols, dev, whole=False):
    from apse_uav_amd.structures.instances import Boxes, Instances
    from apse_uav_amd.structures.window_mask import MaskList
    from apse_uav_amd.utils.mots_evaluation import _repack
    H, W = size
    masks, boxes = [], []
    for _ in range(n):
        if whole:
            win, rect = np.ones((H, W), bool), (0, 0, W, H)
        else:
            r, c = rows + int(g.integers(-10, 11)), cols + int(g.integers(-10, 11))
            x0, y0 = int(g.integers(0, W - c)), int(g.integers(0, H - r))
            win, rect = blob(g, r, c), (x0, y0, x0 + c, y0 + r)
        masks.append(_repack(win, rect, size, dev))
        boxes.append([float(v) for v in rect])
    inst = Instances(size)
    inst.pred_boxes = Boxes(torch.tensor(boxes, dtype=torch.float32))
    inst.scores = torch.from_numpy(g.random(n).astype(np.float32))
    inst.pred_classes = torch.tensor([(0, 2)[k % 2] for k in range(n)], dtype=torch.int64)
    inst.ids = list(range(1, n + 1))
    inst.pred_masks = MaskList(masks)
    return inst


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("rle_encode_time.py: no GPU visible (a time needs the device)")
    from apse_uav_amd.utils import coco_eval, mots_evaluation, rle_device
    dev = torch.device("cuda:0")
    print(json.dumps(dict(box=platform.node(), gpu=torch.cuda.get_device_name(0))))
    cases = [("4k_8_objects", (2160, 3840), 8, 110, 250, False), ("kitti_10_objects", (375, 1242), 10, 200, 100, False),
             ("4k_whole_frame", (2160, 3840), 1, 0, 0, True)]
    device_of = rle_device.device_of
    for name, size, n, rows, cols, whole in cases:
        inst = make_instances(np.random.default_rng(n), n, size, rows, cols, dev, whole)
        writers = (("file_lines_from_instances", lambda: mots_evaluation.file_lines_from_instances(inst, 0, size)),
                   ("instances_to_coco_json", lambda: coco_eval.instances_to_coco_json(inst, 1)))
        for wname, fn in writers:
            rle_device.device_of = lambda masks: None
            try:
                host_ms, host_out = median_ms(fn, args.host_reps, 1)
            finally:
                rle_device.device_of = device_of
            device_ms, device_out = median_ms(fn, args.reps, args.warmup)
            print(json.dumps(dict(case=name, size=list(size), objects=n, writer=wname, host_ms=round(host_ms, 3),
                                  device_ms=round(device_ms, 3), speedup=round(host_ms / device_ms, 1),
                                  equal=bool(host_out == device_out))), flush=True)


if __name__ == "__main__":
    main()
