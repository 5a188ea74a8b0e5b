#!/usr/bin/env python3
"""Per-frame cost of the online MOTS chain (render id map -> split -> overlaps against a ground-truth frame) on one GPU.

    python tools/mots_chain_cost.py [--size 375x1242] [--objects 8] [--reps 50]

Builds ``--objects`` tracked objects with random mask windows (about 1/4 x 1/4 of the frame each) and a ground truth of as many
objects plus two ignore pieces, then runs MotsEvaluator.add_frame ``--reps`` times.  Prints the wall time per frame (host
preparation and the two small read-backs included); kernel times: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="375x1242")
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args(argv)
    import tempfile
    from PIL import Image
    from apse_uav_amd.structures.instances import Instances
    from apse_uav_amd.structures.window_mask import MaskList
    from apse_uav_amd.utils import mots_eval as me
    from apse_uav_amd.utils.mots_evaluation import _repack
    H, W = [int(v) for v in args.size.split("x")]
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    n = args.objects
    inst = Instances((H, W))
    masks, gt = [], np.zeros((H, W), np.uint16)
    for k in range(n):
        x0, y0 = int(g.integers(0, W - W // 4)), int(g.integers(0, H - H // 4))
        x1, y1 = x0 + W // 4, y0 + H // 4
        win = g.random((y1 - y0, x1 - x0)) < 0.8
        masks.append(_repack(win, (x0, y0, x1, y1), (H, W), dev))
        gt[y0 + 2:y1, x0 + 3:x1] = 1001 + k if k % 2 else 2001 + k
    gt[:H // 10, :W // 12] = 10000
    gt[H - H // 10:, W - W // 12:] = 10001
    inst.pred_classes = torch.as_tensor([2 if k % 2 else 0 for k in range(n)])
    inst.scores = list(torch.as_tensor(g.random(n).astype(np.float32)))
    inst.ids = list(range(1, n + 1))
    inst.pred_masks = MaskList(masks)
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "0000"))
        Image.fromarray(gt).save(os.path.join(d, "0000", "000000.png"))
        with open(os.path.join(d, "s.seqmap"), "w") as fh:
            fh.write("0000 empty 000000 000000\n")
        ev = me.MotsEvaluator(d, os.path.join(d, "s.seqmap"), dev)
        ev.begin_sequence("0000")
        for _ in range(3):
            ev.add_frame(0, inst, (H, W))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            ev.add_frame(0, inst, (H, W))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        res = ev.finish()
    print("size %dx%d objects %d: %.3f ms per frame (wall, add_frame); cars TP %d FP %d" % (
        H, W, n, dt * 1e3, res[1][1].tp, res[1][1].fp))


if __name__ == "__main__":
    main()
