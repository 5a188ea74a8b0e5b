#!/usr/bin/env python3
"""Frame time of a C4 Mask R-CNN (Base-RCNN-C4 / Res5ROIHeads) on the HIP path: 4K synthetic sequence, R-101-C4 shapes
(blocks 3, 4, 23 + res5 3), f32, batch 1, 1000 proposals per frame, timed with HIP events on the launch stream like bench.py.

    python tools/c4_frame_time.py [--steps 30] [--warmup 5] [--classes 4]

Each step is one whole TrackPredictor call on a new frame: resize + backbone + RPN + res5 on the 1000 proposals + box
inference + mask branch + the read of the results.  Prints one JSON line: frames/s over the timed steps, the p50 / min / max
per-frame time, the proposal and detection counts and the algorithmic FLOPs of a frame (apse_flops)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    args = ap.parse_args()

    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import R101_C4_BLOCKS, synthetic_c4_state

    K = args.classes
    bias = [0.0] * K + [-10.0]                  # background down: every proposal yields candidates (a busy frame)
    sd = synthetic_c4_state(0, R101_C4_BLOCKS, num_classes=K, cls_gain=2.0, cls_bias=bias)
    cfg = setup_cfg(score_thresh=0.5, num_classes=K, arch="C4")
    pr = TrackPredictor(cfg, state_dict=sd)
    seq = SyntheticSequence("dynamic", args.height, args.width)
    frames = [seq.frame(t) for t in range(8)]

    for t in range(args.warmup):
        pr(frames[t % len(frames)])
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    times = []
    t_all0, t_all1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_all0.record(stream)
    for t in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out, _ = pr(frames[t % len(frames)])
        e1.record(stream)
        times.append((e0, e1))
    t_all1.record(stream)
    torch.cuda.synchronize()
    per = [a.elapsed_time(b) for a, b in times]
    total = t_all0.elapsed_time(t_all1)
    res = pr.model.last_results
    props = int(res.prop_count[0])
    dets = int(res.total)
    print(json.dumps(dict(
        metric="C4 4K frames/sec", value=round(1000.0 * args.steps / total, 3), unit="frames/s", dtype="f32", batch=1,
        model="R-101-C4 shapes (synthetic weights)", frame=[args.height, args.width], steps=args.steps, warmup=args.warmup,
        p50_ms_per_frame=round(statistics.median(per), 3), min_ms=round(min(per), 3), max_ms=round(max(per), 3),
        proposals=props, detections=dets, gflop_per_frame=round(pr.model.flops(1, props, dets) / 1e9, 1))))


if __name__ == "__main__":
    main()
