#!/usr/bin/env python3
"""Trunk and tail duration of one forward with the tail lane OFF, and the lane counters of an announced loop with it ON (every
forward of that loop but the first runs ahead of a read, so its tail goes to the lane).

usage: python tools/lane_probe.py [HxW ...] [--blocks 1,1,1,1] [--min-size 256 --max-size 448]

"trunk" is what stays on the caller's stream up to the FPN (resize + apse_backbone, FPN included: an upper bound of stem..res5),
"tail" everything from apse_rpn_levels on (RPN convolutions included: an upper bound of the lane's share).  Where the trunk is
shorter than the tail the next frame's first FPN step has to wait for the lane (tests/test_gpu_tail_lane.py uses such shapes);
the third counter of apse_lane_stats says how often that happened in eight frames.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def model_for(cfg, sd, head, frames, lane):
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    m = TrackRCNN(cfg)
    m.to("cuda")
    m.load_state_dict(sd)
    m.attach_association_head(head)
    m.tail_lane = lane
    m.preprocess_frames(frames[0:1])
    m.run(1)
    m.read(1)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", default=["270x480", "375x1242"])
    ap.add_argument("--blocks", default="1,1,1,1")
    ap.add_argument("--min-size", type=int, default=256)
    ap.add_argument("--max-size", type=int, default=448)
    args = ap.parse_args()
    from apse_uav_amd import _lib
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks.association_head import AssociationHead
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_association_state, synthetic_detector_state
    sd = synthetic_detector_state(0, tuple(int(v) for v in args.blocks.split(",")))
    head = AssociationHead(roi_size=10, input_depth=256)
    head.load_state_dict(synthetic_association_state(1))
    cfg = setup_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = args.min_size, args.max_size
    for size in args.sizes:
        H, W = [int(v) for v in size.split("x")]
        seq = SyntheticSequence("dynamic", H, W)
        frames = torch.stack([torch.from_numpy(seq.frame(5 * t)) for t in range(9)]).cuda()
        off = model_for(cfg, sd, head, frames, False)
        s = _lib.stream_ptr()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        trunk, tail = [], []
        for j in range(1, 9):
            ev[0].record()
            off.preprocess_frames(frames[j:j + 1])
            off._call("apse_backbone", 1, s)
            ev[1].record()
            for fn in ("apse_rpn", "apse_box_head", "apse_mask_tail", "apse_embed"):
                off._call(fn, 1, s)
            ev[2].record()
            off.read(1)
            torch.cuda.synchronize()
            trunk.append(ev[0].elapsed_time(ev[1]))
            tail.append(ev[1].elapsed_time(ev[2]))
        on = model_for(cfg, sd, head, frames, True)
        on.preprocess_frames(frames[0:1])
        on.run(1)
        for j in range(8):
            on.read_begin(1)
            on.preprocess_frames(frames[j + 1:j + 2])
            on.run(1)
            on.read_end(1)
        on.read(1)
        st = on.lane_stats()
        print("%dx%d lane off: trunk %.3f ms, tail %.3f ms (median of 8); lane on, announced loop: forwards %d, joins %d, "
              "FPN waits not yet complete %d, drains %d"
              % (H, W, sorted(trunk)[4], sorted(tail)[4], st[0], st[1], st[2], st[3]))


if __name__ == "__main__":
    main()
