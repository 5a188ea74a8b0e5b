#!/usr/bin/env python3
"""Times one association-head training step on the GPU with HIP events; prints one JSON line.

  feature_pass_ms   the six-frame RoI-feature pass of MOTSloader.get_training_batch at KITTI size (375 x 1242, seeded
                    R-101-FPN weights, roi 10): backbone + roi_pool per frame, what every epoch pays without the cache
  head_step_ms      head forward (fc + F.normalize), batch_hard_triplet_loss, backward and the SGD step on those RoIs
  step_uncached_ms  feature pass + head step (epoch 1, or every epoch without --cache-features)
  step_cached_ms    cached batch lookup + head step (epochs 2..N with --cache-features)
Medians over --iters timed repetitions after --warmup."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--objects", type=int, default=8, help="ground-truth objects per frame")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.roi_features_generator import RoiFeaturesGenerator
    from apse_uav_amd.networks.association_head import AssociationHead
    from apse_uav_amd.online_triplet_loss.losses import batch_hard_triplet_loss
    from apse_uav_amd.optim import SGD
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_detector_state

    H, W = 375, 1242
    gen = RoiFeaturesGenerator(setup_cfg(), roi_size=10, state_dict=synthetic_detector_state(0, (3, 4, 23, 3)))
    seq = SyntheticSequence("dynamic", H, W)
    frames = [np.ascontiguousarray(seq.frame(t)) for t in range(args.frames)]
    g = np.random.default_rng(3)
    objs = []
    for t in range(args.frames):
        x = g.uniform(0, W - 120, args.objects)
        y = g.uniform(0, H - 90, args.objects)
        w = g.uniform(20, 120, args.objects)
        h = g.uniform(20, 90, args.objects)
        ids = 1000 + np.arange(args.objects) % max(2, args.objects // 2) + 1000 * (np.arange(args.objects) % 2)
        objs.append(np.stack([np.full(args.objects, t), ids, x, y, w, h], 1))

    def feature_pass():
        out = [gen.get_rois_features(frames[t], objs[t]) for t in range(args.frames)]
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

    ids, rois = feature_pass()
    head = AssociationHead(roi_size=10, input_depth=256).to("cuda")
    head.train()
    opt = SGD(head.parameters(), lr=0.01, momentum=0.9)

    def head_step(i, r):
        opt.zero_grad()
        loss = batch_hard_triplet_loss(i, head(r), margin=0.2, device="cuda")
        loss.backward()
        opt.step()
        return loss

    cache = {}

    def cached_step():
        if "b" not in cache:
            cache["b"] = feature_pass()
        head_step(*cache["b"])

    res = dict(metric="assoc_train_step", frame=[H, W], frames=args.frames, rois=int(rois.shape[0]), roi_size=10,
               feature_pass_ms=timed(feature_pass, args.warmup, args.iters),
               head_step_ms=timed(lambda: head_step(ids, rois), args.warmup, args.iters),
               step_uncached_ms=timed(lambda: head_step(*feature_pass()), args.warmup, args.iters),
               step_cached_ms=timed(cached_step, args.warmup, args.iters))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
