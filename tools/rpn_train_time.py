#!/usr/bin/env python3
"""Times one RPN-head training step on the GPU with HIP events (medians after warm-up) at 1, 2 and 4 images of 800 x 1333 (268569
anchors each, 256 sampled anchors per image); prints one JSON line per (images, ground truths per image).  The frozen backbone is
run once outside the timed region (it is the detector's own forward).

  label_ms     apse_rpn_anchor_labels, once per image (the three labelling launches)
  sample_ms    subsample_labels per image (torch: nonzero + randperm on the device)
  gather_ms    apse_rpn_patches, once per image
  gemm_ms      the three forward GEMMs, three weight gradients and two data gradients on the sampled rows
  loss_ms      loss forward + backward
  other_ms     ReLU mask and the three bias sums
  sgd_ms       apse_uav_amd.optim.SGD step over the 6 parameters
  step_ms      RPNHead forward + backward + SGD as tools/finetune_rpn.py runs them (without the loader)
"""
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
    ap.add_argument("--images", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--gts", type=int, nargs="*", default=[20, 200], help="ground truths per image")
    ap.add_argument("--frame", type=int, nargs=2, default=[800, 1333])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.networks import box_head as bh
    from apse_uav_amd.networks import rpn_head as rh
    from apse_uav_amd.optim import SGD
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils.box_train import subsample_labels
    from apse_uav_amd.weights import synthetic_detector_state

    dev = "cuda"
    H, W = args.frame
    cfg = setup_cfg(num_classes=4)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = min(H, W), max(H, W)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    model = TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1))).model
    model.backbone_frames(torch.from_numpy(SyntheticSequence("dynamic", H, W).frame(0)[None]).cuda())
    shapes = model.rpn_level_shapes()
    A = 3 * sum(h * w for h, w in shapes)
    for G in args.gts:
        g = torch.Generator().manual_seed(G)
        xy = torch.rand(G, 2, generator=g) * torch.tensor([W - 80.0, H - 80.0])
        gt = torch.cat([xy, xy + 16 + torch.rand(G, 2, generator=g) * 64], 1).to(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        labels, idx, _ = rh.anchor_labels(shapes, gt)
        pos, neg = subsample_labels(labels, 256, 0.5, 0, gen)
        sel = torch.cat([pos, neg])
        for images in args.images:
            row = {"images": images, "gts_per_image": G, "anchors_per_image": A, "rows": int(sel.numel()) * images,
                   "positives_per_image": int(pos.numel())}
            row["label_ms"] = timed(lambda: [rh.anchor_labels(shapes, gt) for _ in range(images)], args.warmup, args.iters)
            row["sample_ms"] = timed(lambda: [subsample_labels(labels, 256, 0.5, 0, gen) for _ in range(images)], args.warmup, args.iters)
            row["gather_ms"] = timed(lambda: [model.rpn_patches(sel) for _ in range(images)], args.warmup, args.iters)
            parts = [model.rpn_patches(sel) for _ in range(images)]
            x = torch.cat([p[0] for p in parts])
            slots = torch.cat([p[1] for p in parts])
            anchors = torch.cat([p[2] for p in parts])
            lab = torch.cat([torch.ones_like(pos), torch.zeros_like(neg)] * images).to(torch.int32)
            matched = gt[idx[sel].long()].repeat(images, 1).contiguous()
            S, norm = x.shape[0], 256 * images
            torch.manual_seed(0)
            head = rh.RPNHead(dev)
            params = list(head.parameters())
            opt = SGD(params, lr=0.02, momentum=0.9)

            def step():
                opt.zero_grad()
                losses = head(x, slots, lab, anchors, matched, images)
                (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
                opt.step()
            row["step_ms"] = timed(step, args.warmup, args.iters)
            w = rh._flat([p.detach() for p in params])
            logits, deltas, h = rh.head_outputs(x, w, keep=True)
            ws = rh.train_workspace(0, 0, S, dev)
            wsb = bh._workspace(S, 1, dev)
            dl, dd = rh.loss_backward(logits, deltas, slots, lab, anchors, matched, norm)
            g1 = torch.randn_like(h)

            def gemms():
                rh.head_outputs(x, w)
                bh.fc_wgrad(dl, h)
                bh.fc_wgrad(dd, h)
                dh = bh.fc_dgrad(dl, w[2])
                bh.fc_dgrad(dd, w[4], into=dh)
                bh.fc_wgrad(g1, x)
            row["gemm_ms"] = timed(gemms, args.warmup, args.iters)

            def loss():
                rh.loss_forward(logits, deltas, slots, lab, anchors, matched, norm, ws)
                rh.loss_backward(logits, deltas, slots, lab, anchors, matched, norm)
            row["loss_ms"] = timed(loss, args.warmup, args.iters)

            def other():
                bh.relu_grad(h, g1)
                bh.bias_grad(dl, wsb)
                bh.bias_grad(dd, wsb)
                bh.bias_grad(g1, wsb)
            row["other_ms"] = timed(other, args.warmup, args.iters)
            for p in params:
                p.grad = torch.zeros_like(p)
            row["sgd_ms"] = timed(opt.step, args.warmup, args.iters)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
