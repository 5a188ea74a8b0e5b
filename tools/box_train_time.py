#!/usr/bin/env python3
"""Times one box-head training step on the GPU with HIP events (medians after warm-up); prints one JSON line per (RoIs, classes).

  forward_ms        feature permutation + the four FC layers with saved activations + loss
  wgrad_ms / dgrad_ms / other_ms   backward split: the four weight gradients (MFMA GEMM), the three data gradients, the rest
                                   (loss gradient, ReLU masks, bias sums)
  sgd_ms            apse_uav_amd.optim.SGD step over the 8 parameters
  step_ms           forward + backward + SGD as BoxHead runs them
  fc1_forward_ms    fc1's forward launch alone (2 n 1024 12544 FLOP)
  fc1_wgrad_ms      fc1's weight-gradient launch alone, its TFLOP/s from the same FLOP count and the fraction of the 157.3 TFLOP/s
                    f32 matrix peak
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

F32_MATRIX_PEAK_TFLOPS = 157.3


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
    ap.add_argument("--rois", type=int, nargs="*", default=[1024, 512])
    ap.add_argument("--classes", type=int, nargs="*", default=[4, 80])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from apse_uav_amd.networks import box_head as bh
    from apse_uav_amd.optim import SGD

    dev = "cuda"
    for n in args.rois:
        for K in args.classes:
            g = torch.Generator().manual_seed(n)
            torch.manual_seed(0)
            head = bh.BoxHead(K, dev)
            params = list(head.parameters())
            opt = SGD(params, lr=0.02, momentum=0.9)
            x = torch.relu(torch.randn(n, 7, 7, 256, generator=g)).to(dev)
            labels = torch.full((n,), K, dtype=torch.int32)
            fg = torch.rand(n, generator=g) < 0.25
            labels[fg] = torch.randint(0, K, (int(fg.sum()),), generator=g).to(torch.int32)
            labels = labels.to(dev)
            xy = torch.rand(n, 2, generator=g) * 400
            pb = torch.cat([xy, xy + 8 + torch.rand(n, 2, generator=g) * 200], 1).to(dev)
            gb = (pb + (torch.rand(n, 4, generator=g).to(dev) - 0.5) * 4).contiguous()
            row = {"rois": n, "classes": K}

            def step():
                opt.zero_grad()
                losses = head(x, labels, pb, gb)
                (losses["loss_cls"] + losses["loss_box_reg"]).backward()
                opt.step()
            row["step_ms"] = timed(step, args.warmup, args.iters)
            det = [p.detach() for p in params]
            ws = bh._workspace(n, K, dev)
            state = {}

            def fwd():
                state["lg"], state["dl"], state["acts"] = bh.head_outputs(x, det, ws, keep=True)
                state["out"] = bh.loss_forward(state["lg"], state["dl"], labels, pb, gb, ws)
            row["forward_ms"] = timed(fwd, args.warmup, args.iters)
            lg, dl, (xp, a1, a2) = state["lg"], state["dl"], state["acts"]
            dlg, ddl = bh.loss_backward(lg, dl, labels, pb, gb)
            g2 = torch.randn_like(a2)

            def wgrads():
                bh.fc_wgrad(dlg, a2)
                bh.fc_wgrad(ddl, a2)
                bh.fc_wgrad(g2, a1)
                bh.fc_wgrad(g2, xp)
            row["wgrad_ms"] = timed(wgrads, args.warmup, args.iters)

            def dgrads():
                da2 = bh.fc_dgrad(dlg, det[4])
                bh.fc_dgrad(ddl, det[6], into=da2)
                bh.fc_dgrad(g2, det[2])
            row["dgrad_ms"] = timed(dgrads, args.warmup, args.iters)

            def other():
                bh.loss_backward(lg, dl, labels, pb, gb)
                bh.bias_grad(dlg, ws)
                bh.bias_grad(ddl, ws)
                for a in (a2, a1):
                    bh.relu_grad(a, g2)
                    bh.bias_grad(g2, ws)
            row["other_ms"] = timed(other, args.warmup, args.iters)
            for p in params:
                p.grad = torch.zeros_like(p)
            row["sgd_ms"] = timed(opt.step, args.warmup, args.iters)
            flops = 2.0 * n * 1024 * 12544
            row["permute_ms"] = timed(lambda: bh.permute_features(x), args.warmup, args.iters)
            row["fc1_forward_ms"] = timed(lambda: bh.fc_forward(xp, det[0], det[1], True, ws), args.warmup, args.iters)
            one = timed(lambda: bh.fc_wgrad(g2, xp), args.warmup, args.iters)
            row["fc1_wgrad_ms"] = one
            row["fc1_wgrad_tflops"] = flops / one / 1e9
            row["fc1_wgrad_peak_fraction"] = flops / one / 1e9 / F32_MATRIX_PEAK_TFLOPS
            print(json.dumps(row))


if __name__ == "__main__":
    main()
