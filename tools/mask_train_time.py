#!/usr/bin/env python3
"""Times one mask-head training step on the GPU with HIP events (medians after warm-up); prints one JSON line per RoI count.

  roi_features_ms   backbone (KITTI-size frame, seeded R-50-FPN-shaped weights) + apse_mask_roi_features for the RoIs
  forward_ms        head forward with saved activations + loss
  wgrad_ms / dgrad_ms / other_ms   backward split: weight gradients (MFMA implicit GEMM), data gradients, the rest
                                   (loss gradient, predictor, ReLU masks, bias sums)
  sgd_ms            apse_uav_amd.optim.SGD step over the 12 parameters
  step_ms           forward + backward + SGD as MaskHead runs them
  wgrad3x3_tflops   one 3x3 weight-gradient launch (with its reduce pass) against the 157.3 TFLOP/s f32 matrix peak
  fwd3x3_ratio      that launch's time over the inference kernel's (apse_conv2d, conv_igemm_f32) on the same layer: equal FLOPs
"""
import argparse
import ctypes as C
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
    ap.add_argument("--rois", type=int, nargs="*", default=[16, 64, 256])
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-backbone", action="store_true")
    args = ap.parse_args()
    from apse_uav_amd import _lib
    from apse_uav_amd.networks import mask_head as mh
    from apse_uav_amd.optim import SGD

    lib = _lib.load()
    dev = "cuda"
    K = args.classes
    model = None
    if not args.no_backbone:
        from apse_uav_amd.config import setup_cfg
        from apse_uav_amd.engines.track_predictor import TrackPredictor
        from apse_uav_amd.synthetic import SyntheticSequence
        from apse_uav_amd.weights import synthetic_detector_state
        cfg = setup_cfg(num_classes=K)
        pred = TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (3, 4, 6, 3), num_classes=K))
        model = pred.model
        frame = torch.from_numpy(SyntheticSequence("dynamic", 375, 1242).frame(0)[None]).cuda()
    for n in args.rois:
        g = torch.Generator().manual_seed(n)
        head = mh.MaskHead(K, dev)
        torch.manual_seed(0)
        params = list(head.parameters())
        opt = SGD(params, lr=0.02, momentum=0.9)
        x = torch.relu(torch.randn(n, 14, 14, 256, generator=g)).to(dev)
        cls = torch.randint(0, K, (n,), generator=g)
        tg = (torch.rand(n, 28, 28, generator=g) < 0.4).to(dev)
        row = {"rois": n, "classes": K}
        if model is not None:
            rg = np.random.default_rng(n)
            x0, y0 = rg.uniform(0, 1000, n), rg.uniform(0, 250, n)
            boxes = np.stack([x0, y0, x0 + rg.uniform(8, 200, n), y0 + rg.uniform(8, 100, n)], 1).astype(np.float32)

            def feat():
                model.backbone_frames(frame)
                model.mask_roi_features(boxes)
            row["roi_features_ms"] = timed(feat, args.warmup, args.iters)

        def step():
            opt.zero_grad()
            loss = head(x, cls, tg)["loss_mask"]
            loss.backward()
            opt.step()
        row["step_ms"] = timed(step, args.warmup, args.iters)
        # pieces, on the operator wrappers
        det = [p.detach() for p in params]
        ws = mh._workspace(n, K, dev)
        clsd, tgd = cls.to(torch.int32).to(dev), tg.to(torch.uint8)
        state = {}

        def fwd():
            state["lg"], state["acts"] = mh.head_logits(x, det, ws, keep=True)
            state["out"] = mh.loss_forward(state["lg"], clsd, tgd, ws)
        row["forward_ms"] = timed(fwd, args.warmup, args.iters)
        lg, acts = state["lg"], state["acts"]
        d = mh.loss_backward(lg, clsd, tgd)
        g5, _, _ = mh.predictor_backward(d, acts[5], clsd, det[10].reshape(K, 256), ws)
        g4 = torch.randn_like(acts[4])

        def wgrads():
            mh.weight_grad(acts[4], g5, 1, ws)
            for i in range(4):
                mh.weight_grad(g4, acts[i], 0, ws)
        row["wgrad_ms"] = timed(wgrads, args.warmup, args.iters)

        def dgrads():
            pk, _ = mh.pack_weight(det[8], None, 0, 256, 256, 2, 2)
            mh.conv_forward(g5, pk, None, 256, 2, 2, 2, 0, False, False, ws)
            for i in range(1, 4):
                pk, _ = mh.pack_weight(det[2 * i], None, 1, 256, 256, 3, 3)
                mh.conv3x3(g4, pk, None, False)
        row["dgrad_ms"] = timed(dgrads, args.warmup, args.iters)

        def other():
            dd = mh.loss_backward(lg, clsd, tgd)
            mh.predictor_backward(dd, acts[5], clsd, det[10].reshape(K, 256), ws)
            mh.bias_grad(g5, ws)
            mh.relu_grad(acts[4], g4)
            for i in range(4):
                mh.bias_grad(g4, ws)
                if i:
                    mh.relu_grad(acts[i], g4)
        row["other_ms"] = timed(other, args.warmup, args.iters)
        for p in params:
            p.grad = torch.zeros_like(p)
        row["sgd_ms"] = timed(opt.step, args.warmup, args.iters)
        one = timed(lambda: mh.weight_grad(g4, acts[0], 0, ws), args.warmup, args.iters)
        flops = 2.0 * 256 * 2304 * n * 196
        row["wgrad3x3_ms"] = one
        row["wgrad3x3_tflops"] = flops / one / 1e9
        row["wgrad3x3_peak_fraction"] = flops / one / 1e9 / 157.3
        pk, bp = mh.pack_weight(det[0], det[1], 0, 256, 256, 3, 3)
        row["train_fwd3x3_ms"] = timed(lambda: mh.conv3x3(x, pk, bp, True), args.warmup, args.iters)
        dsc = _lib.ConvDesc()
        dsc.B, dsc.H, dsc.W, dsc.Cin, dsc.Cout, dsc.KH, dsc.KW, dsc.stride, dsc.pad = n, 14, 14, 256, 256, 3, 3, 1, 1
        dsc.relu, dsc.cfg = 1, -1
        y = torch.empty_like(x)
        cws = torch.empty(64 * n * 196 * 256 // 8 + 1024, device=dev)

        def inf():
            rc = lib.apse_conv2d(C.byref(dsc), _lib.ptr(x), _lib.ptr(pk), _lib.ptr(bp), None, _lib.ptr(y), _lib.ptr(cws),
                                 cws.numel() * 4, _lib.stream_ptr())
            assert rc == 0, rc
        row["infer_fwd3x3_ms"] = timed(inf, args.warmup, args.iters)
        row["fwd3x3_ratio"] = one / row["infer_fwd3x3_ms"]
        print(json.dumps(row))


if __name__ == "__main__":
    main()
