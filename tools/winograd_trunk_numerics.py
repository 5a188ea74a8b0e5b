#!/usr/bin/env python3
"""CPU experiment behind the f32 trunk's Winograd layers (plan.hip, winograd_trunk_layer): what the extra rounding of F(2x2,3x3)
does to the maps and to the decisions when it travels through the whole backbone.

The oracle runs a 2160 x 3840 frame of the bench's synthetic sequences with the bench's weights (R-101-FPN) three ways:
  direct    the oracle as it is (torch f32 convolutions);
  winograd  the conv2 layers of --stages (default: the plan's set, res2 / res3 / res5), fpn_output4 and the RPN conv at p4 through
            apse_uav_amd.winograd.emulate (the numpy statement of the kernel's operation order, with the Cin split plan.hip gives
            the layer), frozen BN folded as plan.hip folds it;
  float64   the same backbone in double (frame 0 of the run only).
Printed per frame: max |delta| / max |ref| of res2 .. p6, proposal rows in place, detections, boxes, scores, differing mask pixels,
and, through the oracle tracker, whether ids and CSV line text agree.  The MFMA rounds differently from numpy: this removes an
objection, the GPU tests decide.

usage: winograd_trunk_numerics.py [--stages res2,res3,res5] [--frames dynamic:0,3,6,9,12,15,18,21 static:0] [--threads 16]
(about a minute per frame)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from apse_uav_amd import winograd  # noqa: E402
from apse_uav_amd.synthetic import SyntheticSequence  # noqa: E402
from apse_uav_amd.weights import UAV4K_R101_CLS_BIAS, synthetic_association_state, synthetic_detector_state  # noqa: E402
from oracle import tracker as otr  # noqa: E402
from oracle.detector import DetectorOracle, resize_shape  # noqa: E402

H, W = 2160, 3840
BLOCKS = (3, 4, 23, 3)
SPLIT = {64: 1, 128: 2, 256: 3, 512: 5}          # Cin -> the plan's Cin split at these map sizes
MAPS = ("res2", "res3", "res4", "res5", "p2", "p3", "p4", "p5", "p6")


class WinogradTrunk(DetectorOracle):
    """The oracle with the plan's trunk Winograd set emulated."""

    def __init__(self, sd, cfg, p4_hw, stages):
        super().__init__(sd, cfg)
        self.p4_hw, self.stages = p4_hw, stages

    def _conv(self, x, name, stride=1, padding=0, relu=False, store=True):
        trunk = name.endswith(".conv2") and any((".bottom_up." + s + ".") in name for s in self.stages)
        p4 = tuple(x.shape[-2:]) == self.p4_hw and name in ("backbone.fpn_output4", "proposal_generator.rpn_head.conv")
        if not (trunk or p4):
            return super()._conv(x, name, stride, padding, relu, store)
        w = self.sd[name + ".weight"]
        if (name + ".norm.weight") in self.sd:
            scale = self.sd[name + ".norm.weight"] * (1.0 / torch.sqrt(self.sd[name + ".norm.running_var"] + 1e-5))
            b = self.sd[name + ".norm.bias"] - self.sd[name + ".norm.running_mean"] * scale
            w = w * scale.view(-1, 1, 1, 1)
        else:
            b = self.sd[name + ".bias"]
        y = winograd.emulate(x[0].permute(1, 2, 0).contiguous().numpy(), w.numpy(), b.numpy(), relu, split=SPLIT[w.shape[1]])
        return torch.from_numpy(np.ascontiguousarray(y)).permute(2, 0, 1).unsqueeze(0).contiguous()


class Float64(DetectorOracle):
    def __init__(self, sd, cfg=None):
        super().__init__(sd, cfg)
        self.sd = {k: v.double() for k, v in self.sd.items()}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", nargs="+", default=["dynamic:0,3,6,9,12,15,18,21", "static:0"])
    ap.add_argument("--stages", default="res2,res3,res5", help="stages whose conv2 layers go through the emulation")
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    sd = synthetic_detector_state(0, BLOCKS, cls_bias=UAV4K_R101_CLS_BIAS)
    asd = synthetic_association_state(1)
    cfg = dict(depth_blocks=BLOCKS)
    ih, iw = resize_shape(H, W)
    p4_hw = (-(-ih // 32) * 2, -(-iw // 32) * 2)
    direct, wino, f64 = DetectorOracle(sd, cfg), WinogradTrunk(sd, cfg, p4_hw, tuple(args.stages.split(","))), Float64(sd, cfg)
    print("frame %dx%d resized %dx%d, blocks %s, conv2 of %s + fpn_output4 + rpn conv at p4, splits %s" % (H, W, ih, iw, BLOCKS, args.stages, SPLIT),
          flush=True)
    first = True
    for spec in args.frames:
        kind, idxs = spec.split(":")
        seq = SyntheticSequence(kind, H, W)
        trackers = otr.TrackerOracle(), otr.TrackerOracle()
        for t, fi in enumerate(int(v) for v in idxs.split(",")):
            img = np.asarray(Image.fromarray(seq.frame(fi)).resize((iw, ih), Image.BILINEAR))
            chw = torch.as_tensor(img.astype("float32").transpose(2, 0, 1))
            t0 = time.time()
            posts, lines, ids = [], [], []
            with torch.no_grad():
                for o, tk in zip((direct, wino), trackers):
                    post = o.inference(chw, H, W)
                    rois = otr.features_rois(post["features"]["p2"], post["boxes"], W)
                    emb = otr.association_head(rois, asd["fc.weight"], asd["fc.bias"])
                    rec = tk.next_frame(dict(boxes=post["boxes"], scores=post["scores"], classes=post["classes"],
                                             masks=list(zip(post["mask_windows"], post["mask_rects"])), emb=emb))
                    posts.append(post); lines.append(otr.log_oneline(rec, 1, t)[0]); ids.append(rec["ids"])
                ref = f64.backbone(f64.preprocess(chw.double()).double()) if first else None
            pa, pb = posts
            print("%s %d (%.0f s)" % (kind, fi, time.time() - t0))
            for k in MAPS:
                a, b = pa["features"][k], pb["features"][k]
                line = "  %-4s direct vs winograd %.3e" % (k, rel(b, a))
                if ref is not None:
                    line += "   direct vs f64 %.3e   winograd vs f64 %.3e" % (rel(a.double(), ref[k]), rel(b.double(), ref[k]))
                print(line)
            A, B = pa["proposals"]["boxes"], pb["proposals"]["boxes"]
            same = int((A - B).abs().max(dim=1).values.lt(1e-3).sum()) if A.shape == B.shape else -1
            print("  proposals %d, rows in place %d" % (A.shape[0], same))
            n = (pa["boxes"].shape[0], pb["boxes"].shape[0])
            out = "  detections %d / %d" % n
            if n[0] == n[1]:
                rects = all(tuple(x) == tuple(y) for x, y in zip(pa["mask_rects"], pb["mask_rects"]))
                bad = sum(int((x != y).sum()) for x, y in zip(pa["mask_windows"], pb["mask_windows"])) if rects else -1
                out += ", classes equal %s, boxes max |d| %.2e px, scores max |d| %.2e, mask rects equal %s, mask pixels differing %d of %d" % (
                    bool(torch.equal(pa["classes"], pb["classes"])), float((pa["boxes"] - pb["boxes"]).abs().max()) if n[0] else 0.0,
                    float((pa["scores"] - pb["scores"]).abs().max()) if n[0] else 0.0, rects, bad, sum(int(x.sum()) for x in pa["mask_windows"]))
            print(out)
            print("  ids equal %s, csv line equal %s" % (ids[0] == ids[1], lines[0] == lines[1]), flush=True)
            first = False


if __name__ == "__main__":
    main()
