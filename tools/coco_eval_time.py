#!/usr/bin/env python3
"""Wall and kernel time of COCO evaluation (utils/coco_eval.py) on a COCO-val-sized synthetic set.

    python tools/coco_eval_time.py [--images 5000] [--dets 100] [--iou-type bbox segm]

5000 images of about 640x480, 80 categories, about 7.3 ground truths per image (about 36k; 1 % crowd as RLE, the rest polygons
of 6 to 16 vertices), 100 detections per image (box-sized results; for 'segm' the detections are device WindowMask windows, as
the online evaluator gets them from the predictor).  Prints evaluate() and accumulate() wall time, and the GPU time between HIP
events around each call (kernels plus the uploads and read-backs of the call).  Run under ``rocprofv3 --kernel-trace --stats``
for the per-kernel split.
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_set(n_img, n_det, seed=0, segm=False):
    import torch
    from apse_uav_amd.structures.window_mask import WindowMask
    from apse_uav_amd.utils import rle
    g = np.random.default_rng(seed)
    images, anns, res = [], [], []
    dev = torch.device("cuda", torch.cuda.current_device())
    for i in range(n_img):
        h, w = (480, 640) if g.random() < .6 else (int(g.integers(360, 500)), 640)
        images.append(dict(id=i + 1, height=h, width=w))
        n_gt = int(g.poisson(7.3))
        boxes = []
        for _ in range(n_gt):
            bw, bh = float(g.uniform(4, w / 3)), float(g.uniform(4, h / 3))
            x, y = float(g.uniform(0, w - bw)), float(g.uniform(0, h - bh))
            c = int(g.integers(0, 80))
            a = dict(id=len(anns) + 1, image_id=i + 1, category_id=c, bbox=[x, y, bw, bh], iscrowd=int(g.random() < .01))
            if a["iscrowd"]:
                m = np.zeros((h, w), np.uint8)
                m[int(y):int(y + bh), int(x):int(x + bw)] = 1
                a["segmentation"] = dict(size=[h, w], counts=rle.counts_from_mask(m))
                a["area"] = float(m.sum())
            else:
                k = int(g.integers(6, 17))
                t = np.sort(g.uniform(0, 2 * np.pi, k))
                px = x + bw / 2 + bw / 2 * np.cos(t) * g.uniform(.6, 1, k)
                py = y + bh / 2 + bh / 2 * np.sin(t) * g.uniform(.6, 1, k)
                a["segmentation"] = [np.stack([px, py], 1).reshape(-1).tolist()]
                a["area"] = bw * bh * .6
            anns.append(a)
            boxes.append((c, x, y, bw, bh))
        for k in range(n_det):
            if boxes and g.random() < .5:
                c, x, y, bw, bh = boxes[int(g.integers(0, len(boxes)))]
                x, y = x + g.normal(0, 3), y + g.normal(0, 3)
            else:
                c = int(g.integers(0, 80))
                bw, bh = float(g.uniform(4, w / 3)), float(g.uniform(4, h / 3))
                x, y = float(g.uniform(0, w - bw)), float(g.uniform(0, h - bh))
            x, y = float(min(max(x, 0), w - bw)), float(min(max(y, 0), h - bh))
            r = dict(image_id=i + 1, category_id=c, bbox=[x, y, bw, bh], score=float(g.random()))
            res.append(r)
    if segm:                                              # filled box windows on the device, one pool
        rects = np.array([[int(r["bbox"][0]), int(r["bbox"][1]), int(r["bbox"][0] + r["bbox"][2]) + 1,
                           int(r["bbox"][1] + r["bbox"][3]) + 1] for r in res], np.int64)
        hw = {im["id"]: (im["height"], im["width"]) for im in images}
        for k, r in enumerate(res):
            hh, ww = hw[r["image_id"]]
            rects[k, 2], rects[k, 3] = min(rects[k, 2], ww), min(rects[k, 3], hh)
        wpr = ((rects[:, 2] + 63) >> 6) - (rects[:, 0] >> 6)
        words = wpr * (rects[:, 3] - rects[:, 1])
        off = np.concatenate([[0], np.cumsum(words)])
        pool = torch.full((int(off[-1]),), -1, dtype=torch.int64, device=dev)
        for k, r in enumerate(res):
            bits = pool[off[k]:off[k + 1]].view(int(rects[k, 3] - rects[k, 1]), int(wpr[k]))
            r["segmentation"] = WindowMask(bits, rects[k], hw[r["image_id"]], (-1, -1), 0)
    cats = [dict(id=c, name=str(c)) for c in range(80)]
    return dict(images=images, annotations=anns, categories=cats), res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--iou-type", nargs="+", default=["bbox", "segm"])
    args = ap.parse_args(argv)
    import torch
    from apse_uav_amd.utils.coco import COCO
    from apse_uav_amd.utils.coco_eval import COCOeval
    for iou_type in args.iou_type:
        t0 = time.time()
        ds, res = make_set(args.images, args.dets, segm=iou_type == "segm")
        with contextlib.redirect_stdout(io.StringIO()):
            gt = COCO.from_dataset(ds)
            dt = gt.loadRes(res)
        print("%s: %d images, %d ground truths (%d crowd), %d detections (built in %.1f s)" % (
            iou_type, len(ds["images"]), len(ds["annotations"]), sum(a["iscrowd"] for a in ds["annotations"]), len(res),
            time.time() - t0))
        ev = COCOeval(gt, dt, iou_type)
        times = {}
        for step in ("evaluate", "accumulate"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            w0 = time.time()
            e0.record()
            with contextlib.redirect_stdout(io.StringIO()):
                getattr(ev, step)()
            e1.record()
            torch.cuda.synchronize()
            times[step] = (time.time() - w0, e0.elapsed_time(e1) / 1e3)
        ev.summarize()
        for step, (wall, gpu) in times.items():
            print("%s %-10s wall %7.2f s   GPU (events) %7.3f s" % (iou_type, step, wall, gpu))


if __name__ == "__main__":
    main()
