#!/usr/bin/env python3
"""Times the mask-cropped association features on the GPU with HIP events; prints one JSON line.

  embed_ms          apse_embed (RoI features + association FC + normalise) at 3840 x 2160 on given boxes, R-101-FPN seeded
                    weights: per dtype (f32, bf16) and detection count (8, 100), "pool" = roi_pool at the box (the default) and
                    "crop" = roi_align of p2 * the detection's mask from the mask tail's bit planes (cfg.APSE.CROP_FEATURES);
                    mask_fill is the share of box pixels the masks cover (seeded weights give nearly empty masks, and a sample
                    whose mask taps are all zero skips its feature loads), so "roi_filled" times the RoI kernel alone
                    (apse_roi_features_windows, no FC) on the same boxes with an ellipse filling each box
  generator_ms      RoiFeaturesGenerator's masked RoI stage for 10 objects at 375 x 1242, host time included (wall clock around
                    mask preparation + upload + kernels + sync, the backbone excluded): "dense" = RLE decoded on the host,
                    [n][H][W] u8 upload, resize into the f32 scratch, roi_align_masked; "windows" = RLE -> bit windows on the
                    device (apse_mots_rle_to_bits), apse_roi_features_windows
Medians over --iters timed repetitions after --warmup."""
import argparse
import json
import os
import sys
import time

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


def wall(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def boxes_for(n, H, W, seed):
    """n vehicle-sized boxes (frame pixels) inside an H x W frame"""
    g = np.random.default_rng(seed)
    w, h = g.uniform(0.04, 0.09, n) * W, g.uniform(0.04, 0.09, n) * H
    x, y = g.uniform(0, W - w), g.uniform(0, H - h)
    return np.stack([x, y, x + w, y + h], axis=1).astype(np.float32)


def embed_times(args, sd, asd):
    from apse_uav_amd import _lib
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks.association_head import AssociationHead
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    from apse_uav_amd.structures import device_windows as dw
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import resample
    H, W = 2160, 3840
    dev = torch.device("cuda", torch.cuda.current_device())
    yy, xx = torch.meshgrid(torch.arange(H, device=dev) + 0.5, torch.arange(W, device=dev) + 0.5, indexing="ij")
    frame = torch.from_numpy(np.ascontiguousarray(SyntheticSequence("dynamic", H, W).frame(0)))[None].cuda()
    out = {}
    for dtype in args.dtypes.split(","):
        cfg = setup_cfg()
        cfg.APSE.DTYPE = dtype
        model = TrackRCNN(cfg)
        model.load_state_dict(sd)
        head = AssociationHead(roi_size=10, input_depth=256)
        head.load_state_dict(asd)
        model.attach_association_head(head)
        ih, iw = resample.resize_shortest_edge(H, W, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
        for n in (8, 100):
            fb = boxes_for(n, H, W, n)
            given = (fb * np.array([iw / W, ih / H] * 2, np.float32), np.zeros(n, np.int32), np.array([n], np.int32))
            model.set_crop_features(False)
            model.preprocess_frames(frame)
            model.run(1, given)
            res = model.read(1)
            fill = float(res.mass[:n].sum() / ((fb[:, 2] - fb[:, 0]) * (fb[:, 3] - fb[:, 1])).sum())
            s = _lib.stream_ptr()
            row = {"mask_fill": round(fill, 3)}
            for name, on in (("pool", False), ("crop", True)):
                model.set_crop_features(on)
                row[name] = round(timed(lambda: model._call("apse_embed", 1, s), args.warmup, args.iters), 4)
            words = []
            for x0, y0, x1, y1 in fb.tolist():
                ell = ((xx - (x0 + x1) / 2) / ((x1 - x0) / 2)) ** 2 + ((yy - (y0 + y1) / 2) / ((y1 - y0) / 2)) ** 2 <= 1
                words.append(dw.masks_words([ell], (H, W), dev)[3][0])
            torch.cuda.synchronize()
            win = dw.upload(dw.fill_windows([(0, 0, W, H)] * n, [w.shape[1] for w in words], [w.data_ptr() for w in words]), dev)
            fb_d, roi = torch.from_numpy(fb).to(dev), torch.empty((n, 256, 10, 10), device=dev)
            row["roi_filled"] = round(timed(lambda: model._call("apse_roi_features_windows", 0, _lib.ptr(fb_d), _lib.ptr(win), n, 10,
                                                                _lib.ptr(roi), s), args.warmup, args.iters), 4)
            out["%s/%d" % (dtype, n)] = row
        model._drop_ctx()
    return out


def generator_times(args, sd):
    from apse_uav_amd import _lib
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.roi_features_generator import RoiFeaturesGenerator
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import rle
    from apse_uav_amd.utils.COCO_utils import DeviceBitmasks
    H, W, n = 375, 1242, 10
    gen = RoiFeaturesGenerator(setup_cfg(), roi_size=10, state_dict=sd)
    frame = np.ascontiguousarray(SyntheticSequence("dynamic", H, W).frame(0))
    boxes = boxes_for(n, H, W, 5)
    boxes = np.stack([boxes[:, 0], boxes[:, 1], np.maximum(boxes[:, 2], boxes[:, 0] + 60), np.maximum(boxes[:, 3], boxes[:, 1] + 40)], 1)
    boxes = np.minimum(boxes, np.array([W, H, W, H], np.float32)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = []
    for x0, y0, x1, y1 in boxes:                  # an ellipse inside each box
        cx, cy, rx, ry = (x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0) / 2, (y1 - y0) / 2
        masks.append(rle.encode((((xx + 0.5 - cx) / rx) ** 2 + ((yy + 0.5 - cy) / ry) ** 2 <= 1).astype(np.uint8)))
    objects = np.stack([np.zeros(n), np.arange(n) + 1, boxes[:, 0], boxes[:, 1], boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], 1)
    gen.get_rois_features(frame, objects, masks)                    # builds the context, leaves p2 of this frame in it
    m, dev = gen.model, gen.device
    boxes_d = torch.from_numpy(boxes).to(dev)
    rois = [torch.zeros((n, 256, 10, 10), device=dev) for _ in range(2)]

    def dense():
        md = torch.from_numpy(gen._masks_dense(masks, H, W)).to(dev)
        m._call("apse_roi_features", 0, _lib.ptr(boxes_d), _lib.ptr(md), n, 10, _lib.ptr(rois[0]), _lib.stream_ptr())
        torch.cuda.synchronize()

    def windows():
        bm = DeviceBitmasks(masks, (H, W), dev)
        m._call("apse_roi_features_windows", 0, _lib.ptr(boxes_d), _lib.ptr(bm.windows), n, 10, _lib.ptr(rois[1]), _lib.stream_ptr())
        torch.cuda.synchronize()

    out = {"dense": round(wall(dense, args.warmup, args.iters), 4), "windows": round(wall(windows, args.warmup, args.iters), 4)}
    out["equal"] = bool(torch.equal(rois[0], rois[1]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--blocks", default="3,4,23,3")
    args = ap.parse_args()
    from apse_uav_amd.weights import synthetic_association_state, synthetic_detector_state
    sd = synthetic_detector_state(0, tuple(int(v) for v in args.blocks.split(",")))
    asd = synthetic_association_state(1)
    print(json.dumps({"embed_ms": embed_times(args, sd, asd), "generator_ms": generator_times(args, sd)}))


if __name__ == "__main__":
    main()
