#!/usr/bin/env python3
"""Times the pieces joint RPN / box-head training adds, on the GPU with HIP events (medians after warm-up) at an 800 x 1344
training image; prints one JSON line per measurement.

  rpn_test_ms        apse_rpn: the RPN convolutions and the context's test-time selection (1000 per level, 1000)
  rpn_train_1000_ms  apse_rpn_train_proposals at (1000, 1000): the same convolutions and the training selection's kernels
  rpn_train_2000_ms  ... at (2000, 1000), the reference yaml's training limits
  rpn_train_2048_ms  ... at (2048, 2048), the entry's limits
  set_rpn_head_ms    apse_set_rpn_head: the device-side re-packing of the six tensors into the plan's buffers
  step_ms            one whole joint step per batch of 1, 2 and 4 images: per image the frozen backbone, anchor labelling and
                     sampling, patch gather, training proposals, proposal labelling and sampling, ROIAlign 7; then both heads
                     forward and backward (the box rows in chunks of 1024), SGD over the 14 tensors and the weight refresh
  backbone_ms        the frozen backbone alone, per image (inside step_ms)

--mask adds the mask head as the joint loop's third head (tools/finetune_uav.py --mask) and prints, beside step_ms,
  step_mask_ms       the same step with the mask rows: per image the foreground proposals' ROIAlign 14, the polygon upload and
                     apse_coco_mask_targets, then MaskHead forward and backward and SGD over the 26 tensors (mask_rows = the rows)
  targets_device_ms  apse_coco_mask_targets alone for --target-rows rows (512: 4 images x 128) of one image's jittered ground-truth
                     boxes, with the upload of that image's polygons and the read of the info word
  targets_host_ms    utils.COCO_utils.mask_targets, the host path, for the same rows (wall clock: it blocks on every object)
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
    ap.add_argument("--gts", type=int, default=20, help="ground truths per image")
    ap.add_argument("--frame", type=int, nargs=2, default=[800, 1344])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--mask", action="store_true", help="also time the step with the mask head's rows, and the targets alone")
    ap.add_argument("--target-rows", type=int, default=512)
    args = ap.parse_args()
    from apse_uav_amd import _lib
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.networks.box_head import BoxHead
    from apse_uav_amd.networks.mask_head import MaskHead
    from apse_uav_amd.networks.rpn_head import RPNHead
    from apse_uav_amd.optim import SGD
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils.box_train import label_and_sample_proposals
    from apse_uav_amd.utils.COCO_utils import DevicePolygons, mask_targets, mask_targets_device, select_mask_rows
    from apse_uav_amd.utils.joint_train import box_losses_chunked
    from apse_uav_amd.utils.rpn_train import label_and_sample_anchors
    from apse_uav_amd.weights import synthetic_detector_state

    dev, K = "cuda", 4
    H, W = args.frame
    cfg = setup_cfg(num_classes=K)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = min(H, W), max(H, W)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    state = synthetic_detector_state(0, (1, 1, 1, 1), num_classes=K)
    model = TrackPredictor(cfg, state_dict=state).model
    frame = torch.from_numpy(SyntheticSequence("dynamic", H, W).frame(0)[None]).cuda()
    model.backbone_frames(frame)
    lib, s = _lib.load(), _lib.stream_ptr()
    row = {"frame": [H, W], "device": torch.cuda.get_device_name(0)}
    row["backbone_ms"] = timed(lambda: model.backbone_frames(frame), args.warmup, args.iters)
    row["rpn_test_ms"] = timed(lambda: model._call("apse_rpn", 1, s), args.warmup, args.iters)
    boxes = torch.empty((1, 2048, 4), device=dev)
    scores = torch.empty((1, 2048), device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    for pre, post in ((1000, 1000), (2000, 1000), (2048, 2048)):
        nbytes = int(lib.apse_rpn_train_proposals_workspace_bytes(1, pre))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        row["rpn_train_%d_ms" % pre] = timed(lambda: model._call("apse_rpn_train_proposals", 1, pre, post, _lib.ptr(boxes), _lib.ptr(scores),
                                                                 _lib.ptr(count), _lib.ptr(ws), nbytes, s), args.warmup, args.iters)
        row["count_%d" % pre] = int(count.cpu()[0])
    rpn = RPNHead(dev)
    rpn.load_state_dict(state)
    six = [p.detach().contiguous() for p in rpn.parameters()]
    row["set_rpn_head_ms"] = timed(lambda: model._call("apse_set_rpn_head", *[_lib.ptr(t) for t in six], s), args.warmup, args.iters)
    print(json.dumps(row), flush=True)

    g = torch.Generator().manual_seed(args.gts)
    xy = torch.rand(args.gts, 2, generator=g) * torch.tensor([W - 80.0, H - 80.0])
    gt = torch.cat([xy, xy + 16 + torch.rand(args.gts, 2, generator=g) * 64], 1).to(dev)
    cls = torch.randint(0, K, (args.gts,), generator=g).to(dev, torch.int32)
    # every ground truth's polygon: an octagon inside its box (8 vertices, as a typical COCO part is short)
    gth = gt.cpu().numpy().astype(np.float64)
    cx, cy, rx, ry = (gth[:, 0] + gth[:, 2]) / 2, (gth[:, 1] + gth[:, 3]) / 2, (gth[:, 2] - gth[:, 0]) / 2, (gth[:, 3] - gth[:, 1]) / 2
    ang = np.arange(8) * (np.pi / 4) + 0.2
    polys = [[np.stack([cx[k] + rx[k] * np.cos(ang), cy[k] + ry[k] * np.sin(ang)], 1).reshape(-1).tolist()] for k in range(args.gts)]
    if args.mask:
        import time
        n = args.target_rows
        pick = torch.randint(0, args.gts, (n,), generator=g)
        jit = gt[pick.to(dev)] + (torch.rand(n, 4, generator=g) * 8 - 4).to(dev)
        matched = pick.to(dev, torch.int32)
        dev_ms = timed(lambda: mask_targets_device(DevicePolygons(polys, dev), jit, matched), args.warmup, args.iters)
        boxes_host, per_roi = jit.cpu().numpy(), [polys[int(k)] for k in pick]
        host = []
        for it in range(1 + max(1, args.iters // 3)):             # the first call warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = mask_targets(per_roi, boxes_host, dev)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        same = bool(torch.equal(want, mask_targets_device(DevicePolygons(polys, dev), jit, matched)))
        print(json.dumps({"target_rows": n, "targets_device_ms": dev_ms, "targets_host_ms": float(np.median(host[1:])),
                          "bytes_equal": same}), flush=True)
    for images, with_mask in [(i, m) for i in args.images for m in ((False, True) if args.mask else (False,))]:
        box = BoxHead(K, dev)
        box.load_state_dict(state)
        rpn = RPNHead(dev)
        rpn.load_state_dict(state)
        heads = [rpn, box]
        if with_mask:
            mask = MaskHead(K, dev)
            mask.load_state_dict(state)
            heads.append(mask)
        opt = SGD([p for h in heads for p in h.parameters()], lr=0.001, momentum=0.9)
        ga, gb = torch.Generator(device=dev), torch.Generator(device=dev)
        ga.manual_seed(0)
        gb.manual_seed(1)
        rows = {}

        def step():
            r_items, b_items, m_items = [], [], []
            for _ in range(images):
                model.backbone_frames(frame)
                sel, rl, rm, _ = label_and_sample_anchors(model, gt, 256, 0.5, ga)
                patches, slots, anchors, _ = model.rpn_patches(sel)
                props = model.train_proposals(1)[0][0]
                sb, bl, bm, _, bi = label_and_sample_proposals(props, gt, cls, K, 512, 0.25, gb, return_index=True)
                r_items.append((patches, slots, rl, anchors, rm))
                b_items.append((model.box_roi_features(sb), bl, sb, bm))
                if with_mask:                                   # JointTrainLoader._mask_rows
                    pd = DevicePolygons(polys, dev)
                    lh = bl.cpu().numpy()
                    keep, _ = select_mask_rows(lh, bi.cpu().numpy(), pd.parts, K)
                    kd = torch.from_numpy(keep).to(dev)
                    mb = sb[kd].contiguous()
                    m_items.append((model.mask_roi_features(mb), torch.from_numpy(lh[keep].astype(np.int64)),
                                    mask_targets_device(pd, mb, bi[kd])))
            r = tuple(torch.cat([i[k] for i in r_items]) for k in range(5))
            b = tuple(torch.cat([i[k] for i in b_items]) for k in range(4))
            rows["rpn"], rows["box"] = int(r[0].shape[0]), int(b[0].shape[0])
            losses = dict(rpn(*r, images))
            losses.update(box_losses_chunked(box, *b, [int(i[0].shape[0]) for i in b_items]))
            if with_mask:
                m = tuple(torch.cat([i[k] for i in m_items]) for k in range(3))
                rows["mask"] = int(m[0].shape[0])
                losses.update(mask(*m))
            opt.zero_grad()
            sum(losses.values()).backward()
            opt.step()
            model.set_rpn_head(rpn)
        ms = timed(step, args.warmup, args.iters)
        out = {"images": images, "gts_per_image": args.gts, "rpn_rows": rows["rpn"], "box_rows": rows["box"]}
        if with_mask:
            out["mask_rows"] = rows["mask"]
        out["step_mask_ms" if with_mask else "step_ms"] = ms
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
