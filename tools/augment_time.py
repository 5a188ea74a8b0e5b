#!/usr/bin/env python3
"""Times the training augmentation on the GPU (HIP events, the median of --iters runs after --warmup); one JSON line per row.

  --kernel   apse_augment_u8 (both passes; u8 + f32 CHW outputs) at 800 x 1333 and 2160 x 3840, next to a device-to-device
             copy on the same card -- of the image (3 B / pixel each way) and of as many bytes as the kernels move (6 read + 15
             written per pixel) -- and the numpy oracle (tests/augment_ref.py) over 16 host threads, one strip of rows each
  --step     a whole mask-head training step (loader + head forward / backward + SGD) on generated 540 x 960 images, R-50-FPN
             shaped seeded weights: the plain loader, the augmenting loader over three sizes with its context cache, and the
             same with APSE.CONTEXT_CACHE = 1 (a context rebuild at almost every image)
  --memory   device memory one more cached context takes (torch.cuda.mem_get_info around the first visit of a second image
             size), R-50 and R-101 shaped weights, 1080 x 1920 frames at short edges 704 and 640
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

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


def oracle_threads(img, wb, ws, wc, lw, threads=16):
    """tests/augment_ref.py over ``threads`` strips of rows (numpy releases the GIL): seconds for the whole chain."""
    import augment_ref as A
    strips = np.array_split(np.arange(img.shape[0]), threads)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        sat = list(ex.map(lambda r: A.saturation(A.brightness(img[r[0]:r[-1] + 1], wb), ws), strips))
        S = sum(ex.map(A.image_sum, sat))
        s = np.float32(np.float64(1.0 - wc) * (np.float64(S) / np.float64(img.size)))

        def rest(a):
            return A.lighting(A.to_u8(s + np.float32(wc) * a.astype(np.float32)), lw)
        out = list(ex.map(rest, sat))
    dt = time.perf_counter() - t0
    return dt, np.concatenate(out), S


def kernel_rows(args):
    from apse_uav_amd import _lib
    from apse_uav_amd.utils import augment
    lib = _lib.load()
    p = augment.AugmentParams(True, 1.07, 0.93, 1.05, (0.2, -0.1, 0.15))
    for h, w in ((800, 1333), (2160, 3840)):
        img = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        src = torch.from_numpy(img[None]).cuda()
        out, chw = torch.empty_like(src), torch.empty((1, 3, h, w), device="cuda")
        sums = torch.empty((1,), dtype=torch.int64, device="cuda")
        cp = (augment._CParams * 1)()
        cp[0].flip, cp[0].brightness, cp[0].saturation, cp[0].contrast = 1, p.brightness, p.saturation, p.contrast
        for c in range(3):
            cp[0].lighting_vec[c] = float(p.lighting_vec()[c])

        def run(o=out, f=chw):
            rc = lib.apse_augment_u8(_lib.ptr(src), 1, h, w, cp, _lib.ptr(o), _lib.ptr(f), _lib.ptr(sums), _lib.stream_ptr())
            assert rc == 0, rc
        row = {"mode": "kernel", "h": h, "w": w, "augment_ms": timed(run, args.warmup, args.iters),
               "augment_u8_only_ms": timed(lambda: run(out, None), args.warmup, args.iters),
               "augment_chw_only_ms": timed(lambda: run(None, chw), args.warmup, args.iters)}
        dst = torch.empty_like(src)
        row["copy_image_ms"] = timed(lambda: dst.copy_(src), args.warmup, args.iters)
        n = h * w * 21 // 2                                    # a copy reads n and writes n: 21 bytes per pixel in all
        a, b = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        row["copy_same_bytes_ms"] = timed(lambda: b.copy_(a), args.warmup, args.iters)
        row["ratio_to_copy_same_bytes"] = row["augment_ms"] / row["copy_same_bytes_ms"]
        row["augment_gbps"] = h * w * 21 / row["augment_ms"] / 1e6
        host = [oracle_threads(img, p.brightness, p.saturation, p.contrast, p.lighting) for _ in range(3)]
        row["oracle_16_threads_ms"] = 1e3 * float(np.median([t[0] for t in host]))
        row["equal_to_oracle"] = bool(np.array_equal(out.cpu().numpy()[0], host[0][1][:, ::-1])) and int(sums[0]) == host[0][2]
        print(json.dumps(row), flush=True)


def _predictor(blocks, K=4, cache=1):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.CONTEXT_CACHE = cache
    return TrackPredictor(cfg, state_dict=synthetic_detector_state(0, blocks, num_classes=K))


def step_rows(args):
    from PIL import Image
    from apse_uav_amd.networks import mask_head as mh
    from apse_uav_amd.optim import SGD
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils import COCO_utils
    K, H, W = 4, 540, 960
    root = tempfile.mkdtemp(prefix="augment_time_")
    seq, g, dicts = SyntheticSequence("dynamic", H, W), np.random.default_rng(0), []
    for i in range(8):
        name = os.path.join(root, "%03d.png" % i)
        Image.fromarray(seq.frame(i)[:, :, ::-1].copy()).save(name)
        anns = []
        for _ in range(8):
            bw, bh = float(g.integers(16, 300)), float(g.integers(16, 120))
            x, y = float(g.integers(0, W - int(bw))), float(g.integers(0, H - int(bh)))
            anns.append({"bbox": [x, y, bw, bh], "bbox_mode": 1, "category_id": int(g.integers(0, K)), "iscrowd": 0,
                         "segmentation": [[x, y, x + bw, y, x + bw, y + bh, x, y + bh]]})
        dicts.append({"file_name": name, "image_id": i + 1, "height": H, "width": W, "annotations": anns})
    pred = _predictor((3, 4, 6, 3), K)
    model = pred.model
    sizes = (640, 704, 800)
    for label, kw, cache in (("plain", {}, None), ("augment_3_sizes_cached", dict(augment=True, flip=True, min_sizes=sizes), None),
                             ("augment_3_sizes_cache_1", dict(augment=True, flip=True, min_sizes=sizes), 1),
                             ("augment_1_size", dict(augment=True, flip=True), None)):
        model.cfg.APSE.CONTEXT_CACHE = 1
        loader = COCO_utils.MaskTrainLoader(dicts, model, ims_per_batch=2, seed=0, **kw)
        if cache is not None:
            model.cfg.APSE.CONTEXT_CACHE = cache                 # after the loader raised it
        torch.manual_seed(0)
        head = mh.MaskHead(K, "cuda")
        opt = SGD(list(head.parameters()), lr=0.02, momentum=0.9)
        built0, load_ms, step_ms = model.contexts_built, [], []
        for it in range(args.warmup + args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            feats, cls, tg = next(loader)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            opt.zero_grad()
            head(feats, cls, tg)["loss_mask"].backward()
            opt.step()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= args.warmup:
                load_ms.append(1e3 * (t1 - t0))
                step_ms.append(1e3 * (t2 - t0))
        print(json.dumps({"mode": "step", "loader": label, "context_cache": int(model.cfg.APSE.CONTEXT_CACHE), "ims_per_batch": 2,
                          "loader_ms": float(np.median(load_ms)), "step_ms": float(np.median(step_ms)),
                          "step_mean_ms": float(np.mean(step_ms)), "contexts_built": model.contexts_built - built0}), flush=True)


def memory_rows(args):
    H, W = 1080, 1920
    for name, blocks in (("R-50", (3, 4, 6, 3)), ("R-101", (3, 4, 23, 3))):
        pred = _predictor(blocks, cache=2)
        model = pred.model
        from apse_uav_amd.utils import resample
        used = []
        for size in (704, 640):
            ih, iw = resample.resize_shortest_edge(H, W, size, 1333)
            img = torch.zeros((1, 3, ih, iw), device="cuda")
            torch.cuda.synchronize()
            free0, _ = torch.cuda.mem_get_info()
            model.backbone_images(img, (H, W))
            torch.cuda.synchronize()
            free1, _ = torch.cuda.mem_get_info()
            used.append((ih, iw, (free0 - free1) / 2 ** 20))
        print(json.dumps({"mode": "memory", "model": name, "first_context": used[0], "second_context": used[1],
                          "contexts": len(model._cache)}), flush=True)
        del pred, model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not (args.kernel or args.step or args.memory):
        args.kernel = True
    if args.kernel:
        kernel_rows(args)
    if args.step:
        step_rows(args)
    if args.memory:
        memory_rows(args)


if __name__ == "__main__":
    main()
