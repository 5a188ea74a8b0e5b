#!/usr/bin/env python3
"""What YUV input buys at the entry point: ``RcnnTracker.next_frame`` at 3840 x 2160 (R-101-FPN shapes, synthetic weights, the
model of bench.py) from

    host BGR      an HxWx3 array in pageable memory (24.9 MB staged and sent per frame),
    host NV12     a YuvFrame over a host array (12.4 MB),
    device NV12   a YuvFrame over a CUDA tensor (a decoder surface: nothing staged, nothing sent),

each with and without ``upcoming=``, in f32 and bf16, batch 1: frames/s over the timed steps (wall clock) and the p50 of a
call.  And, by HIP events on the launch stream, the stand-alone converter (apse_yuv_to_bgr) and the resize (horizontal +
vertical pass, apse_resize_normalize) with BGR and with NV12 row staging -- the two differ in the horizontal pass only.

    python tools/ingest_time.py [--steps 24] [--warmup 4] [--dtypes f32,bf16] [--matrix bt709]

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def entry_rates(tracker, frames, steps, warmup, ahead):
    n = len(frames)
    tracker.reset_tracker()
    lat, t0 = [], 0.0
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        ts = time.perf_counter()
        objs = tracker.next_frame(frames[i % n], upcoming=frames[(i + 1) % n] if ahead else None)
        tracker.log_line(objs, 1, i)
        if i >= warmup:
            lat.append(time.perf_counter() - ts)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"frames_per_s": round(steps / dt, 2), "p50_ms": round(1000.0 * float(np.median(lat)), 3)}


def event_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    s = torch.cuda.current_stream()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(s)
        fn()
        b.record(s)
    torch.cuda.synchronize()
    return round(float(np.median([a.elapsed_time(b) for a, b in ev])), 4)


def kernel_times(H, W, nv12, bgr, matrix, min_size, max_size):
    from apse_uav_amd import _lib
    from apse_uav_amd.structures.yuv_frame import matrix_index
    from apse_uav_amd.utils import resample
    lib = _lib.load()
    oh, ow = resample.resize_shortest_edge(H, W, min_size, max_size)
    ph, pw = (oh + 31) // 32 * 32, (ow + 31) // 32 * 32
    hb, hc, hk = resample.precompute_coeffs(W, ow)
    vb, vc, vk = resample.precompute_coeffs(H, oh)
    t = [torch.from_numpy(a).cuda() for a in (hb, hc, vb, vc)]
    src_y, src_b = torch.from_numpy(nv12.data).cuda(), torch.from_numpy(bgr).cuda()
    dst = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    tmp = torch.empty((H, ow, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, ph, pw, 4), device="cuda")
    mean = (C.c_float * 3)(103.530, 116.280, 123.675)
    m, s = matrix_index(matrix), _lib.stream_ptr()

    def conv():
        _lib.check(lib.apse_yuv_to_bgr(_lib.ptr(src_y), _lib.ptr(dst), 1, H, W, nv12.pitch, 0, m, s), None, "apse_yuv_to_bgr")

    def rs_bgr():
        _lib.check(lib.apse_resize_normalize(_lib.ptr(src_b), _lib.ptr(tmp), _lib.ptr(out), None, _lib.ptr(t[0]), _lib.ptr(t[1]), hk, _lib.ptr(t[2]),
                                             _lib.ptr(t[3]), vk, 1, H, W, oh, ow, ph, pw, C.byref(mean), s), None, "apse_resize_normalize")

    def rs_yuv():
        _lib.check(lib.apse_resize_normalize_yuv(_lib.ptr(src_y), nv12.pitch, 0, m, _lib.ptr(tmp), _lib.ptr(out), None, _lib.ptr(t[0]), _lib.ptr(t[1]),
                                                 hk, _lib.ptr(t[2]), _lib.ptr(t[3]), vk, 1, H, W, oh, ow, ph, pw, C.byref(mean), s), None,
                   "apse_resize_normalize_yuv")
    return {"yuv_to_bgr_ms": event_ms(conv), "resize_bgr_staging_ms": event_ms(rs_bgr), "resize_nv12_staging_ms": event_ms(rs_yuv),
            "horizontal_taps": hk, "what": "HIP events, median of 20; resize = horizontal + vertical pass, one 3840x2160 frame"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--blocks", type=str, default="3,4,23,3")
    ap.add_argument("--dtypes", type=str, default="f32,bf16")
    ap.add_argument("--matrix", type=str, default="bt709")
    args = ap.parse_args()

    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.structures.yuv_frame import YuvFrame
    from apse_uav_amd.synthetic import SyntheticSequence, bgr_to_nv12
    from apse_uav_amd.utils.hostinfo import usable_cpus
    from apse_uav_amd.weights import UAV4K_R101_CLS_BIAS, synthetic_association_state, synthetic_detector_state
    torch.set_num_threads(max(1, min(torch.get_num_threads(), usable_cpus())))
    H, W = args.height, args.width
    blocks = tuple(int(v) for v in args.blocks.split(","))
    sd = synthetic_detector_state(0, blocks, cls_bias=UAV4K_R101_CLS_BIAS) if blocks == (3, 4, 23, 3) else synthetic_detector_state(0, blocks)
    asd = synthetic_association_state(1)
    seq = SyntheticSequence("dynamic", H, W)
    bgr = [seq.frame(t) for t in range(6)]
    nv12 = [bgr_to_nv12(f, args.matrix) for f in bgr]
    dev = [YuvFrame(torch.from_numpy(y.data).cuda(), y.width, "NV12") for y in nv12]
    out = {"frame": "%dx%d" % (W, H), "matrix": args.matrix, "steps": args.steps, "modes": {}}
    for dtype in args.dtypes.split(","):
        for name, fmt, frames in (("host_bgr", "BGR", bgr), ("host_nv12", "NV12", nv12), ("device_nv12", "NV12", dev)):
            cfg = setup_cfg()
            cfg.APSE.DTYPE = dtype
            cfg.INPUT.FORMAT = fmt
            cfg.APSE.YUV_MATRIX = args.matrix
            tr = RcnnTracker(cfg, (H, W), asd, detector_state=sd)
            for ahead in (False, True):
                key = "%s/%s%s" % (dtype, name, "/upcoming" if ahead else "")
                out["modes"][key] = entry_rates(tr, frames, args.steps, args.warmup, ahead)
            del tr
    cfg = setup_cfg()
    out["kernels"] = kernel_times(H, W, nv12[0], bgr[0], args.matrix, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
