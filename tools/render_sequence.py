"""Rendered tracking on one GPU: a synthetic sequence through RcnnTracker, every frame drawn by TrackVisualizer (the HIP renderer)
and written as a PNG through Pillow -- the image half of visualize_uav.py:208-215.

    python tools/render_sequence.py [--size 2160x3840] [--frames 16] [--given-boxes] [--resize 1920x1080] [--out-dir DIR]

--given-boxes feeds the synthetic vehicles' boxes as detected_instances (tools/run_sequence.py), so seeded weights still produce
objects with masks.  Printed: objects per frame; HIP-event times of the tracker step (next_frame) and of whole
draw_instance_predictions calls on a device frame, out of place and in place (host preparation of the items included; kernel
times: run it under rocprofv3 --kernel-trace --stats); and the end-to-end rate including get_image().
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="2160x3840", help="HxW of the synthetic frames")
    ap.add_argument("--kind", default="dynamic", choices=["static", "dynamic"])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--given-boxes", action="store_true")
    ap.add_argument("--resize", default="", help="WxH of the written PNGs (Pillow bilinear); default: frame size")
    ap.add_argument("--out-dir", default="", help="PNG directory (default: no files written)")
    ap.add_argument("--reps", type=int, default=50, help="repetitions of each timed render")
    ap.add_argument("--input-format", default="bgr", choices=["bgr", "nv12", "i420"],
                    help="frame format handed to the tracker (cfg.INPUT.FORMAT); nv12 / i420: the BGR frames are encoded on the "
                         "host first (apse_uav_amd/synthetic.py), as a stand-in for a video decoder's output")
    ap.add_argument("--yuv-matrix", default="cv601", choices=["cv601", "bt601", "bt709", "bt601-full", "bt709-full"],
                    help="YUV -> BGR conversion of nv12 / i420 input (cfg.APSE.YUV_MATRIX)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("render_sequence.py: no GPU visible (the renderer has no CPU fallback)")
    from PIL import Image
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.utils.track_visualizer import TrackVisualizer
    from apse_uav_amd.weights import UAV4K_R101_CLS_BIAS, synthetic_association_state, synthetic_detector_state
    H, W = [int(v) for v in args.size.split("x")]
    cfg = setup_cfg()
    cfg.INPUT.FORMAT = args.input_format.upper()
    cfg.APSE.YUV_MATRIX = args.yuv_matrix
    tracker = RcnnTracker(cfg, (H, W), synthetic_association_state(1),
                          detector_state=synthetic_detector_state(0, cls_bias=UAV4K_R101_CLS_BIAS))
    seq = SyntheticSequence(args.kind, H, W)
    given_fn = None
    if args.given_boxes:
        from run_sequence import synthetic_given_fn
        given_fn = synthetic_given_fn(seq, H, W, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    vis = TrackVisualizer({"thing_classes": ["car", "truck", "bus", "van"]})
    vis.yuv_matrix = args.yuv_matrix
    from apse_uav_amd.synthetic import encoded_source
    from apse_uav_amd.utils.preprocess import yuv_to_bgr
    get_frame = encoded_source(seq.frame, cfg.INPUT.FORMAT, args.yuv_matrix)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
    size = tuple(int(v) for v in args.resize.split("x")) if args.resize else None
    step_ms, oop_ms, inp_ms, counts = [], [], [], []
    t0 = time.perf_counter()
    for t in range(args.frames):
        frame = get_frame(t)                  # BGR, or its NV12 / I420 encoding: tracked and drawn as it is
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if given_fn is not None:
            tracker.frame_count += 1
            dets = tracker.predictor.predict_batch([frame], given=given_fn([t]))[0][0]["instances"]
            objs = tracker._finish_frame(dets, None)
        else:
            objs = tracker.next_frame(frame)
        b.record()
        img = vis.draw_instance_predictions(frame, objs).get_image()
        step_ms.append(a.elapsed_time(b))
        counts.append(len(objs))
        if args.out_dir:
            im = Image.fromarray(img)
            if size:
                im = im.resize(size, Image.BILINEAR)
            im.save(os.path.join(args.out_dir, "image_%04d.png" % (t + 1)))
        dev = torch.from_numpy(frame).to("cuda") if cfg.INPUT.FORMAT == "BGR" else yuv_to_bgr(frame, args.yuv_matrix)
        oop_ms.append(_events_ms(lambda: vis.draw_instance_predictions(dev, objs), args.reps))
        inp_ms.append(_events_ms(lambda: vis.draw_instance_predictions(dev, objs, inplace=True), args.reps))
    dt = time.perf_counter() - t0
    print("frames %d at %dx%d, objects per frame %s" % (args.frames, H, W, counts))
    print("tracker step (events around next_frame): median %.3f ms" % float(np.median(step_ms)))
    print("render out of place: median %.1f us, in place: median %.1f us (device frame, HIP events, %d reps)"
          % (1e3 * float(np.median(oop_ms)), 1e3 * float(np.median(inp_ms)), args.reps))
    print("end to end incl. render, get_image()%s and the timing reps: %.2f frames/s"
          % (" and PNG writes" if args.out_dir else "", args.frames / dt))


if __name__ == "__main__":
    main()
