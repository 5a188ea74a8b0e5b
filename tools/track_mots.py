#!/usr/bin/env python3
"""Track the sequences of a KITTI MOTS seqmap and write or score the results: the --mots_evaluation mode of the reference's
standard_rcnn_tracker_test.py.

    python tools/track_mots.py SEQMAP --images IMAGE_DIR [--output DIR] [--eval GT_DIR] [--no-write] [--txt]
                               [--detector-state FILE] [--association-state FILE] [--metric NAME]

IMAGE_DIR holds one folder of PNG / JPEG / BMP frames per sequence (datasets/data_tracking_image_2/training/image_02 in the
reference); frames are read with Pillow.  For every frame the tracker's objects become the u16 id map of
result_image_from_objects(crop_overlapping_masks(objects)), rendered on the device, written as DIR/SEQ/000000.png, ...
(default output/evaluation_results, as the reference).  --eval GT_DIR scores the tracker online against the ground truth
(utils/mots_eval.MotsEvaluator) and prints eval.py's tables; --no-write skips the PNGs.  Without state files the tracker runs
on the seeded synthetic weights (apse_uav_amd.weights), which exercises the pipeline but detects nothing meaningful.
--txt also writes DIR/SEQ.txt, the MOTS text result format: per frame the file_lines_from_instances lines of the cropped
objects (frame index frame_count - 1, as the reference's commented-out writer), encoded on the device from the mask windows.
--metric mask_iou tracks without an association head (no --association-state needed): centroid-aligned mask IoU >= 0.7.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXTENSIONS = ("jpg", "jpeg", "png", "bmp")


def image_files(path):
    return [f for f in sorted(os.listdir(path)) if f.split(".")[-1].lower() in EXTENSIONS]


def frame_txt_lines(objects, frame_idx, size):
    """The MOTS .txt lines of one frame: file_lines_from_instances(crop_overlapping_masks(objects)); ``objects`` keeps its
    masks (the crop works on a copy of the list)."""
    from apse_uav_amd.structures.instances import Instances
    from apse_uav_amd.structures.window_mask import MaskList
    from apse_uav_amd.utils.mots_evaluation import crop_overlapping_masks, file_lines_from_instances
    clone = Instances(tuple(size))
    clone.pred_classes, clone.scores, clone.ids = objects.pred_classes, list(objects.scores), list(objects.ids)
    clone.pred_masks = MaskList(objects.pred_masks)
    crop_overlapping_masks(clone)
    return file_lines_from_instances(clone, frame_idx, size)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("seqmap")
    ap.add_argument("--images", required=True, help="folder of per-sequence image folders")
    ap.add_argument("--output", default="output/evaluation_results")
    ap.add_argument("--eval", default="", help="ground-truth folder: score online")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--txt", action="store_true", help="also write OUTPUT/SEQ.txt (MOTS text results)")
    ap.add_argument("--detector-state", default="", help="torch.load-able detector state dict")
    ap.add_argument("--association-state", default="", help="torch.load-able association head state dict")
    ap.add_argument("--metric", default="embeddings", choices=["embeddings", "mask_iou"], help="association metric")
    ap.add_argument("--crop-features", action="store_true",
                    help="associate on mask-cropped RoI features (cfg.APSE.CROP_FEATURES): for a head trained with --crop-features")
    ap.add_argument("--input-format", default="bgr", choices=["bgr", "nv12", "i420"],
                    help="frame format handed to the tracker (cfg.INPUT.FORMAT); nv12 / i420: the BGR frames are encoded on the "
                         "host first (apse_uav_amd/synthetic.py), as a stand-in for a video decoder's output")
    ap.add_argument("--yuv-matrix", default="cv601", choices=["cv601", "bt601", "bt709", "bt601-full", "bt709-full"],
                    help="YUV -> BGR conversion of nv12 / i420 input (cfg.APSE.YUV_MATRIX)")
    args = ap.parse_args(argv)
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        sys.exit("track_mots.py: no GPU visible (the tracker has no CPU fallback)")
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.utils.mots_eval import MotsEvaluator, render_idmap
    from apse_uav_amd.utils.mots_evaluation import parse_mots_seqmap
    from apse_uav_amd.synthetic import encoded_source
    from apse_uav_amd.weights import synthetic_association_state, synthetic_detector_state
    det = torch.load(args.detector_state) if args.detector_state else synthetic_detector_state(0)
    assoc = torch.load(args.association_state) if args.association_state else synthetic_association_state(1)
    if args.metric != "embeddings" and not args.association_state:
        assoc = None
    sequences, _ = parse_mots_seqmap(args.seqmap)
    print("Running evaluation for sequences:")
    for s in sequences:
        print(s)
    evaluator = MotsEvaluator(args.eval, args.seqmap) if args.eval else None
    for seq in sequences:
        seq_path = os.path.join(args.images, seq)
        names = image_files(seq_path)
        first = np.asarray(Image.open(os.path.join(seq_path, names[0])).convert("RGB"))
        size = first.shape[:2]
        cfg = setup_cfg()
        cfg.INPUT.FORMAT = args.input_format.upper()
        cfg.APSE.YUV_MATRIX = args.yuv_matrix
        cfg.APSE.CROP_FEATURES = bool(args.crop_features)
        tracker = RcnnTracker(cfg, size, assoc, association_metric=args.metric, detector_state=det)
        encode = encoded_source(lambda f: f, cfg.INPUT.FORMAT, args.yuv_matrix)
        out_dir = os.path.join(args.output, seq)
        if not args.no_write:
            os.makedirs(out_dir, exist_ok=True)
        txt = []
        if evaluator is not None:
            evaluator.begin_sequence(seq)
        print("\nEvaluating sequence: ", seq)
        for name in names:
            print(name, end="\r")
            frame = np.ascontiguousarray(np.asarray(Image.open(os.path.join(seq_path, name)).convert("RGB"))[:, :, ::-1])
            objects = tracker.next_frame(encode(frame))          # BGR, as cv2.imread gives the reference (or its YUV encoding)
            frame_idx = tracker.frame_count - 1
            if evaluator is not None:
                evaluator.add_frame(frame_idx, objects, size)
            if not args.no_write:
                img = render_idmap(objects, size).cpu().numpy()
                Image.fromarray(img).save(os.path.join(out_dir, "%06d.png" % frame_idx))
            if args.txt:
                txt.append(frame_txt_lines(objects, frame_idx, size) if len(objects) else "")
        if args.txt:
            os.makedirs(args.output, exist_ok=True)
            with open(os.path.join(args.output, seq + ".txt"), "w") as fh:
                fh.write("".join(txt))
        if evaluator is not None:
            evaluator.end_sequence()
    if evaluator is not None:
        print()
        evaluator.finish(out=print)


if __name__ == "__main__":
    main()
