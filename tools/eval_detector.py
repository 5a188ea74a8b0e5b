#!/usr/bin/env python3
"""Box and mask AP of a detector checkpoint on a COCO-format dataset, on the GPU: the reference's ``do_test``
(dcnn/scripts/train/finetune_uav.py, finetune_segmentation.py) for iouType 'bbox' and 'segm'.

    python tools/eval_detector.py --images DIR --annotations GT_JSON --weights W.pth \
        [--num-classes K] [--score-thresh 0.05] [--arch FPN|C4] [--dtype f32|bf16|f16] [--out results.json]
    python tools/eval_detector.py --synthetic N        # dry run: seeded weights, generated images and ground truth

Class k of the model is category ``sorted(catIds)[k]`` (detectron2's contiguous ids; the identity for the reference's
``detectron2_dataset_to_coco`` ids 0..K-1).  Images are taken grouped by size: the predictor rebuilds its context whenever the
frame size changes (networks/track_rcnn.py ``_ensure_ctx``), and COCO mixes hundreds of sizes.  Detections are scored online
(utils/coco_eval.py CocoEvaluator: masks stay on the device); ``--out`` also writes them as ``instances_to_coco_json`` results.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_dataset(root, n, seed=0, num_classes=4):
    """apse_uav_amd.synthetic.synthetic_dataset (it lives in the package, where the fine-tune loop reaches it too)."""
    from apse_uav_amd.synthetic import synthetic_dataset as impl
    return impl(root, n, seed, num_classes)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", default="")
    ap.add_argument("--annotations", default="")
    ap.add_argument("--weights", default="")
    ap.add_argument("--num-classes", type=int, default=0, help="default: the number of categories")
    ap.add_argument("--score-thresh", type=float, default=0.05)
    ap.add_argument("--arch", default="FPN", choices=["FPN", "C4"])
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16"])
    ap.add_argument("--out", default="")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    args = ap.parse_args(argv)

    import torch
    from PIL import Image
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.utils.coco import COCO
    from apse_uav_amd.utils.coco_eval import CocoEvaluator, instances_to_coco_json

    tmp = None
    state = None
    if args.synthetic:
        from apse_uav_amd.weights import synthetic_c4_state, synthetic_detector_state
        tmp = tempfile.TemporaryDirectory()
        args.images = tmp.name
        args.annotations = synthetic_dataset(tmp.name, args.synthetic)
        k = args.num_classes or 4
        state = synthetic_c4_state(0, (1, 1, 1, 1), num_classes=k) if args.arch == "C4" else \
            synthetic_detector_state(0, (1, 1, 1, 1), num_classes=k)
    elif not (args.images and args.annotations and args.weights):
        ap.error("--images, --annotations and --weights are required (or --synthetic N)")

    gt = COCO(args.annotations)
    cats = sorted(gt.getCatIds())
    K = args.num_classes or len(cats)
    if K > len(cats):
        ap.error("--num-classes %d: the annotations define only %d categories" % (K, len(cats)))
    cfg = setup_cfg(weights=args.weights if state is None else "", score_thresh=args.score_thresh, num_classes=K, arch=args.arch)
    cfg.APSE.DTYPE = args.dtype
    pred = TrackPredictor(cfg, state_dict=state)
    imgs = gt.loadImgs(sorted(gt.getImgIds()))
    order = sorted(imgs, key=lambda im: (int(im["height"]), int(im["width"]), im["id"]))
    online = CocoEvaluator(gt, category_ids=cats[:K])
    results = [] if args.out else None
    n_det = 0
    built0 = pred.model.contexts_built
    t0 = time.time()
    for im in order:
        frame = np.asarray(Image.open(os.path.join(args.images, im["file_name"])).convert("RGB"))[:, :, ::-1].copy()
        if frame.shape[:2] != (im["height"], im["width"]):
            raise ValueError("%s is %dx%d, the annotations say %dx%d" % (im["file_name"], frame.shape[0], frame.shape[1],
                                                                           im["height"], im["width"]))
        inst = pred(frame)[0]["instances"]
        n_det += len(inst)
        online.add(im["id"], inst)
        if results is not None:
            for r in instances_to_coco_json(inst, im["id"]):
                r["category_id"] = cats[r["category_id"]]
                results.append(r)
    torch.cuda.synchronize()
    sizes = len({(int(im["height"]), int(im["width"])) for im in order})
    print("%d images of %d sizes, %d detections, %d contexts built, %.2f s" % (len(order), sizes, n_det,
                                                                            pred.model.contexts_built - built0, time.time() - t0))
    if results is not None:
        with open(args.out, "w") as fh:
            json.dump(results, fh)
    out = {}
    for iou_type in ("bbox", "segm"):
        print("Evaluation results for %s:" % iou_type)
        out[iou_type] = online.evaluate(iou_type).stats
    if tmp is not None:
        tmp.cleanup()
    return out


if __name__ == "__main__":
    main()
