#!/usr/bin/env python3
"""COCO box / mask AP of a results file on the GPU, with pycocotools' output (only the DONE (t=...) times differ).

    python tools/coco_eval.py GT_JSON RESULTS_JSON --iou-type bbox|segm

GT_JSON is a COCO annotation file, RESULTS_JSON a list of detections (``instances_to_coco_json`` / detectron2's
coco_instances_results.json).  The IoU, matching and accumulation run in HIP (utils/coco_eval.py).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("gt_json")
    ap.add_argument("results_json")
    ap.add_argument("--iou-type", default="bbox", choices=["bbox", "segm"])
    args = ap.parse_args(argv)
    from apse_uav_amd.utils.coco import COCO
    from apse_uav_amd.utils.coco_eval import COCOeval
    coco_gt = COCO(args.gt_json)
    coco_dt = coco_gt.loadRes(args.results_json)
    ev = COCOeval(coco_gt, coco_dt, args.iou_type)
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev


if __name__ == "__main__":
    main()
