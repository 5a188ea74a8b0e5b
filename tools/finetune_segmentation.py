#!/usr/bin/env python
"""Fine-tune the mask head of a box detector on the GPU -- counterpart of dcnn/scripts/train/finetune_segmentation.py.

Everything is frozen except ``roi_heads.mask_head.*``; the ground-truth boxes are the proposals; ``loss_mask`` is optimised with
momentum SGD (lr 0.02, momentum 0.9) under detectron2's WarmupMultiStepLR; every CHECKPOINT_PERIOD iterations the held-out
images are scored (segm AP / AR, ground-truth boxes and classes given to the detector with score 1) and a checkpoint with the
merged full detector is written.  The reference passes the boxes through its box head as proposals; this project has no
proposals-given box head, so the boxes go straight to the mask branch (``detected_instances``).

  python tools/finetune_segmentation.py --images DIR --annotations FILE.json --weights detector.pth --classes car truck bus person --out DIR
  python tools/finetune_segmentation.py --synthetic 12 --iters 40 --out DIR          # dry run on generated data, seeded weights
  python tools/finetune_segmentation.py ... --resume                                 # continue from DIR/<name>_last.pth
  python tools/finetune_segmentation.py ... --mask-format bitmask                    # RLE segmentations too (BitMasks targets)
  python tools/finetune_segmentation.py --mots DATASET --seqmap FILE --weights detector.pth --out DIR     # KITTI MOTS ground truth
  python tools/finetune_segmentation.py --synthetic 12 --mots --iters 20 --out DIR   # dry run on a generated MOTS dataset

Checkpoint keys (the reference's): model, optimizer, scheduler, iteration, kfold_split, k_folds, best_precision, best_recall,
training_results -- plus ``loader`` (the sampling state) so that a resumed run repeats the uninterrupted one bit for bit.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apse_uav_amd.utils import finetune as ft                                   # noqa: E402
from apse_uav_amd.networks.mask_head import PREFIX                              # noqa: E402
from apse_uav_amd.utils.finetune import holdout_split                           # noqa: E402,F401


def do_test(pred, dicts, coco_gt):
    """segm COCOeval stats (12 numbers) of the predictor's masks for the ground-truth boxes and classes of ``dicts``; None
    when there is nothing to score."""
    import torch
    from PIL import Image
    from apse_uav_amd.utils import resample
    from apse_uav_amd.utils.coco_eval import CocoEvaluator
    ev = CocoEvaluator(coco_gt)
    total = 0
    cap = int(pred.cfg.TEST.DETECTIONS_PER_IMAGE)
    for d in dicts:
        frame = np.asarray(Image.open(d["file_name"]).convert("RGB"))[:, :, ::-1].copy()
        H, W = frame.shape[:2]
        ih, iw = resample.resize_shortest_edge(H, W, pred.cfg.INPUT.MIN_SIZE_TEST, pred.cfg.INPUT.MAX_SIZE_TEST)
        anns = d["annotations"][:cap]
        b = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in anns],
                     np.float64).reshape(-1, 4) * np.array([iw / W, ih / H, iw / W, ih / H])
        classes = np.array([a["category_id"] for a in anns], np.int32)
        with torch.no_grad():
            insts, _ = pred.model.inference_frames(torch.from_numpy(frame[None]).to(pred.model.device),
                                                   given=(b.astype(np.float32), classes, np.array([len(anns)], np.int32)))
        ev.add(d["image_id"], insts[0])
        total += len(insts[0])
    if total == 0:
        return None
    return [float(v) for v in ev.evaluate("segm").stats]


class MaskTask(ft.Task):
    what = "mask-head"
    do_test = staticmethod(do_test)
    precomputed_proposals = True        # the ground-truth boxes as proposals, as the reference's dictionaries have them
    context_cache = None                # CONTEXT_CACHE is left to the loader (it raises it on the device path)
    best_needs_score = True             # _bestAP / _bestAR only when the held-out images gave a score
    resume_takes_detector = False       # --resume keeps the start detector as the frozen part
    loader_state_optional = True        # checkpoints from before the loader's state was saved resume too

    def num_classes(self, args, detector, dicts):
        K = ft.detector_classes(detector)                               # the detector's classes (+ background)
        if max(a["category_id"] for d in dicts for a in d["annotations"]) >= K:
            raise ValueError("the annotations map to more classes than the detector's %d" % K)
        return K

    def build_heads(self, args, cfg, detector, K):
        from apse_uav_amd.networks.mask_head import MaskHead
        head = MaskHead(K, "cuda")
        if any(k.startswith(PREFIX) for k in detector):
            head.load_state_dict(detector)
        self.heads = [head]
        return detector

    def merged_state(self, detector):
        from apse_uav_amd.networks.mask_head import merge_full_mask_rcnn
        return merge_full_mask_rcnn(detector, self.heads[0].state_dict())

    def make_loader(self, args, dicts, model, K, sizes):
        from apse_uav_amd.utils.COCO_utils import MaskTrainLoader
        return MaskTrainLoader(dicts, model, args.ims_per_batch, args.seed, args.flip, args.cache_features, augment=args.augment,
                               mask_format=ft.mask_format(args), **sizes)

    def losses(self, batch, loader, args):
        return self.heads[0](*batch)

    def report(self, losses, loader):
        value = float(losses["loss_mask"])
        return value, "loss: {}".format(value)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ft.add_common_arguments(ap, "R_50_FPN_UAV_SEGM", "mask head, if any,")
    ap.add_argument("--cache-features", action="store_true")
    args = ap.parse_args(argv)
    detector = ft.load_start(args, ap)
    if args.synthetic:
        detector = {k: v for k, v in detector.items() if not k.startswith(PREFIX)}          # a box detector: no mask head
    return ft.run(MaskTask(), args, detector)


if __name__ == "__main__":
    main()
