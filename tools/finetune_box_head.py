#!/usr/bin/env python
"""Fine-tune the box branch of a detector on the GPU -- the ``roi_heads`` half of dcnn/scripts/train/finetune_uav.py and
finetune_faster_rcnn_aerial.py.

Everything is frozen except ``roi_heads.box_head.fc{1,2}`` and ``roi_heads.box_predictor.{cls_score,bbox_pred}``; the proposals
are the detector's own RPN output (its test-time selection) with the ground-truth boxes appended, labelled and sampled as
detectron2's ``ROIHeads.label_and_sample_proposals`` does (512 per image, a quarter foreground); ``loss_cls + loss_box_reg`` is
optimised with momentum SGD under detectron2's WarmupMultiStepLR; every CHECKPOINT_PERIOD iterations the held-out images are
scored (bbox AP / AR) and a checkpoint with the merged full detector is written.

``--classes`` with a class count other than the checkpoint's keeps fc1 / fc2 and re-initialises the two predictor layers (and
the mask predictor, whose channels are per class): a COCO model to three or four vehicle classes.

  python tools/finetune_box_head.py --images DIR --annotations FILE.json --weights detector.pth --classes car truck bus --out DIR
  python tools/finetune_box_head.py --synthetic 6 --iters 12 --checkpoint-period 4 --out DIR     # dry run on generated data
  python tools/finetune_box_head.py ... --resume                                                 # continue from DIR/<name>_last.pth

Checkpoint keys: model, optimizer, scheduler, iteration, kfold_split, k_folds, best_precision, best_recall, training_results,
loader (the image order, the augmentation draws and the sampling generator), so that a resumed run repeats the uninterrupted one
bit for bit.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apse_uav_amd.utils import finetune as ft                                   # noqa: E402
from apse_uav_amd.utils.finetune import adapt_detector, holdout_split           # noqa: E402,F401
from apse_uav_amd.utils.finetune import bbox_scores as do_test                  # noqa: E402


class BoxTask(ft.Task):
    what = "box-head"
    num_classes = staticmethod(ft.trained_classes)
    do_test = staticmethod(do_test)

    def build_heads(self, args, cfg, detector, K):
        from apse_uav_amd.networks.box_head import BoxHead
        detector, changed = adapt_detector(detector, K)
        head = BoxHead(K, "cuda")
        head.load_state_dict(detector, keep_predictor=changed)          # another class count: fc1 / fc2 only, fresh predictors
        self.heads = [head]
        return detector

    def merged_state(self, detector):
        from apse_uav_amd.networks.box_head import merge_box_head
        return merge_box_head(detector, self.heads[0].state_dict())

    def make_loader(self, args, dicts, model, K, sizes):
        from apse_uav_amd.utils.box_train import BoxTrainLoader
        return BoxTrainLoader(dicts, model, args.ims_per_batch, args.seed, args.flip, augment=args.augment, num_classes=K,
                              train_topk=tuple(int(v) for v in args.train_topk.split(",")) if args.train_topk else None, **sizes)

    def losses(self, batch, loader, args):
        return self.heads[0](*batch)

    def counts(self, loader):
        return "\tfg/bg: {}".format(loader.last_counts)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ft.add_common_arguments(ap, "R_50_FPN_UAV_BOX", "box branch")
    ap.add_argument("--train-topk", default="", metavar="PRE,POST",
                    help="train on the RPN's training-time selection, e.g. 2000,1000 as the reference's yaml (default: the "
                         "test-time selection)")
    args = ap.parse_args(argv)
    return ft.run(BoxTask(), args, ft.load_start(args, ap))


if __name__ == "__main__":
    main()
