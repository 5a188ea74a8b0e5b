#!/usr/bin/env python
"""Fine-tune the RPN head of a detector on the GPU -- the ``proposal_generator`` half of dcnn/scripts/train/finetune_uav.py and
finetune_faster_rcnn_aerial.py.

Everything is frozen except ``proposal_generator.rpn_head.{conv,objectness_logits,anchor_deltas}``; the anchors of p2 .. p6 are
labelled against the ground-truth boxes and sampled as detectron2's ``RPNOutputs._get_ground_truth`` does (IoU 0.3 / 0.7 with
low-quality matches, 256 per image, half positive); ``loss_rpn_cls + loss_rpn_loc`` is optimised with momentum SGD under
detectron2's WarmupMultiStepLR; every CHECKPOINT_PERIOD iterations the recall of the detector's proposals on the held-out images
(at 100 and at 1000 proposals, IoU 0.5) is written to results.txt and a checkpoint with the merged full detector is written.
``--classes`` only filters the annotations: the RPN is class-agnostic and the detector keeps its class count.  Run
tools/finetune_box_head.py on the resulting checkpoint to adapt the box head to the new proposals.

  python tools/finetune_rpn.py --images DIR --annotations FILE.json --weights detector.pth --out DIR
  python tools/finetune_rpn.py --synthetic 6 --iters 12 --checkpoint-period 4 --out DIR     # dry run on generated data
  python tools/finetune_rpn.py ... --resume                                                 # continue from DIR/<name>_last.pth

Checkpoint keys: model, optimizer, scheduler, iteration, kfold_split, k_folds, best_recall, training_results, loader (the image
order, the augmentation draws and the sampling generator), so that a resumed run repeats the uninterrupted one bit for bit.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apse_uav_amd.utils import finetune as ft                                   # noqa: E402
from apse_uav_amd.utils.finetune import holdout_split                           # noqa: E402,F401
from apse_uav_amd.utils.finetune import proposal_scores as do_test              # noqa: E402


class RpnTask(ft.Task):
    what = "RPN-head"
    header = "\t\tAR@100\tAR@1000\n"
    precision_index, recall_index = None, 0                             # no precision: no _bestAP, no best_precision key
    summary_keys = ("recall_before", "recall_after")
    summary_num_classes = False
    summary_predictor = True
    coco_ground_truth = False

    def build_heads(self, args, cfg, detector, K):
        from apse_uav_amd.networks.rpn_head import RPNHead
        head = RPNHead.from_cfg(cfg, "cuda")
        head.load_state_dict(detector)
        self.heads = [head]
        return detector

    def merged_state(self, detector):
        from apse_uav_amd.networks.rpn_head import merge_rpn_head
        return merge_rpn_head(detector, self.heads[0].state_dict())

    def make_loader(self, args, dicts, model, K, sizes):
        from apse_uav_amd.utils.rpn_train import RpnTrainLoader
        return RpnTrainLoader(dicts, model, args.ims_per_batch, args.seed, args.flip, augment=args.augment, **sizes)

    def losses(self, batch, loader, args):
        return self.heads[0](*batch, args.ims_per_batch)

    def counts(self, loader):
        return "\tpos/neg: {}".format(loader.last_counts)

    def do_test(self, pred, dicts, coco_gt):
        return do_test(pred, dicts)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ft.add_common_arguments(ap, "R_50_FPN_UAV_RPN", "RPN head")
    args = ap.parse_args(argv)
    return ft.run(RpnTask(), args, ft.load_start(args, ap))


if __name__ == "__main__":
    main()
