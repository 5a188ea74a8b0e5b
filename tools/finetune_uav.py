#!/usr/bin/env python
"""Fine-tune the RPN head and the box branch of a detector jointly on the GPU -- dcnn/scripts/train/finetune_uav.py and
finetune_faster_rcnn_aerial.py with ``to_train=['proposal_generator', 'roi_heads']``: one loop, one optimiser.

Everything is frozen except ``proposal_generator.rpn_head.{conv,objectness_logits,anchor_deltas}``, ``roi_heads.box_head.fc{1,2}``
and ``roi_heads.box_predictor.{cls_score,bbox_pred}`` (14 tensors).  Per step and image the frozen backbone runs once; the anchors
are labelled and sampled as ``RPNOutputs._get_ground_truth`` does (256 per image); the box head's proposals come from the RPN
head AS IT IS AT THAT STEP, selected with detectron2's training limits (2000 per level before NMS, 1000 after), the ground truths
are appended, and 512 per image are sampled as ``ROIHeads.label_and_sample_proposals`` does.  ``loss_rpn_cls + loss_rpn_loc +
loss_cls + loss_box_reg`` is optimised with one momentum SGD under detectron2's WarmupMultiStepLR, and after every optimiser step
the new RPN head is written into the live detector contexts (``TrackRCNN.set_rpn_head``: no rebuild).  At most 4 images per batch
(4 x 256 RPN rows is one step's limit); their up to 2048 box rows go through the box head in chunks of whole images
(utils/joint_train.py box_losses_chunked).  Every CHECKPOINT_PERIOD iterations the held-out images are scored (bbox AP / AR, and
the recall of the proposals at 100 and 1000) and a checkpoint with the merged full detector is written.

  python tools/finetune_uav.py --images DIR --annotations FILE.json --weights detector.pth --classes car truck bus --out DIR
  python tools/finetune_uav.py --synthetic 6 --iters 12 --checkpoint-period 4 --out DIR     # dry run on generated data
  python tools/finetune_uav.py ... --resume                                                 # continue from DIR/<name>_last.pth
  python tools/finetune_uav.py ... --mask                                                   # the mask head too, in the same loop
  python tools/finetune_uav.py ... --mask --mask-format bitmask                             # ... on RLE segmentations (BitMasks targets)
  python tools/finetune_uav.py --mots DATASET --seqmap FILE --weights detector.pth --mask --out DIR     # KITTI MOTS ground truth

``--mask`` adds ``roi_heads.mask_head.*`` (12 tensors) as a third head under the same SGD and schedule, as detectron2's
``StandardROIHeads._forward_mask`` trains it: on the sampled FOREGROUND PROPOSALS of every image (at most 128 per image), each
matched ground truth's polygons cropped to the proposal box (``apse_coco_mask_targets``).  Every image feeds the RPN and box losses;
annotations with polygons also feed ``loss_mask`` (box-only data mixes in freely; a step without mask rows has ``loss_mask`` 0).
results.txt then carries the 12 segm COCOeval numbers of the predictor's own detections after the other columns.

Checkpoint keys: model, optimizer, scheduler, iteration, kfold_split, k_folds, best_precision, best_recall, training_results,
loader (the image order, the augmentation draws and both sampling generators), so that a resumed run repeats the uninterrupted
one bit for bit.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apse_uav_amd.utils import finetune as ft                                   # noqa: E402
from apse_uav_amd.utils.finetune import adapt_detector, holdout_split           # noqa: E402,F401

MAX_IMS = 4
SEGM_COLUMNS = "".join("\tsegm_" + c for c in ft.AP_COLUMNS.split())


def results_header(mask=False):
    """First line of results.txt: the bbox columns and the proposal recall, with ``--mask`` followed by the segm columns."""
    return ft.AP_COLUMNS + "\tprop_AR@100\tprop_AR@1000" + (SEGM_COLUMNS if mask else "") + "\n"


def merged_state(detector, rpn_head, box_head, mask_head=None):
    from apse_uav_amd.networks.box_head import merge_box_head
    from apse_uav_amd.networks.mask_head import merge_full_mask_rcnn
    from apse_uav_amd.networks.rpn_head import merge_rpn_head
    state = merge_box_head(merge_rpn_head(detector, rpn_head.state_dict()), box_head.state_dict())
    return state if mask_head is None else merge_full_mask_rcnn(state, mask_head.state_dict())


def has_polygons(dicts):
    return any(a.get("segmentation") for d in dicts for a in d["annotations"])


def do_test(pred, dicts, coco_gt, mask=False):
    """The 12 bbox COCOeval numbers (zeros when nothing was detected) followed by the proposal recall at 100 and 1000 (IoU 0.5)
    of the predictor on ``dicts``; None when there is no ground truth.  ``mask``: followed by the 12 segm COCOeval numbers of the
    masks the predictor gives its own boxes (zeros when nothing was detected or ``dicts`` hold no polygon)."""
    recall = ft.proposal_scores(pred, dicts)
    if recall is None:
        return None
    if not mask:
        ap = ft.bbox_scores(pred, dicts, coco_gt)
        return (ap if ap is not None else [0.0] * 12) + recall
    segm = has_polygons(dicts)
    res = ft.detection_scores(pred, dicts, coco_gt, ("bbox", "segm") if segm else ("bbox",))
    if res is None:
        return [0.0] * 12 + recall + [0.0] * 12
    return res[0] + recall + (res[1] if segm else [0.0] * 12)


class JointTask(ft.Task):
    what = "joint detection-head"
    precision_index, recall_index = 0, 12                               # AP, and the proposals' recall at 100
    summary_keys = ("before", "after")
    summary_predictor = True
    num_classes = staticmethod(ft.trained_classes)

    def __init__(self, mask=False):
        self.mask = bool(mask)                                          # --mask: the mask head is the third head
        self.header = results_header(self.mask)
        self.keep_box_only = self.mask                                  # box-only annotations train the RPN and box heads

    def do_test(self, pred, dicts, coco_gt):
        return do_test(pred, dicts, coco_gt, self.mask)

    def build_heads(self, args, cfg, detector, K):
        from apse_uav_amd.networks.box_head import BoxHead
        from apse_uav_amd.networks.rpn_head import RPNHead
        detector, changed = adapt_detector(detector, K)
        rpn_head = RPNHead.from_cfg(cfg, "cuda")
        rpn_head.load_state_dict(detector)
        box_head = BoxHead(K, "cuda")
        box_head.load_state_dict(detector, keep_predictor=changed)      # another class count: fc1 / fc2 only, fresh predictors
        self.heads = [rpn_head, box_head]
        if self.mask:
            from apse_uav_amd.networks.mask_head import PREFIX, MaskHead
            mask_head = MaskHead(K, "cuda")
            if any(k.startswith(PREFIX) for k in detector):             # (adapt_detector re-initialised a predictor of another K)
                mask_head.load_state_dict(detector)
            self.heads.append(mask_head)
        return detector

    def merged_state(self, detector):
        return merged_state(detector, *self.heads)

    def optimizer(self, args, params):                                  # --optimizer: only this tool has it
        import torch
        if args.optimizer == "torch":
            return torch.optim.SGD(params, lr=args.lr, momentum=args.momentum)
        return super().optimizer(args, params)

    def make_loader(self, args, dicts, model, K, sizes):
        from apse_uav_amd.utils.joint_train import JointTrainLoader
        return JointTrainLoader(dicts, model, args.ims_per_batch, args.seed, args.flip, augment=args.augment, num_classes=K,
                                mask=self.mask, mask_format=ft.mask_format(args), **sizes)

    def losses(self, batch, loader, args):
        from apse_uav_amd.utils.joint_train import box_losses_chunked
        rpn, box = batch[:2]
        losses = dict(self.heads[0](*rpn, args.ims_per_batch))
        losses.update(box_losses_chunked(self.heads[1], *box, loader.last_box_rows))
        if self.mask:
            losses.update(self.heads[2](*batch[2]))                     # no mask rows: a zero that reaches every parameter
        return losses

    def after_step(self, pred):
        pred.model.set_rpn_head(self.heads[0])                          # the next step's proposals come from this head

    def counts(self, loader):
        text = "\tpos/neg: {}\tfg/bg: {}".format(loader.last_rpn_counts, loader.last_box_counts)
        return text + ("\tmask rows: {}".format(loader.last_mask_rows) if self.mask else "")

    def push(self, pred):
        """Every head into the predictor.  The RPN head goes into the live contexts and the model's state; the mask and box
        branches then each replace their own keys of that state and mark the contexts for a rebuild, so none undoes another."""
        pred.model.set_rpn_head(self.heads[0])
        for head in self.heads[:0:-1]:                                  # the mask head (if any), then the box branch
            head.push_into(pred)

    def state(self):
        return {k: v.cpu() for head in self.heads for k, v in head.state_dict(head.prefix).items()}


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ft.add_common_arguments(ap, "R_50_FPN_UAV", "pair of heads")
    ap.add_argument("--optimizer", choices=("apse", "torch"), default="apse", help="apse_uav_amd.optim.SGD (HIP) or torch.optim.SGD")
    ap.add_argument("--mask", action="store_true",
                    help="train the mask head in the same loop, on the sampled foreground proposals (annotations without polygons "
                         "feed the RPN and box losses only); results.txt gains the segm columns")
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if not 1 <= args.ims_per_batch <= MAX_IMS:
        ap.error("--ims-per-batch must be 1 .. %d (%d x 256 RPN rows is the limit of one step)" % (MAX_IMS, MAX_IMS))
    return ft.run(JointTask(args.mask), args, ft.load_start(args, ap))


if __name__ == "__main__":
    main()
