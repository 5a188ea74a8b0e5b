"""The data side of RPN-head training: detectron2's ``RPNOutputs._get_ground_truth`` + ``subsample_labels`` on the device, the
loader that turns dataset dictionaries into the sampled anchors' input patches (networks/rpn_head.py consumes them,
tools/finetune_rpn.py is the loop), and the recall of the detector's proposals.
"""
import numpy as np
import torch

from ..networks import box_head as bh
from ..networks import rpn_head as rh
from .box_train import SamplingLoader, subsample_labels


def label_and_sample_anchors(model, gt_boxes, batch_size_per_image=256, positive_fraction=0.5, generator=None,
                             iou_thresholds=(0.3, 0.7), image=0):
    """One image's RPN training targets, on the device.  ``model``: a TrackRCNN (FPN) whose context holds the image (after
    ``backbone_frames`` / ``backbone_images``); gt_boxes f32 [G][4] in resized-image pixels.  apse_rpn_anchor_labels labels every
    anchor (1 / 0 / -1), ``utils.box_train.subsample_labels`` draws at most ``batch_size_per_image`` of them, positives first.
    -> (anchor indices int64 [n], labels int32 [n] (1 positive, 0 negative), matched ground-truth boxes f32 [n][4] (zeros without a
    ground truth), (num_pos, num_neg))."""
    dev = model.device
    gt = torch.as_tensor(gt_boxes, dtype=torch.float32).reshape(-1, 4).to(dev).contiguous()
    labels, idx, _ = model.rpn_anchor_targets(gt, image, iou_thresholds)
    pos, neg = subsample_labels(labels, batch_size_per_image, positive_fraction, 0, generator)
    sel = torch.cat([pos, neg])
    matched = gt[idx[sel].long()] if gt.shape[0] else torch.zeros((sel.numel(), 4), dtype=torch.float32, device=dev)
    lab01 = torch.cat([torch.ones_like(pos), torch.zeros_like(neg)]).to(torch.int32)
    return sel, lab01, matched, (int(pos.numel()), int(neg.numel()))


class RpnTrainLoader(SamplingLoader):
    """Yields (patches f32 [n][2304], slots int32 [n], labels int32 [n], anchor_boxes f32 [n][4], gt_boxes f32 [n][4]) per batch of
    ``ims_per_batch`` images, endlessly, in a seeded shuffled order.  ``model``: a TrackRCNN (FPN, f32) with the frozen detector's
    weights.  Per image: the image and annotation path of MaskTrainLoader (test size on the host, or the device path with
    ``augment`` / ``min_sizes``), the frozen backbone, ``label_and_sample_anchors`` with a device generator seeded from ``seed``,
    then the patch gather at the sampled anchors.  Crowd annotations are dropped.  ``state_dict`` also carries the sampling
    generator's state.  The losses of a batch are divided by ``batch_size_per_image x ims_per_batch``: pass ``ims_per_batch`` as
    RPNHead.forward's ``num_images``."""

    def __init__(self, dicts, model, ims_per_batch=2, seed=0, flip=False, augment=False, min_sizes=None, max_size=None,
                 sampling="choice", batch_size_per_image=256, positive_fraction=0.5, iou_thresholds=(0.3, 0.7)):
        if getattr(model, "c4", False):
            raise NotImplementedError("RPN-head training covers FPN models (p2 .. p6, 3 anchors per position)")
        super().__init__(dicts, model, ims_per_batch, seed, flip, False, rh.MAX_ROWS, augment, min_sizes, max_size, sampling)
        self.batch_size_per_image = int(batch_size_per_image)
        self.positive_fraction = float(positive_fraction)
        self.iou_thresholds = (float(iou_thresholds[0]), float(iou_thresholds[1]))
        if self.ims_per_batch * self.batch_size_per_image > rh.MAX_ROWS:
            raise ValueError("%d images x %d anchors exceed the %d rows of one step (APSE_BOX_TRAIN_MAX_N)"
                             % (self.ims_per_batch, self.batch_size_per_image, rh.MAX_ROWS))
        self.seed_generators(generator=seed)
        self.last_counts = []                 # (num_pos, num_neg) per image of the last batch

    def _sample(self, boxes, polys, classes, d):
        model = self.model
        gt, _ = self.ground_truth(boxes, classes, d)
        sel, labels, matched, counts = label_and_sample_anchors(model, gt, self.batch_size_per_image, self.positive_fraction,
                                                                self.generator, self.iou_thresholds)
        patches, slots, anchor_boxes, _ = model.rpn_patches(sel)
        return patches, slots, labels, anchor_boxes, matched, counts

    def __next__(self):
        items = self.next_items()
        self.last_counts = [i[5] for i in items]
        return tuple(torch.cat([i[k] for i in items]) for k in range(5))


def proposal_recall(model, dicts, iou=0.5, limits=(100, 1000)):
    """Recall of the detector's post-NMS proposals (its test-time selection, best score first) against the ground-truth boxes of
    ``dicts`` at the test size: the share of non-crowd ground truths that some proposal among the first ``limit`` overlaps with
    IoU >= ``iou``.  apse_box_match does the matching with the roles swapped: the ground truths are its "proposals", the proposals
    its "ground truths" (at most 4096 of them).  -> {limit: recall}, or None without any ground truth."""
    from PIL import Image
    from . import resample
    hits = {int(k): 0 for k in limits}
    total = 0
    for d in dicts:
        frame = np.asarray(Image.open(d["file_name"]).convert("RGB"))[:, :, ::-1].copy()
        H, W = frame.shape[:2]
        boxes = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]]
                          for a in d["annotations"] if not a.get("iscrowd", 0)], np.float64).reshape(-1, 4)
        if boxes.shape[0] == 0:
            continue
        ih, iw = resample.resize_shortest_edge(H, W, model.cfg.INPUT.MIN_SIZE_TEST, model.cfg.INPUT.MAX_SIZE_TEST)
        gt = torch.from_numpy((boxes * np.array([iw / W, ih / H, iw / W, ih / H])).astype(np.float32)).to(model.device).contiguous()
        props = model.rpn_proposals(frames=torch.from_numpy(frame[None]).to(model.device))[0]
        total += gt.shape[0]
        for k in hits:
            top = props[:min(k, 4096)].contiguous()
            if top.shape[0] == 0:
                continue
            zeros = torch.zeros(top.shape[0], dtype=torch.int32, device=model.device)
            _, best, _ = bh.box_match(gt, top, zeros, 1, iou)
            hits[k] += int((best >= iou).sum())
    if total == 0:
        return None
    return {k: v / total for k, v in hits.items()}
