"""The data side of box-head training: detectron2's ``ROIHeads.label_and_sample_proposals`` on the device and the loader that turns
dataset dictionaries into sampled RoI features (networks/box_head.py consumes them, tools/finetune_box_head.py is the loop).
"""
import numpy as np
import torch

from ..networks import box_head as bh
from .COCO_utils import MaskTrainLoader


def subsample_labels(labels, num_samples, positive_fraction, bg_label, generator=None):
    """detectron2.modeling.sampling.subsample_labels: at most ``int(num_samples * positive_fraction)`` foreground rows
    (label != -1, != bg_label) and background rows up to ``num_samples``, each a ``torch.randperm`` draw from ``generator`` on the
    generator's device (default: the labels').  -> (positive indices, negative indices), on the labels' device."""
    positive = torch.nonzero((labels != -1) & (labels != bg_label)).squeeze(1)
    negative = torch.nonzero(labels == bg_label).squeeze(1)
    num_pos = min(positive.numel(), int(num_samples * positive_fraction))
    num_neg = min(negative.numel(), num_samples - num_pos)
    dev = generator.device if generator is not None else labels.device
    perm1 = torch.randperm(positive.numel(), generator=generator, device=dev)[:num_pos].to(labels.device)
    perm2 = torch.randperm(negative.numel(), generator=generator, device=dev)[:num_neg].to(labels.device)
    return positive[perm1], negative[perm2]


def label_and_sample_proposals(proposals, gt_boxes, gt_classes, num_classes, batch_size_per_image=512, positive_fraction=0.25,
                               generator=None, iou_thresh=0.5, return_index=False):
    """ROIHeads.label_and_sample_proposals for one image, on the device.  proposals f32 [P][4], gt_boxes f32 [G][4], gt_classes
    [G], all in resized-image pixels.  The ground-truth boxes are appended after the proposals (PROPOSAL_APPEND_GT),
    apse_box_match labels the candidates, subsample_labels draws the rows, foreground first.
    -> (boxes f32 [n][4], labels int32 [n] (num_classes = background), matched ground-truth boxes f32 [n][4] (zeros without a
    ground truth), (num_fg, num_bg)); with ``return_index`` also the matched ground-truth index of every row, int32 [n] (-1
    without a ground truth), as the last entry."""
    dev = proposals.device
    if not proposals.is_cuda:
        raise bh._lib.ApseError("label_and_sample_proposals needs GPU tensors (no CPU fallback)")
    gt = torch.as_tensor(gt_boxes, dtype=torch.float32).reshape(-1, 4).to(dev).contiguous()
    cls = torch.as_tensor(gt_classes).reshape(-1).to(dev, torch.int32).contiguous()
    cand = torch.cat([proposals.to(torch.float32).reshape(-1, 4), gt]).contiguous()
    idx, _, labels = bh.box_match(cand, gt, cls, num_classes, iou_thresh)
    pos, neg = subsample_labels(labels, batch_size_per_image, positive_fraction, num_classes, generator)
    sel = torch.cat([pos, neg])
    matched = gt[idx[sel].long()] if gt.shape[0] else torch.zeros((sel.numel(), 4), dtype=torch.float32, device=dev)
    out = (cand[sel], labels[sel], matched, (int(pos.numel()), int(neg.numel())))
    if return_index:
        out += (idx[sel] if gt.shape[0] else torch.full((sel.numel(),), -1, dtype=torch.int32, device=dev),)
    return out


class SamplingLoader(MaskTrainLoader):
    """What the loaders that sample rows on the device share on top of MaskTrainLoader: the ground truth of an image on the
    device and named device generators whose states travel in ``state_dict``.  A subclass calls ``seed_generators`` once and
    overrides ``_sample``."""

    def seed_generators(self, **seeds):
        """One ``torch.Generator`` on the model's device per name, seeded, as an attribute of that name; ``state_dict`` carries
        their states under the same names, in this order."""
        self._generators = {}
        for name, seed in seeds.items():
            g = torch.Generator(device=self.model.device)
            g.manual_seed(int(seed))
            self._generators[name] = g
            setattr(self, name, g)

    def state_dict(self):
        sd = super().state_dict()
        for name, g in self._generators.items():
            sd[name] = g.get_state().clone()
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        for name, g in self._generators.items():
            g.set_state(sd[name].cpu())

    def ground_truth(self, boxes, classes, d):
        """The image's non-crowd annotations on the device: (boxes f32 [G][4], classes int32 [G])."""
        dev = self.model.device
        keep = [i for i, a in enumerate(d["annotations"]) if not a.get("iscrowd", 0)]
        gt = torch.from_numpy(np.asarray(boxes, np.float64)[keep].astype(np.float32)).reshape(-1, 4).to(dev)
        return gt, torch.as_tensor(classes)[keep].to(dev, torch.int32)


class BoxTrainLoader(SamplingLoader):
    """Yields (roi_features [n][7][7][256], labels int32 [n], proposal_boxes f32 [n][4], gt_boxes f32 [n][4]) per batch of
    ``ims_per_batch`` images, endlessly, in a seeded shuffled order.  ``model``: a TrackRCNN (FPN) with the frozen detector's
    weights.  Per image: the image and annotation path of MaskTrainLoader (test size on the host, or the device path with
    ``augment`` / ``min_sizes``), the context's own RPN (its test-time selection), ``label_and_sample_proposals`` with a device
    generator seeded from ``seed``, then ROIAlign 7 of the sampled boxes.  Crowd annotations are dropped.  ``state_dict`` also
    carries the sampling generator's state.  ``train_topk`` = (pre, post): the proposals are ``model.train_proposals(1, pre, post)``,
    detectron2's training-time selection (2000 per level, 1000), instead of the test-time one."""

    def __init__(self, dicts, model, ims_per_batch=2, seed=0, flip=False, augment=False, min_sizes=None, max_size=None,
                 sampling="choice", num_classes=None, batch_size_per_image=512, positive_fraction=0.25, iou_thresh=0.5,
                 train_topk=None):
        if getattr(model, "c4", False):
            raise NotImplementedError("box-head training covers FPN models; under C4 (Res5ROIHeads) the box branch is the res5 stage")
        super().__init__(dicts, model, ims_per_batch, seed, flip, False, bh.MAX_ROIS, augment, min_sizes, max_size, sampling)
        self.num_classes = int(num_classes if num_classes is not None else model.cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        self.batch_size_per_image = int(batch_size_per_image)
        self.positive_fraction = float(positive_fraction)
        self.iou_thresh = float(iou_thresh)
        self.train_topk = None if train_topk is None else (int(train_topk[0]), int(train_topk[1]))
        if self.ims_per_batch * self.batch_size_per_image > bh.MAX_ROIS:
            raise ValueError("%d images x %d RoIs exceed the %d RoIs of one step (APSE_BOX_TRAIN_MAX_N)"
                             % (self.ims_per_batch, self.batch_size_per_image, bh.MAX_ROIS))
        self.seed_generators(generator=seed)
        self.last_counts = []                 # (num_fg, num_bg) per image of the last batch

    def _sample(self, boxes, polys, classes, d):
        model = self.model
        gt, cls = self.ground_truth(boxes, classes, d)
        props = model.train_proposals(1, *self.train_topk)[0][0] if self.train_topk else model.proposals_after_backbone(1)[0]
        sb, labels, matched, counts = label_and_sample_proposals(props, gt, cls, self.num_classes, self.batch_size_per_image,
                                                                 self.positive_fraction, self.generator, self.iou_thresh)
        return model.box_roi_features(sb), labels, sb, matched, counts

    def __next__(self):
        items = self.next_items()
        self.last_counts = [i[4] for i in items]
        return tuple(torch.cat([i[k] for i in items]) for k in range(4))
