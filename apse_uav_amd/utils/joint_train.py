"""The data side of joint RPN / box-head training (tools/finetune_uav.py): one backbone run per image feeds both heads, and the
box head's proposals come from the RPN head as it is at that step (``TrackRCNN.set_rpn_head`` follows every optimiser step), at
detectron2's training limits (``TrackRCNN.train_proposals``).  With ``mask=True`` the sampled foreground proposals also become
mask-head rows, their targets made on the device (``apse_coco_mask_targets``).
"""
import numpy as np
import torch

from ..networks import box_head as bh
from ..networks import mask_head as mh
from ..networks import rpn_head as rh
from .box_train import SamplingLoader, label_and_sample_proposals
from .COCO_utils import DevicePolygons, bitmask_targets_device, mask_targets_device, select_mask_rows
from .rpn_train import label_and_sample_anchors


def box_chunks(rows_per_image, max_rows=bh.MAX_ROIS):
    """Splits a batch's box rows into chunks of whole images with at most ``max_rows`` rows each (APSE_BOX_TRAIN_MAX_N), in
    image order.  -> [(first row, one past the last row)]."""
    chunks, start, end = [], 0, 0
    for n in rows_per_image:
        n = int(n)
        if n > max_rows:
            raise ValueError("an image has %d box rows, a step takes at most %d (APSE_BOX_TRAIN_MAX_N)" % (n, max_rows))
        if end - start + n > max_rows:
            chunks.append((start, end))
            start = end
        end += n
    if end > start:
        chunks.append((start, end))
    return chunks


def box_losses_chunked(head, feats, labels, prop_boxes, gt_boxes, rows_per_image):
    """``head(feats, labels, prop_boxes, gt_boxes)`` for more rows than one step takes: every chunk of ``box_chunks`` goes through
    the head on its own and its two losses are weighted by n_chunk / n_total.  loss_cls is a mean over rows and loss_box_reg a sum
    divided by the row count, so the weighted sum is the loss over all rows; summed in chunk order, its backward accumulates the
    gradients in chunk order.  One chunk: the head's own result, untouched."""
    chunks = box_chunks(rows_per_image)
    total = int(feats.shape[0])
    if len(chunks) <= 1:
        return head(feats, labels, prop_boxes, gt_boxes)
    out = None
    for (a, b) in chunks:
        part = head(feats[a:b], labels[a:b], prop_boxes[a:b], gt_boxes[a:b])
        w = float(b - a) / float(total)
        part = {k: v * w for k, v in part.items()}
        out = part if out is None else {k: out[k] + part[k] for k in out}
    return out


def check_mask_rows(ims_per_batch, box_batch_size_per_image, box_positive_fraction, max_rows=mh.MAX_ROIS):
    """The most mask rows a batch can have -- every image's foreground quota, floor(batch size x positive fraction) -- against the
    rows ``MaskHead`` takes in one step; raises ValueError past them.  -> that bound."""
    bound = int(ims_per_batch) * int(int(box_batch_size_per_image) * float(box_positive_fraction))
    if bound > max_rows:
        raise ValueError("%d images x %d foreground RoIs exceed the %d mask rows of one step (APSE_MASK_TRAIN_MAX_N)"
                         % (int(ims_per_batch), int(int(box_batch_size_per_image) * float(box_positive_fraction)), max_rows))
    return bound


class JointTrainLoader(SamplingLoader):
    """Yields (rpn, box) per batch of ``ims_per_batch`` images, endlessly, in a seeded shuffled order:

    * rpn = (patches f32 [n][2304], slots int32 [n], labels int32 [n], anchor_boxes f32 [n][4], gt_boxes f32 [n][4]), the tuple
      of RpnTrainLoader;
    * box = (roi_features [m][7][7][256], labels int32 [m], proposal_boxes f32 [m][4], gt_boxes f32 [m][4]), the tuple of
      BoxTrainLoader; ``last_box_rows`` holds m per image (m may exceed one step's rows: ``box_losses_chunked``).

    With ``mask=True`` it yields (rpn, box, mask): mask = (roi_features f32 [f][14][14][256], classes int64 [f] on the host, targets
    uint8 [f][28][28]), the tuple of MaskTrainLoader, for the sampled box rows that are foreground (label < K, in sampling order:
    detectron2's ``select_foreground_proposals``) and whose matched ground truth has at least one polygon part.  The features are
    ``mask_roi_features`` of those PROPOSAL boxes and the targets ``apse_coco_mask_targets`` of the matched polygons cropped to them
    (``mask_rcnn_loss``), against the image's polygons uploaded once.  An image or annotation without polygons gives RPN and box
    rows only.  ``last_mask_rows`` holds f per image and ``last_mask_skipped`` the foreground rows dropped for lack of polygons.
    The mask rows draw no random numbers: rpn and box are the same bits with ``mask`` on and off, and so is ``state_dict``.
    ``mask_format="bitmask"``: the annotations may hold RLE segmentations; the image's ``DeviceBitmasks`` is built once, remapped
    with the image's nearest-neighbour maps, and the targets are ``apse_bitmask_targets`` (``BitMasks.crop_and_resize``) of the
    matched ground truth under the proposals; "has a polygon part" reads "has a segmentation".

    ``model``: a TrackRCNN (FPN, f32).  Per image: the image and annotation path of MaskTrainLoader, the frozen backbone once,
    then ``label_and_sample_anchors`` and ``rpn_patches`` for the RPN rows, then ``train_proposals`` on the context's current RPN
    head (cfg.MODEL.RPN.PRE / POST_NMS_TOPK_TRAIN), ``label_and_sample_proposals`` with the ground truths appended and
    ``box_roi_features`` for the box rows.  Two device generators, both seeded from ``seed``, drawn in
    that order (anchors, then proposals) for every image; ``state_dict`` carries both."""

    def __init__(self, dicts, model, ims_per_batch=2, seed=0, flip=False, augment=False, min_sizes=None, max_size=None,
                 sampling="choice", num_classes=None, rpn_batch_size_per_image=256, rpn_positive_fraction=0.5,
                 rpn_iou_thresholds=(0.3, 0.7), box_batch_size_per_image=512, box_positive_fraction=0.25, box_iou_thresh=0.5,
                 mask=False, mask_format="polygon"):
        if getattr(model, "c4", False):
            raise NotImplementedError("joint detection-head training covers FPN models (p2 .. p6)")
        self.mask = bool(mask)
        if self.mask:
            check_mask_rows(ims_per_batch, box_batch_size_per_image, box_positive_fraction)
        super().__init__(dicts, model, ims_per_batch, seed, flip, False, bh.MAX_ROIS, augment, min_sizes, max_size, sampling,
                         mask_format)
        self.num_classes = int(num_classes if num_classes is not None else model.cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        self.rpn_batch_size_per_image, self.rpn_positive_fraction = int(rpn_batch_size_per_image), float(rpn_positive_fraction)
        self.rpn_iou_thresholds = (float(rpn_iou_thresholds[0]), float(rpn_iou_thresholds[1]))
        self.box_batch_size_per_image, self.box_positive_fraction = int(box_batch_size_per_image), float(box_positive_fraction)
        self.box_iou_thresh = float(box_iou_thresh)
        if self.ims_per_batch * self.rpn_batch_size_per_image > rh.MAX_ROWS:
            raise ValueError("%d images x %d anchors exceed the %d RPN rows of one step (APSE_BOX_TRAIN_MAX_N)"
                             % (self.ims_per_batch, self.rpn_batch_size_per_image, rh.MAX_ROWS))
        if self.box_batch_size_per_image > bh.MAX_ROIS:
            raise ValueError("%d RoIs per image exceed the %d of one chunk (APSE_BOX_TRAIN_MAX_N)" % (self.box_batch_size_per_image, bh.MAX_ROIS))
        self.seed_generators(rpn_generator=seed, box_generator=int(seed) + 1)
        self.last_rpn_counts = []             # (num_pos, num_neg) per image of the last batch
        self.last_box_counts = []             # (num_fg, num_bg) per image of the last batch
        self.last_box_rows = []               # box rows per image of the last batch
        self.last_proposals = []              # the training proposals (boxes [count][4]) per image of the last batch
        self.last_mask_rows = []              # mask=True: mask rows per image of the last batch
        self.last_mask_skipped = []           # mask=True: foreground rows without polygons per image of the last batch

    def _sample(self, boxes, polys, classes, d):
        model = self.model
        gt, cls = self.ground_truth(boxes, classes, d)
        sel, rlabels, rmatched, rcounts = label_and_sample_anchors(model, gt, self.rpn_batch_size_per_image, self.rpn_positive_fraction,
                                                                   self.rpn_generator, self.rpn_iou_thresholds)
        patches, slots, anchor_boxes, _ = model.rpn_patches(sel)
        props = model.train_proposals(1)[0][0]
        sampled = label_and_sample_proposals(props, gt, cls, self.num_classes, self.box_batch_size_per_image, self.box_positive_fraction,
                                             self.box_generator, self.box_iou_thresh, return_index=self.mask)
        sb, blabels, bmatched, bcounts = sampled[:4]
        rpn = (patches, slots, rlabels, anchor_boxes, rmatched)
        box = (model.box_roi_features(sb), blabels, sb, bmatched)
        if not self.mask:
            return rpn, box, rcounts, bcounts, props
        return rpn, box, rcounts, bcounts, props, self._mask_rows(sb, blabels, sampled[4], polys, d)

    def _mask_rows(self, boxes, labels, matched, polys, d):
        """The mask item of one image from its sampled box rows: ((features, classes, targets), rows skipped).  ``matched`` indexes
        the ground truths ``ground_truth`` kept (the non-crowd annotations), so the polygons are filtered the same way."""
        model = self.model
        keep = [i for i, a in enumerate(d["annotations"]) if not a.get("iscrowd", 0)]
        labels_host = labels.cpu().numpy()
        if self.mask_format == "bitmask":                    # polys: the image's BitmaskSource; has_mask in place of parts > 0
            gt_dev = polys.select(keep).device_bitmasks(model.device)
            has, targets_of = gt_dev.has_mask, bitmask_targets_device
        else:
            gt_dev = DevicePolygons([polys[i] for i in keep], model.device)
            has, targets_of = gt_dev.parts, mask_targets_device
        rows, skipped = select_mask_rows(labels_host, matched.cpu().numpy(), has, self.num_classes)
        rows_dev = torch.from_numpy(rows).to(model.device)
        mboxes = boxes[rows_dev].contiguous()
        targets = targets_of(gt_dev, mboxes, matched[rows_dev])
        classes = torch.from_numpy(labels_host[rows].astype(np.int64))
        return (model.mask_roi_features(mboxes), classes, targets), skipped

    def __next__(self):
        items = self.next_items()
        self.last_rpn_counts = [i[2] for i in items]
        self.last_box_counts = [i[3] for i in items]
        self.last_box_rows = [int(i[1][1].shape[0]) for i in items]
        self.last_proposals = [i[4] for i in items]
        rpn = tuple(torch.cat([i[0][k] for i in items]) for k in range(5))
        box = tuple(torch.cat([i[1][k] for i in items]) for k in range(4))
        if not self.mask:
            return rpn, box
        self.last_mask_rows = [int(i[5][0][1].shape[0]) for i in items]
        self.last_mask_skipped = [i[5][1] for i in items]
        return rpn, box, tuple(torch.cat([i[5][0][k] for i in items]) for k in range(3))
