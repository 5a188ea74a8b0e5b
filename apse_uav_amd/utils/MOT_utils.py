"""MOTloader / MOTSloader -- counterpart of dcnn/utils/MOT_utils.py:25-245: the association-head training data.

Same constructors, attributes and ``get_training_batch`` as the reference; ground truth is read by the plain host functions
below (no GPU), frames with PIL as BGR (what cv2.imread returns), masks with utils/rle.py and boxes with ``rle_to_bbox``,
a restatement of pycocotools' rleToBbox.  RoI features come from RoiFeaturesGenerator (the HIP backbone + roi_pool, or with
``MOTSloader(crop_features=True)`` the mask-cropped roi_align of the frame's RLE masks, turned into bit windows on the device).

    MOTS layout: <dataset>/instances_txt/<seq>.txt, <dataset>/training/image_02/<seq>/%06d.png, a seqmap file
    MOT layout:  <sequence>/seqinfo.ini, <sequence>/gt/gt.txt (rows with conf == 1), <sequence>/img1/%06d.jpg

``MOTSloader(cache_features=True)`` keeps each batch's (ids, rois) on the device once it has been computed, so epochs 2..N
skip the frozen backbone.  The results are the same (the backbone is deterministic).  The cost is the RoI tensor of every
object of the dataset: 256 x roi_size^2 x 4 bytes each, 100 KB at roi_size 10.
"""
import math
import os

import numpy as np
import torch
from PIL import Image

from ..config import is_c4
from ..engines.roi_features_generator import RoiFeaturesGenerator
from . import rle
from .mots_evaluation import parse_mots_seqmap

IGNORE_ID = 10000


def rle_to_bbox(counts, h, w):
    """pycocotools rleToBbox (maskApi.c) on uncompressed counts (column-major, first run = zeros) -> [xs, ys, w, h] floats.
    An odd trailing count is dropped; no runs left -> zeros; a run of ones that crosses a column boundary sets ys = 0,
    ye = h - 1.  Pixel positions use the C code's unsigned 32-bit arithmetic."""
    counts = [int(c) for c in counts]
    m = (len(counts) // 2) * 2
    if m == 0:
        return [0.0, 0.0, 0.0, 0.0]
    h, w = int(h), int(w)
    xs, ys, xe, ye = w, h, 0, 0
    cc = 0
    xp = 0
    for j in range(m):
        cc = (cc + counts[j]) & 0xFFFFFFFF
        t = (cc - (j % 2)) & 0xFFFFFFFF
        y = t % h
        x = (t - y) // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, h - 1
        xs, xe = min(xs, x), max(xe, x)
        ys, ye = min(ys, y), max(ye, y)
    return [float(xs), float(ys), float(xe - xs + 1), float(ye - ys + 1)]


def mask_to_bbox(mask):
    """pycocotools.mask.toBbox of one RLE dict {'size': [h, w], 'counts': str | bytes | list}."""
    h, w = mask["size"]
    counts = mask["counts"]
    if isinstance(counts, bytes):
        counts = counts.decode("ascii")
    if not isinstance(counts, (list, tuple)):
        counts = rle.string_to_counts(counts)
    return rle_to_bbox(counts, h, w)


def parse_mots_instances(path):
    """One instances_txt file (MOT_utils.py:167-200): rows [frame, id, x, y, w, h] (int64, boxes int() of toBbox) and the
    RLE dicts of the same objects.  Id 10000 (ignore regions) is dropped; every class is kept."""
    objects, masks = [], []
    with open(path, "r") as f:
        for line in f.readlines():
            info = line.split(" ")
            if len(info) < 6:
                continue
            frame_num, ob_id = int(info[0]), int(info[1])
            height, width = int(info[3]), int(info[4])
            mask = {"size": [height, width], "counts": info[5].strip()}
            bbox = [int(c) for c in mask_to_bbox(mask)]
            if ob_id != IGNORE_ID:
                masks.append(mask)
                objects.append([frame_num, ob_id, bbox[0], bbox[1], bbox[2], bbox[3]])
    arr = np.array(objects, dtype=np.int64) if objects else np.zeros((0, 6), np.int64)
    return arr, masks


def read_seqinfo(sequence_path):
    """seqinfo.ini as a dict of 'key=value' lines (MOT_utils.py:46-57)."""
    out = {}
    with open(os.path.join(sequence_path, "seqinfo.ini"), "r") as f:
        for line in f.readlines():
            el = line.split("=")
            if len(el) > 1:
                out[el[0]] = el[1].strip()
    return out


def parse_mot_gt(path):
    """gt/gt.txt (MOT_utils.py:60-71): the first 7 columns <frame>, <id>, <bb_left>, <bb_top>, <bb_width>, <bb_height>, <conf>
    as ints, rows with conf == 1 only."""
    with open(path, "r") as f:
        rows = [[int(el) for el in line.split(",")[:7]] for line in f.readlines() if line.strip()]
    arr = np.array(rows, dtype=np.int64) if rows else np.zeros((0, 7), np.int64)
    return arr[np.where(arr[:, 6] == 1)]


def frames_with_objects(objects):
    """Sorted distinct frame numbers of object rows (np.unique of column 0)."""
    return np.unique(np.asarray(objects)[:, 0]) if len(objects) else np.zeros((0,), np.int64)


def batch_frames(frames, frames_in_batch, batch_idx):
    """Frame numbers of batch ``batch_idx``: ``frames_in_batch`` consecutive entries of ``frames`` (MOT_utils.py:236-240)."""
    return [frames[k + batch_idx * frames_in_batch] for k in range(frames_in_batch)]


def read_frame_bgr(path):
    """u8 [H, W, 3] BGR, as cv2.imread returns it; None when the file does not exist (cv2.imread's failure value)."""
    if not os.path.exists(path):
        return None
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _idmap_rows(path):
    """One instances/<seq>/%06d.png id map (u16, value = class * 1000 + instance) -> [(id, RLE dict)] in ascending id order."""
    with Image.open(path) as im:
        idmap = np.asarray(im)
    if idmap.ndim != 2:
        raise ValueError("%s is not a single-channel id map" % path)
    return [(int(v), rle.encode((idmap == v).astype(np.uint8))) for v in np.unique(idmap) if v != 0]


def generate_mots_dataset_dictionaries(dataset_path, seqmap_path, class_names=("car", "pedestrian")):
    """KITTI MOTS / MOTSChallenge ground truth as detectron2-style dataset dictionaries in bitmask form (utils/COCO_utils.py
    ``generate_coco_dataset_dictionaries(mask_format="bitmask")``): one dictionary per frame that has objects, from
    <dataset>/instances_txt/<seq>.txt (``parse_mots_instances``) or, without it, the id maps <dataset>/instances/<seq>/%06d.png.
    MOTS class ids 1, 2 (id // 1000) become 0, 1 -- ``class_names`` in that order; ignore regions (class 10) and any other class
    are dropped.  ``bbox`` is ``rle_to_bbox`` of the mask (XYWH), ``segmentation`` the RLE dict, ``image_id`` counts the kept
    frames over all sequences.  A frame whose image (<dataset>/training/image_02/<seq>/%06d.png) is missing is refused."""
    names, _ = parse_mots_seqmap(seqmap_path)
    K = len(class_names)
    out = []
    for seq in names:
        txt = os.path.join(dataset_path, "instances_txt", seq + ".txt")
        per_frame = {}
        if os.path.exists(txt):
            rows, masks = parse_mots_instances(txt)
            for row, mask in zip(rows.tolist(), masks):
                per_frame.setdefault(int(row[0]), []).append((int(row[1]), mask))
        else:
            folder = os.path.join(dataset_path, "instances", seq)
            if not os.path.isdir(folder):
                raise FileNotFoundError("sequence %s: neither %s nor %s exists" % (seq, txt, folder))
            for fn in sorted(os.listdir(folder)):
                if fn.endswith(".png"):
                    per_frame[int(os.path.splitext(fn)[0])] = _idmap_rows(os.path.join(folder, fn))
        for frame in sorted(per_frame):
            anns = []
            size = None
            for ob_id, mask in per_frame[frame]:
                cls = ob_id // 1000
                if ob_id == IGNORE_ID or cls < 1 or cls > K:
                    continue
                h, w = (int(v) for v in mask["size"])
                if size is not None and size != (h, w):
                    raise ValueError("sequence %s frame %d: masks of sizes %s and %s" % (seq, frame, size, (h, w)))
                size = (h, w)
                bbox = mask_to_bbox(mask)
                if bbox[2] <= 0 or bbox[3] <= 0:
                    continue                                 # an all-zero mask: no object
                anns.append({"bbox": bbox, "bbox_mode": 1, "category_id": cls - 1, "segmentation": mask, "iscrowd": 0,
                             "track_id": ob_id})
            if not anns:
                continue
            image = os.path.join(dataset_path, "training", "image_02", seq, "%06d.png" % frame)
            if not os.path.exists(image):
                raise FileNotFoundError("sequence %s frame %d: the image %s is missing" % (seq, frame, image))
            b = np.array([a["bbox"] for a in anns], np.float32).reshape(-1, 4)
            out.append({"file_name": image, "image_id": len(out), "height": size[0], "width": size[1], "annotations": anns,
                        "sequence": seq, "frame": frame,
                        "proposal_boxes": np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1),
                        "proposal_objectness_logits": np.ones(len(anns), np.float32), "proposal_bbox_mode": 0})
    return out


class MOTloader:
    """Training data of the association head from one MOT sequence (MOT_utils.py:25-130)."""

    def __init__(self, config, sequence_path, frames_in_batch=8, roi_size=8):
        self.config = config
        self.frames_in_batch = frames_in_batch
        self.sequence_path = sequence_path
        self.sequence_info = self.read_seqinfo()
        self.frames_in_sequence = int(self.sequence_info['seqLength'])
        self.num_of_batches = math.floor(self.frames_in_sequence / self.frames_in_batch)
        self.roi_generator = RoiFeaturesGenerator(config=self.config, roi_size=roi_size)
        # <frame>, <id>, <bb_left>, <bb_top>, <bb_width>, <bb_height>, <conf> of the whole sequence
        self.sequence_objects = self.gt_instances_from_sequence()

    def read_seqinfo(self):
        return read_seqinfo(self.sequence_path)

    def gt_instances_from_sequence(self):
        return parse_mot_gt(os.path.join(self.sequence_path, "gt", "gt.txt"))

    def objects_from_frame(self, frame_number):
        return self.sequence_objects[np.where(self.sequence_objects[:, 0] == frame_number)]

    def frame_from_sequence(self, frame_number):
        return read_frame_bgr(os.path.join(self.sequence_path, "img1", "{:06d}.jpg".format(frame_number)))

    def rois_ids_from_frame(self, frame_number):
        frame = self.frame_from_sequence(frame_number)
        return self.roi_generator.get_rois_features(frame, self.objects_from_frame(frame_number))

    def get_training_batch(self, batch_idx):
        """(ids [N], rois [N, C, roi_size, roi_size]) of frames batch_idx * frames_in_batch + 1 .. + frames_in_batch."""
        assert batch_idx < self.num_of_batches
        batch_ids, batch_rois = [], []
        for k in range(self.frames_in_batch):
            ids, rois = self.rois_ids_from_frame((k + 1) + batch_idx * self.frames_in_batch)
            batch_ids.append(ids)
            batch_rois.append(rois)
        return torch.cat(batch_ids), torch.cat(batch_rois)


class MOTSloader:
    """Training data of the association head from KITTI MOTS-layout sequences (MOT_utils.py:134-245)."""

    def __init__(self, config, dataset_path, seqmap_path, frames_in_batch=8, roi_size=8, cache_features=False, crop_features=False):
        if crop_features and is_c4(config):
            raise NotImplementedError("crop_features cuts the RoI features from the FPN level p2: not available for C4 "
                                      "(Res5ROIHeads) models")
        self.crop_features = bool(crop_features)
        self.config = config
        self.frames_in_batch = frames_in_batch
        self.dataset_path = dataset_path
        self.seqmap_names, self.seqmap_lengths = parse_mots_seqmap(seqmap_path)
        self.num_of_sequences = len(self.seqmap_names)
        self.roi_generator = RoiFeaturesGenerator(config=self.config, roi_size=roi_size)
        # seqname -> ([frame, id, x, y, w, h] rows, RLE dicts)
        self.sequence_objects = self.gt_instances_from_sequence()
        self.frames_with_objects_per_seq = self.find_frames_with_objects()
        self.batches_per_sequence = [math.floor(len(self.frames_with_objects_per_seq[seq]) / self.frames_in_batch)
                                     for seq in self.seqmap_names]
        self.num_of_batches = np.array(self.batches_per_sequence).sum()
        self.cache_features = cache_features
        self._cache = {}

    def find_frames_with_objects(self):
        return {seq: frames_with_objects(self.sequence_objects[seq][0]) for seq in self.seqmap_names}

    def gt_instances_from_sequence(self):
        return {seq: parse_mots_instances(os.path.join(self.dataset_path, "instances_txt", seq + ".txt"))
                for seq in self.seqmap_names}

    def objects_masks_from_frame(self, sequence_name, frame_number):
        objects, masks = self.sequence_objects[sequence_name]
        idx = np.where(objects[:, 0] == frame_number)
        return objects[idx], [masks[i] for i in idx[0].tolist()]

    def frame_from_sequence(self, sequence_name, frame_number):
        return read_frame_bgr(os.path.join(self.dataset_path, "training", "image_02", sequence_name,
                                           "{:06d}.png".format(frame_number)))

    def rois_ids_from_frame(self, sequence_name, frame_number):
        frame = self.frame_from_sequence(sequence_name, frame_number)
        frame_objects, frame_masks = self.objects_masks_from_frame(sequence_name, frame_number)
        return self.roi_generator.get_rois_features(frame, frame_objects, frame_masks if self.crop_features else None)

    def get_training_batch(self, sequence_idx, batch_idx):
        """(ids [N], rois [N, C, roi_size, roi_size]) of ``frames_in_batch`` consecutive frames with objects."""
        assert batch_idx < self.batches_per_sequence[sequence_idx]
        assert sequence_idx < self.num_of_sequences
        key = (sequence_idx, batch_idx)
        if key in self._cache:
            return self._cache[key]
        seqname = self.seqmap_names[sequence_idx]
        batch_ids, batch_rois = [], []
        for frame_number in batch_frames(self.frames_with_objects_per_seq[seqname], self.frames_in_batch, batch_idx):
            ids, rois = self.rois_ids_from_frame(seqname, frame_number)
            batch_ids.append(ids)
            batch_rois.append(rois)
        out = (torch.cat(batch_ids), torch.cat(batch_rois))
        if self.cache_features:
            self._cache[key] = out
        return out
