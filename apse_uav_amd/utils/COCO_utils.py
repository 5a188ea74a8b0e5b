"""Dataset side of mask-head fine-tuning -- counterpart of dcnn/utils/COCO_utils.py and of the detectron2 pieces
dcnn/scripts/train/finetune_segmentation.py leans on (dataset dictionaries, ``PolygonMasks.crop_and_resize``, the train loader).

* ``generate_coco_dataset_dictionaries``: COCO json -> detectron2-style dataset dictionaries with the reference's filtering
  (non-crowd annotations of the allowed class names, category ids mapped), ground-truth boxes as precomputed proposals.
  The reference's line ``annotation_dict['segmentation'] = ann['segmentation'],`` wraps the polygon list in a 1-tuple by accident;
  here the list itself is stored.  RLE (dict) segmentations are refused: the reference drops crowds, and non-crowd COCO
  annotations are polygons -- unless ``mask_format="bitmask"``, which keeps them.
* ``DeviceBitmasks`` / ``nearest_maps`` / ``bitmask_targets_device`` / ``bitmask_targets``: detectron2's INPUT.MASK_FORMAT =
  "bitmask" -- RLE, dense and ``WindowMask`` ground truth as bit windows on the device, resized / flipped with Pillow's
  nearest-neighbour map (``apse_mots_remap_windows``), targets by ``BitMasks.crop_and_resize`` (``apse_bitmask_targets``).  The
  loaders take ``mask_format="bitmask"``; DESIGN.md "Bitmask ground truth".
* ``detectron2_dataset_to_coco``: the dictionaries back to a COCO dataset (for ``utils.coco.COCO.from_dataset`` / ``COCOeval``).
* ``mask_targets``: ``PolygonMasks.crop_and_resize`` (``rasterize_polygons_within_box``) at 28 x 28: the polygon transform on the
  host in float64, the rasterisation by ``apse_coco_poly_to_bits`` (equal to pycocotools ``frPyObjects`` + ``merge``).
* ``DevicePolygons`` / ``mask_targets_device``: the same targets for boxes that are new every step (the joint loop's sampled
  proposals), in one launch of ``apse_coco_mask_targets`` against an image's polygons uploaded once; ``select_mask_rows`` picks the rows.
* ``MaskTrainLoader``: batches of ``IMS_PER_BATCH`` images -> RoI features of the ground-truth boxes from the frozen backbone
  (test-size resize with an optional seeded horizontal flip; or, with ``augment`` / ``min_sizes``, the reference mapper's
  multi-scale resize, flip and colour chain on the GPU: utils/augment.py), classes and 28 x 28 targets.  Ground truths appear once: detectron2 appends
  the ground truth to proposals that already are the ground truth, and an exact duplicate of every RoI leaves a mean loss and its
  gradient unchanged.
"""
import json
import os

import numpy as np
import torch

from . import coco as cocomod
from . import resample

MASK_SIZE = 28
XYWH_ABS = 1          # detectron2 BoxMode.XYWH_ABS
MASK_FORMATS = ("polygon", "bitmask")


def generate_coco_dataset_dictionaries(json_file, imgfolder, allowed_classes=None, category_mapping=None,
                                       precomputed_proposals=True, keep_box_only=False, mask_format="polygon"):
    """-> list of {file_name, image_id, height, width, annotations: [{bbox (XYWH), bbox_mode, category_id, segmentation, iscrowd}],
    proposal_boxes (XYXY f32 [k, 4]), proposal_objectness_logits, proposal_bbox_mode}.  ``allowed_classes``: category NAMES to
    keep (None: all); ``category_mapping``: {json category id: training class index} (None: the sorted kept ids -> 0..K-1).
    Images left without annotations are dropped, as the reference does.  An annotation without a segmentation is dropped too,
    unless ``keep_box_only`` (the joint loop with the mask head, where box-only data feeds the RPN and box losses): it is then
    kept with ``segmentation`` [].  ``mask_format`` "polygon" refuses an RLE (dict) segmentation; "bitmask" (detectron2's
    INPUT.MASK_FORMAT) keeps it as it is, beside polygon lists, for ``DeviceBitmasks``."""
    if mask_format not in MASK_FORMATS:
        raise ValueError("mask_format must be one of %s, got %r" % (MASK_FORMATS, mask_format))
    with open(json_file) as fh:
        data = json.load(fh)
    names = {c["id"]: c["name"] for c in data["categories"]}
    keep_ids = sorted(i for i, nm in names.items() if allowed_classes is None or nm in allowed_classes)
    if category_mapping is None:
        category_mapping = {cid: k for k, cid in enumerate(keep_ids)}
    by_img = {}
    for ann in data["annotations"]:
        by_img.setdefault(ann["image_id"], []).append(ann)
    out = []
    for img in data["images"]:
        anns = []
        for ann in by_img.get(img["id"], []):
            if ann.get("iscrowd", 0) or ann["category_id"] not in keep_ids or ann["category_id"] not in category_mapping:
                continue
            seg = ann.get("segmentation")
            if isinstance(seg, dict) and mask_format == "bitmask":
                if "counts" not in seg or "size" not in seg:
                    raise ValueError("annotation %s: an RLE segmentation needs 'counts' and 'size'" % ann.get("id"))
            elif isinstance(seg, dict):
                raise ValueError("annotation %s: RLE segmentations are not supported for mask-head training (non-crowd COCO "
                                 "annotations are polygons)" % ann.get("id"))
            if not seg:
                if not keep_box_only:
                    continue
                seg = []
            anns.append({"bbox": [float(v) for v in ann["bbox"]], "bbox_mode": XYWH_ABS,
                         "category_id": int(category_mapping[ann["category_id"]]),
                         # the list itself (not the reference's 1-tuple); an RLE dict as it is
                         "segmentation": seg if isinstance(seg, dict) else [list(map(float, p)) for p in seg],
                         "iscrowd": 0})
        if not anns:
            continue
        d = {"file_name": os.path.join(imgfolder, img["file_name"]), "image_id": img["id"], "height": int(img["height"]),
             "width": int(img["width"]), "annotations": anns}
        if precomputed_proposals:
            b = np.array([a["bbox"] for a in anns], np.float32).reshape(-1, 4)
            d["proposal_boxes"] = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1)
            d["proposal_objectness_logits"] = np.ones(len(anns), np.float32)
            d["proposal_bbox_mode"] = 0                                              # XYXY_ABS
        out.append(d)
    return out


def detectron2_dataset_to_coco(dicts, class_names=None):
    """Dataset dictionaries -> COCO dataset dict (category ids = training class indices)."""
    images, anns, cats = [], [], set()
    for d in dicts:
        images.append({"id": d["image_id"], "file_name": os.path.basename(d["file_name"]), "height": d["height"], "width": d["width"]})
        for a in d["annotations"]:
            x, y, w, h = a["bbox"]
            area = float(w * h)
            anns.append({"id": len(anns) + 1, "image_id": d["image_id"], "category_id": a["category_id"], "bbox": [x, y, w, h],
                         "area": area, "iscrowd": a.get("iscrowd", 0), "segmentation": a["segmentation"]})
            cats.add(a["category_id"])
    K = (max(cats) + 1) if cats else 0
    if class_names is not None:
        K = max(K, len(class_names))
    categories = [{"id": k, "name": class_names[k] if class_names is not None and k < len(class_names) else "class%d" % k}
                  for k in range(K)]
    return {"images": images, "annotations": anns, "categories": categories}


def crop_and_resize_polygons(polygons, box, mask_size=MASK_SIZE):
    """detectron2 ``rasterize_polygons_within_box`` up to the rasterisation: polygons (flat x, y lists) shifted by the box origin
    and scaled by mask_size / max(extent, 0.1), in float64; one multiply of the whole array when the two ratios are equal."""
    x0, y0, x1, y1 = (float(v) for v in box)
    w, h = x1 - x0, y1 - y0
    out = []
    for p in polygons:
        q = np.array(p, np.float64)
        q = q[:2 * (len(q) // 2)].copy()
        q[0::2] = q[0::2] - x0
        q[1::2] = q[1::2] - y0
        out.append(q)
    rh, rw = mask_size / max(h, 0.1), mask_size / max(w, 0.1)
    if rh == rw:
        for q in out:
            q *= rh
    else:
        for q in out:
            q[0::2] *= rw
            q[1::2] *= rh
    return out


def mask_targets(polygons_per_roi, boxes, device, mask_size=MASK_SIZE):
    """``PolygonMasks.crop_and_resize(boxes, mask_size)``: uint8 [n][mask_size][mask_size] on the device (1 = inside)."""
    n = len(polygons_per_roi)
    if n == 0:
        return torch.zeros((0, mask_size, mask_size), dtype=torch.uint8, device=device)
    objs = []
    for polys, box in zip(polygons_per_roi, np.asarray(boxes, np.float64).reshape(-1, 4)):
        parts = [q.reshape(-1, 2) for q in crop_and_resize_polygons(polys, box, mask_size)]
        objs.append((parts, mask_size, mask_size))
    windows, keep = cocomod.polygons_to_windows(objs, device)
    dense = cocomod.windows_to_dense(windows, mask_size, mask_size)
    del keep
    return torch.from_numpy(dense.astype(np.uint8)).to(device)


class DevicePolygons:
    """The polygons of one image on the device, as ``apse_coco_mask_targets`` reads them: xy f64 [n_verts][2], part_vert_off int32
    [n_parts + 1], obj_part_off int32 [n_obj + 1] (the arrays of ``coco.poly_layout`` without the edge shares, rects and windows).
    ``polygons_per_object``: per object a list of flat x, y lists in resized-image pixels; every part is cut to whole pairs, as
    ``crop_and_resize_polygons`` cuts it.  ``parts`` (host int64 [n_obj]) counts each object's parts."""

    def __init__(self, polygons_per_object, device):
        parts = [np.asarray(p, np.float64).reshape(-1)[:2 * (len(p) // 2)] for ps in polygons_per_object for p in ps]
        self.parts = np.array([len(ps) for ps in polygons_per_object], np.int64)
        part_vert_off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) // 2 for p in parts], out=part_vert_off[1:])
        obj_part_off = np.zeros(len(self.parts) + 1, np.int64)
        np.cumsum(self.parts, out=obj_part_off[1:])
        xy = np.concatenate(parts) if parts else np.zeros(0, np.float64)
        self.n_obj, self.n_parts, self.n_verts = len(self.parts), len(parts), int(part_vert_off[-1])
        self.device = torch.device(device)
        self.xy = torch.from_numpy(np.ascontiguousarray(xy, np.float64)).to(self.device)
        self.part_vert_off = torch.from_numpy(part_vert_off.astype(np.int32)).to(self.device)
        self.obj_part_off = torch.from_numpy(obj_part_off.astype(np.int32)).to(self.device)


def mask_targets_device(polygons, rois, matched, mask_size=MASK_SIZE, out=None):
    """``mask_targets`` for proposals that are new every step (``apse_coco_mask_targets``): ``polygons`` a DevicePolygons of the image,
    ``rois`` f32 [n][4] and ``matched`` int32 [n] (each row's object) on the device -> uint8 [n][mask_size][mask_size] on the device,
    byte for byte ``mask_targets([polygons of matched[r]], rois)``.  One launch; the only host step is the read of the info word
    afterwards, which raises the host path's ValueError for coordinates outside the rasteriser's range.  ``out``: a uint8 buffer
    of at least n rows to write into (rows past n stay untouched); the result is its first n rows."""
    from .. import _lib
    from ..networks.head_base import _check
    dev = polygons.device
    rois = torch.as_tensor(rois, dtype=torch.float32).reshape(-1, 4).to(dev).contiguous()
    matched = torch.as_tensor(matched).reshape(-1).to(dev, torch.int32).contiguous()
    n = int(rois.shape[0])
    if int(matched.shape[0]) != n:
        raise ValueError("mask_targets_device: %d boxes, %d matched indices" % (n, int(matched.shape[0])))
    if out is None:
        out = torch.empty((n, mask_size, mask_size), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() != 3 or out.shape[0] < n or \
            tuple(out.shape[1:]) != (mask_size, mask_size) or out.device != rois.device:
        raise ValueError("mask_targets_device: out must be a contiguous uint8 [>= n][%d][%d] tensor on the device" % (mask_size, mask_size))
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(_lib.load().apse_coco_mask_targets(_lib.ptr(polygons.xy), _lib.ptr(polygons.part_vert_off), polygons.n_parts,
                                         _lib.ptr(polygons.obj_part_off), polygons.n_obj, polygons.n_verts, _lib.ptr(rois),
                                         _lib.ptr(matched), n, int(mask_size), _lib.ptr(out), _lib.ptr(info), _lib.stream_ptr()),
           "apse_coco_mask_targets")
    if n and int(info.cpu()[0]):
        raise ValueError("polygon coordinates must be finite and below %.0f in magnitude" % cocomod._COORD_MAX)
    return out[:n]


def select_mask_rows(labels, matched, parts_per_gt, num_classes):
    """detectron2's ``select_foreground_proposals`` on the sampled box rows of one image, then the rows whose ground truth has a
    polygon: ``labels`` [n] (num_classes = background, -1 = ignored), ``matched`` [n] ground-truth index per row, ``parts_per_gt``
    [G] polygon parts per ground truth, all on the host.  -> (kept row indices int64, in sampling order; the number of foreground
    rows dropped for lack of polygons)."""
    labels = np.asarray(labels).reshape(-1)
    matched = np.asarray(matched).reshape(-1).astype(np.int64)
    parts = np.asarray(parts_per_gt, np.int64).reshape(-1)
    fg = np.nonzero((labels != -1) & (labels != num_classes))[0]
    m = matched[fg]
    inside = (m >= 0) & (m < len(parts))
    has = np.zeros(len(fg), bool)
    has[inside] = parts[m[inside]] > 0
    return fg[has].astype(np.int64), int(len(fg) - has.sum())


# ---------------------------------------------------------------- bitmask ground truth (detectron2 INPUT.MASK_FORMAT = "bitmask")
def nearest_maps(src, dst, flip_before=False, flip_after=False, vertical=False):
    """The source index of every destination index of ``Image.resize(..., Image.NEAREST)`` from ``src`` to ``dst`` pixels along
    one axis (``vertical``: rows), int32 [dst] -- what detectron2's ``ResizeTransform.apply_segmentation`` does to a mask.  Taken
    from Pillow itself, by resizing an index ramp of mode "I": Pillow steps the source coordinate incrementally, so
    floor((x + 0.5) * src / dst) is not always its answer.  ``flip_before`` mirrors the source first (the host-flip path of
    ``MaskTrainLoader.prepare_image``), ``flip_after`` mirrors the result (``prepare_augmented``: resize, then flip)."""
    from PIL import Image
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError("nearest_maps: sizes must be positive, got %d -> %d" % (src, dst))
    ramp = np.arange(src, dtype=np.int32)
    if vertical:
        m = np.asarray(Image.fromarray(ramp.reshape(src, 1)).resize((1, dst), Image.NEAREST))[:, 0]
    else:
        m = np.asarray(Image.fromarray(ramp.reshape(1, src)).resize((dst, 1), Image.NEAREST))[0]
    m = m.astype(np.int32)
    if flip_before:
        m = src - 1 - m
    if flip_after:
        m = m[::-1]
    return np.ascontiguousarray(m)


def _map_range(m, lo, hi):
    """The half-open range of indices i with lo <= m[i] < hi for a monotone map; (0, 0) when there is none."""
    idx = np.nonzero((m >= lo) & (m < hi))[0]
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


def _is_polygon_list(seg):
    return isinstance(seg, (list, tuple)) and len(seg) > 0


class DeviceBitmasks:
    """The masks of one image's objects as bit windows on the device (include/apse_hip.h ``apse_mots_window``), uploaded once:
    what ``apse_bitmask_targets`` reads.  A segmentation is an RLE dict (compressed string / bytes or a plain count list; its
    ``size`` must equal ``frame_hw``), a ``WindowMask`` of that frame, a dense bool / u8 [H][W] array or tensor, or a polygon
    list (rasterised at ``frame_hw`` by ``apse_coco_poly_to_bits``).  ``[]`` or ``None`` is "no mask": an empty window, and
    ``has_mask`` (host bool [n_obj]) is False there -- the analogue of ``DevicePolygons.parts == 0``.  ``host`` is the host copy
    of the window structs and ``windows`` the device one."""

    def __init__(self, segmentations, frame_hw, device):
        from ..structures import device_windows as dw
        from ..structures.window_mask import WindowMask
        from . import mots_eval as me
        H, W = (int(v) for v in frame_hw)
        dev = torch.device(device)
        n = len(segmentations)
        if n > me.MAX_OBJECTS:
            raise ValueError("%d objects in one image, more than %d" % (n, me.MAX_OBJECTS))
        host = dw.fill_windows(np.zeros((n, 4), np.int64), np.zeros(n, np.int64), np.zeros(n, np.uint64)) if n else \
            dw.fill_windows((), (), ())
        has = np.zeros(n, bool)
        polys, rles, words, keep = [], [], [], []
        for k, seg in enumerate(segmentations):
            if seg is None or (isinstance(seg, (list, tuple)) and len(seg) == 0):
                continue
            has[k] = True
            if isinstance(seg, dict):
                if "counts" not in seg or "size" not in seg:
                    raise ValueError("segmentation %d: an RLE dict needs 'counts' and 'size'" % k)
                counts, rh, rw = cocomod.rle_counts(seg)
                if (rh, rw) != (H, W):
                    raise ValueError("segmentation %d: an RLE of size %dx%d in a frame of %dx%d" % (k, rh, rw, H, W))
                rles.append((k, counts))
            elif isinstance(seg, (list, tuple)):
                parts = []
                for p in seg:
                    a = np.asarray(p, np.float64).reshape(-1)
                    parts.append(a[:2 * (len(a) // 2)].reshape(-1, 2))
                polys.append((k, parts))
            elif isinstance(seg, WindowMask):
                if tuple(int(v) for v in seg.frame_size) != (H, W):
                    raise ValueError("segmentation %d: a WindowMask of frame %s in a frame of %dx%d" % (k, tuple(seg.frame_size), H, W))
                words.append((k, seg))
            elif isinstance(seg, np.ndarray) or torch.is_tensor(seg):
                if tuple(seg.shape) != (H, W):
                    raise ValueError("segmentation %d: a dense mask of shape %s in a frame of %dx%d" % (k, tuple(seg.shape), H, W))
                if isinstance(seg, np.ndarray):
                    seg = torch.from_numpy(np.ascontiguousarray(seg != 0))
                words.append((k, seg if seg.dtype == torch.bool else seg != 0))
            else:
                raise ValueError("segmentation %d: unsupported type %s" % (k, type(seg).__name__))
        if polys:
            win, kp = cocomod.polygons_to_windows([(parts, H, W) for _, parts in polys], dev)
            host[[k for k, _ in polys]] = dw.read_back(win)
            keep.append(kp)
        if rles:
            win, kp = me.rle_masks([c for _, c in rles], H, W, dev)
            host[[k for k, _ in rles]] = dw.read_back(win)
            keep.append(kp)
        if words:
            rects, wprs, ptrs, *kp = dw.masks_words([m for _, m in words], (H, W), dev)
            host[[k for k, _ in words]] = dw.fill_windows(rects, wprs, ptrs)
            keep.append(kp)
        self._set(host, (H, W), dev, has, keep)

    def _set(self, host, frame_hw, dev, has_mask, keep):
        from ..structures import device_windows as dw
        self.host, self.frame_hw, self.device, self.has_mask, self.keep = host, frame_hw, dev, has_mask, keep
        self.n_obj = len(host)
        self.windows = dw.upload(host, dev)

    @classmethod
    def _from(cls, host, frame_hw, dev, has_mask, keep):
        self = cls.__new__(cls)
        self._set(host, frame_hw, dev, has_mask, keep)
        return self

    @classmethod
    def merged(cls, n, groups, frame_hw, device):
        """``n`` objects from DeviceBitmasks of one frame: ``groups`` = [(object indices, DeviceBitmasks of those objects)];
        an object in no group has no mask."""
        from ..structures import device_windows as dw
        host = dw.fill_windows(np.zeros((n, 4), np.int64), np.zeros(n, np.int64), np.zeros(n, np.uint64)) if n else \
            dw.fill_windows((), (), ())
        has = np.zeros(n, bool)
        keep = []
        for idx, bm in groups:
            if tuple(bm.frame_hw) != tuple(int(v) for v in frame_hw):
                raise ValueError("merged: bitmasks of frame %s in a frame of %s" % (tuple(bm.frame_hw), tuple(frame_hw)))
            if len(idx):
                host[list(idx)] = bm.host
                has[list(idx)] = bm.has_mask
            keep.append(bm)
        return cls._from(host, tuple(int(v) for v in frame_hw), torch.device(device), has, keep)

    def transformed(self, image_hw, xmap, ymap):
        """These masks after a nearest-neighbour resize and / or flip (``nearest_maps``): a DeviceBitmasks in the image of
        ``image_hw`` whose pixel (x, y) is this one's (``xmap[x]``, ``ymap[y]``), through ``apse_mots_remap_windows``.  The
        destination rects come from the source rects and the (monotone) maps here on the host."""
        from .. import _lib
        from ..structures import device_windows as dw
        h, w = (int(v) for v in image_hw)
        xmap = np.ascontiguousarray(xmap, np.int32).reshape(-1)
        ymap = np.ascontiguousarray(ymap, np.int32).reshape(-1)
        H, W = self.frame_hw
        if len(xmap) != w or len(ymap) != h:
            raise ValueError("transformed: maps of %d columns and %d rows for an image of %dx%d" % (len(xmap), len(ymap), h, w))
        if len(xmap) and (xmap.min() < 0 or xmap.max() >= W) or len(ymap) and (ymap.min() < 0 or ymap.max() >= H):
            raise ValueError("transformed: a map entry outside the %dx%d frame" % (H, W))
        for m in (xmap, ymap):
            d = np.diff(m)
            if len(d) and not ((d >= 0).all() or (d <= 0).all()):
                raise ValueError("transformed: the maps must be monotone")
        rects = np.zeros((self.n_obj, 4), np.int64)
        for k in range(self.n_obj):
            x0, y0, x1, y1 = (int(v) for v in self.host["rect"][k])
            if x1 <= x0 or y1 <= y0 or not int(self.host["bits"][k]):
                continue
            (dx0, dx1), (dy0, dy1) = _map_range(xmap, x0, x1), _map_range(ymap, y0, y1)
            if dx1 > dx0 and dy1 > dy0:
                rects[k] = dx0, dy0, dx1, dy1
        arr, pool = dw.pooled_windows(rects, self.device)
        dst = dw.upload(arr, self.device)
        xm, ym = torch.from_numpy(xmap).to(self.device), torch.from_numpy(ymap).to(self.device)
        _lib.check(_lib.load().apse_mots_remap_windows(_lib.ptr(self.windows), self.n_obj, H, W, _lib.ptr(xm), _lib.ptr(ym), h, w,
                                                       _lib.ptr(dst), _lib.ptr(arr), _lib.stream_ptr()), None,
                   "apse_mots_remap_windows")
        return DeviceBitmasks._from(arr, (h, w), self.device, self.has_mask.copy(), [pool, xm, ym, self])


def bitmask_targets_device(bitmasks, rois, matched, mask_size=MASK_SIZE, out=None):
    """``BitMasks.crop_and_resize`` for proposals that are new every step (``apse_bitmask_targets``), with the contract of
    ``mask_targets_device``: ``bitmasks`` a DeviceBitmasks in image coordinates, ``rois`` f32 [n][4] and ``matched`` int32 [n] on
    the device -> uint8 [n][mask_size][mask_size] on the device.  One launch, no host step.  ``out``: a uint8 buffer of at
    least n rows to write into (rows past n stay untouched); the result is its first n rows."""
    from .. import _lib
    dev = bitmasks.device
    rois = torch.as_tensor(rois, dtype=torch.float32).reshape(-1, 4).to(dev).contiguous()
    matched = torch.as_tensor(matched).reshape(-1).to(dev, torch.int32).contiguous()
    n = int(rois.shape[0])
    if int(matched.shape[0]) != n:
        raise ValueError("bitmask_targets_device: %d boxes, %d matched indices" % (n, int(matched.shape[0])))
    if out is None:
        out = torch.empty((n, mask_size, mask_size), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() != 3 or out.shape[0] < n or \
            tuple(out.shape[1:]) != (mask_size, mask_size) or out.device != rois.device:
        raise ValueError("bitmask_targets_device: out must be a contiguous uint8 [>= n][%d][%d] tensor on the device" % (mask_size, mask_size))
    h, w = bitmasks.frame_hw
    _lib.check(_lib.load().apse_bitmask_targets(_lib.ptr(bitmasks.windows), bitmasks.n_obj, h, w, _lib.ptr(rois), _lib.ptr(matched), n,
                                                int(mask_size), _lib.ptr(out), _lib.stream_ptr()), None, "apse_bitmask_targets")
    return out[:n]


def bitmask_targets(segmentations, boxes, frame_hw, device, mask_size=MASK_SIZE):
    """``BitMasks.crop_and_resize(boxes, mask_size)`` of ground-truth boxes: segmentation r under box r (the analogue of
    ``mask_targets``); uint8 [n][mask_size][mask_size] on the device."""
    n = len(segmentations)
    if n == 0:
        return torch.zeros((0, mask_size, mask_size), dtype=torch.uint8, device=device)
    bm = DeviceBitmasks(segmentations, frame_hw, device)
    return bitmask_targets_device(bm, np.asarray(boxes, np.float64).reshape(-1, 4).astype(np.float32), np.arange(n, dtype=np.int32),
                                  mask_size)


class BitmaskSource:
    """One image's segmentations on their way through a loader in bitmask mode, in place of the polygon lists: ``segs`` as the
    dataset stores them (frame coordinates), ``polys`` the polygon objects transformed to the image as the polygon path
    transforms them ([] for the others), and the maps of the image's resize / flip.  ``device_bitmasks`` builds the image's
    DeviceBitmasks: polygons are rasterised at the image size (detectron2 transforms polygons first, ``polygons_to_bitmask``
    after), RLE / dense / WindowMask objects are uploaded in the frame and remapped."""

    def __init__(self, segs, polys, frame_hw, image_hw, xmap, ymap):
        self.segs, self.polys, self.frame_hw, self.image_hw, self.xmap, self.ymap = list(segs), list(polys), frame_hw, image_hw, xmap, ymap

    def __len__(self):
        return len(self.segs)

    def select(self, idx):
        return BitmaskSource([self.segs[i] for i in idx], [self.polys[i] for i in idx], self.frame_hw, self.image_hw, self.xmap, self.ymap)

    def device_bitmasks(self, device):
        poly_idx = [k for k, s in enumerate(self.segs) if _is_polygon_list(s)]
        raw_idx = [k for k, s in enumerate(self.segs) if not _is_polygon_list(s) and s is not None and not isinstance(s, (list, tuple))]
        groups = []
        if poly_idx:
            groups.append((poly_idx, DeviceBitmasks([self.polys[k] for k in poly_idx], self.image_hw, device)))
        if raw_idx:
            raw = DeviceBitmasks([self.segs[k] for k in raw_idx], self.frame_hw, device)
            groups.append((raw_idx, raw.transformed(self.image_hw, self.xmap, self.ymap)))
        return DeviceBitmasks.merged(len(self.segs), groups, self.image_hw, device)


def split_polygon_segmentations(segs, mask_format="bitmask"):
    """Bitmask mode: the polygon objects of ``segs`` as polygon lists, [] for every other object (they take no polygon
    transform).  Polygon mode: ``segs`` itself, and an RLE dict among them is refused."""
    if mask_format != "bitmask":
        if any(isinstance(s, dict) for s in segs):
            raise ValueError("RLE segmentations need mask_format=\"bitmask\"")
        return segs
    return [s if _is_polygon_list(s) else [] for s in segs]


def flip_annotations(boxes, polygons_per_roi, width):
    """Horizontal flip of XYXY boxes and polygons (detectron2 HFlipTransform: x -> width - x)."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4).copy()
    x0 = width - b[:, 2]
    x1 = width - b[:, 0]
    b[:, 0], b[:, 2] = x0, x1
    polys = []
    for ps in polygons_per_roi:
        qs = []
        for p in ps:
            q = np.array(p, np.float64)
            q[0::2] = width - q[0::2]
            qs.append(q)
        polys.append(qs)
    return b, polys


class MaskTrainLoader:
    """Yields (roi_features [n][14][14][256], classes int64 [n] (host), targets uint8 [n][28][28]) per batch of ``ims_per_batch``
    images, endlessly, in a seeded shuffled order.  ``model``: a TrackRCNN (FPN) with the frozen detector's weights.
    ``cache_features=True`` keeps every image's RoI features and targets on the device after the first visit (196 KB per object
    for the features); it is off when ``flip`` is on, where an image has two versions.  A batch with more than ``max_rois``
    ground truths (APSE_MASK_TRAIN_MAX_N) keeps the first ``max_rois``.

    With ``augment`` false and ``min_sizes`` None an image is resized to the TEST size inside the context and ``flip`` mirrors it
    on the host.  Otherwise the image takes the reference mapper's path on the device (utils/augment.py): ``resize_frames`` to a
    short edge drawn from ``min_sizes`` (``sampling`` "choice", or "range" = any integer between two sizes; capped by ``max_size``;
    None = the test size), then ``augment_images`` -- the flip when ``flip`` is on and drawn, and with ``augment`` the brightness /
    saturation / contrast / lighting chain; a step that is off gets its identity parameter -- then ``preprocess_images``, the
    backbone and the RoI features; boxes and polygons go through ``transform_annotations``.  The draws per image, in order: size
    (only with several sizes), flip (only when on), then brightness, saturation, contrast, lighting.  ``cache_features`` is off
    on that path.  Every image size has a context of its own, so the loader raises ``model.cfg.APSE.CONTEXT_CACHE`` to at least
    ``len(min_sizes)`` (8 for "range") -- the model then keeps that many contexts alive instead of rebuilding one per image."""

    def __init__(self, dicts, model, ims_per_batch=2, seed=0, flip=False, cache_features=False, max_rois=1024, augment=False,
                 min_sizes=None, max_size=None, sampling="choice", mask_format="polygon"):
        if getattr(model, "c4", False):
            raise NotImplementedError("mask-head training covers FPN models; C4 (Res5ROIHeads) shares res5 with the box branch")
        if mask_format not in MASK_FORMATS:
            raise ValueError("mask_format must be one of %s, got %r" % (MASK_FORMATS, mask_format))
        self.mask_format = mask_format
        self.dicts = list(dicts)
        self.model = model
        self.ims_per_batch = int(ims_per_batch)
        self.flip = bool(flip)
        self.augment = bool(augment)
        self.device_path = self.augment or min_sizes is not None
        self.min_sizes = tuple(int(v) for v in min_sizes) if min_sizes is not None else (int(model.cfg.INPUT.MIN_SIZE_TEST),)
        self.max_size = int(max_size) if max_size is not None else int(model.cfg.INPUT.MAX_SIZE_TEST)
        self.sampling = sampling
        if self.device_path:
            from . import augment as aug
            aug.draw_size(np.random.default_rng(0), self.min_sizes, sampling)          # refuses a bad sampling / size list now
            want = 8 if sampling == "range" else len(self.min_sizes)
            if int(model.cfg.APSE.get("CONTEXT_CACHE", 1)) < want:
                model.cfg.APSE.CONTEXT_CACHE = want
            cache_features = False
        self.cache = {} if (cache_features and not flip) else None
        self.max_rois = int(max_rois)
        self.rng = np.random.default_rng(seed)
        self._order = []

    def state_dict(self):
        return {"rng": self.rng.bit_generator.state, "order": list(self._order)}

    def load_state_dict(self, sd):
        self.rng.bit_generator.state = sd["rng"]
        self._order = list(sd["order"])

    @staticmethod
    def read_annotated(d):
        """The image of a dataset dictionary and its annotations as they are stored: (frame BGR uint8 [H][W][3], boxes f64 [G][4]
        XYXY, polygons, classes int64 [G]).  An image whose size is not the annotated one is refused."""
        from PIL import Image
        frame = np.asarray(Image.open(d["file_name"]).convert("RGB"))[:, :, ::-1].copy()
        H, W = frame.shape[:2]
        if (H, W) != (d["height"], d["width"]):
            raise ValueError("%s is %dx%d, the annotations say %dx%d" % (d["file_name"], H, W, d["height"], d["width"]))
        boxes = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]]
                          for a in d["annotations"]], np.float64).reshape(-1, 4)
        polys = [a.get("segmentation") or [] for a in d["annotations"]]          # a box-only annotation: no parts
        classes = torch.tensor([a["category_id"] for a in d["annotations"]], dtype=torch.int64)
        return frame, boxes, polys, classes

    def prepare_image(self, d, flipped=False):
        """One image through the frozen backbone at the test size: (boxes f64 [G][4] in resized-image pixels, polygons, classes)."""
        model = self.model
        frame, boxes, polys, classes = self.read_annotated(d)
        H, W = frame.shape[:2]
        segs = polys
        polys = split_polygon_segmentations(segs, self.mask_format)
        if flipped:
            frame = frame[:, ::-1].copy()
            boxes, polys = flip_annotations(boxes, polys, W)
        ih, iw = resample.resize_shortest_edge(H, W, model.cfg.INPUT.MIN_SIZE_TEST, model.cfg.INPUT.MAX_SIZE_TEST)
        sx, sy = iw / W, ih / H                                   # detectron2's ResizeTransform scales boxes and polygons alike
        boxes = boxes * np.array([sx, sy, sx, sy])
        polys = [[np.array(p, np.float64) * np.tile([sx, sy], len(p) // 2) for p in ps] for ps in polys]
        model.backbone_frames(torch.from_numpy(frame[None]).to(model.device))
        if self.mask_format == "bitmask":                         # the source is flipped first, then resized
            polys = BitmaskSource(segs, polys, (H, W), (ih, iw), nearest_maps(W, iw, flip_before=flipped),
                                  nearest_maps(H, ih, vertical=True))
        return boxes, polys, classes

    def prepare_augmented(self, d, size, params):
        """One image down the device path: resized to short edge ``size``, augmented with ``params`` (utils.augment.AugmentParams),
        through the frozen backbone: (transformed boxes f64 [G][4], polygons, classes)."""
        from . import augment as aug
        model = self.model
        frame, boxes, polys, classes = self.read_annotated(d)
        H, W = frame.shape[:2]
        ih, iw = resample.resize_shortest_edge(H, W, size, self.max_size)
        segs = polys
        polys = split_polygon_segmentations(segs, self.mask_format)
        boxes, polys = aug.transform_annotations(boxes, polys, (H, W), (ih, iw), params.flip)
        if self.mask_format == "bitmask":                         # resized first, then flipped
            polys = BitmaskSource(segs, polys, (H, W), (ih, iw), nearest_maps(W, iw, flip_after=bool(params.flip)),
                                  nearest_maps(H, ih, vertical=True))
        resized = aug.resize_frames(torch.from_numpy(frame[None]).to(model.device), ih, iw)
        _, chw, _ = aug.augment_images(resized, [params], want_u8=False)
        model.backbone_images(chw, (H, W))
        return boxes, polys, classes

    def _sample(self, boxes, polys, classes, d):
        """The item of one image whose backbone has just run, from its transformed annotations: here (features, classes, targets)
        of the ground-truth boxes.  The loaders that subclass this one override it."""
        feats = self.model.mask_roi_features(boxes.astype(np.float32))
        if self.mask_format == "bitmask":
            bm = polys.device_bitmasks(self.model.device)
            return feats, classes, bitmask_targets_device(bm, boxes.astype(np.float32), np.arange(len(boxes), dtype=np.int32))
        return feats, classes, mask_targets(polys, boxes, self.model.device)

    def image_item(self, d, flipped=False):
        """One image through the frozen backbone at the test size, then ``_sample``."""
        key = d["image_id"]
        if self.cache is not None and key in self.cache:
            return self.cache[key]
        item = self._sample(*self.prepare_image(d, flipped), d)
        if self.cache is not None:
            self.cache[key] = item
        return item

    def augmented_item(self, d, size, params):
        """``prepare_augmented``, then ``_sample``."""
        return self._sample(*self.prepare_augmented(d, size, params), d)

    def __iter__(self):
        return self

    def next_items(self):
        """The per-image items (``image_item`` / ``augmented_item``) of the next batch, with the draws in their fixed order: the
        image order, then per image the size and augmentation parameters or the host flip.  The loaders that subclass this one
        share it and differ in how they join the items."""
        items = []
        for _ in range(self.ims_per_batch):
            if not self._order:
                self._order = [int(i) for i in self.rng.permutation(len(self.dicts))]
            d = self.dicts[self._order.pop(0)]
            if self.device_path:
                from . import augment as aug
                size = aug.draw_size(self.rng, self.min_sizes, self.sampling)
                items.append(self.augmented_item(d, size, aug.draw_params(self.rng, self.flip, self.augment)))
                continue
            flipped = bool(self.flip and self.rng.random() < 0.5)
            items.append(self.image_item(d, flipped))
        return items

    def __next__(self):
        items = self.next_items()
        feats = torch.cat([i[0] for i in items])[:self.max_rois]
        return feats, torch.cat([i[1] for i in items])[:self.max_rois], torch.cat([i[2] for i in items])[:self.max_rois]
