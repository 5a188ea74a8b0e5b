"""COCO ground truth and results: the pycocotools 2.0 ``COCO`` surface the reference's evaluation uses, and its masks on the GPU.

The reference scores detectors with pycocotools (dcnn/scripts/train/finetune_uav.py ``do_test``, finetune_segmentation.py); its
ground truth comes from dcnn/utils/COCO_utils.py ``detectron2_dataset_to_coco``.  pycocotools is not a dependency of this build.
The index and ``loadRes`` are restated here as host bookkeeping; every mask becomes a bit window in the ``WindowMask`` layout on
the device (include/apse_hip.h ``apse_mots_window``):

 * polygons (and the 4-number box form that ``frPyObjects`` reads as XYWH boxes) go through ``apse_coco_poly_to_bits``, equal to
   ``rleFrPoly`` + ``merge`` pixel for pixel; the host only sizes every edge's share (``poly_layout``);
 * RLE (compressed strings through ``rle.string_to_counts``, or plain count lists) goes through ``apse_mots_rle_to_bits``;
 * the predictor's ``WindowMask`` windows are used as they are.

``area`` / ``toBbox`` of an RLE (used by ``loadRes`` for results without a box) are maskApi's host loops over the counts.
"""
import copy
import ctypes as C
import itertools
import json
import time
from collections import defaultdict

import numpy as np
import torch

from .. import _lib
from ..structures import device_windows as dw
from ..structures.window_mask import WindowMask
from . import mots_eval as me
from . import rle as rlemod

MAX_POLY_OBJECTS = 1 << 20
_COORD_MAX = 2.0 ** 31 / 5.0 - 1.0


def _is_array_like(obj):
    return hasattr(obj, "__iter__") and hasattr(obj, "__len__")


# ---------------------------------------------------------------- maskApi host loops (RLE bookkeeping)
def rle_counts(segm):
    """RLE dict (compressed string / bytes or plain list) -> (counts list, h, w)."""
    h, w = (int(v) for v in segm["size"])
    counts = segm["counts"]
    if not isinstance(counts, (list, tuple)):
        counts = rlemod.string_to_counts(counts)
    return [int(c) for c in counts], h, w


def area(segm):
    """maskApi rleArea: the ones-runs of an RLE dict (a list of dicts: a list of areas)."""
    if isinstance(segm, list):
        return [area(s) for s in segm]
    counts, _, _ = rle_counts(segm)
    return int(sum(counts[1::2]))


def toBbox(segm):
    """maskApi rleToBbox, literally (a trailing zeros run is dropped, an all-zeros RLE is [0, 0, 0, 0]); [x, y, w, h] f64."""
    if isinstance(segm, list):
        return np.array([toBbox(s) for s in segm])
    counts, h, w = rle_counts(segm)
    m = (len(counts) // 2) * 2
    if m == 0:
        return np.zeros(4)
    xs, ys, xe, ye, cc, xp = w, h, 0, 0, 0, 0
    for j in range(m):
        cc += counts[j]
        t = cc - j % 2
        y = t % h
        x = (t - y) // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, h - 1
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return np.array([xs, ys, xe - xs + 1, ye - ys + 1], dtype=np.float64)


def polygon_parts(segm):
    """A polygon-list segmentation -> list of f64 vertex arrays [k, 2].  pycocotools ``frPyObjects`` reads a list whose first entry
    holds exactly 4 numbers as XYWH boxes (``frBbox``: the polygon xs,ys xs,ye xe,ye xe,ys)."""
    if len(segm) == 0:
        return []
    if len(segm[0]) == 4:
        parts = []
        for bb in segm:
            if len(bb) != 4:
                raise ValueError("a box-form segmentation needs 4 numbers per entry, got %d" % len(bb))
            xs, ys = float(bb[0]), float(bb[1])
            xe, ye = xs + float(bb[2]), ys + float(bb[3])
            parts.append(np.array([[xs, ys], [xs, ye], [xe, ye], [xe, ys]], np.float64))
        return parts
    out = []
    for p in segm:
        a = np.asarray(p, np.float64)
        out.append(a[:2 * (len(a) // 2)].reshape(-1, 2))
    return out


# ---------------------------------------------------------------- masks -> device windows
def poly_layout(objs):
    """objs: [(parts [f64 [k, 2]], h, w)] -> host arrays of ``apse_coco_poly_to_bits``: xy [n_verts, 2], part_vert_off,
    obj_part_off, obj_hw [n, 2], edge_off [n_verts + 1] (every edge's y-boundary point count, scanned) and each object's window
    rect (columns that hold a point, full height; to the right edge when a part holds an odd number of points)."""
    n = len(objs)
    parts = [p for o in objs for p in o[0]]
    plen = np.array([len(p) for p in parts], np.int64)
    part_vert_off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum(plen, out=part_vert_off[1:])
    npart = np.array([len(o[0]) for o in objs], np.int64)
    obj_part_off = np.zeros(n + 1, np.int64)
    np.cumsum(npart, out=obj_part_off[1:])
    hw = np.array([[o[1], o[2]] for o in objs], np.int64).reshape(n, 2)
    xy = np.concatenate(parts).astype(np.float64) if len(parts) and part_vert_off[-1] else np.zeros((0, 2), np.float64)
    if xy.size and (not np.isfinite(xy).all() or np.abs(xy).max() > _COORD_MAX):
        raise ValueError("polygon coordinates must be finite and below %.0f in magnitude" % _COORD_MAX)
    nv = len(xy)
    part_of = np.repeat(np.arange(len(parts)), plen)
    obj_of_part = np.repeat(np.arange(n), npart)
    X = (5.0 * xy[:, 0] + .5).astype(np.int64)                  # C (int): truncation toward zero
    nxt = np.arange(nv) + 1
    nonempty = plen > 0
    nxt[part_vert_off[1:][nonempty] - 1] = part_vert_off[:-1][nonempty]
    lo, hi = np.minimum(X, X[nxt]) if nv else X, np.maximum(X, X[nxt]) if nv else X
    wv = hw[obj_of_part[part_of], 1] if nv else np.zeros(0, np.int64)
    xa = np.where(lo > 2, (lo + 2) // 5, 0)
    xb = np.where(hi >= 3, np.minimum(wv - 1, (hi - 3) // 5), -1)
    cnt = np.maximum(xb - xa + 1, 0)
    edge_off = np.zeros(nv + 1, np.int64)
    np.cumsum(cnt, out=edge_off[1:])
    obj_of_v = obj_of_part[part_of] if nv else np.zeros(0, np.int64)
    x0 = np.full(n, np.iinfo(np.int64).max)
    x1 = np.full(n, -1)
    has = cnt > 0
    np.minimum.at(x0, obj_of_v[has], xa[has])
    np.maximum.at(x1, obj_of_v[has], xb[has])
    odd_part = (np.bincount(part_of, weights=cnt, minlength=len(parts)).astype(np.int64) & 1) if len(parts) else np.zeros(0, np.int64)
    odd_obj = np.bincount(obj_of_part, weights=odd_part, minlength=n) > 0 if len(parts) else np.zeros(n, bool)
    rects = np.zeros((n, 4), np.int64)
    live = x1 >= 0
    rects[live, 0] = x0[live]
    rects[live, 2] = np.where(odd_obj[live], hw[live, 1], x1[live] + 1)
    rects[live, 3] = hw[live, 0]
    return dict(xy=xy, part_vert_off=part_vert_off, obj_part_off=obj_part_off, hw=hw, edge_off=edge_off, rects=rects)


def polygons_to_windows(objs, dev):
    """[(parts, h, w)] -> (windows uint8 [n, 32] on the device, buffers to keep alive).  Raises when the device's edge counts
    disagree with the host's (a bug, never data)."""
    lib = _lib.load()
    n = len(objs)
    if n == 0:
        return dw.no_windows(dev), ()
    if n > MAX_POLY_OBJECTS:
        parts = [polygons_to_windows(objs[i:i + MAX_POLY_OBJECTS], dev) for i in range(0, n, MAX_POLY_OBJECTS)]
        return torch.cat([p[0] for p in parts]), tuple(p[1] for p in parts)
    L = poly_layout(objs)
    arr, pool = dw.pooled_windows(L["rects"], dev)
    windows = dw.upload(arr, dev)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    xy = torch.from_numpy(np.ascontiguousarray(L["xy"]).reshape(-1)).to(dev)
    pvo, opo, eo = i32(L["part_vert_off"]), i32(L["obj_part_off"]), i32(L["edge_off"])
    hw_host = np.ascontiguousarray(L["hw"], np.int32)
    hw = i32(hw_host)
    toggles = torch.empty(max(int(L["edge_off"][-1]), 1), dtype=torch.int32, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.apse_coco_poly_to_bits(_lib.ptr(xy), _lib.ptr(pvo), len(L["part_vert_off"]) - 1, _lib.ptr(opo), n, _lib.ptr(hw),
                                          _lib.ptr(hw_host), _lib.ptr(eo), len(L["xy"]), _lib.ptr(toggles), _lib.ptr(windows),
                                          _lib.ptr(info), _lib.stream_ptr()), None, "apse_coco_poly_to_bits")
    if int(info.cpu()[0]):
        raise RuntimeError("apse_coco_poly_to_bits: device and host edge counts disagree")
    return windows, (pool, xy, pvo, opo, eo, hw, toggles)


def window_masks_to_windows(masks, dev):
    """WindowMask list -> (windows uint8 [n, 32] on the device, buffers to keep alive); the bits are used in place."""
    rects, wprs, ptrs, keep, _ = dw.masks_words(masks, None, dev)            # (no dense masks here: no frame size)
    return dw.upload(dw.fill_windows(rects, wprs, ptrs), dev), keep


def segm_to_windows(items, dev):
    """items: [(segmentation, h, w)] where h, w is the image size (used by polygons) -> (windows uint8 [n, 32] device, sizes
    [(h, w)], keep).  A segmentation is a polygon list, an RLE dict (compressed or plain counts) or a WindowMask."""
    n = len(items)
    windows = torch.zeros((n, dw.STRUCT_BYTES), dtype=torch.uint8, device=dev)
    sizes = [None] * n
    keep = []
    polys, rles, wms = [], defaultdict(list), []
    for k, (segm, h, w) in enumerate(items):
        if isinstance(segm, WindowMask):
            wms.append(k)
            sizes[k] = tuple(int(v) for v in segm.frame_size)
        elif isinstance(segm, list):
            polys.append(k)
            sizes[k] = (int(h), int(w))
        elif isinstance(segm, dict) and "counts" in segm and "size" in segm:
            counts, rh, rw = rle_counts(segm)
            rles[(rh, rw)].append((k, counts))
            sizes[k] = (rh, rw)
        else:
            raise ValueError("unsupported segmentation of type %s" % type(segm).__name__)
    if polys:
        win, kp = polygons_to_windows([(polygon_parts(items[k][0]), items[k][1], items[k][2]) for k in polys], dev)
        windows[torch.as_tensor(polys, device=dev)] = win
        keep.append(kp)
    for (h, w), lst in rles.items():
        for i in range(0, len(lst), me.MAX_OBJECTS):
            chunk = lst[i:i + me.MAX_OBJECTS]
            win, kp = me.rle_masks([c for _, c in chunk], h, w, dev)
            windows[torch.as_tensor([k for k, _ in chunk], device=dev)] = win
            keep.append(kp)
    if wms:
        win, kp = window_masks_to_windows([items[k][0] for k in wms], dev)
        windows[torch.as_tensor(wms, device=dev)] = win
        keep.append(kp)
    return windows, sizes, keep


def windows_to_dense(windows, h, w):
    """Device windows -> host bool [n, h, w] (tests and ``annToMask``): each window drawn alone by ``apse_mots_render_idmap``
    (an apse_mots_object has the window's layout, with the score where the area is)."""
    lib = _lib.load()
    arr = dw.read_back(windows).view(dw.OBJ_DTYPE)
    arr["score"] = 0
    objs = dw.upload(arr, windows.device)
    out = np.zeros((len(arr), h, w), bool)
    idmap = torch.empty((h, w), dtype=torch.uint16, device=windows.device)
    one = (C.c_int * 1)(1)
    for k in range(len(arr)):
        _lib.check(lib.apse_mots_render_idmap(_lib.ptr(objs[k:k + 1]), one, 1, h, w, _lib.ptr(idmap), _lib.stream_ptr()), None,
                   "apse_mots_render_idmap")
        out[k] = (idmap != 0).cpu().numpy()
    return out


# ---------------------------------------------------------------- COCO
class COCO:
    """pycocotools.coco.COCO: the index, the getters, ``loadRes`` and ``annToRLE`` / ``annToMask``."""

    def __init__(self, annotation_file=None):
        self.dataset, self.anns, self.cats, self.imgs = dict(), dict(), dict(), dict()
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        if annotation_file is not None:
            print("loading annotations into memory...")
            tic = time.time()
            with open(annotation_file, "r") as fh:
                dataset = json.load(fh)
            assert type(dataset) == dict, "annotation file format {} not supported".format(type(dataset))
            print("Done (t={:0.2f}s)".format(time.time() - tic))
            self.dataset = dataset
            self.createIndex()

    @classmethod
    def from_dataset(cls, dataset, verbose=True):
        """A COCO over an in-memory dataset dict (no file)."""
        c = cls()
        c.dataset = dataset
        c.createIndex(verbose)
        return c

    def createIndex(self, verbose=True):
        if verbose:
            print("creating index...")
        anns, cats, imgs = {}, {}, {}
        imgToAnns, catToImgs = defaultdict(list), defaultdict(list)
        if "annotations" in self.dataset:
            for ann in self.dataset["annotations"]:
                imgToAnns[ann["image_id"]].append(ann)
                anns[ann["id"]] = ann
        if "images" in self.dataset:
            for img in self.dataset["images"]:
                imgs[img["id"]] = img
        if "categories" in self.dataset:
            for cat in self.dataset["categories"]:
                cats[cat["id"]] = cat
        if "annotations" in self.dataset and "categories" in self.dataset:
            for ann in self.dataset["annotations"]:
                catToImgs[ann["category_id"]].append(ann["image_id"])
        if verbose:
            print("index created!")
        self.anns, self.imgToAnns, self.catToImgs, self.imgs, self.cats = anns, imgToAnns, catToImgs, imgs, cats

    def getAnnIds(self, imgIds=[], catIds=[], areaRng=[], iscrowd=None):
        imgIds = imgIds if _is_array_like(imgIds) else [imgIds]
        catIds = catIds if _is_array_like(catIds) else [catIds]
        if len(imgIds) == len(catIds) == len(areaRng) == 0:
            anns = self.dataset["annotations"]
        else:
            if not len(imgIds) == 0:
                lists = [self.imgToAnns[imgId] for imgId in imgIds if imgId in self.imgToAnns]
                anns = list(itertools.chain.from_iterable(lists))
            else:
                anns = self.dataset["annotations"]
            anns = anns if len(catIds) == 0 else [ann for ann in anns if ann["category_id"] in catIds]
            anns = anns if len(areaRng) == 0 else [ann for ann in anns if areaRng[0] < ann["area"] < areaRng[1]]
        if iscrowd is not None:
            return [ann["id"] for ann in anns if ann["iscrowd"] == iscrowd]
        return [ann["id"] for ann in anns]

    def getCatIds(self, catNms=[], supNms=[], catIds=[]):
        catNms = catNms if _is_array_like(catNms) else [catNms]
        supNms = supNms if _is_array_like(supNms) else [supNms]
        catIds = catIds if _is_array_like(catIds) else [catIds]
        if len(catNms) == len(supNms) == len(catIds) == 0:
            cats = self.dataset["categories"]
        else:
            cats = self.dataset["categories"]
            cats = cats if len(catNms) == 0 else [cat for cat in cats if cat["name"] in catNms]
            cats = cats if len(supNms) == 0 else [cat for cat in cats if cat["supercategory"] in supNms]
            cats = cats if len(catIds) == 0 else [cat for cat in cats if cat["id"] in catIds]
        return [cat["id"] for cat in cats]

    def getImgIds(self, imgIds=[], catIds=[]):
        imgIds = imgIds if _is_array_like(imgIds) else [imgIds]
        catIds = catIds if _is_array_like(catIds) else [catIds]
        if len(imgIds) == len(catIds) == 0:
            ids = self.imgs.keys()
        else:
            ids = set(imgIds)
            for i, catId in enumerate(catIds):
                if i == 0 and len(ids) == 0:
                    ids = set(self.catToImgs[catId])
                else:
                    ids &= set(self.catToImgs[catId])
        return list(ids)

    def loadAnns(self, ids=[]):
        if _is_array_like(ids):
            return [self.anns[i] for i in ids]
        return [self.anns[ids]]

    def loadCats(self, ids=[]):
        if _is_array_like(ids):
            return [self.cats[i] for i in ids]
        return [self.cats[ids]]

    def loadImgs(self, ids=[]):
        if _is_array_like(ids):
            return [self.imgs[i] for i in ids]
        return [self.imgs[ids]]

    def loadRes(self, resFile):
        """pycocotools' field rules: results with a non-empty ``bbox`` (judged on the first) get ``area = w*h``, a box polygon when
        ``segmentation`` is missing, ``id = index + 1`` and ``iscrowd = 0``; results with only ``segmentation`` (compressed RLE or
        a WindowMask) get the mask area and ``toBbox``.  A list is used in place (its dicts gain those fields)."""
        res = COCO()
        res.dataset["images"] = [img for img in self.dataset["images"]]
        print("Loading and preparing results...")
        tic = time.time()
        if isinstance(resFile, str):
            with open(resFile) as fh:
                anns = json.load(fh)
        else:
            anns = resFile
        assert type(anns) == list, "results in not an array of objects"
        annsImgIds = [ann["image_id"] for ann in anns]
        assert set(annsImgIds) == (set(annsImgIds) & set(self.getImgIds())), "Results do not correspond to current coco set"
        if len(anns) and "bbox" in anns[0] and not anns[0]["bbox"] == []:
            res.dataset["categories"] = copy.deepcopy(self.dataset["categories"])
            for id, ann in enumerate(anns):
                bb = ann["bbox"]
                x1, x2, y1, y2 = [bb[0], bb[0] + bb[2], bb[1], bb[1] + bb[3]]
                if "segmentation" not in ann:
                    ann["segmentation"] = [[x1, y1, x1, y2, x2, y2, x2, y1]]
                ann["area"] = bb[2] * bb[3]
                ann["id"] = id + 1
                ann["iscrowd"] = 0
        elif len(anns) and "segmentation" in anns[0]:
            res.dataset["categories"] = copy.deepcopy(self.dataset["categories"])
            for id, ann in enumerate(anns):
                segm = ann["segmentation"]
                if isinstance(segm, WindowMask):
                    ann["area"] = segm.mass
                    if "bbox" not in ann:
                        raise ValueError("a WindowMask result needs its bbox")
                else:
                    ann["area"] = area(segm)
                    if "bbox" not in ann:
                        ann["bbox"] = toBbox(segm)
                ann["id"] = id + 1
                ann["iscrowd"] = 0
        elif len(anns) and "keypoints" in anns[0]:
            raise NotImplementedError("keypoint results are not supported")
        print("DONE (t={:0.2f}s)".format(time.time() - tic))
        res.dataset["annotations"] = anns
        res.createIndex()
        return res

    def annToRLE(self, ann, device=None):
        """The annotation's mask as a compressed RLE dict (``counts`` bytes), through the device windows."""
        segm = ann["segmentation"]
        if isinstance(segm, dict) and not isinstance(segm["counts"], list):
            return segm
        m = self.annToMask(ann, device)
        return rlemod.encode(m)

    def annToMask(self, ann, device=None):
        t = self.imgs[ann["image_id"]]
        windows, sizes, keep = segm_to_windows([(ann["segmentation"], t["height"], t["width"])], dw.default_device(device))
        h, w = sizes[0]
        return windows_to_dense(windows, h, w)[0].astype(np.uint8)
