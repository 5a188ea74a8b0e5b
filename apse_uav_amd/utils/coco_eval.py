"""COCO box and mask AP on the GPU: pycocotools 2.0 ``COCOeval`` for iouType 'bbox' and 'segm', and detectron2 0.1.2's
``instances_to_coco_json``.

The reference computes AP with pycocotools (dcnn/scripts/train/finetune_uav.py ``do_test``: ``COCOeval(..., 'bbox')``,
finetune_segmentation.py: ``'segm'``).  Here the per-pair and per-group work runs in HIP (csrc/coco_eval.hip): box IoU, mask IoU
from exact popcounts (``apse_mots_overlaps``, an f64 division of integers), the greedy matching of every (image, category, area
range, threshold) and the accumulation (a stable sort of every category's scores, counts, precision envelope, recall lookups).
The host keeps pycocotools' bookkeeping: the index, the (image, category) groups, ``summarize``.

 * ``COCOeval(cocoGt, cocoDt, iouType)``: ``evaluate()``, ``accumulate()``, ``summarize()``, ``stats``, ``eval``; ``evalImgs`` and
   ``ious`` are read back from the device only when read.
 * ``instances_to_coco_json(instances, img_id)``: the predictor's ``Instances`` -> result dicts (compressed RLE masks).
 * ``CocoEvaluator(coco_gt)``: online, ``add(img_id, instances)`` per image; the masks stay on the device and nothing goes
   through JSON, with results equal to the JSON path bit for bit.

Rules and limits: DESIGN.md "COCO evaluation".  ``iouType='keypoints'`` and ``useCats=0`` are refused.
"""
import copy
import datetime
import time

import numpy as np
import torch

from .. import _lib
from ..structures.device_windows import default_device
from ..structures.window_mask import WindowMask
from . import coco as cocomod
from . import mots_eval as me
from . import rle as rlemod
from . import rle_device


class Params:
    """pycocotools' detection parameters."""

    def setDetParams(self):
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ["all", "small", "medium", "large"]
        self.useCats = 1

    def __init__(self, iouType="segm"):
        if iouType == "segm" or iouType == "bbox":
            self.setDetParams()
        elif iouType == "keypoints":
            raise NotImplementedError("iouType 'keypoints' is not supported (detection only: 'bbox', 'segm')")
        else:
            raise Exception("iouType not supported")
        self.iouType = iouType
        self.useSegm = None


def _to_dev(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


class COCOeval:
    """pycocotools.cocoeval.COCOeval for 'bbox' and 'segm' on the GPU."""

    def __init__(self, cocoGt=None, cocoDt=None, iouType="segm", device=None):
        if not iouType:
            print("iouType not specified. use default iouType segm")
        self.cocoGt = cocoGt
        self.cocoDt = cocoDt
        self.eval = {}
        self.params = Params(iouType=iouType)
        self._paramsEval = {}
        self.stats = []
        self.device = device
        self._state = None
        self._evalImgs = None
        self._ious = None
        if cocoGt is not None:
            self.params.imgIds = sorted(cocoGt.getImgIds())
            self.params.catIds = sorted(cocoGt.getCatIds())

    # ------------------------------------------------------------ evaluate
    def _prepare(self):
        p = self.params
        gts = self.cocoGt.loadAnns(self.cocoGt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        dts = self.cocoDt.loadAnns(self.cocoDt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        for gt in gts:
            gt["ignore"] = gt["ignore"] if "ignore" in gt else 0
            gt["ignore"] = "iscrowd" in gt and gt["iscrowd"]
        return gts, dts

    def evaluate(self):
        tic = time.time()
        print("Running per image evaluation...")
        p = self.params
        if p.useSegm is not None:
            p.iouType = "segm" if p.useSegm == 1 else "bbox"
            print("useSegm (deprecated) is not None. Running {} evaluation".format(p.iouType))
        print("Evaluate annotation type *{}*".format(p.iouType))
        if p.iouType not in ("bbox", "segm"):
            raise NotImplementedError("iouType %r is not supported (detection only: 'bbox', 'segm')" % p.iouType)
        if not p.useCats:
            raise NotImplementedError("useCats=0 is not supported: detections are evaluated per category")
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self.params = p
        gts, dts = self._prepare()
        self._state = self._run(gts, dts)
        self._evalImgs = None
        self._ious = None
        self._paramsEval = copy.deepcopy(self.params)
        toc = time.time()
        print("DONE (t={:0.2f}s).".format(toc - tic))

    def _run(self, gts, dts):
        """Groups on the host, IoU and matching on the device; the outputs stay there."""
        p = self.params
        dev = default_device(self.device)
        lib = _lib.load()
        I, K = len(p.imgIds), len(p.catIds)
        img_ix = {int(v): n for n, v in enumerate(p.imgIds)}
        cat_ix = {int(v): n for n, v in enumerate(p.catIds)}
        g_key = np.array([cat_ix[int(g["category_id"])] * I + img_ix[int(g["image_id"])] for g in gts], np.int64)
        d_key = np.array([cat_ix[int(d["category_id"])] * I + img_ix[int(d["image_id"])] for d in dts], np.int64)
        d_score = np.array([d["score"] for d in dts], np.float64)
        g_order = np.argsort(g_key, kind="mergesort")
        d_order = np.lexsort((-d_score, d_key))                # group, then descending score; ties keep file order
        g_key, d_key = g_key[g_order], d_key[d_order]
        maxdet = p.maxDets[-1]
        keys = np.unique(np.concatenate([g_key, d_key]))
        # detections: rank inside the group, cut to maxDets[-1]
        first = np.searchsorted(d_key, d_key, side="left")
        rank = np.arange(len(d_key)) - first
        keep = rank < maxdet
        d_order, d_key = d_order[keep], d_key[keep]
        gts_s = [gts[i] for i in g_order]
        dts_s = [dts[i] for i in d_order]
        gt_off = np.searchsorted(g_key, keys, side="left").astype(np.int64)
        gt_off = np.append(gt_off, len(g_key))
        dt_off = np.searchsorted(d_key, keys, side="left").astype(np.int64)
        dt_off = np.append(dt_off, len(d_key))
        G = np.diff(gt_off)
        D = np.diff(dt_off)
        n_groups = len(keys)
        pairs = D * G
        iou_off = np.zeros(n_groups + 1, np.int64)
        np.cumsum(pairs, out=iou_off[1:])
        n_gt, n_dt = len(gts_s), len(dts_s)
        gt_crowd = np.array([int(g["iscrowd"]) for g in gts_s], np.int32)
        gt_area = np.array([g["area"] for g in gts_s], np.float64)
        gt_id = np.array([g["id"] for g in gts_s], np.int64)
        dt_area = np.array([d["area"] for d in dts_s], np.float64)
        dt_id = np.array([d["id"] for d in dts_s], np.int64)
        dt_score = np.array([d["score"] for d in dts_s], np.float64)
        max_dt = int(D.max()) if n_groups else 0
        max_gt = int(G.max()) if n_groups else 0
        i32 = lambda a: _to_dev(a, np.int32, dev)
        t_dt_off, t_gt_off, t_iou_off = i32(dt_off), i32(gt_off), _to_dev(iou_off[:-1] if n_groups else np.zeros(1), np.int64, dev)
        t_crowd = i32(gt_crowd if n_gt else np.zeros(1))
        n_pairs = int(iou_off[-1])
        iou = torch.zeros(max(n_pairs, 1), dtype=torch.float64, device=dev)
        if p.iouType == "bbox":
            gb = np.array([g["bbox"] for g in gts_s], np.float64).reshape(n_gt, 4)
            db = np.array([d["bbox"] for d in dts_s], np.float64).reshape(n_dt, 4)
            t_gb = _to_dev(gb if n_gt else np.zeros((1, 4)), np.float64, dev)
            t_db = _to_dev(db if n_dt else np.zeros((1, 4)), np.float64, dev)
            _lib.check(lib.apse_coco_box_iou(_lib.ptr(t_dt_off), _lib.ptr(t_gt_off), _lib.ptr(t_iou_off), n_groups, max_dt, max_gt,
                                             _lib.ptr(t_db), _lib.ptr(t_gb), _lib.ptr(t_crowd), _lib.ptr(iou), _lib.stream_ptr()),
                       None, "apse_coco_box_iou")
        else:
            iou_host = self._mask_ious(gts_s, dts_s, gt_off, dt_off, iou_off, gt_crowd, n_pairs)
            iou = _to_dev(iou_host if n_pairs else np.zeros(1), np.float64, dev)
        A, T = len(p.areaRng), len(p.iouThrs)
        dt_match = torch.empty(max(A * T * n_dt, 1), dtype=torch.int64, device=dev)
        dt_ignore = torch.empty(max(A * T * n_dt, 1), dtype=torch.uint8, device=dev)
        gt_match = torch.empty(max(A * T * n_gt, 1), dtype=torch.int64, device=dev)
        gt_ignore = torch.empty(max(A * n_gt, 1), dtype=torch.uint8, device=dev)
        t_dt_area, t_dt_id = _to_dev(dt_area if n_dt else np.zeros(1), np.float64, dev), _to_dev(dt_id if n_dt else np.zeros(1), np.int64, dev)
        t_gt_area, t_gt_id = _to_dev(gt_area if n_gt else np.zeros(1), np.float64, dev), _to_dev(gt_id if n_gt else np.zeros(1), np.int64, dev)
        rng = np.ascontiguousarray(np.asarray(p.areaRng, np.float64).reshape(A, 2))
        thr = np.ascontiguousarray(np.asarray(p.iouThrs, np.float64))
        _lib.check(lib.apse_coco_match(_lib.ptr(t_dt_off), _lib.ptr(t_gt_off), _lib.ptr(t_iou_off), n_groups, max_dt, max_gt,
                                       _lib.ptr(iou), _lib.ptr(t_dt_area), _lib.ptr(t_dt_id), n_dt, _lib.ptr(t_gt_area),
                                       _lib.ptr(t_crowd), _lib.ptr(t_gt_id), n_gt, _lib.ptr(rng), A, _lib.ptr(thr), T,
                                       _lib.ptr(dt_match), _lib.ptr(dt_ignore), _lib.ptr(gt_match), _lib.ptr(gt_ignore),
                                       _lib.stream_ptr()), None, "apse_coco_match")
        cat_gt_off = np.searchsorted(g_key, np.arange(K + 1, dtype=np.int64) * I, side="left")
        return dict(keys=keys, I=I, K=K, gt_off=gt_off, dt_off=dt_off, iou_off=iou_off, gts=gts_s, dts=dts_s, iou=iou,
                    dt_match=dt_match, dt_ignore=dt_ignore, gt_match=gt_match, gt_ignore=gt_ignore, dt_score=dt_score,
                    t_dt_score=_to_dev(dt_score if n_dt else np.zeros(1), np.float64, dev), cat_gt_off=cat_gt_off,
                    n_gt=n_gt, n_dt=n_dt, A=A, T=T)

    def _mask_ious(self, gts, dts, gt_off, dt_off, iou_off, gt_crowd, n_pairs):
        """maskApi rleIou on the device windows: |a & b|, |a|, |b| by popcounts, IoU = i / (|a| + |b| - i) (i / |a| against
        crowd), 0 when i == 0, an f64 division of exact integers."""
        dev = default_device(self.device)
        out = np.zeros(n_pairs, np.float64)
        if n_pairs == 0:
            return out
        imgs = self.cocoGt.imgs
        items = [(g["segmentation"], imgs[g["image_id"]]["height"], imgs[g["image_id"]]["width"]) for g in gts]
        items += [(d["segmentation"], imgs[d["image_id"]]["height"], imgs[d["image_id"]]["width"]) for d in dts]
        windows, sizes, keep = cocomod.segm_to_windows(items, dev)
        n_gt = len(gts)
        a_idx, b_idx = [], []
        G = np.diff(gt_off)
        D = np.diff(dt_off)
        for k in np.flatnonzero(G * D):
            g0, d0 = int(gt_off[k]), int(dt_off[k])
            gs, ds = int(G[k]), int(D[k])
            both = set(sizes[g0:g0 + gs]) | set(sizes[n_gt + d0:n_gt + d0 + ds])
            if len(both) > 1:
                raise ValueError("masks of one image differ in size: %s" % sorted(both))
            dd, gg = np.meshgrid(np.arange(ds), np.arange(gs), indexing="ij")
            a_idx.append((n_gt + d0 + dd).reshape(-1))
            b_idx.append((g0 + gg).reshape(-1))
            del dd, gg
        a_idx = np.concatenate(a_idx)
        b_idx = np.concatenate(b_idx)
        res = np.zeros((n_pairs, 3), np.int64)
        for p0 in range(0, n_pairs, me.MAX_PAIRS):
            chunk = np.stack([a_idx[p0:p0 + me.MAX_PAIRS], b_idx[p0:p0 + me.MAX_PAIRS]], 1)
            res[p0:p0 + len(chunk)] = me.overlaps(windows, chunk)
        del keep
        i, ua, ub = res[:, 0], res[:, 1], res[:, 2]
        crowd = gt_crowd[b_idx].astype(bool)
        u = np.where(crowd, ua, ua + ub - i)
        nz = i > 0
        out[nz] = i[nz].astype(np.float64) / u[nz].astype(np.float64)
        return out

    # ------------------------------------------------------------ read-backs
    @property
    def ious(self):
        """{(imgId, catId): [D][G] f64 array, or [] when the group has no detection or no ground truth}."""
        if self._ious is None and self._state is not None:
            s = self._state
            p = self.params
            iou = s["iou"].cpu().numpy()
            where = {int(k): n for n, k in enumerate(s["keys"])}
            out = {}
            for i, imgId in enumerate(p.imgIds):
                for k, catId in enumerate(p.catIds):
                    n = where.get(k * s["I"] + i)
                    if n is None:
                        out[imgId, catId] = []
                        continue
                    G = int(s["gt_off"][n + 1] - s["gt_off"][n])
                    D = int(s["dt_off"][n + 1] - s["dt_off"][n])
                    out[imgId, catId] = iou[s["iou_off"][n]:s["iou_off"][n] + D * G].reshape(D, G) if D and G else []
            self._ious = out
        return self._ious if self._ious is not None else {}

    @property
    def evalImgs(self):
        """evaluateImg's dicts for every (category, area range, image), None for a group without detections and ground truths."""
        if self._evalImgs is None and self._state is not None:
            s = self._state
            p = self.params
            A, T, I = s["A"], s["T"], s["I"]
            dm = s["dt_match"].cpu().numpy()[:A * T * s["n_dt"]].reshape(A, T, s["n_dt"]).astype(np.float64)
            di = s["dt_ignore"].cpu().numpy()[:A * T * s["n_dt"]].reshape(A, T, s["n_dt"]).astype(bool)
            gm = s["gt_match"].cpu().numpy()[:A * T * s["n_gt"]].reshape(A, T, s["n_gt"]).astype(np.float64)
            gi = s["gt_ignore"].cpu().numpy()[:A * s["n_gt"]].reshape(A, s["n_gt"]).astype(np.int64)
            where = {int(k): n for n, k in enumerate(s["keys"])}
            out = []
            maxDet = p.maxDets[-1]
            for k, catId in enumerate(p.catIds):
                for a, aRng in enumerate(p.areaRng):
                    for i, imgId in enumerate(p.imgIds):
                        n = where.get(k * I + i)
                        if n is None:
                            out.append(None)
                            continue
                        g0, g1 = int(s["gt_off"][n]), int(s["gt_off"][n + 1])
                        d0, d1 = int(s["dt_off"][n]), int(s["dt_off"][n + 1])
                        gtind = np.argsort(gi[a, g0:g1], kind="mergesort")
                        gts = [s["gts"][g0 + j] for j in gtind]
                        dts = s["dts"][d0:d1]
                        out.append({"image_id": imgId, "category_id": catId, "aRng": aRng, "maxDet": maxDet,
                                    "dtIds": [d["id"] for d in dts], "gtIds": [g["id"] for g in gts],
                                    "dtMatches": dm[a, :, d0:d1], "gtMatches": gm[a, :, g0:g1][:, gtind],
                                    "dtScores": [d["score"] for d in dts], "gtIgnore": gi[a, g0:g1][gtind],
                                    "dtIgnore": di[a, :, d0:d1]})
            self._evalImgs = out
        return self._evalImgs if self._evalImgs is not None else []

    # ------------------------------------------------------------ accumulate / summarize
    def accumulate(self, p=None):
        print("Accumulating evaluation results...")
        tic = time.time()
        if self._state is None:
            print("Please run evaluate() first")
            raise RuntimeError("accumulate() needs evaluate() first")
        if p is None:
            p = self.params
        # the device buffers of evaluate() have its shapes: any other image, category, area range, maxDets or IoU threshold list
        # (a different p, or self.params edited in place since) would index past them
        pe = self._paramsEval
        if (p.useCats != pe.useCats or list(p.catIds) != list(pe.catIds) or list(p.imgIds) != list(pe.imgIds)
                or [tuple(a) for a in p.areaRng] != [tuple(a) for a in pe.areaRng] or list(p.maxDets) != list(pe.maxDets)
                or not np.array_equal(np.asarray(p.iouThrs, np.float64), np.asarray(pe.iouThrs, np.float64))):
            raise ValueError("accumulate() with images, categories, area ranges, maxDets or IoU thresholds other than "
                             "evaluate()'s; run evaluate() again")
        s = self._state
        lib = _lib.load()
        dev = default_device(self.device)
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        I = s["I"]
        keys = s["keys"]
        D = np.diff(s["dt_off"])
        starts = s["dt_off"][:-1]
        cat_of = keys // I if len(keys) else keys
        segs, seg_len = [], []
        for maxDet in p.maxDets:                               # segment m * K + k: the first maxDet of each image, image order
            take = np.minimum(D, maxDet)
            idx = np.repeat(starts - np.concatenate([[0], np.cumsum(take)[:-1]]) if len(take) else starts, take) + \
                np.arange(int(take.sum()))
            segs.append(idx)
            seg_len.append(np.bincount(cat_of, weights=take, minlength=K).astype(np.int64) if len(keys) else np.zeros(K, np.int64))
        seg_idx = np.concatenate(segs).astype(np.int32) if segs else np.zeros(0, np.int32)
        lens = np.concatenate(seg_len)
        seg_off = np.zeros(K * M + 1, np.int64)
        np.cumsum(lens, out=seg_off[1:])
        n_keys = int(seg_off[-1])
        max_seg = int(lens.max()) if len(lens) else 0
        ws = torch.empty(lib.apse_coco_accumulate_workspace_bytes(n_keys), dtype=torch.uint8, device=dev)
        prec = torch.empty(T * R * K * A * M, dtype=torch.float64, device=dev)
        rec = torch.empty(T * K * A * M, dtype=torch.float64, device=dev)
        scr = torch.empty(T * R * K * A * M, dtype=torch.float64, device=dev)
        t_seg_off = _to_dev(seg_off, np.int32, dev)
        t_seg_idx = _to_dev(seg_idx if n_keys else np.zeros(1), np.int32, dev)
        t_cat = _to_dev(s["cat_gt_off"], np.int32, dev)
        t_rec = _to_dev(np.asarray(p.recThrs, np.float64), np.float64, dev)
        _lib.check(lib.apse_coco_accumulate(_lib.ptr(s["t_dt_score"]), _lib.ptr(s["dt_match"]), _lib.ptr(s["dt_ignore"]), s["n_dt"],
                                            _lib.ptr(s["gt_ignore"]), s["n_gt"], _lib.ptr(t_cat), _lib.ptr(t_seg_off),
                                            _lib.ptr(t_seg_idx), n_keys, max_seg, _lib.ptr(t_rec), T, R, K, A, M, _lib.ptr(prec),
                                            _lib.ptr(rec), _lib.ptr(scr), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   None, "apse_coco_accumulate")
        self.eval = {
            "params": p,
            "counts": [T, R, K, A, M],
            "date": datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S"),
            "precision": prec.cpu().numpy().reshape(T, R, K, A, M),
            "recall": rec.cpu().numpy().reshape(T, K, A, M),
            "scores": scr.cpu().numpy().reshape(T, R, K, A, M),
        }
        toc = time.time()
        print("DONE (t={:0.2f}s).".format(toc - tic))

    def summarize(self):
        def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
            p = self.params
            iStr = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
            titleStr = "Average Precision" if ap == 1 else "Average Recall"
            typeStr = "(AP)" if ap == 1 else "(AR)"
            iouStr = "{:0.2f}:{:0.2f}".format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else "{:0.2f}".format(iouThr)
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            if ap == 1:
                s = self.eval["precision"]
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval["recall"]
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            print(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
            return mean_s

        def _summarizeDets():
            stats = np.zeros((12,))
            stats[0] = _summarize(1)
            stats[1] = _summarize(1, iouThr=.5, maxDets=self.params.maxDets[2])
            stats[2] = _summarize(1, iouThr=.75, maxDets=self.params.maxDets[2])
            stats[3] = _summarize(1, areaRng="small", maxDets=self.params.maxDets[2])
            stats[4] = _summarize(1, areaRng="medium", maxDets=self.params.maxDets[2])
            stats[5] = _summarize(1, areaRng="large", maxDets=self.params.maxDets[2])
            stats[6] = _summarize(0, maxDets=self.params.maxDets[0])
            stats[7] = _summarize(0, maxDets=self.params.maxDets[1])
            stats[8] = _summarize(0, maxDets=self.params.maxDets[2])
            stats[9] = _summarize(0, areaRng="small", maxDets=self.params.maxDets[2])
            stats[10] = _summarize(0, areaRng="medium", maxDets=self.params.maxDets[2])
            stats[11] = _summarize(0, areaRng="large", maxDets=self.params.maxDets[2])
            return stats

        if not self.eval:
            raise Exception("Please run accumulate() first")
        self.stats = _summarizeDets()

    def __str__(self):
        self.summarize()
        return ""


# ---------------------------------------------------------------- detectron2 0.1.2 evaluation/coco_evaluation.py
def _xywh_f32(instances):
    boxes = instances.pred_boxes.tensor
    boxes = boxes.cpu().numpy().astype(np.float32, copy=True) if isinstance(boxes, torch.Tensor) else \
        np.array(boxes, np.float32)
    boxes[:, 2] -= boxes[:, 0]                              # BoxMode XYXY_ABS -> XYWH_ABS, in f32
    boxes[:, 3] -= boxes[:, 1]
    return boxes


def instances_to_coco_json(instances, img_id):
    """detectron2 0.1.2 ``instances_to_coco_json``: XYWH boxes computed in f32, f32 scores as Python floats, ``category_id`` =
    the class index, masks as compressed RLE with ``counts`` decoded to str.  WindowMasks on a GPU are encoded there from their
    windows (utils/rle_device.py); other masks through the dense host frame."""
    num_instance = len(instances)
    if num_instance == 0:
        return []
    boxes = _xywh_f32(instances).tolist()
    scores = instances.scores.tolist()
    classes = instances.pred_classes.tolist()
    has_mask = instances.has("pred_masks")
    if has_mask:
        rles = []
        masks = list(instances.pred_masks)
        if rle_device.device_of(masks) is not None and len({tuple(m.frame_size) for m in masks}) == 1:
            rles = rle_device.encode_masks(masks, masks[0].frame_size)     # on the GPU, from the windows
            for r in rles:
                r["counts"] = r["counts"].decode("utf-8")
            masks = []
        for mask in masks:
            dense = mask.dense() if isinstance(mask, WindowMask) else torch.as_tensor(mask)
            r = rlemod.encode(dense.cpu().numpy().astype(np.uint8))
            r["counts"] = r["counts"].decode("utf-8")
            rles.append(r)
    results = []
    for k in range(num_instance):
        result = {"image_id": img_id, "category_id": classes[k], "bbox": boxes[k], "score": scores[k]}
        if has_mask:
            result["segmentation"] = rles[k]
        results.append(result)
    return results


class CocoEvaluator:
    """Online COCO evaluation of predictor outputs: ``add(img_id, instances)`` per image (``TrackPredictor`` outputs), then
    ``evaluate(iou_type)``.  The results are the fields of ``instances_to_coco_json`` (``category_ids[class]`` when a mapping is
    given), but masks stay the device's ``WindowMask`` windows; the scores equal the JSON path's bit for bit."""

    def __init__(self, coco_gt, category_ids=None, device=None):
        self.coco_gt = coco_gt
        self.category_ids = list(category_ids) if category_ids is not None else None
        self.device = device
        self.results = []

    def add(self, img_id, instances):
        n = len(instances)
        if n == 0:
            return
        boxes = _xywh_f32(instances).tolist()
        scores = instances.scores.tolist()
        classes = instances.pred_classes.tolist()
        masks = instances.pred_masks if instances.has("pred_masks") else None
        for k in range(n):
            cat = classes[k] if self.category_ids is None else self.category_ids[classes[k]]
            r = {"image_id": img_id, "category_id": cat, "bbox": boxes[k], "score": scores[k]}
            if masks is not None:
                m = masks[k]
                if not isinstance(m, WindowMask):
                    dense = torch.as_tensor(m)
                    m = {"size": list(dense.shape), "counts": rlemod.counts_from_mask(dense.cpu().numpy())}
                r["segmentation"] = m
            self.results.append(r)

    def evaluate(self, iou_type="bbox"):
        """COCOeval over everything added so far: evaluate, accumulate, summarize; returns the COCOeval."""
        res = self.coco_gt.loadRes([dict(r) for r in self.results])
        ev = COCOeval(self.coco_gt, res, iou_type, device=self.device)
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
        return ev
