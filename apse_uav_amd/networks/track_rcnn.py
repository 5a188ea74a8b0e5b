"""TrackRCNN -- counterpart of /root/reference/dcnn/networks/track_rcnn.py:5-58.

The reference subclasses detectron2's GeneralizedRCNN and returns ``(postprocessed results,
FPN feature dict)`` from ``inference``.  Here the whole per-frame computation is one enqueue
sequence of hand-written HIP kernels inside ``libapse_hip.so`` (include/apse_hip.h): this class
owns the library context, feeds it weights (detectron2 state_dict key names) and turns the
results block into the reference's return types.  There is no CPU fallback.
"""
import collections
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..structures.instances import Boxes, Instances
from ..structures.window_mask import MaskList, WindowMask
from ..structures.yuv_frame import FORMATS, YuvBatch, YuvFrame, matrix_index
from ..utils import resample
from ..config import check_c4_supported, is_c4
from ..weights import blocks_from_state, is_c4_state


class _Shape:
    def __init__(self, channels, stride):
        self.channels, self.stride = channels, stride


class _Backbone:
    """``model.backbone.output_shape()`` as read by rcnn_tracker.py:53.  FPN: p2..p6, padded to /32; C4 (Res5ROIHeads):
    res4 only, unpadded (detectron2's ResNet backbone has size_divisibility 0)."""

    def __init__(self, c4=False):
        self.c4 = c4
        self.size_divisibility = 0 if c4 else 32

    def output_shape(self):
        if self.c4:
            return {"res4": _Shape(1024, 16)}
        return {"p%d" % l: _Shape(256, 2 ** l) for l in range(2, 7)}


def c4_res4_size(image_h, image_w):
    """res4 of the unpadded C4 trunk: the stem (7x7 / 2, pad 3), the max-pool (3x3 / 2, pad 1) and the stride-2 1x1 of res3
    and res4 each map n -> (n - 1) // 2 + 1."""
    h, w = image_h, image_w
    for _ in range(4):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h, w


class LazyFeatures(dict):
    """{"p2".."p6"} (C4: {"res4"}): NCHW f32 CUDA tensors, exported from the context on first access."""

    def __init__(self, model, batch):
        super().__init__()
        self._model, self._batch = model, batch

    def __missing__(self, key):
        if self._model.backbone.c4 and key not in self.keys():
            raise KeyError(key)                # C4 exports res4 only (FPN models still export res2..res5 / stem on demand)
        t = self._model.export_feature(key, self._batch)
        self[key] = t
        return t

    def keys(self):
        return ["res4"] if self._model.backbone.c4 else ["p2", "p3", "p4", "p5", "p6"]


class FrameResults:
    """Host view of one forward's results block (apse_results_layout)."""

    def __init__(self, raw, lay, batch):
        self.raw, self.lay, self.batch = raw, lay, batch
        n, kd, e = lay.n_max, lay.dets_per_image, lay.embed_dim

        def arr(off, dtype, shape):
            cnt = int(np.prod(shape))
            return np.frombuffer(raw, dtype=dtype, count=cnt, offset=off).reshape(shape)

        self.total = int(arr(lay.total, np.int32, (1,))[0])
        self.offset = arr(lay.offset, np.int32, (lay.max_batch + 1,))
        self.prop_count = arr(lay.prop_count, np.int32, (lay.max_batch,))
        self.img = arr(lay.img, np.int32, (n,))
        self.cls = arr(lay.cls, np.int32, (n,))
        self.roi = arr(lay.roi, np.int32, (n,))
        self.score = arr(lay.score, np.float32, (n,))
        self.box_resized = arr(lay.box_resized, np.float32, (n, 4))
        self.box = arr(lay.box, np.float32, (n, 4))
        self.valid = arr(lay.valid, np.int32, (n,))
        self.rect = arr(lay.rect, np.int32, (n, 4))
        self.mass = arr(lay.mass, np.int32, (n,))
        self.centroid = arr(lay.centroid, np.int32, (n, 2))
        self.closest = arr(lay.closest, np.int32, (n, kd, 2))
        self.embedding = arr(lay.embedding, np.float32, (n, e))

    def image_slice(self, b):
        return int(self.offset[b]), int(self.offset[b + 1])

    def record(self, b):
        """Self-contained per-frame record (what a rank ships to rank 0 in sharded mode):
        only detections whose scaled box is non-empty (detector_postprocess drops the others)."""
        lo, hi = self.image_slice(b)
        keep = np.nonzero(self.valid[lo:hi])[0]
        idx = lo + keep
        return dict(
            boxes=self.box[idx].copy(), scores=self.score[idx].copy(), classes=self.cls[idx].astype(np.int64),
            centroids=self.centroid[idx].copy(), mass=self.mass[idx].copy(), rects=self.rect[idx].copy(),
            closest=self.closest[idx][:, keep, :].copy(), embeddings=self.embedding[idx].copy(), packed_index=idx.copy())


class TrackRCNN:
    def __init__(self, cfg):
        self.cfg = cfg
        self.device = torch.device(cfg.MODEL.DEVICE)
        self.c4 = is_c4(cfg)
        if self.c4:
            check_c4_supported(cfg)
        self.backbone = _Backbone(self.c4)
        self.training = False
        self._state = None
        self._assoc = None
        self._ctx = None
        self._ctx_key = None
        # live contexts, least recently used first: key -> (ctx, results layout, pinned host block, config struct).  At most
        # cfg.APSE.CONTEXT_CACHE of them (default 1: a size change rebuilds, as TrackPredictor's pre-staging assumes); the
        # current one is mirrored in _ctx / _ctx_key / _lay / _host / _cfg_c
        self._cache = collections.OrderedDict()
        self.contexts_built = 0               # apse_create calls so far (one per frame / image size change, weights, head)
        self._lay = None
        self._host = None
        self._camera = None                   # FramePreprocessor: undistort + gamma fused into preprocess_frames
        self.tail_lane = None                 # None: cfg.APSE.TAIL_LANE; False: contexts without the tail lane (apse_config.tail_lane)
        self.crop_features = bool(cfg.APSE.get("CROP_FEATURES", False))      # apse_set_crop_features of every context
        self._input_tag = None                # frames (objects) the network input was pre-staged with, or None
        self._running_tag = None              # (frames, rpn_levels) whose forward is already enqueued and not yet read, or None
        self.last_results = None
        # set_rpn_head: the six device tensors a live context's RPN head was last replaced with, their version, and the version
        # every live context holds (key -> version; a context is built from _state, which set_rpn_head keeps current)
        self._rpn_head = None
        self._rpn_head_version = 0
        self._ctx_head_version = {}

    # ---- nn.Module-like surface the reference touches
    def to(self, device):
        self.device = torch.device(device)
        return self

    def eval(self):
        self.training = False
        return self

    def load_state_dict(self, sd):
        self._state = {k: v.detach().to(torch.float32).cpu().contiguous() for k, v in sd.items()}
        self._drop_ctx()

    def attach_association_head(self, head):
        """Fuses the tracker's AssociationHead (rcnn_tracker.py:55-57) into the per-frame launch sequence."""
        self._assoc = head
        self._drop_ctx()

    def set_camera(self, preproc):
        """``preproc``: utils.preprocess.FramePreprocessor (camera matrix, distortion, gamma LUT) or None.  The context then runs
        undistort + gamma inside ``apse_preprocess_frames`` (include/apse_hip.h: apse_set_camera)."""
        self._camera = preproc
        for entry in self._cache.values():
            self._push_camera(entry[0])

    def _push_camera(self, ctx):
        lib = _lib.load()
        pc = self._camera
        if pc is None:
            _lib.check(lib.apse_set_camera(ctx, None, None, 0, None, 0, 0), ctx, "apse_set_camera")
            return
        _lib.check(lib.apse_set_camera(ctx, pc.mtx.ctypes.data_as(C.POINTER(C.c_double)), pc.dist.ctypes.data_as(C.POINTER(C.c_double)),
                                       int(pc.dist.size), _lib.ptr(pc.lut_host), int(pc.undistort), int(pc.gamma_correct)),
                   ctx, "apse_set_camera")

    def set_crop_features(self, on):
        """The association features of every context, live, cached or built later: ``roi_pool`` of p2 at the box (False, the
        default ``cfg.APSE.CROP_FEATURES``) or ``roi_align`` of p2 * the detection's mask (apse_set_crop_features; FPN only)."""
        on = bool(on)
        if on and self.c4:
            raise NotImplementedError("crop features read the FPN level p2: not available for C4 (Res5ROIHeads) models")
        self.crop_features = on
        for entry in self._cache.values():
            _lib.check(_lib.load().apse_set_crop_features(entry[0], int(on)), entry[0], "apse_set_crop_features")

    def _drop_ctx(self):
        """Destroys every live context (the current one and the cached ones)."""
        self._input_tag = None
        self._running_tag = None
        self._ctx = None
        self._ctx_key = None
        self._ctx_head_version = {}
        while self._cache:
            _, entry = self._cache.popitem(last=False)
            _lib.load().apse_destroy(entry[0])

    def __del__(self):
        try:
            self._drop_ctx()
        except Exception:
            pass

    # ---- context
    def _ensure_ctx(self, frame_hw, image_hw):
        key = (tuple(frame_hw), tuple(image_hw))
        if self._ctx is not None and self._ctx_key == key:
            return
        keep = int(self.cfg.APSE.get("CONTEXT_CACHE", 1))
        if keep <= 1:
            self._drop_ctx()
        else:
            self._input_tag = None
            self._running_tag = None
            if key in self._cache:
                self._cache.move_to_end(key)
                self._ctx, self._lay, self._host, self._cfg_c = self._cache[key]
                self._ctx_key = key
                return
            self._ctx = None
            self._ctx_key = None
            while len(self._cache) >= keep:
                old, entry = self._cache.popitem(last=False)        # the least recently used one
                self._ctx_head_version.pop(old, None)
                _lib.load().apse_destroy(entry[0])
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.ApseError("the apse_uav hot path needs a ROCm GPU (cfg.MODEL.DEVICE=%s): no CPU fallback" % self.device)
        if self._state is None:
            raise _lib.ApseError("no detector weights loaded")
        if is_c4_state(self._state) != self.c4:
            raise _lib.ApseError("the detector weights are a %s checkpoint but the config is %s (MODEL.ROI_HEADS.NAME = %s)"
                                 % ("C4" if is_c4_state(self._state) else "FPN", "C4" if self.c4 else "FPN",
                                    self.cfg.MODEL.ROI_HEADS.NAME))
        lib = _lib.load()
        cfg = self.cfg
        c = _lib.ConfigArch()
        c.struct_size = C.sizeof(_lib.ConfigArch)
        c.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        c.max_batch = int(cfg.APSE.MAX_BATCH)
        c.frame_h, c.frame_w = int(frame_hw[0]), int(frame_hw[1])
        c.image_h, c.image_w = int(image_hw[0]), int(image_hw[1])
        blocks = blocks_from_state(self._state)
        for i in range(4):
            c.blocks[i] = blocks[i]
        c.num_classes = int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        c.score_thresh = float(cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST)
        c.box_nms = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        c.rpn_nms = float(cfg.MODEL.RPN.NMS_THRESH)
        c.mask_thresh = 0.5
        c.rpn_pre_topk = int(cfg.MODEL.RPN.PRE_NMS_TOPK_TEST)
        c.rpn_post_topk = int(cfg.MODEL.RPN.POST_NMS_TOPK_TEST)
        c.dets_per_image = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        for i in range(3):
            c.pixel_mean[i] = float(cfg.MODEL.PIXEL_MEAN[i])
        roi = self._assoc.roi_size if self._assoc is not None else 10
        c.assoc_roi = roi
        c.embed_dim = self._assoc.embedding_dim if self._assoc is not None else 128
        ph = (c.image_h + 31) // 32 * 32
        pw = (c.image_w + 31) // 32 * 32
        c.assoc_scale = (pw // 4) / float(c.frame_w)          # features.size()[3] / image_size[1]  (rcnn_tracker.py:165)
        depth = 256
        c.arch = 0
        if self.c4:
            c.arch = 1
            depth = 1024
            c.assoc_scale = c4_res4_size(c.image_h, c.image_w)[1] / float(c.frame_w)
        c.compute_dtype = {"f32": 0, "bf16": 1, "f16": 2, "fp16": 2}[str(cfg.APSE.DTYPE)]
        c.storage16 = int(bool(cfg.APSE.get("STORAGE16", True))) if c.compute_dtype else 0
        lane = bool(cfg.APSE.get("TAIL_LANE", True)) if self.tail_lane is None else bool(self.tail_lane)
        if not lane and hasattr(lib, "apse_lane_stats"):
            # the default layout stays the one without the field, and so does a lane-off context on a build from before the lane
            # (loaded through APSE_HIP_LIB for an A/B run: it has no apse_lane_stats, no lane, and refuses the longer layout)
            c, short = _lib.ConfigLane(), c
            C.memmove(C.byref(c), C.byref(short), C.sizeof(_lib.ConfigArch))
            c.struct_size = C.sizeof(_lib.ConfigLane)
            c.tail_lane = -1
        ctx = C.c_void_p()
        _lib.check(lib.apse_create(C.byref(c), C.byref(ctx)), None, "apse_create: " + lib.apse_last_error(None).decode())
        try:
            sd = dict(self._state)
            if self._assoc is not None:
                sd["association.fc.weight"] = self._assoc.fc.weight
                sd["association.fc.bias"] = self._assoc.fc.bias
            else:
                sd["association.fc.weight"] = torch.zeros(c.embed_dim, depth * roi * roi)
                sd["association.fc.bias"] = torch.zeros(c.embed_dim)
            for name, t in sd.items():
                if name.startswith("proposal_generator.anchor_generator") or name in ("pixel_mean", "pixel_std"):
                    continue
                a = np.ascontiguousarray(t.numpy(), dtype=np.float32)
                shp = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(lib.apse_set_weight(ctx, name.encode(), _lib.ptr(a), shp, a.ndim), ctx, "apse_set_weight")
            _lib.check(lib.apse_finalize_weights(ctx), ctx, "apse_finalize_weights")
            hb, hc, hk = resample.precompute_coeffs(c.frame_w, c.image_w)
            vb, vc, vk = resample.precompute_coeffs(c.frame_h, c.image_h)
            _lib.check(lib.apse_set_resize_tables(ctx, _lib.ptr(hb), _lib.ptr(hc), hk, _lib.ptr(vb), _lib.ptr(vc), vk), ctx,
                       "apse_set_resize_tables")
            lay = _lib.ResultsLayout()
            _lib.check(lib.apse_results_describe(ctx, C.byref(lay)), ctx, "apse_results_describe")
            if self.crop_features:
                _lib.check(lib.apse_set_crop_features(ctx, 1), ctx, "apse_set_crop_features")
        except Exception:
            lib.apse_destroy(ctx)
            raise
        self._ctx, self._ctx_key, self._lay = ctx, key, lay
        self.contexts_built += 1
        self._host = torch.empty(lay.bytes, dtype=torch.uint8).pin_memory()
        self._cfg_c = c
        self._cache[key] = (ctx, lay, self._host, c)
        self._ctx_head_version[key] = self._rpn_head_version      # built from _state, which holds the current head
        if self._camera is not None:
            self._push_camera(ctx)

    # ---- stage calls (each enqueues on the current stream)
    def _call(self, fn, *args):
        lib = _lib.load()
        _lib.check(getattr(lib, fn)(self._ctx, *args), self._ctx, fn)

    def preprocess_frames(self, frames, tag=None):
        """frames: uint8 CUDA tensor [B, H, W, 3] (BGR).  Fused PIL-exact resize + normalise + pad.  ``tag``: what the network
        input now holds, for a caller that stages the NEXT frame's input behind the current forward (TrackPredictor._prestage);
        any other write of the input clears it.  Or a ``YuvBatch`` / device ``YuvFrame`` (structures/yuv_frame.py): NV12 / I420
        frames, converted with ``cfg.APSE.YUV_MATRIX`` inside the resize's row staging (``apse_preprocess_frames_yuv``) -- the
        network input holds the bytes of the BGR path on ``utils.preprocess.yuv_to_bgr`` of the same frames."""
        yuv = None
        if isinstance(frames, YuvFrame):
            frames = YuvBatch.of([frames])
        if isinstance(frames, YuvBatch):
            yuv, frames = frames, frames.dev
            if not frames.is_cuda:
                raise _lib.ApseError("preprocess_frames needs device frames: upload a host YuvFrame first (TrackPredictor does)")
            B, H, W, _ = yuv.shape
        else:
            B, H, W, _ = frames.shape
        ih, iw = resample.resize_shortest_edge(H, W, self.cfg.INPUT.MIN_SIZE_TEST, self.cfg.INPUT.MAX_SIZE_TEST)
        self._ensure_ctx((H, W), (ih, iw))
        self._input_tag = None
        self._running_tag = None
        if yuv is not None:
            self._call("apse_preprocess_frames_yuv", _lib.ptr(frames), B, yuv.pitch, FORMATS[yuv.format],
                       matrix_index(self.cfg.APSE.get("YUV_MATRIX", "cv601")), _lib.stream_ptr())
        else:
            self._call("apse_preprocess_frames", _lib.ptr(frames.contiguous()), B, _lib.stream_ptr())
        self._input_tag = tag
        return B

    def preprocess_images(self, images, frame_hw):
        """images: f32 CUDA tensor [B, 3, h, w] already resized (the reference's model input)."""
        B, _, h, w = images.shape
        self._ensure_ctx(frame_hw, (h, w))
        self._input_tag = None
        self._running_tag = None
        self._call("apse_preprocess_images", _lib.ptr(images.contiguous()), B, _lib.stream_ptr())
        return B

    def run(self, batch, given=None, rpn_levels=31):
        self._running_tag = None              # any forward invalidates a speculatively enqueued one (TrackPredictor run-ahead)
        self._refresh_rpn_head()
        s = _lib.stream_ptr()
        self._call("apse_backbone", batch, s)
        if given is None:
            self._call("apse_rpn_levels", batch, int(rpn_levels), s)
            self._call("apse_box_head", batch, s)
        else:
            boxes, classes, counts = given
            boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
            classes = np.ascontiguousarray(classes, np.int32)
            counts = np.ascontiguousarray(counts, np.int32)
            self._call("apse_set_detections", _lib.ptr(boxes), _lib.ptr(classes), None, _lib.ptr(counts), batch, s)
        self._call("apse_mask_tail", batch, s)
        self._call("apse_embed", batch, s)

    def read(self, batch):
        self.read_begin(batch)
        return self.read_end(batch)

    def read_begin(self, batch):
        """Enqueues the D2H of the results block; ``read_end`` waits for THAT copy only, so kernels enqueued in between (the next
        frame's ``preprocess_frames``) run behind the current forward without delaying its results."""
        self._call("apse_read_results_begin", C.c_void_p(self._host.data_ptr()), self._lay.bytes, _lib.stream_ptr())

    def read_end(self, batch):
        self._call("apse_read_results_end", C.c_void_p(self._host.data_ptr()))
        raw = self._host.numpy().tobytes()
        self.last_results = FrameResults(raw, self._lay, batch)
        return self.last_results

    def lane_stats(self):
        """apse_lane_stats: (forwards with their tail on the lane, joins that had to wait, FPN waits not yet complete at enqueue,
        host drains)."""
        out = (C.c_longlong * 4)()
        self._call("apse_lane_stats", C.byref(out))
        return tuple(int(v) for v in out)

    def export_feature(self, name, batch):
        shp = (C.c_int * 3)()
        self._call("apse_feature_shape", name.encode(), C.byref(shp))
        out = torch.empty((batch, shp[0], shp[1], shp[2]), dtype=torch.float32, device=self.device)
        self._call("apse_export_feature", name.encode(), _lib.ptr(out), batch, _lib.stream_ptr())
        return out

    def debug_tensor(self, name, dtype=torch.float32):
        n = C.c_size_t()
        self._call("apse_debug_tensor", name.encode(), None, 0, C.byref(n), _lib.stream_ptr())
        out = torch.empty(n.value // torch.empty((), dtype=dtype).element_size(), dtype=dtype, device=self.device)
        self._call("apse_debug_tensor", name.encode(), _lib.ptr(out), n.value, C.byref(n), _lib.stream_ptr())
        return out

    def backbone_frames(self, frames):
        """Preprocess uint8 CUDA frames [B, H, W, 3] (BGR) and run the backbone only (stem .. FPN): what ``mask_roi_features``
        and ``export_feature`` read afterwards."""
        B = self.preprocess_frames(frames)
        self._running_tag = None
        self._call("apse_backbone", B, _lib.stream_ptr())
        return B

    def backbone_images(self, images, frame_hw):
        """``backbone_frames`` from already-resized f32 CHW images [B, 3, h, w] of frames of size ``frame_hw`` (the training
        loader's augmented images, utils/augment.py)."""
        B = self.preprocess_images(images, frame_hw)
        self._call("apse_backbone", B, _lib.stream_ptr())
        return B

    def mask_roi_features(self, boxes, image=0):
        """ROIAlign 14x14 of ``boxes`` ([n][4] x1,y1,x2,y2 in resized-image pixels, any n) over p2..p5 of image ``image`` of the last
        ``apse_backbone`` run: f32 [n][14][14][256], the values the mask branch pools for the same boxes (apse_mask_roi_features;
        FPN models only -- the mask-head training input, networks/mask_head.py)."""
        if self.c4:
            raise NotImplementedError("mask_roi_features pools p2..p5: not available for C4 (Res5ROIHeads) models")
        b = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).to(self.device).contiguous()
        out = torch.empty((b.shape[0], 14, 14, 256), dtype=torch.float32, device=self.device)
        self._call("apse_mask_roi_features", int(image), _lib.ptr(b), b.shape[0], _lib.ptr(out), _lib.stream_ptr())
        return out

    def box_roi_features(self, boxes, image=0):
        """ROIAlign 7x7 of ``boxes`` ([n][4] x1,y1,x2,y2 in resized-image pixels, any n) over p2..p5 of image ``image`` of the last
        ``apse_backbone`` run: f32 [n][7][7][256], the values the box branch pools for the same boxes (apse_box_roi_features;
        FPN models only -- the box-head training input, networks/box_head.py)."""
        if self.c4:
            raise NotImplementedError("box_roi_features pools p2..p5: not available for C4 (Res5ROIHeads) models")
        b = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).to(self.device).contiguous()
        out = torch.empty((b.shape[0], 7, 7, 256), dtype=torch.float32, device=self.device)
        self._call("apse_box_roi_features", int(image), _lib.ptr(b), b.shape[0], _lib.ptr(out), _lib.stream_ptr())
        return out

    def rpn_proposals(self, frames=None, images=None, frame_hw=None):
        """Preprocess (uint8 CUDA ``frames`` [B, H, W, 3], or already-resized f32 CHW ``images`` [B, 3, h, w] of frames of size
        ``frame_hw``), run ``apse_backbone`` and ``apse_rpn`` only, and return per image the f32 device tensor [count][4] of the
        context's proposals in resized-image pixels (apse_proposals; FPN models only).  The FPN maps stay in place for
        ``box_roi_features``."""
        if self.c4:
            raise NotImplementedError("rpn_proposals feeds box-head training, which pools p2..p5: not available for C4 "
                                      "(Res5ROIHeads) models")
        if (frames is None) == (images is None):
            raise ValueError("rpn_proposals takes frames or images (with frame_hw)")
        B = self.backbone_frames(frames) if frames is not None else self.backbone_images(images, frame_hw)
        return self.proposals_after_backbone(B)

    def proposals_after_backbone(self, batch):
        """``apse_rpn`` on the FPN maps of the last ``backbone_frames`` / ``backbone_images`` run of ``batch`` images, and its
        proposals per image (see ``rpn_proposals``)."""
        if self.c4:
            raise NotImplementedError("rpn_proposals feeds box-head training, which pools p2..p5: not available for C4 "
                                      "(Res5ROIHeads) models")
        B = int(batch)
        self._running_tag = None
        self._refresh_rpn_head()
        s = _lib.stream_ptr()
        self._call("apse_rpn", B, s)
        post = int(self._cfg_c.rpn_post_topk)
        boxes = torch.empty((B, post, 4), dtype=torch.float32, device=self.device)
        counts = torch.empty(B, dtype=torch.int32, device=self.device)
        for b in range(B):
            self._call("apse_proposals", b, _lib.ptr(boxes[b]), C.c_void_p(counts[b:].data_ptr()), s)
        host = counts.cpu()
        return [boxes[b, :int(host[b])] for b in range(B)]

    def set_rpn_head(self, head):
        """Replaces the RPN head of the live contexts with ``head``'s weights (networks.rpn_head.RPNHead, or a mapping of its six
        tensors under the bare or the ``proposal_generator.rpn_head.`` names) without rebuilding them: the joint trainer calls
        this after every optimiser step (apse_set_rpn_head; FPN f32 models only).  The tensors are copied and given a version
        number; the current context is refreshed before its next RPN run, a cached one (cfg.APSE.CONTEXT_CACHE > 1) when it is
        used again, and ``_state`` is updated so that a context built later starts from the same head."""
        from . import rpn_head as rh
        if self.c4:
            raise NotImplementedError("set_rpn_head covers FPN models (p2 .. p6): not available for C4 (Res5ROIHeads) models")
        if self._state is None:
            raise _lib.ApseError("set_rpn_head: the detector has no weights loaded")
        sd = head.state_dict() if hasattr(head, "state_dict") else dict(head)
        ts = []
        for name in rh._names():
            t = sd.get(name, sd.get(rh.PREFIX + name))
            if t is None:
                raise KeyError("set_rpn_head: missing %s" % name)
            t = torch.as_tensor(t).detach()
            if tuple(t.shape) != tuple(rh.SHAPES[name]):
                raise ValueError("set_rpn_head: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(rh.SHAPES[name])))
            ts.append(t.to(self.device, torch.float32, copy=True).contiguous())
        self._rpn_head = ts
        self._rpn_head_version += 1
        for name, t in zip(rh._names(), ts):
            self._state[rh.PREFIX + name] = t.cpu()

    def _refresh_rpn_head(self):
        """Brings the current context's RPN head up to the version of the last ``set_rpn_head``."""
        if self._rpn_head is None or self._ctx is None or self._ctx_head_version.get(self._ctx_key) == self._rpn_head_version:
            return
        self._call("apse_set_rpn_head", *[_lib.ptr(t) for t in self._rpn_head], _lib.stream_ptr())
        self._ctx_head_version[self._ctx_key] = self._rpn_head_version

    def train_proposals(self, batch, pre_topk=None, post_topk=None):
        """The proposals a training step sees, for the ``batch`` images of the last ``backbone_frames`` / ``backbone_images``
        run: the context's RPN convolutions (current head) and find_top_rpn_proposals at the training limits, by default
        cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN per level and POST_NMS_TOPK_TRAIN (2000, 1000; each up to 2048).  Returns per image
        (boxes f32 [count][4] in resized-image pixels, scores f32 [count]) on the device, best first.  The training counterpart
        of ``proposals_after_backbone``; the context's own proposals and results are left alone (apse_rpn_train_proposals; FPN
        f32 models only)."""
        if self.c4:
            raise NotImplementedError("train_proposals feeds box-head training, which pools p2..p5: not available for C4 "
                                      "(Res5ROIHeads) models")
        B = int(batch)
        pre = int(self.cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN if pre_topk is None else pre_topk)
        post = int(self.cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN if post_topk is None else post_topk)
        self._running_tag = None
        self._refresh_rpn_head()
        nbytes = int(_lib.load().apse_rpn_train_proposals_workspace_bytes(B, pre))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        boxes = torch.empty((B, max(post, 1), 4), dtype=torch.float32, device=self.device)
        scores = torch.empty((B, max(post, 1)), dtype=torch.float32, device=self.device)
        counts = torch.empty(B, dtype=torch.int32, device=self.device)
        self._call("apse_rpn_train_proposals", B, pre, post, _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(counts), _lib.ptr(ws),
                   nbytes, _lib.stream_ptr())
        host = counts.cpu()
        return [(boxes[b, :int(host[b])], scores[b, :int(host[b])]) for b in range(B)]

    def rpn_level_shapes(self):
        """The (H, W) of p2 .. p6 of the current context: the five anchor grids (3 anchors per position, (level, y, x, a) order)."""
        if self.c4:
            raise NotImplementedError("RPN-head training covers FPN models (p2 .. p6): not available for C4 (Res5ROIHeads) models")
        out = []
        for name in ("p2", "p3", "p4", "p5", "p6"):
            shp = (C.c_int * 3)()
            self._call("apse_feature_shape", name.encode(), C.byref(shp))
            out.append((int(shp[1]), int(shp[2])))
        return out

    def rpn_anchor_targets(self, gt_boxes, image=0, iou_thresholds=(0.3, 0.7)):
        """RPNOutputs._get_ground_truth without the random draw for the anchors of the current context against ``gt_boxes``
        ([G][4] in resized-image pixels): (labels int32 [A] in {1, 0, -1}, matched_idx int32 [A], matched_iou f32 [A]) on the device
        (apse_rpn_anchor_labels; FPN models only).  The images of a batch share one size and so one set of anchors: ``image`` only
        has to name an image of the batch."""
        from . import rpn_head
        shapes = self.rpn_level_shapes()
        if not 0 <= int(image) < int(self._cfg_c.max_batch):
            raise ValueError("rpn_anchor_targets: image %d is outside the context's batch of %d" % (image, self._cfg_c.max_batch))
        gt = torch.as_tensor(gt_boxes, dtype=torch.float32).reshape(-1, 4).to(self.device)
        return rpn_head.anchor_labels(shapes, gt, iou_thresholds[0], iou_thresholds[1])

    def rpn_patches(self, anchor_idx, image=0):
        """For the anchors ``anchor_idx`` ([S] global indices) of image ``image`` of the last ``apse_backbone`` run: (patches f32
        [S][2304] in rpn_head.conv's (c, kh, kw) input order, slots int32 [S], anchor boxes f32 [S][4], levels int32 [S]) on the device
        (apse_rpn_patches; FPN models with f32 maps only -- the RPN-head training input, networks/rpn_head.py)."""
        if self.c4:
            raise NotImplementedError("rpn_patches reads p2 .. p6: not available for C4 (Res5ROIHeads) models")
        idx = torch.as_tensor(anchor_idx).reshape(-1).to(self.device, torch.int32).contiguous()
        S = idx.shape[0]
        x = torch.empty((S, 2304), dtype=torch.float32, device=self.device)
        slots = torch.empty(S, dtype=torch.int32, device=self.device)
        boxes = torch.empty((S, 4), dtype=torch.float32, device=self.device)
        levels = torch.empty(S, dtype=torch.int32, device=self.device)
        self._call("apse_rpn_patches", int(image), _lib.ptr(idx), S, _lib.ptr(x), _lib.ptr(slots), _lib.ptr(boxes), _lib.ptr(levels),
                   _lib.stream_ptr())
        return x, slots, boxes, levels

    def flops(self, batch, proposals, detections):
        return float(_lib.load().apse_flops(self._ctx, batch, proposals, detections))

    # ---- results -> reference types
    def instances_from(self, res, b, want_masks=True):
        frame_hw = self._ctx_key[0]
        rec = res.record(b)
        n = len(rec["scores"])
        inst = Instances(frame_hw)
        inst.pred_boxes = Boxes(torch.from_numpy(rec["boxes"]))
        inst.scores = torch.from_numpy(rec["scores"])
        inst.pred_classes = torch.from_numpy(rec["classes"])
        masks = MaskList()
        lib = _lib.load()
        rects = np.ascontiguousarray(rec["rects"], np.int32).reshape(n, 4)
        # every window of the frame out of the bit planes with ONE launch into one pooled buffer (views per detection);
        # more than 100 detections cannot occur per image (TEST.DETECTIONS_PER_IMAGE <= 100)
        live = [k for k in range(n) if want_masks and rects[k, 2] > rects[k, 0] and rects[k, 3] > rects[k, 1]]
        pool, offs = None, {}
        if live:
            nw = ((rects[live, 2] + 63) >> 6) - (rects[live, 0] >> 6)
            words = nw.astype(np.int64) * (rects[live, 3] - rects[live, 1])
            off = np.zeros(len(live) + 1, np.int64)
            np.cumsum(words, out=off[1:])
            pool = torch.empty((int(off[-1]),), dtype=torch.int64, device=self.device)
            dets = np.ascontiguousarray(rec["packed_index"][live], np.int32)
            lrects = np.ascontiguousarray(rects[live])
            _lib.check(lib.apse_copy_mask_windows(self._ctx, len(live), _lib.ptr(dets), _lib.ptr(lrects), _lib.ptr(pool),
                                                  _lib.ptr(np.ascontiguousarray(off[:-1])), _lib.stream_ptr()), self._ctx, "apse_copy_mask_windows")
            offs = {k: (int(off[j]), int(off[j + 1]), int(nw[j])) for j, k in enumerate(live)}
        for k in range(n):
            x0, y0, x1, y1 = [int(v) for v in rects[k]]
            bits = None
            if k in offs:
                lo, hi, w = offs[k]
                bits = pool[lo:hi].view(y1 - y0, w)
            masks.append(WindowMask(bits, (x0, y0, x1, y1), frame_hw, rec["centroids"][k], rec["mass"][k]))
        inst.pred_masks = masks
        inst._record = rec
        return inst

    def _inference_images(self, batched_inputs, detected_instances, do_postprocess, rpn_levels):
        """Shared body of ``inference`` (track_rcnn.py:16-58) and ``SelectiveMaskRCNN.scan`` (selective_rcnn.py:27-84):
        the reference's model input -- resized f32 CHW images -- through normalise + pad and the whole launch sequence."""
        assert not self.training
        if not do_postprocess:
            raise NotImplementedError("do_postprocess=False is not on the CSV path and is not provided")
        B = len(batched_inputs)
        imgs = torch.stack([bi["image"].to(torch.float32) for bi in batched_inputs]).to(self.device)
        frame_hw = (int(batched_inputs[0]["height"]), int(batched_inputs[0]["width"]))
        self.preprocess_images(imgs, frame_hw)
        given = None
        if detected_instances is not None:
            assert len(detected_instances) == B
            boxes = np.concatenate([d.pred_boxes.tensor.cpu().numpy().reshape(-1, 4) for d in detected_instances])
            classes = np.concatenate([np.asarray(d.pred_classes.cpu()).reshape(-1) for d in detected_instances])
            counts = np.asarray([len(d) for d in detected_instances], np.int32)
            given = (boxes, classes, counts)
        self.run(B, given, rpn_levels)
        res = self.read(B)
        return [{"instances": self.instances_from(res, b)} for b in range(B)], B

    def inference(self, batched_inputs, detected_instances=None, do_postprocess=True):
        """Same contract as track_rcnn.py:16-58: ``batched_inputs`` = list of
        {"image": f32 CHW tensor (resized, BGR), "height", "width"}; returns
        (list of {"instances": Instances}, feature dict).  ``detected_instances``: list of Instances
        with ``pred_boxes`` (resized-image pixels) and ``pred_classes`` -> box branch skipped."""
        out, B = self._inference_images(batched_inputs, detected_instances, do_postprocess, 31)
        return out, LazyFeatures(self, B)

    def inference_frames(self, frames, given=None, want_masks=True, rpn_levels=31):
        """Fused path: uint8 CUDA frames [B, H, W, 3] -> (list of Instances, feature dict)."""
        B = self.preprocess_frames(frames)
        self.run(B, given, rpn_levels)
        res = self.read(B)
        return [self.instances_from(res, b, want_masks) for b in range(B)], LazyFeatures(self, B)
