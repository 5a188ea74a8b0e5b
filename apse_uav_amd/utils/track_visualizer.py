"""TrackVisualizer -- counterpart of the reference's dcnn/utils/track_visualizer.py (detectron2's VideoVisualizer + matplotlib).

``draw_instance_predictions(frame, predictions)`` draws the boxes, masks and labels of the tracked objects with the HIP renderer
(csrc/render.hip, ``apse_render_instances``) straight from the mask windows' bit words: no dense mask is built, nothing leaves the
device until ``VisImage.get_image()``.  The picture follows the integer rules of DESIGN.md "Track rendering" (drawing order, label
text, placement and size as in the reference's ``overlay_instances``; a 5x7 bitmap font, no anti-aliasing, one stable colour per
track id).  ``visualize_tracks`` is visualize_uav.py:74-82 without cv2.
"""
import colorsys
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from ..structures import device_windows as dw
from ..structures.yuv_frame import YuvFrame

MAX_ITEMS_PER_IMAGE = 100
_GOLDEN = 0.6180339887498949


class ColorMode:
    """detectron2.utils.visualizer.ColorMode values."""
    IMAGE = 0
    SEGMENTATION = 1
    IMAGE_BW = 2


def frame_constants(H, W):
    """(D, t_box, t_edge): the default font size of the reference's VisImage and the box / mask-edge line widths."""
    D = max(math.floor(math.sqrt(H * W) / 90), 10)
    return D, max(D // 4, 1), max(D // 15, 1)


def label_scale(h, H, W):
    """Glyph scale of a label whose instance is ``h`` pixels tall (track_visualizer.py:184-190), f64."""
    D = frame_constants(H, W)[0]
    size = float(np.clip((float(h) / np.sqrt(float(H) * float(W)) - 0.02) / 0.08 + 1, 1.2, 2)) * 0.5 * D
    return max(1, math.floor(size / 9 + 0.5))


def render_scale_breaks(H, W):
    """f32 table: entry i is the least f32 height at which ``label_scale`` reaches i + 2 (-inf when every height does).  The
    renderer's scale is 1 + the number of entries <= the height, so the device decides it by comparisons alone."""
    top = label_scale(math.inf, H, W)
    breaks = []
    for k in range(2, top + 1):
        if label_scale(-math.inf, H, W) >= k:
            breaks.append(-np.inf)
            continue
        lo, hi = 0, int(np.float32(4.0 * math.sqrt(H * W)).view(np.int32))     # bit patterns of non-negative f32, ordered
        while lo < hi:                                                          # least pattern with scale >= k
            mid = (lo + hi) // 2
            if label_scale(float(np.int32(mid).view(np.float32)), H, W) >= k:
                hi = mid
            else:
                lo = mid + 1
        breaks.append(float(np.int32(lo).view(np.float32)))
    if len(breaks) > 64:
        raise ValueError("frame too large for the label scale table")
    return np.asarray(breaks, np.float32)


def track_color(track_id):
    """Stable RGB colour of a track id: golden-ratio hue, saturation 0.65, value 0.95, rounded to u8."""
    h = (_GOLDEN * int(track_id)) % 1.0
    return tuple(int(math.floor(255.0 * v + 0.5)) for v in colorsys.hsv_to_rgb(h, 0.65, 0.95))


def create_text_labels(classes, scores, ids, class_names):
    """_create_text_labels (track_visualizer.py:15-33): "{name} {score}%\\nid: {id}" with more than one class name, else
    "{score}%"."""
    if scores is None:
        return None
    if classes is not None and class_names is not None and len(class_names) > 1:
        return ["{} {:.0f}%\nid: {}".format(class_names[int(c)], float(s) * 100, i) for c, s, i in zip(classes, scores, ids)]
    return ["{:.0f}%".format(float(s) * 100) for s in scores]


def draw_order(boxes):
    """Descending f32 box area, ties in input order (track_visualizer.py:141, as a stable sort)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    areas = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return np.argsort(-areas, kind="stable")


class VisImage:
    """The rendered frame.  ``tensor``: device u8 [H, W, 3]; ``get_image()``: the host array (pinned buffer + event)."""

    def __init__(self, tensor):
        self.tensor = tensor

    def get_image(self):
        host = torch.empty(self.tensor.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(self.tensor, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.tensor.device))
        done.synchronize()
        return host.numpy()


def _metadata_get(metadata, key):
    if metadata is None:
        return None
    return metadata.get(key, None)


def _column(predictions, name):
    return predictions.get(name) if predictions.has(name) else None


class TrackVisualizer:
    def __init__(self, metadata, instance_mode=ColorMode.IMAGE, device=None):
        if instance_mode == ColorMode.IMAGE_BW:
            raise NotImplementedError("ColorMode.IMAGE_BW (grayscale background) is not implemented by the HIP renderer")
        self.metadata = metadata
        self._instance_mode = instance_mode
        self.device = dw.default_device(device)
        self._uploader = None
        self._breaks = {}
        self.yuv_matrix = "cv601"             # conversion of YuvFrame input (cfg.APSE.YUV_MATRIX of the run that made the frames)

    def _frame(self, frame, inplace):
        """-> (source [1, H, W, 3] device, output [1, H, W, 3] device, uploader slot or None)."""
        if isinstance(frame, YuvFrame):                   # NV12 / I420: drawn on its BGR conversion (a new device frame)
            from .preprocess import yuv_to_bgr
            frame = yuv_to_bgr(frame, self.yuv_matrix)
        if isinstance(frame, np.ndarray):
            if inplace:
                raise ValueError("inplace=True needs a device frame")
            if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
                raise ValueError("frame must be an HxWx3 uint8 array")
            if self._uploader is None:
                from ..engines.track_predictor import FrameUploader
                self._uploader = FrameUploader(self.device, "BGR")          # "BGR": bytes go up as they are
            sl = self._uploader.begin([frame], torch.cuda.current_stream(self.device))
            return sl.dev, torch.empty_like(sl.dev), sl
        if not (frame.is_cuda and frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 3 and frame.is_contiguous()):
            raise ValueError("frame must be a contiguous HxWx3 uint8 device tensor or a host array")
        src = frame.unsqueeze(0)
        return src, (src if inplace else torch.empty_like(src)), None

    def draw_instance_predictions(self, frame, predictions, inplace=False, bgr=False):
        """Draws ``predictions`` (ObjectInstances from RcnnTracker.next_frame, or Instances from TrackPredictor) on ``frame``
        (host HxWx3 uint8 array or device tensor).  ``bgr``: the frame's bytes are B, G, R.  ``inplace`` draws into the device
        frame itself.  Returns a VisImage."""
        src, out, slot = self._frame(frame, inplace)
        H, W = int(src.shape[1]), int(src.shape[2])
        n = len(predictions)
        if n > MAX_ITEMS_PER_IMAGE:
            raise ValueError("at most %d instances per frame (got %d)" % (MAX_ITEMS_PER_IMAGE, n))
        lib = _lib.load()
        stream = torch.cuda.current_stream(self.device)
        items_host, labels, masks_keep = self._items(predictions, n, H, W)
        label_bytes = b"".join(labels)
        if H not in self._breaks.get(W, {}):
            self._breaks.setdefault(W, {})[H] = render_scale_breaks(H, W)
        breaks = self._breaks[W][H]
        dev_blob = ws = None
        items_ptr = labels_ptr = None
        if n:
            isz = C.sizeof(items_host)
            blob = torch.empty(isz + len(label_bytes), dtype=torch.uint8, pin_memory=True)
            C.memmove(blob.data_ptr(), C.addressof(items_host), isz)
            if label_bytes:
                C.memmove(blob.data_ptr() + isz, label_bytes, len(label_bytes))
            dev_blob = blob.to(self.device, non_blocking=True)
            items_ptr = C.c_void_p(dev_blob.data_ptr())
            labels_ptr = C.c_void_p(dev_blob.data_ptr() + isz) if label_bytes else None
        ws_bytes = lib.apse_render_workspace_bytes(H, W, n)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=self.device)
        _lib.check(lib.apse_render_instances(_lib.ptr(src), _lib.ptr(out), 1, H, W, int(bool(bgr)), items_ptr, n, labels_ptr,
                                             len(label_bytes), _lib.ptr(breaks), len(breaks), _lib.ptr(ws), ws_bytes,
                                             C.c_void_p(stream.cuda_stream)), None, "apse_render_instances")
        if slot is not None:
            from ..engines.track_predictor import FrameUploader
            FrameUploader.release(slot, stream)
        del masks_keep                   # device buffers: the caching allocator reuses them in stream order only
        return VisImage(out[0])

    def _items(self, predictions, n, H, W):
        items = (_lib.RenderItem * max(n, 1))()
        if n == 0:
            return items, [], []
        ids = _column(predictions, "ids")
        ids = [int(i) for i in ids] if ids is not None else list(range(1, n + 1))
        pb = predictions.pred_boxes
        if isinstance(pb, (list, tuple)):
            boxes = np.stack([np.asarray(b.tensor.detach().cpu(), np.float32).reshape(-1, 4)[0] for b in pb])
        else:
            boxes = np.asarray(pb.tensor.detach().cpu(), np.float32).reshape(-1, 4)
        scores = _column(predictions, "scores")
        classes = _column(predictions, "pred_classes")
        scores = [float(s) for s in scores] if scores is not None else None
        classes = [int(c) for c in classes] if classes is not None else None
        texts = create_text_labels(classes, scores, ids, _metadata_get(self.metadata, "thing_classes"))
        masks = _column(predictions, "pred_masks")
        order = draw_order(boxes)
        labels, keep, off = [], [], 0
        for j, k in enumerate(order):
            it = items[j]
            it.image = 0
            it.box[:] = [float(v) for v in boxes[k]]
            it.rgb[:] = list(track_color(ids[k])) + [0]
            text = texts[k].encode("ascii", "replace") if texts is not None else b""
            it.label_off, it.label_len = off, len(text)
            labels.append(text)
            off += len(text)
            if masks is None or masks[k] is None:
                continue
            rect, wpr, bits, _ = dw.mask_words(masks[k], k, (H, W), self.device, dense_hw_only=True)
            if bits is not None:                             # an empty mask is left out: the item's bits stay NULL
                keep.append(bits)
                it.bits = bits.data_ptr()
                it.rect[:] = list(rect)
                it.words_per_row = wpr
        return items, labels, keep


def visualize_tracks(frame_bgr, objects, visualizer):
    """visualize_uav.py:74-82: the tracked objects drawn on a BGR frame, returned as a BGR host array (no cv2 round trip: the
    renderer writes the colours in B, G, R byte order)."""
    return visualizer.draw_instance_predictions(frame_bgr, objects, bgr=True).get_image()
