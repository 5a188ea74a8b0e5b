"""Mask geometry helpers -- counterpart of /root/reference/dcnn/utils/mask_utils.py:6-38.

``get_mask_centroid(mask)`` -> (x, y) floats, 1-based, floor of the masked coordinate mean;
``compute_closest_point(mask, the_point)`` -> (x, y) of the first row-major mask pixel with the
smallest f32 squared distance.  Both run on the GPU (HIP kernels behind the C ABI); ``mask`` is
a :class:`WindowMask` (centroid already computed with the paste) or a dense bool CUDA tensor.

The IoU helpers of :41-77 (dead code in the reference: undefined ``self``) are restated from their rule:
``translate_and_crop_mask(mask, (dx, dy))`` moves every pixel by the ``int()``-truncated vector, fills with zeros and crops to
the frame; ``compute_masks_iou(detection_mask, object_mask)`` translates the detection by (object centroid - detection
centroid) and returns f32(|T(det) & obj|) / f32(|T(det)| + |obj| - |T(det) & obj|) as a Python float -- what
``torch.true_divide`` of the two integer sums gives.  ``masks_iou_matrix(det_masks, obj_masks)`` is the same for every pair
with one launch of ``apse_mots_shift_overlaps`` (exact integer counts on the bit windows) and one D2H copy; the division is
host arithmetic.  The reference has no defined result for an empty mask (its centroid is nan and ``int(nan)`` raises): here a
pair with an empty mask on either side has IoU 0.0.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..structures import device_windows as dw
from ..structures.device_windows import MAX_PAIRS          # noqa: F401  (read and patched here by tests and tools)
from ..structures.window_mask import WindowMask


def _dense_u8(mask):
    if isinstance(mask, WindowMask):
        mask = mask.dense()
    if not mask.is_cuda:
        raise _lib.ApseError("mask_utils needs the mask on the GPU (no CPU fallback)")
    return mask.to(torch.uint8).contiguous()


def get_mask_centroid(mask):
    if isinstance(mask, WindowMask):
        return mask.centroid
    m = _dense_u8(mask)
    out = (C.c_int * 3)()
    _lib.check(_lib.load().apse_mask_centroid_dense(_lib.ptr(m), m.shape[0], m.shape[1], C.byref(out), _lib.stream_ptr()),
               None, "apse_mask_centroid_dense")
    if out[2] == 0:
        return (float("nan"), float("nan"))
    return (float(out[0]), float(out[1]))


def compute_closest_point(mask, the_point):
    m = _dense_u8(mask)
    out = (C.c_int * 2)()
    _lib.check(_lib.load().apse_mask_closest_dense(_lib.ptr(m), m.shape[0], m.shape[1], float(the_point[0]),
                                                   float(the_point[1]), C.byref(out), _lib.stream_ptr()),
               None, "apse_mask_closest_dense")
    if out[0] < 0:
        raise RuntimeError("compute_closest_point: empty mask")
    return (float(out[0]), float(out[1]))


# ---------------------------------------------------------------- mask IoU (mask_utils.py:41-77)
def translate_and_crop_mask(mask, translation_vector):
    """Dense bool device tensor [H, W]: pixel (x, y) of ``mask`` lands on (x + int(dx), y + int(dy)); zero fill, cropped to the
    frame.  API compatibility (device slicing); the association uses the bit-window kernel instead."""
    if isinstance(mask, WindowMask):
        mask = mask.dense()
    H, W = (int(v) for v in mask.shape)
    dx, dy = int(translation_vector[0]), int(translation_vector[1])
    out = torch.zeros((H, W), dtype=mask.dtype, device=mask.device)
    if abs(dx) >= W or abs(dy) >= H:
        return out
    out[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = mask[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return out


def _frame_size(mask):
    return tuple(int(v) for v in (mask.frame_size if isinstance(mask, WindowMask) else mask.shape))


def _device_of(masks):
    for m in masks:
        if isinstance(m, WindowMask):
            if m.bits is not None and m.bits.is_cuda:
                return m.bits.device
        elif m.is_cuda:
            return m.device
    return dw.default_device()


def frame_windows(masks, frame, dev):
    """Masks of one frame size -> (apse_mots_window array uint8 [n, 32] on the device, buffers it points into).  A WindowMask
    is used in place; a dense device tensor is packed (structures/device_windows.py).  Nothing is moved from the host."""
    for m in masks:
        if _frame_size(m) != frame:
            raise ValueError("masks of different sizes: %s and %s" % (_frame_size(m), frame))
    rects, wprs, ptrs, *keep = dw.masks_words(masks, frame, dev, host_bits="refuse")
    return dw.upload(dw.fill_windows(rects, wprs, ptrs), dev), keep


def shift_overlaps(windows, quads, frame):
    """windows uint8 [n, 32] (device), quads int32 [P, 4] host rows (a, b, dx, dy) -> int32 [P, 3] host array of |T(a) & b|,
    |T(a)|, |b| (include/apse_hip.h apse_mots_shift_overlaps).  One launch and one D2H copy per MAX_PAIRS pairs."""
    lib = _lib.load()
    quads = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
    P = quads.shape[0]
    out = np.zeros((P, 3), np.int32)
    for p0 in range(0, P, MAX_PAIRS):
        q = torch.from_numpy(quads[p0:p0 + MAX_PAIRS]).to(windows.device)
        res = torch.empty((q.shape[0], 3), dtype=torch.int32, device=windows.device)
        _lib.check(lib.apse_mots_shift_overlaps(_lib.ptr(windows), windows.shape[0], _lib.ptr(q), q.shape[0], frame[0], frame[1],
                                                _lib.ptr(res), _lib.stream_ptr()), None, "apse_mots_shift_overlaps")
        out[p0:p0 + MAX_PAIRS] = res.cpu().numpy()
    return out


def _iou_f32(counts):
    """[P, 3] integer counts -> f32 IoU: both integers rounded to f32, divided in f32 (torch.true_divide); 0 where the union is
    empty."""
    inter = counts[:, 0].astype(np.int64)
    union = counts[:, 1].astype(np.int64) + counts[:, 2].astype(np.int64) - inter
    out = np.zeros(len(counts), np.float32)
    ok = union > 0
    out[ok] = inter[ok].astype(np.float32) / union[ok].astype(np.float32)
    return out


def masks_iou_matrix(det_masks, obj_masks, det_centroids=None):
    """np.float32 [N, O]: entry (n, o) is compute_masks_iou(det_masks[n], obj_masks[o]).  One kernel launch and one D2H copy of
    3 N O ints (per 65536 pairs); a pair with an empty mask on either side is 0.0."""
    det_masks, obj_masks = list(det_masks), list(obj_masks)
    N, O = len(det_masks), len(obj_masks)
    iou = np.zeros((N, O), np.float32)
    if N == 0 or O == 0:
        return iou
    frame = _frame_size(det_masks[0])
    dev = _device_of(det_masks + obj_masks)
    windows, keep = frame_windows(det_masks + obj_masks, frame, dev)
    dc = list(det_centroids) if det_centroids is not None else [get_mask_centroid(m) for m in det_masks]
    oc = [get_mask_centroid(m) for m in obj_masks]
    # (dx, dy) = int(object centroid - detection centroid) for every pair; a nan (an empty mask on either side) leaves 0.0
    shift = np.asarray(oc, np.float64).reshape(1, O, 2) - np.asarray(dc, np.float64).reshape(N, 1, 2)
    ok = ~np.isnan(shift).any(axis=2)
    n_idx, o_idx = np.nonzero(ok)
    if len(n_idx):
        quads = np.stack([n_idx, N + o_idx, np.trunc(shift[ok][:, 0]), np.trunc(shift[ok][:, 1])], axis=1).astype(np.int32)
        iou[ok] = _iou_f32(shift_overlaps(windows, quads, frame))
    del keep
    return iou


def compute_masks_iou(detection_mask, object_mask, detection_centroid=None):
    centroids = None if detection_centroid is None else [detection_centroid]
    return float(masks_iou_matrix([detection_mask], [object_mask], centroids)[0, 0])
