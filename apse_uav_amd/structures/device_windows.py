"""The ``apse_mots_window`` / ``apse_mots_object`` arrays every mask entry of the C ABI takes (include/apse_hip.h), built here and
nowhere else.

A caller turns its masks into (rect, words per row, device words) with ``masks_words``, or lays rects out in one pooled
buffer with ``pool_layout``; ``fill_windows`` / ``fill_objects`` write the host structs column by column (numpy structured arrays
in the C layout) and ``upload`` gives the uint8 [n, 32] device tensor the entries read.  The entries that also want the host
copy take ``_lib.ptr`` of the same array.

An empty mask (no bits, or an empty rect) keeps its rect and has a NULL pointer and the words per row its rect needs: every kernel
that reads these structs returns on a NULL pointer or an empty rect, and the host-side limit checks accept the struct.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .window_mask import WindowMask

MAX_OBJECTS = 1024                  # APSE_MOTS_MAX_OBJECTS   (tests/test_rle_ref.py holds the three to the header)
MAX_PAIRS = 65536                   # APSE_MOTS_MAX_PAIRS
SEG_ROWS = 64                       # APSE_MOTS_RLE_SEG_ROWS

WIN_DTYPE = np.dtype([("rect", "<i4", (4,)), ("words_per_row", "<i4"), ("area", "<i4"), ("bits", "<u8")])
OBJ_DTYPE = np.dtype([("rect", "<i4", (4,)), ("words_per_row", "<i4"), ("score", "<f4"), ("bits", "<u8")])
for _dtype, _struct in ((WIN_DTYPE, _lib.MotsWindow), (OBJ_DTYPE, _lib.MotsObject)):
    assert _dtype.itemsize == C.sizeof(_struct)
    assert {k: v[1] for k, v in _dtype.fields.items()} == {k: getattr(_struct, k).offset for k, _ in _struct._fields_}
STRUCT_BYTES = WIN_DTYPE.itemsize   # of both structs


def default_device(device=None):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def words_per_row(rect):
    """64-pixel word columns the rect (x0, y0, x1, y1) touches; 0 for an empty rect."""
    x0, y0, x1, y1 = rect
    return ((x1 + 63) >> 6) - (x0 >> 6) if x1 > x0 and y1 > y0 else 0


def pool_layout(rects, wprs=None):
    """rects [n, 4] -> (words per row int64 [n], word offsets int64 [n + 1], total words) of the windows laid end to end in one
    buffer.  An empty rect takes no words.  ``wprs``: row strides to use instead of what each rect needs (0: no words)."""
    x0, y0, x1, y1 = np.asarray(rects, np.int64).reshape(-1, 4).T
    wpr = ((x1 + 63) >> 6) - (x0 >> 6) if wprs is None else np.asarray(wprs, np.int64)
    wpr = wpr * ((x1 > x0) & (y1 > y0))
    off = np.zeros(len(wpr) + 1, np.int64)
    np.cumsum(wpr * (y1 - y0), out=off[1:])
    return wpr, off, int(off[-1])


def masks_words(masks, frame_hw, dev, first=0, host_bits="move", windows_only=False, dense_hw_only=False):
    """Masks ``first``, ``first + 1``, ... of a call -> (rects, words per row, device addresses of the words (0: an empty mask),
    the contiguous int64 words on ``dev`` or None, the dense tensors that were packed): lists, all but the last one entry per
    mask.  The tensors must outlive the launches that read the addresses.
    A WindowMask's words are used in place; a dense [H, W] tensor is packed with ``apse_render_pack_mask`` and the whole frame is
    its window.  What the callers differ in:
      ``host_bits``      "move": words or a dense mask on another device are copied to ``dev``; "refuse": ApseError unless on a GPU,
                         and words are used where they are
      ``windows_only``   the result writers: TypeError for anything but a WindowMask, and the words must be int64
      ``dense_hw_only``  the visualizer: ValueError unless a dense mask is a tensor of shape ``frame_hw``"""
    refuse = host_bits == "refuse"
    rects, wprs, ptrs, words, packed = [], [], [], [], []
    for k, m in enumerate(masks, first):
        if isinstance(m, WindowMask):
            rect, bits = m.rect, m.bits
            if bits is not None:
                if refuse and not bits.is_cuda:
                    raise _lib.ApseError("mask_utils needs the mask on the GPU (no CPU fallback)")
                rows, shape = rect[3] - rect[1], bits.shape
                if rows <= 0 or rect[2] <= rect[0] or 0 in shape:
                    bits = None
            if bits is None:                                 # an empty mask: its rect, no words
                rects.append(rect)
                wprs.append(words_per_row(rect))
                ptrs.append(0)
                words.append(None)
                continue
            if not refuse and bits.device != dev:            # (a .to() with nothing to do costs more than the comparison)
                bits = bits.to(dev)
            short = len(shape) != 2 or shape[0] < rows
            if windows_only and (short or bits.dtype != torch.int64):
                raise ValueError("mask %d: %s %s bit words for a window of %d rows" % (k, tuple(shape), bits.dtype, rows))
            if short:
                raise ValueError("mask %d: %s bit words for a window of %d rows" % (k, tuple(shape), rows))
            if not bits.is_contiguous():
                bits = bits.contiguous()
        elif windows_only:
            raise TypeError("mask %d is %s: the device writers take WindowMask only" % (k, type(m).__name__))
        else:
            bits = _pack_dense(m, frame_hw, dev, refuse, dense_hw_only, packed)
            rect, shape = (0, 0, frame_hw[1], frame_hw[0]), bits.shape
        rects.append(rect)
        wprs.append(shape[1])
        ptrs.append(bits.data_ptr())
        words.append(bits)
    return rects, wprs, ptrs, words, packed


def _pack_dense(m, frame_hw, dev, refuse, hw_only, packed):
    H, W = frame_hw
    if hw_only and (not torch.is_tensor(m) or tuple(m.shape) != (H, W)):
        raise ValueError("pred_masks entries must be WindowMask or dense [H, W] bool tensors")
    dense = torch.as_tensor(m)
    if refuse and not dense.is_cuda:
        raise _lib.ApseError("mask_utils needs the mask on the GPU (no CPU fallback)")
    dense = dense.to(dev).contiguous()
    if dense.dtype != torch.uint8:                           # bool is 0 / 1 bytes already: no copy
        dense = dense.view(torch.uint8) if dense.dtype == torch.bool else dense.to(torch.uint8)
    bits = torch.empty((H, (W + 63) >> 6), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().apse_render_pack_mask(_lib.ptr(dense), H, W, _lib.ptr(bits), _lib.stream_ptr()), None,
               "apse_render_pack_mask")
    packed.append(dense)
    return bits


def mask_words(m, k, frame_hw, dev, **policy):
    """``masks_words`` of one mask: (rect, words per row, words on ``dev`` or None, the dense tensor that was packed or None)."""
    rects, wprs, _, words, packed = masks_words([m], frame_hw, dev, k, **policy)
    return rects[0], wprs[0], words[0], packed[0] if packed else None


def _fill(dtype, rects, wprs, ptrs):
    arr = np.zeros(len(wprs), dtype)
    if len(arr):
        arr["rect"], arr["words_per_row"], arr["bits"] = rects, wprs, ptrs
    return arr


def fill_windows(rects, wprs, ptrs):
    """Host apse_mots_window [n] (WIN_DTYPE), filled column by column; ``area`` is 0."""
    return _fill(WIN_DTYPE, rects, wprs, ptrs)


def fill_objects(rects, wprs, ptrs, scores):
    """Host apse_mots_object [n] (OBJ_DTYPE), filled column by column."""
    arr = _fill(OBJ_DTYPE, rects, wprs, ptrs)
    arr["score"] = scores
    return arr


def pooled_windows(rects, dev):
    """rects [n, 4] -> (host apse_mots_window [n], pool): one int64 buffer on ``dev`` (not zeroed) and every non-empty rect's
    window in it, end to end; an empty rect is an empty mask."""
    wpr, off, words = pool_layout(rects)
    pool = torch.empty(max(words, 1), dtype=torch.int64, device=dev)
    return fill_windows(rects, wpr, np.where(wpr > 0, pool.data_ptr() + 8 * off[:-1], 0)), pool


def upload(arr, dev):
    """Host struct array -> the uint8 [n, 32] tensor on ``dev`` that the entries take."""
    return torch.from_numpy(arr.view(np.uint8).reshape(len(arr), arr.dtype.itemsize)).to(dev)


def no_windows(dev):
    """The device array of no masks: uint8 [0, 32]."""
    return upload(fill_windows((), (), ()), dev)


def read_back(windows):
    """Device uint8 [n, 32] window array -> a host WIN_DTYPE [n] copy."""
    return windows.cpu().numpy().view(WIN_DTYPE).reshape(-1).copy()


def score_ranks(scores):
    """{score: dense rank as a float}: the device compares these instead of the scores, so its order is exactly that of the
    host's f64 comparisons (equal scores, equal ranks)."""
    return {s: float(r) for r, s in enumerate(sorted(set(scores)))}
