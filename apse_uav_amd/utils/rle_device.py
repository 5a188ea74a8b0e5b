"""Result masks encoded on the GPU: the overlap crop and the COCO RLE of the writers, on the bit windows.

``WindowMask`` words go through csrc/rle_encode.hip (include/apse_hip.h "Result writers") and only the encoded bytes come back:
no dense frame is built on either side.

 * ``encode_masks(masks, image_size, compressed=True)``  the ``rle.encode`` dict of every mask: one launch sequence
   (``apse_mots_bits_to_rle`` then ``apse_mots_rle_pack``) and one device-to-host copy per call, one more round when the first
   capacity guess was short.  ``masks`` is a list of ``WindowMask`` or a device ``apse_mots_window`` array (``split_idmap``'s
   uint8 [n, 32] tensor), whose structs are first read back for the host-side limit checks.
 * ``crop_overlaps(objects)``  the masks ``crop_overlapping_masks`` leaves, as new ``WindowMask`` objects.
 * ``device_of(masks)``  the GPU the writers may use for these masks, or None (then they keep their host code).
Limits: frames as include/apse_hip.h; any number of masks (calls are cut at APSE_MOTS_MAX_OBJECTS).  There is no dense fallback:
a mask that is no ``WindowMask`` is refused.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..structures.window_mask import WindowMask

MAX_OBJECTS = 1024                  # APSE_MOTS_MAX_OBJECTS      (tests/test_rle_ref.py holds both copies to the header)
SEG_ROWS = 64                       # APSE_MOTS_RLE_SEG_ROWS
_WIN_BYTES = C.sizeof(_lib.MotsWindow)


def device_of(masks):
    """The GPU of ``masks`` when every one is a WindowMask whose bits live on that GPU or that has none; None otherwise (or
    when none has bits and no GPU is visible)."""
    dev = None
    for m in masks:
        if not isinstance(m, WindowMask):
            return None
        if m.bits is None:
            continue
        if m.bits.device.type != "cuda" or (dev is not None and m.bits.device != dev):
            return None
        dev = m.bits.device
    if dev is None and torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _to_device(arr, n, dev):
    host = np.frombuffer(bytes(arr), dtype=np.uint8).reshape(n, C.sizeof(arr._type_))
    return torch.from_numpy(host.copy()).to(dev)


def _mask_fields(m, k, dev):
    """rect, words per row and the contiguous device words (or None) of one WindowMask."""
    if not isinstance(m, WindowMask):
        raise TypeError("mask %d is %s: the device writers take WindowMask only" % (k, type(m).__name__))
    x0, y0, x1, y1 = m.rect
    bits = m.bits
    if bits is None or x1 <= x0 or y1 <= y0 or bits.numel() == 0:
        return m.rect, (((x1 + 63) >> 6) - (x0 >> 6)) if x1 > x0 and y1 > y0 else 0, None
    bits = bits.to(dev).contiguous()
    if bits.dim() != 2 or bits.dtype != torch.int64 or bits.shape[0] < y1 - y0:
        raise ValueError("mask %d: %s %s bit words for a window of %d rows" % (k, tuple(bits.shape), bits.dtype, y1 - y0))
    return m.rect, int(bits.shape[1]), bits


def _value_bytes(hw):
    """Most bytes one value of the compressed string takes for an h x w image: m groups hold -2^(5m-1) <= x < 2^(5m-1)."""
    m = 1
    while (1 << (5 * m - 1)) <= hw:
        m += 1
    return m


def _encode_chunk(arr, windows, keep, n, h, w, compressed):
    """One call's worth (n <= MAX_OBJECTS).  ``keep`` is not read: it holds the tensors the windows point into until the copy
    back has synchronised."""
    lib = _lib.load()
    dev = windows.device
    ws_bytes = lib.apse_mots_rle_workspace_bytes(arr, n, h, w)
    if ws_bytes == 0:
        raise ValueError("a mask window leaves the %d x %d frame, or the frame is outside the library's limits" % (h, w))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    per_value = _value_bytes(h * w)
    cap = 1024                                               # blobs have a run or two per column: 8 ends per column is roomy
    for k in range(n):
        r = arr[k].rect
        if r[2] > r[0] and r[3] > r[1]:
            cap += 8 * (r[2] - r[0] + 1) + 2
    stream = _lib.stream_ptr()
    for _ in range(2):
        data_cap = cap * per_value if compressed else cap
        if data_cap >= 2 ** 31:
            raise ValueError("%d run ends do not fit one call" % cap)
        # one buffer, one copy: info [4], offsets [n + 1], then the bytes (or the run ends)
        out = torch.empty(4 + n + 1 + ((data_cap + 3) // 4 if compressed else data_cap), dtype=torch.int32, device=dev)
        info, off, data = out[:4], out[4:4 + n + 1], out[4 + n + 1:]
        if compressed:
            ends = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            ends_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        else:
            ends, ends_off = data, off
        _lib.check(lib.apse_mots_bits_to_rle(_lib.ptr(windows), arr, n, h, w, _lib.ptr(ends), cap, _lib.ptr(ends_off),
                                             _lib.ptr(info), _lib.ptr(ws), ws_bytes, stream), None, "apse_mots_bits_to_rle")
        if compressed:
            pws_bytes = lib.apse_mots_rle_pack_workspace_bytes(cap)
            pws = torch.empty(pws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.apse_mots_rle_pack(_lib.ptr(ends), _lib.ptr(ends_off), n, cap, _lib.ptr(data), data_cap,
                                              _lib.ptr(off), _lib.ptr(info[2:]), _lib.ptr(pws), pws_bytes, stream), None,
                       "apse_mots_rle_pack")
        host = out.cpu().numpy()
        need, ok = int(host[0]), int(host[1])
        if need < 0:
            raise RuntimeError("apse_mots_bits_to_rle: the device windows differ from their host copy")
        if ok and (not compressed or int(host[3])):
            offs = host[4:4 + n + 1]
            body = host[4 + n + 1:]
            if compressed:
                raw = body.view(np.uint8)
                return [{"size": [h, w], "counts": raw[offs[k]:offs[k + 1]].tobytes()} for k in range(n)]
            res = []
            for k in range(n):
                e = body[offs[k]:offs[k + 1]].astype(np.int64)
                res.append({"size": [h, w], "counts": np.diff(e, prepend=0).tolist()})
            return res
        if need >= 2 ** 31 - 1:
            raise ValueError("the masks need more run ends than one call holds")
        cap = max(need, 1)                                   # exact now; per_value bytes per end always hold the string
    raise RuntimeError("apse_mots_bits_to_rle: capacity did not converge")


def encode_masks(masks, image_size, compressed=True, count=None):
    """``rle.encode`` of every mask over an ``image_size`` = (h, w) frame: [{"size": [h, w], "counts": bytes}], or lists of
    run lengths with ``compressed=False``.  ``masks``: WindowMasks, or a device uint8 [n, sizeof(apse_mots_window)] tensor of
    which the first ``count`` (default: all) are encoded; the memory its windows point into must stay alive."""
    h, w = (int(v) for v in image_size)
    res = []
    if isinstance(masks, torch.Tensor):
        n = int(masks.shape[0]) if count is None else int(count)
        if n == 0:
            return res
        if masks.dtype != torch.uint8 or masks.dim() != 2 or masks.shape[1] != _WIN_BYTES or masks.device.type != "cuda":
            raise ValueError("a device window array is uint8 [n, %d] on a GPU" % _WIN_BYTES)
        windows = masks[:n].contiguous()
        host = windows.cpu().numpy()
        for k0 in range(0, n, MAX_OBJECTS):
            m = min(MAX_OBJECTS, n - k0)
            arr = (_lib.MotsWindow * m).from_buffer_copy(host[k0:k0 + m].tobytes())
            res += _encode_chunk(arr, windows[k0:k0 + m], None, m, h, w, compressed)
        return res
    masks = list(masks)
    if not masks:
        return res
    dev = device_of(masks)
    if dev is None:
        raise ValueError("encode_masks takes WindowMasks whose bits are on one GPU")
    for k0 in range(0, len(masks), MAX_OBJECTS):
        chunk = masks[k0:k0 + MAX_OBJECTS]
        n = len(chunk)
        arr = (_lib.MotsWindow * n)()
        keep = []
        for k, m in enumerate(chunk):
            rect, wpr, bits = _mask_fields(m, k0 + k, dev)
            arr[k].rect[:] = list(rect)
            arr[k].words_per_row = wpr
            arr[k].area = 0
            arr[k].bits = bits.data_ptr() if bits is not None else None
            keep.append(bits)
        res += _encode_chunk(arr, _to_device(arr, n, dev), keep, n, h, w, compressed)
    return res


def crop_overlaps(objects, with_changed=False):
    """The masks of ``objects`` (ObjectInstances: ``pred_masks``, ``scores``) after ``crop_overlapping_masks``: a pixel stays with
    the object of highest (score, index) among those that hold it.  New WindowMasks of the same rects with bits, mass and the
    1-based floor centroid (NaN for mass 0); ``objects`` is not changed.  ``with_changed``: also the flags of the masks that
    lost pixels."""
    lib = _lib.load()
    masks = list(objects.pred_masks)
    n = len(masks)
    if n == 0:
        return ([], []) if with_changed else []
    if n > MAX_OBJECTS:
        raise ValueError("%d objects in one frame, more than %d" % (n, MAX_OBJECTS))
    dev = device_of(masks)
    if dev is None:
        raise ValueError("crop_overlaps takes WindowMasks whose bits are on one GPU")
    H, W = (int(v) for v in masks[0].frame_size)
    scores = [float(objects.scores[k]) for k in range(n)]
    rank = {s: float(r) for r, s in enumerate(sorted(set(scores)))}   # exact order of the host's f64 comparisons
    arr = (_lib.MotsObject * n)()
    keep, offs, shapes = [], [], []
    words = 0
    for k, m in enumerate(masks):
        if tuple(m.frame_size) != (H, W):
            raise ValueError("masks of different frame sizes in one frame")
        rect, wpr, bits = _mask_fields(m, k, dev)
        arr[k].rect[:] = list(rect)
        arr[k].words_per_row = wpr
        arr[k].score = rank[scores[k]]
        arr[k].bits = bits.data_ptr() if bits is not None else None
        keep.append(bits)
        offs.append(words)
        shapes.append((rect[3] - rect[1], wpr) if bits is not None else None)
        if bits is not None:
            words += (rect[3] - rect[1]) * wpr
    pool = torch.empty(max(words, 1), dtype=torch.int64, device=dev)
    off_t = torch.from_numpy(np.asarray(offs, np.int64)).to(dev)
    stats = torch.empty((n, 4), dtype=torch.int64, device=dev)
    _lib.check(lib.apse_mots_crop_overlaps(_lib.ptr(_to_device(arr, n, dev)), arr, n, H, W, _lib.ptr(pool), words,
                                           _lib.ptr(off_t), _lib.ptr(stats), _lib.stream_ptr()), None,
               "apse_mots_crop_overlaps")
    st = stats.cpu().numpy()
    del keep
    out, changed = [], []
    for k, m in enumerate(masks):
        if shapes[k] is None:
            out.append(WindowMask(None, m.rect, m.frame_size, (-1, -1), 0))
            changed.append(False)
            continue
        before, mass, sx, sy = (int(v) for v in st[k])
        rows, wpr = shapes[k]
        bits = pool[offs[k]:offs[k] + rows * wpr].view(rows, wpr)
        out.append(WindowMask(bits, m.rect, m.frame_size, (sx // mass, sy // mass) if mass else (-1, -1), mass))
        changed.append(mass != before)
    return (out, changed) if with_changed else out
