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
import numpy as np
import torch

from .. import _lib
from ..structures import device_windows as dw
from ..structures.device_windows import MAX_OBJECTS, SEG_ROWS          # noqa: F401  (tests and tools read them here)
from ..structures.window_mask import WindowMask


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
        dev = dw.default_device()
    return dev


def _value_bytes(hw):
    """Most bytes one value of the compressed string takes for an h x w image: m groups hold -2^(5m-1) <= x < 2^(5m-1)."""
    m = 1
    while (1 << (5 * m - 1)) <= hw:
        m += 1
    return m


def _encode_chunk(arr, windows, keep, n, h, w, compressed):
    """One call's worth (n <= MAX_OBJECTS): the host windows ``arr`` (WIN_DTYPE) and their device copy.  ``keep`` is not read: it
    holds the tensors the windows point into until the copy back has synchronised."""
    lib = _lib.load()
    dev = windows.device
    arr_ptr = _lib.ptr(arr)
    ws_bytes = lib.apse_mots_rle_workspace_bytes(arr_ptr, n, h, w)
    if ws_bytes == 0:
        raise ValueError("a mask window leaves the %d x %d frame, or the frame is outside the library's limits" % (h, w))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    per_value = _value_bytes(h * w)
    cap = 1024                                               # blobs have a run or two per column: 8 ends per column is roomy
    for x0, y0, x1, y1 in arr["rect"].tolist():
        if x1 > x0 and y1 > y0:
            cap += 8 * (x1 - x0 + 1) + 2
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
        _lib.check(lib.apse_mots_bits_to_rle(_lib.ptr(windows), arr_ptr, n, h, w, _lib.ptr(ends), cap,
                                             _lib.ptr(ends_off), _lib.ptr(info), _lib.ptr(ws), ws_bytes, stream), None,
                   "apse_mots_bits_to_rle")
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
        if masks.dtype != torch.uint8 or masks.dim() != 2 or masks.shape[1] != dw.STRUCT_BYTES or \
                masks.device.type != "cuda":
            raise ValueError("a device window array is uint8 [n, %d] on a GPU" % dw.STRUCT_BYTES)
        windows = masks[:n].contiguous()
        host = dw.read_back(windows)
        for k0 in range(0, n, MAX_OBJECTS):
            m = min(MAX_OBJECTS, n - k0)
            res += _encode_chunk(host[k0:k0 + m], windows[k0:k0 + m], None, m, h, w, compressed)
        return res
    masks = list(masks)
    if not masks:
        return res
    dev = device_of(masks)
    if dev is None:
        raise ValueError("encode_masks takes WindowMasks whose bits are on one GPU")
    for k0 in range(0, len(masks), MAX_OBJECTS):
        chunk = masks[k0:k0 + MAX_OBJECTS]
        rects, wprs, ptrs, keep, _ = dw.masks_words(chunk, (h, w), dev, k0, windows_only=True)
        arr = dw.fill_windows(rects, wprs, ptrs)
        res += _encode_chunk(arr, dw.upload(arr, dev), keep, len(chunk), h, w, compressed)
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
    if any(tuple(m.frame_size) != (H, W) for m in masks):
        raise ValueError("masks of different frame sizes in one frame")
    rects, wprs, ptrs, keep, _ = dw.masks_words(masks, (H, W), dev, windows_only=True)
    scores = [float(objects.scores[k]) for k in range(n)]
    rank = dw.score_ranks(scores)
    arr = dw.fill_objects(rects, wprs, ptrs, [rank[s] for s in scores])
    # an object without words gets no room in the pool: the kernel writes nothing for it
    strides, offs, words = dw.pool_layout(rects, [wpr if bits is not None else 0 for wpr, bits in zip(wprs, keep)])
    pool = torch.empty(max(words, 1), dtype=torch.int64, device=dev)
    objs, off_t = dw.upload(arr, dev), torch.from_numpy(offs[:-1]).to(dev)
    stats = torch.empty((n, 4), dtype=torch.int64, device=dev)
    _lib.check(lib.apse_mots_crop_overlaps(_lib.ptr(objs), _lib.ptr(arr), n, H, W, _lib.ptr(pool), words,
                                           _lib.ptr(off_t), _lib.ptr(stats), _lib.stream_ptr()), None,
               "apse_mots_crop_overlaps")
    st = stats.cpu().numpy()
    out, changed = [], []
    for k, m in enumerate(masks):
        if keep[k] is None:
            out.append(WindowMask(None, m.rect, m.frame_size, (-1, -1), 0))
            changed.append(False)
            continue
        before, mass, sx, sy = (int(v) for v in st[k])
        bits = pool[offs[k]:offs[k + 1]].view(-1, int(strides[k]))
        out.append(WindowMask(bits, m.rect, m.frame_size, (sx // mass, sy // mass) if mass else (-1, -1), mass))
        changed.append(mass != before)
    return (out, changed) if with_changed else out
