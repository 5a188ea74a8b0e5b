"""Training augmentation on the GPU -- the transforms the reference's ``DatasetMapper`` (dcnn/utils/UAV_utils.py:311-449) applies
to every training image: ``ResizeShortestEdge`` over ``INPUT.MIN_SIZE_TRAIN``, ``RandomFlip``, ``RandomBrightness(0.9, 1.1)``,
``RandomSaturation(0.9, 1.1)``, ``RandomContrast(0.9, 1.1)``, ``RandomLighting(0.2)``, in that order (DESIGN.md "Training
augmentation" has the rules and the type of every operation).

* ``resize_frames``: Pillow's bilinear resize of uint8 frames on the device (``apse_resize_normalize`` with the tables of
  ``utils/resample.py``), uint8 out.
* ``draw_size`` / ``draw_params``: one image's random draws, in the order the loader's generator is consumed.
* ``augment_images``: flip + the four colour blends (``apse_augment_u8``, csrc/augment.hip).
* ``transform_annotations``: detectron2's ``ResizeTransform`` then ``HFlipTransform`` on XYXY boxes and polygons, float64.

There is no host fallback: the kernels run or the call raises.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from . import resample

EIGVEC = np.array([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]], np.float64)
EIGVAL = np.array([0.2175, 0.0188, 0.0045], np.float64)
MAX_BATCH = 64          # APSE_AUGMENT_MAX_BATCH


class AugmentParams:
    """One image's parameters.  A step that is off has its identity value: weight 1.0, ``lighting`` (the three normal draws
    ``lw``) zero; with all of them the image comes back unchanged (mirrored when ``flip``)."""

    def __init__(self, flip=False, brightness=1.0, saturation=1.0, contrast=1.0, lighting=(0.0, 0.0, 0.0)):
        self.flip = bool(flip)
        self.brightness, self.saturation, self.contrast = float(brightness), float(saturation), float(contrast)
        self.lighting = np.asarray(lighting, np.float64).reshape(3).copy()

    def lighting_vec(self):
        """EIGVEC . (lw * EIGVAL) in float64 -- added to the channels as it is (detectron2 never scales it to 0..255)."""
        return EIGVEC.dot(self.lighting * EIGVAL)

    def __repr__(self):
        return "AugmentParams(flip=%r, brightness=%r, saturation=%r, contrast=%r, lighting=%r)" % (
            self.flip, self.brightness, self.saturation, self.contrast, self.lighting.tolist())


def draw_size(rng, min_sizes, sampling="choice"):
    """The short-edge size of one image.  A draw is made only when more than one size is configured: ``"choice"`` one of
    ``min_sizes``, ``"range"`` an integer in [min_sizes[0], min_sizes[1]]."""
    sizes = tuple(int(s) for s in min_sizes)
    if sampling not in ("choice", "range"):
        raise ValueError("MIN_SIZE_TRAIN_SAMPLING must be 'choice' or 'range', not %r" % (sampling,))
    if sampling == "range":
        if len(sizes) != 2:
            raise ValueError("'range' sampling needs two sizes (min, max), got %r" % (sizes,))
        return int(rng.integers(sizes[0], sizes[1] + 1))
    if len(sizes) == 1:
        return sizes[0]
    return sizes[int(rng.integers(0, len(sizes)))]


def draw_params(rng, flip, photometric):
    """One image's draws from ``rng`` (np.random.Generator), after its size: the flip (only when ``flip``: ``random() < 0.5``),
    then -- only when ``photometric`` -- brightness, saturation, contrast = ``uniform(0.9, 1.1)`` each as Python floats and
    ``lw = normal(0, 0.2, 3)``."""
    flipped = bool(rng.random() < 0.5) if flip else False
    if not photometric:
        return AugmentParams(flipped)
    wb, ws, wc = (float(rng.uniform(0.9, 1.1)) for _ in range(3))
    return AugmentParams(flipped, wb, ws, wc, rng.normal(0, 0.2, 3))


class _CParams(C.Structure):
    """apse_augment_params (include/apse_hip.h)."""
    _fields_ = [("flip", C.c_int), ("brightness", C.c_double), ("saturation", C.c_double), ("contrast", C.c_double),
                ("lighting_vec", C.c_double * 3)]


def _check_u8(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] == 3):
        raise ValueError("%s: a uint8 CUDA tensor [B][H][W][3] is required" % what)


_tables = {}


def _resize_tables(n_in, n_out, device):
    key = (n_in, n_out, str(device))
    if key not in _tables:
        if len(_tables) > 64:
            _tables.clear()
        b, c, k = resample.precompute_coeffs(n_in, n_out)
        _tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), k)
    return _tables[key]


def resize_frames(frames_u8_dev, out_h, out_w):
    """uint8 CUDA frames [B][H][W][3] -> uint8 [B][out_h][out_w][3], bit for bit ``PIL.Image.resize((out_w, out_h), BILINEAR)``
    (the two integer passes of ``apse_resize_normalize``; its normalised f32 output goes to a scratch tensor)."""
    _check_u8(frames_u8_dev, "resize_frames")
    src = frames_u8_dev.contiguous()
    B, H, W, _ = src.shape
    out_h, out_w = int(out_h), int(out_w)
    dev = src.device
    hb, hc, hk = _resize_tables(W, out_w, dev)
    vb, vc, vk = _resize_tables(H, out_h, dev)
    ph, pw = (out_h + 31) // 32 * 32, (out_w + 31) // 32 * 32
    tmp = torch.empty((B, H, out_w, 3), dtype=torch.uint8, device=dev)
    scratch = torch.empty((B, ph, pw, 4), dtype=torch.float32, device=dev)
    out = torch.empty((B, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    mean = (C.c_float * 3)(0.0, 0.0, 0.0)
    lib = _lib.load()
    _lib.check(lib.apse_resize_normalize(_lib.ptr(src), _lib.ptr(tmp), _lib.ptr(scratch), _lib.ptr(out), _lib.ptr(hb), _lib.ptr(hc),
                                         hk, _lib.ptr(vb), _lib.ptr(vc), vk, B, H, W, out_h, out_w, ph, pw, C.byref(mean),
                                         _lib.stream_ptr()), None, "apse_resize_normalize")
    return out


def augment_images(images_u8_dev, params, want_u8=True, want_chw=True):
    """uint8 CUDA images [B][h][w][3] (BGR, already resized) + one ``AugmentParams`` per image (or one for all) ->
    (uint8 [B][h][w][3], float32 [B][3][h][w] holding the same integers -- what ``TrackRCNN.preprocess_images`` takes --,
    sums uint64-valued int64 [B]: the sum of each image after the saturation step).  An output that is not wanted is None."""
    _check_u8(images_u8_dev, "augment_images")
    src = images_u8_dev.contiguous()
    B, h, w, _ = src.shape
    if isinstance(params, AugmentParams):
        params = [params] * B
    if len(params) != B:
        raise ValueError("augment_images: %d images but %d parameter sets" % (B, len(params)))
    if not (want_u8 or want_chw):
        raise ValueError("augment_images: no output wanted")
    cp = (_CParams * B)()
    for k, p in enumerate(params):
        cp[k].flip = int(p.flip)
        cp[k].brightness, cp[k].saturation, cp[k].contrast = p.brightness, p.saturation, p.contrast
        v = p.lighting_vec()
        for c in range(3):
            cp[k].lighting_vec[c] = float(v[c])
    dev = src.device
    out_u8 = torch.empty_like(src) if want_u8 else None
    out_chw = torch.empty((B, 3, h, w), dtype=torch.float32, device=dev) if want_chw else None
    sums = torch.empty((B,), dtype=torch.int64, device=dev)
    lib = _lib.load()
    _lib.check(lib.apse_augment_u8(_lib.ptr(src), B, h, w, cp, _lib.ptr(out_u8), _lib.ptr(out_chw), _lib.ptr(sums),
                                   _lib.stream_ptr()), None, "apse_augment_u8")
    return out_u8, out_chw, sums


def transform_annotations(boxes, polygons_per_roi, frame_hw, image_hw, flip):
    """detectron2's ``ResizeTransform`` ((H, W) -> (h, w): x * w / W, y * h / H) then, when ``flip``, ``HFlipTransform``
    (x -> w - x, the box's x0 / x1 swapped) on XYXY boxes [n][4] and per-RoI polygon lists (flat x, y), in float64."""
    from .COCO_utils import flip_annotations
    (H, W), (h, w) = frame_hw, image_hw
    sx, sy = w / W, h / H
    b = np.asarray(boxes, np.float64).reshape(-1, 4) * np.array([sx, sy, sx, sy])
    polys = [[np.array(p, np.float64) * np.tile([sx, sy], len(p) // 2) for p in ps] for ps in polygons_per_roi]
    if flip:
        b, polys = flip_annotations(b, polys, w)
    return b, polys
