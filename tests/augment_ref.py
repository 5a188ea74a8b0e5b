"""Numpy oracle of the training augmentation (DESIGN.md "Training augmentation"): detectron2 0.1.2's RandomFlip, RandomBrightness,
RandomSaturation, RandomContrast and RandomLighting in the order of the reference's DatasetMapper, with the dtype of every
operation written out.  The reference ran under numpy 1.18, whose value-based casting keeps ``python float * float32 array`` in
float32 while a float64 ARRAY operand (the grey image, the lighting vector) promotes to float64; the installed numpy promotes
differently, so nothing here relies on promotion: every operand is converted explicitly before it is used.

Each blend ends in ``clip(x, 0, 255)`` and a truncating conversion to uint8 which the next blend reads.
"""
import numpy as np

EIGVEC = np.array([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]], np.float64)
EIGVAL = np.array([0.2175, 0.0188, 0.0045], np.float64)

f32, f64 = np.float32, np.float64


def to_u8(x):
    """clip to 0..255, then truncate toward zero."""
    return np.clip(x, 0, 255).astype(np.uint8)


def lighting_vec(lw):
    """EIGVEC . (lw * EIGVAL) in float64 (never scaled to 0..255: detectron2 does not)."""
    return EIGVEC.dot(np.asarray(lw, f64) * EIGVAL)


def brightness(img, wb):
    assert img.dtype == np.uint8
    x = f32(wb) * img.astype(f32)
    assert x.dtype == f32
    return to_u8(x)


def saturation(img, ws):
    """The grey value takes channel indices 0, 1, 2 as they come (RGB weights on a BGR image: the reference's behaviour)."""
    assert img.dtype == np.uint8
    v = img.astype(f64)
    gray = (v[..., 0] * f64(0.299) + v[..., 1] * f64(0.587)) + v[..., 2] * f64(0.114)
    inner = (f32(ws) * img.astype(f32))
    assert inner.dtype == f32
    x = (f64(1.0 - ws) * gray)[..., None] + inner.astype(f64)
    assert x.dtype == f64
    return to_u8(x)


def image_sum(img):
    """Exact integer sum of every value of the image."""
    return int(img.sum(dtype=np.uint64))


def contrast(img, wc):
    assert img.dtype == np.uint8
    mean = f64(image_sum(img)) / f64(img.size)
    s = f32(f64(1.0 - wc) * mean)
    x = s + f32(wc) * img.astype(f32)
    assert x.dtype == f32
    return to_u8(x)


def lighting(img, lw):
    assert img.dtype == np.uint8
    x = lighting_vec(lw)[None, None, :] + img.astype(f64)
    return to_u8(x)


def augment(img, flip=False, wb=1.0, ws=1.0, wc=1.0, lw=(0.0, 0.0, 0.0)):
    """uint8 [h][w][3] -> (augmented uint8 [h][w][3], S): S is the sum of the image after the saturation step."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    if flip:
        img = img[:, ::-1]
    a = saturation(brightness(img, wb), ws)
    S = image_sum(a)
    return np.ascontiguousarray(lighting(contrast(a, wc), lw)), S


def augment_all_f64(img, flip=False, wb=1.0, ws=1.0, wc=1.0, lw=(0.0, 0.0, 0.0)):
    """The same chain with every operation in float64: NOT the specification; the host test shows where it disagrees."""
    if flip:
        img = img[:, ::-1]
    a = to_u8(f64(wb) * img.astype(f64))
    v = a.astype(f64)
    gray = (v[..., 0] * 0.299 + v[..., 1] * 0.587) + v[..., 2] * 0.114
    b = to_u8((f64(1.0 - ws) * gray)[..., None] + f64(ws) * v)
    mean = f64(image_sum(b)) / f64(b.size)
    c = to_u8(f64(1.0 - wc) * mean + f64(wc) * b.astype(f64))
    return to_u8(lighting_vec(lw)[None, None, :] + c.astype(f64))
