"""numpy restatements for the bitmask-target tests (DESIGN.md "Bitmask ground truth"); no GPU, no library.

``ref_targets`` is detectron2's ``BitMasks.crop_and_resize`` -- ROIAlign_cpu.cpp with aligned = true, scale 1, sampling_ratio = 0
over the 0 / 1 mask, then ``>= 0.5`` -- with EVERY operation rounded in ``dtype``.  Its float32 form is the contract of
``apse_bitmask_targets`` (byte for byte); its float64 form is the arbiter of how far float32 is from the real-number rule.
The input boxes are float32 values in both forms (float64 takes them exactly).
"""
import numpy as np


def _prep(v, size, dtype):
    """pre_calc_for_bilinear_interpolate along one axis: (valid, low, high, l, h) of coordinates v over ``size`` cells."""
    valid = ~((v < dtype(-1.0)) | (v > dtype(size)) | np.isnan(v))
    v = np.where(valid, v, dtype(0))
    v = np.where(v <= 0, dtype(0), v).astype(dtype)
    lo = v.astype(np.int64)
    top = lo >= size - 1
    hi = np.where(top, size - 1, lo + 1)
    lo = np.where(top, size - 1, lo)
    v = np.where(top, lo.astype(dtype), v).astype(dtype)
    l = (v - lo.astype(dtype)).astype(dtype)
    h = (dtype(1) - l).astype(dtype)
    return valid, lo, hi, l, h


def roi_geometry(roi, mask_size, dtype):
    """(start_w, start_h, bin_w, bin_h, grid_w, grid_h) of one box; the grids are 0 for a non-positive or NaN extent."""
    x1, y1, x2, y2 = (dtype(v) for v in np.asarray(roi, np.float32))
    half = dtype(0.5)
    sw, sh = dtype(x1 - half), dtype(y1 - half)
    rw, rh = dtype(dtype(x2 - half) - sw), dtype(dtype(y2 - half) - sh)
    bw, bh = dtype(rw / dtype(mask_size)), dtype(rh / dtype(mask_size))
    gw = int(np.ceil(bw)) if np.isfinite(bw) and bw > 0 else 0
    gh = int(np.ceil(bh)) if np.isfinite(bh) and bh > 0 else 0
    return sw, sh, bw, bh, gw, gh


def ref_averages(dense, rois, dtype, mask_size=28):
    """The pre-threshold averages, [n][mask_size][mask_size] in ``dtype``: one accumulator per cell, iy outer, ix inner."""
    dense = np.asarray(dense)
    H, W = dense.shape
    m = (dense != 0).astype(dtype)
    rois = np.asarray(rois, np.float32).reshape(-1, 4)
    out = np.zeros((len(rois), mask_size, mask_size), dtype)
    p = np.arange(mask_size).astype(dtype)
    for k, roi in enumerate(rois):
        sw, sh, bw, bh, gw, gh = roi_geometry(roi, mask_size, dtype)
        if gw <= 0 or gh <= 0:
            continue
        iy, ix = np.arange(gh).astype(dtype)[:, None], np.arange(gw).astype(dtype)[:, None]
        y = ((sh + p * bh).astype(dtype)[None, :] + ((iy + dtype(0.5)) * bh).astype(dtype) / dtype(gh)).astype(dtype)      # [gh][ph]
        x = ((sw + p * bw).astype(dtype)[None, :] + ((ix + dtype(0.5)) * bw).astype(dtype) / dtype(gw)).astype(dtype)      # [gw][pw]
        vy, ylo, yhi, ly, hy = (a[:, None, :, None] for a in _prep(y, H, dtype))                # [gh][1][ph][1]
        vx, xlo, xhi, lx, hx = (a[None, :, None, :] for a in _prep(x, W, dtype))                # [1][gw][1][pw]
        w1, w2, w3, w4 = (hy * hx).astype(dtype), (hy * lx).astype(dtype), (ly * hx).astype(dtype), (ly * lx).astype(dtype)
        v1, v2, v3, v4 = m[ylo, xlo], m[ylo, xhi], m[yhi, xlo], m[yhi, xhi]
        val = ((((w1 * v1).astype(dtype) + (w2 * v2).astype(dtype)).astype(dtype) + (w3 * v3).astype(dtype)).astype(dtype)
               + (w4 * v4).astype(dtype)).astype(dtype)
        val = np.where(vy & vx, val, dtype(0)).reshape(gh * gw, mask_size, mask_size)           # sample order: iy outer, ix inner
        acc = np.add.accumulate(val, axis=0, dtype=dtype)[-1]                                   # r[i] = r[i - 1] + a[i], each rounded
        out[k] = (acc / dtype(gh * gw)).astype(dtype)
    return out


def ref_targets(dense, rois, dtype, mask_size=28):
    """uint8 [n][mask_size][mask_size]: 1 where the average is >= 0.5."""
    return (ref_averages(dense, rois, dtype, mask_size) >= dtype(0.5)).astype(np.uint8)


def ref_rows(dense_masks, rois, matched, dtype, mask_size=28):
    """Row r from mask ``matched[r]`` under ``rois[r]``; a ``matched`` outside the list gives a zero row."""
    rois = np.asarray(rois, np.float32).reshape(-1, 4)
    out = np.zeros((len(rois), mask_size, mask_size), np.uint8)
    matched = np.asarray(matched).reshape(-1)
    for obj in np.unique(matched):
        if 0 <= obj < len(dense_masks):
            rows = np.nonzero(matched == obj)[0]
            out[rows] = ref_targets(dense_masks[int(obj)], rois[rows], dtype, mask_size)
    return out


def samples_per_cell(rois, mask_size=28):
    """gh * gw of every box in float32 (0: an empty grid)."""
    return np.array([(lambda g: g[4] * g[5])(roi_geometry(r, mask_size, np.float32)) for r in np.asarray(rois, np.float32).reshape(-1, 4)])


def blobs(rng, h, w, n, empty=()):
    """n seeded dense masks [h][w] (bool): unions of a few ellipses and rectangles with holes; those listed in ``empty`` are blank."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        m = np.zeros((h, w), bool)
        if k not in empty:
            for _ in range(int(rng.integers(1, 4))):
                cy, cx = rng.uniform(0, h), rng.uniform(0, w)
                ry, rx = rng.uniform(2, h / 2.5), rng.uniform(2, w / 2.5)
                if rng.random() < 0.5:
                    m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
                else:
                    m |= (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
            m &= rng.random((h, w)) > 0.03                               # pin holes: the bit taps matter one by one
        out.append(m)
    return out


def random_rois(rng, h, w, n):
    """n seeded float32 boxes that cover the kernel's paths: ordinary boxes (grid 1 .. 3), boxes of 0.9 x the image (grid > 1 in
    both axes), partly and wholly outside the image, beyond (-1, size), zero and negative extents, extents below one pixel."""
    rois = np.zeros((n, 4), np.float64)
    for k in range(n):
        kind = k % 10
        if kind == 0:                                                    # 0.9 x the image
            bw, bh = 0.9 * w, 0.9 * h
            x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
        elif kind == 1:                                                  # partly outside
            bw, bh = rng.uniform(8, w), rng.uniform(8, h)
            x1, y1 = rng.uniform(-bw, w), rng.uniform(-bh, h)
        elif kind == 2:                                                  # wholly outside, beyond (-1, size)
            bw, bh = rng.uniform(4, 40), rng.uniform(4, 40)
            x1, y1 = (w + rng.uniform(2, 30), rng.uniform(0, h)) if rng.random() < 0.5 else (rng.uniform(0, w), -bh - rng.uniform(2, 30))
        elif kind == 3:                                                  # below one pixel
            bw, bh = rng.uniform(0.01, 0.99), rng.uniform(0.01, 0.99)
            x1, y1 = rng.uniform(0, w - 1), rng.uniform(0, h - 1)
        elif kind == 4 and k % 20 == 4:                                  # zero extent
            bw, bh = 0.0, rng.uniform(4, 20)
            x1, y1 = rng.uniform(0, w), rng.uniform(0, h - 20)
        elif kind == 4:                                                  # negative extent
            bw, bh = rng.uniform(4, 20), -rng.uniform(1, 20)
            x1, y1 = rng.uniform(0, w - 20), rng.uniform(20, h)
        else:                                                            # ordinary proposals
            bw, bh = rng.uniform(4, 0.6 * w), rng.uniform(4, 0.6 * h)
            x1, y1 = rng.uniform(-2, w - bw + 2), rng.uniform(-2, h - bh + 2)
        rois[k] = x1, y1, x1 + bw, y1 + bh
    return rois.astype(np.float32)


def gather(dense, xmap, ymap):
    """The remap rule on a dense mask: out[y][x] = dense[ymap[y]][xmap[x]]."""
    return np.asarray(dense)[np.asarray(ymap)[:, None], np.asarray(xmap)[None, :]]


def pillow_map(src, dst, vertical=False):
    """Pillow's own nearest-neighbour map from a resized index ramp (what ``nearest_maps`` must equal)."""
    from PIL import Image
    ramp = np.arange(src, dtype=np.int32)
    if vertical:
        return np.asarray(Image.fromarray(ramp.reshape(src, 1)).resize((1, dst), Image.NEAREST))[:, 0].astype(np.int64)
    return np.asarray(Image.fromarray(ramp.reshape(1, src)).resize((dst, 1), Image.NEAREST))[0].astype(np.int64)
