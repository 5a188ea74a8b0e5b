"""float64 restatement of one detection's mask paste (detectron2 detector_postprocess + paste_masks_in_image, CPU branch), the
reference of tests/test_gpu_mask_tail.py.  Pinned to oracle.ops.paste_mask / DetectorOracle.postprocess by
tests/test_paste_ref.py.

What is f32 and what is f64:
  * f32, emulated one numpy float32 operation at a time (no fused multiply-add), in detectron2's order: the box scale
    f32(frame / image) x box, the clip, ``nonempty``, the integer window, and every pixel's grid coordinate
    (x + 0.5 - x0) / (x1 - x0) * 2 - 1 followed by grid_sample's unnormalise ((g + 1) * M - 1) / 2.  detectron2 computes these
    in f32 and so does the kernel (csrc/mask_tail.hip, -ffp-contract=off), so they are reproduced bit for bit.
  * f64: the sigmoid of the f32 logits, the bilinear weights (zero padding outside [0, M)) and the 4-tap blend.

A pixel whose f64 value lies within AMBIG of the threshold is AMBIGUOUS: an f32 implementation may put it on either side, so the
reference reports it and does not decide it.  The blend is separable: the x terms are computed per column, the y terms per row,
and the window is one broadcast.
"""
import numpy as np

AMBIG = 2.0 ** -20

_F = np.float32


def scale_box(box, frame_hw, image_hw):
    """Boxes.scale(f32(W / w), f32(H / h)) + Boxes.clip((H, W)) + nonempty() -> (f32 box [4], valid)."""
    H, W = frame_hw
    sx, sy = _F(W / image_hw[1]), _F(H / image_hw[0])
    b = np.asarray(box, _F)
    x0, y0, x1, y1 = b[0] * sx, b[1] * sy, b[2] * sx, b[3] * sy
    x0, x1 = [min(max(v, _F(0)), _F(W)) for v in (x0, x1)]
    y0, y1 = [min(max(v, _F(0)), _F(H)) for v in (y0, y1)]
    out = np.array([x0, y0, x1, y1], _F)
    return out, bool((x1 - x0) > _F(0) and (y1 - y0) > _F(0))


def paste_window(box_f32, frame_hw):
    """_do_paste_mask(skip_empty=True)'s integer window of one scaled box: floor(x0) - 1 clamped at 0, ceil(x1) + 1 clamped at W."""
    H, W = frame_hw
    x0, y0, x1, y1 = [float(v) for v in box_f32]
    return (int(max(np.floor(x0) - 1, 0)), int(max(np.floor(y0) - 1, 0)),
            int(min(np.ceil(x1) + 1, W)), int(min(np.ceil(y1) + 1, H)))


def grid_index(coords, lo, hi, M):
    """f32 grid_sample source index of pixel coordinates ``coords`` (ints) for the box edge pair (lo, hi)."""
    g = (np.asarray(coords).astype(_F) + _F(0.5) - _F(lo)) / (_F(hi) - _F(lo)) * _F(2) - _F(1)
    assert g.dtype == _F
    return ((g + _F(1)) * _F(M) - _F(1)) / _F(2)


def _taps(idx, M):
    """f64 bilinear taps of f32 source indices: (i0, w0, i1, w1) with the weight of an index outside [0, M) set to 0."""
    i = idx.astype(np.float64)
    f = np.floor(i)
    w1 = i - f
    w0 = 1.0 - w1
    i0 = f.astype(np.int64)
    i1 = i0 + 1
    ok0 = (i0 >= 0) & (i0 < M)
    ok1 = (i1 >= 0) & (i1 < M)
    return np.where(ok0, i0, 0), np.where(ok0, w0, 0.0), np.where(ok1, i1, 0), np.where(ok1, w1, 0.0)


def paste(logits, box, frame_hw, image_hw, thresh=0.5):
    """logits: f32 [M, M] of the detection's class; box: f32 [4] in network-input pixels.

    Returns dict(box = scaled + clipped f32 box, valid, rect = (x0, y0, x1, y1) window, mask = bool [y1-y0, x1-x0],
    value = f64 pre-threshold values of the window, ambiguous = bool of the window).  For an invalid (empty) box the window
    is detectron2's, and mask / value are empty: detector_postprocess drops the detection."""
    lg = np.asarray(logits, _F)
    M = lg.shape[0]
    assert lg.shape == (M, M)
    b, valid = scale_box(box, frame_hw, image_hw)
    rect = paste_window(b, frame_hw)
    x0, y0, x1, y1 = rect
    if not valid or x1 <= x0 or y1 <= y0:
        z = np.zeros((0, 0))
        return dict(box=b, valid=valid, rect=rect, mask=z.astype(bool), value=z, ambiguous=z.astype(bool))
    prob = 1.0 / (1.0 + np.exp(-lg.astype(np.float64)))
    xi0, xw0, xi1, xw1 = _taps(grid_index(np.arange(x0, x1), b[0], b[2], M), M)
    yi0, yw0, yi1, yw1 = _taps(grid_index(np.arange(y0, y1), b[1], b[3], M), M)
    cols = prob[:, xi0] * xw0 + prob[:, xi1] * xw1                  # [M, nx]: the x blend of every mask row
    value = yw0[:, None] * cols[yi0] + yw1[:, None] * cols[yi1]       # [ny, nx]
    t = float(_F(thresh))
    return dict(box=b, valid=valid, rect=rect, mask=value >= t, value=value, ambiguous=np.abs(value - t) <= AMBIG)


def edge_boxes(frame_hw, image_hw):
    """Network-input boxes (f32 [n, 4]) at the places where a paste goes wrong, placed in FRAME pixels and mapped back by the
    f64 scale: borders crossed and missed, empty and sub-pixel boxes, the full frame, 1-px columns and rows, and box edges on
    both sides of 64-column word boundaries and of the right / bottom border (ceil(x1) + 1 below W, equal to W, clamped to W).
    At an exact scale (1600 x 2666 -> 800 x 1333: 2) every listed frame coordinate is hit exactly."""
    H, W = frame_hw
    sx, sy = W / image_hw[1], H / image_hw[0]
    f = [
        (10.25, 20.5, 200.75, 150.125), (W * 0.3 + 0.4, H * 0.4 + 0.7, W * 0.55 + 0.2, H * 0.8 + 0.9),   # fractional interior
        (-30.5, H * 0.2, 90.25, H * 0.5), (W * 0.4, -12.0, W * 0.6, 40.5),                                # crossing left / top
        (W - 70.5, H * 0.3, W + 33.0, H * 0.6), (W * 0.2, H - 25.25, W * 0.35, H + 60.0),                # crossing right / bottom
        (W + 5.0, 10.0, W + 90.0, 60.0), (-80.0, -40.0, -2.0, -1.0), (20.0, H + 1.0, 60.0, H + 9.0),     # outside: invalid
        (100.0, 50.0, 100.0, 90.0), (100.0, 50.0, 140.0, 50.0),                                          # zero width / height
        (W * 0.5 + 0.35, H * 0.5 + 0.35, W * 0.5 + 0.65, H * 0.5 + 0.65), (63.8, 30.1, 64.1, 30.4),      # 0.3 px
        (0.0, 0.0, W, H), (-5.0, -5.0, W + 5.0, H + 5.0),                                                # full frame
        (64.0, 0.0, 65.0, H), (W - 1.0, 0.0, W, H), (0.0, 0.0, 1.0, H), (127.5, 0.0, 128.5, H),          # 1-px columns
        (0.0, H * 0.5, W, H * 0.5 + 1.0),                                                                # 1-px row
        (63.0, 10.0, 127.0, 80.0), (64.0, 12.0, 128.0, 70.0), (65.0, 14.0, 127.0, 90.0),                 # word boundaries
        (62.5, 16.0, 64.0, 60.0), (1.0, 5.0, 63.0, 50.0), (0.5, 5.0, 64.5, 45.0),
        (W - 130.0, 20.0, W - 2.0, 90.0), (W - 129.0, 30.0, W - 1.0, 95.0), (W - 65.0, 40.0, W - 0.5, 70.0),
        (W - 64.0, 50.0, W, 120.0), (W - 1.5, 60.0, W - 0.25, 99.0),
        (5.0, H - 66.0, 300.0, H - 1.0), (5.0, H - 40.0, 120.0, H - 0.5), (7.0, H - 30.0, 90.0, H - 2.0),
    ]
    out = np.array([(x0 / sx, y0 / sy, x1 / sx, y1 / sy) for x0, y0, x1, y1 in f], np.float64)
    return out.astype(np.float32)
