"""Inputs of the ROI operator tests (tests/test_gpu_roi_ops.py); tests/test_roi_ref.py asserts on the CPU that every edge list
holds what its names claim."""
import numpy as np
import torch

# levels are sized independently (FpnMaps carries H and W per level): p2 wide enough for 17-cell tap windows on a thin box, p5
# large enough for them on both axes
PYR_E = [(160, 160), (40, 40), (40, 40), (128, 128)]
PYR_A = [(48, 84), (24, 42), (12, 21), (6, 11)]           # a 336 x 192 frame, as tests/test_gpu_ops.py
PYR_SMALL = [(12, 21), (6, 11), (3, 6), (2, 3)]           # many rois on little memory
PYR_H1 = [(12, 21), (6, 11), (3, 6), (1, 9)]              # extent 1 on the coarsest level
PYR_W1 = [(12, 21), (6, 11), (3, 6), (9, 1)]
# a frame-sized box per level of a pyramid whose level l map is exactly that box: (box, dims)
FRAME_BOXES = [([0., 0., 100., 108.], 0), ([0., 0., 176., 160.], 1), ([0., 0., 352., 320.], 2), ([0., 0., 704., 640.], 3)]
PYR_F = [(27, 25), (20, 22), (20, 22), (20, 22)]

LEVEL_THRESHOLDS = (112.0, 224.0, 448.0)                   # sqrt(area) at which the level becomes 3, 4, 5
REL = 5e-4                                                 # the neighbours sit this far (relative) from a threshold


def random_boxes(seed, n, fw=336.0, fh=192.0, burn=()):
    """The box distribution of tests/test_gpu_ops.py::test_roi_align_parity, hand-picked rows included.  With seed 3, n 300 and
    burn = that test's four map shapes (drawn from the generator first, as it does) these are its very boxes."""
    g = torch.Generator().manual_seed(seed)
    for shape in burn:
        torch.randn(*shape, generator=g)
    cx = torch.rand(n, generator=g) * (fw - 6)
    cy = torch.rand(n, generator=g) * (fh - 2)
    bw = torch.rand(n, generator=g) ** 2 * (fw - 36) + 1
    bh = torch.rand(n, generator=g) ** 2 * (fh - 12) + 1
    boxes = torch.stack([(cx - bw / 2).clamp(0, fw), (cy - bh / 2).clamp(0, fh), (cx + bw / 2).clamp(0, fw),
                         (cy + bh / 2).clamp(0, fh)], dim=1)
    if n >= 5:
        boxes[0] = torch.tensor([0., 0., fw, fh])
        boxes[1] = torch.tensor([10., 10., 10.5, 10.2])
        boxes[2] = torch.tensor([0., 80., fw, 108.])
        boxes[3] = torch.tensor([-20., -30., 40., 25.])
        boxes[4] = torch.tensor([fw - 36, fh - 22, fw + 64, fh + 68])
    return boxes.numpy().astype(np.float32)


def pool_random_boxes(seed=5, n=40):
    """The boxes of tests/test_gpu_ops.py::test_roi_pool_parity (a 960 x 540 frame on an 84 x 48 map)."""
    g = torch.Generator().manual_seed(seed)
    torch.randn(1, 256, 48, 84, generator=g)
    x1 = torch.rand(n, generator=g) * 800
    y1 = torch.rand(n, generator=g) * 500
    boxes = torch.stack([x1, y1, x1 + torch.rand(n, generator=g) * 300, y1 + torch.rand(n, generator=g) * 150], dim=1)
    boxes[0] = torch.tensor([0., 0., 960., 540.])
    boxes[1] = torch.tensor([955., 530., 960., 540.])
    return boxes.numpy().astype(np.float32)


def align_edge_boxes():
    """(boxes [n][4] f32, names [n]) for PYR_E (a 640 x 640 frame on p2; p5 reaches 4096 px).  Names:
    win16_* / win17_*: the widest tap window of a bin at R = 7 has exactly that many cells on the named axis (y, x or yx);
    thr<T>_lo / _hi / _at: sqrt(area) just below / above / exactly at level threshold T;
    zero_w / zero_h / zero: empty sample grids; inv_*: inverted; out_*: entirely outside the map; part_*: some bins outside;
    frame: the whole frame; big5_*: level-5 boxes in the per-sample form at R = 7."""
    rows = [
        ("win16_x", [3., 300., 423., 324.]), ("win17_x", [3., 300., 424., 324.]),
        ("win16_y", [300., 3., 324., 423.]), ("win17_y", [300., 3., 324., 424.]),
        ("win16_yx", [24., 24., 3384., 3384.]), ("win17_yx", [24., 24., 3392., 3392.]),
    ]
    for t in LEVEL_THRESHOLDS:
        rows += [("thr%d_lo" % t, [16., 16., 16. + t * (1 - REL), 16. + t * (1 - REL)]),
                 ("thr%d_hi" % t, [16., 16., 16. + t * (1 + REL), 16. + t * (1 + REL)]),
                 ("thr%d_at" % t, [16., 16., 16. + t, 16. + t]),
                 ("thr%d_lo_flat" % t, [8., 40., 8. + 2 * t * (1 - REL), 40. + t / 2]),
                 ("thr%d_hi_flat" % t, [8., 40., 8. + 2 * t * (1 + REL), 40. + t / 2])]
    rows += [
        ("zero_w", [50., 20., 50., 90.]), ("zero_h", [20., 50., 90., 50.]), ("zero", [33., 33., 33., 33.]),
        ("inv_x", [90., 20., 50., 60.]), ("inv_y", [20., 90., 60., 50.]), ("inv_xy", [90., 90., 50., 50.]),
        ("out_left", [-300., 100., -40., 200.]), ("out_right", [700., 100., 780., 200.]),
        ("out_top", [100., -300., 200., -40.]), ("out_bottom", [100., 700., 200., 780.]),
        ("part_left", [-60., 10., 30., 60.]), ("part_top", [10., -60., 60., 30.]),
        ("part_right", [600., 300., 700., 380.]), ("part_bottom", [300., 600., 380., 700.]),
        ("frame", [0., 0., 640., 640.]), ("tiny", [10., 10., 10.5, 10.2]), ("corner_cell", [636., 636., 640., 640.]),
        ("big5_a", [100., 60., 3900., 3700.]), ("big5_b", [0., 0., 4096., 4096.]), ("big5_thin", [40., 1000., 4000., 1300.]),
    ]
    return np.array([b for _, b in rows], np.float32), [n for n, _ in rows]


def pool_edge_boxes(scale, H, W):
    """(boxes, names) for roi_pool on a map of H x W at ``scale`` (a power of two, so box * scale is exact): corners on k + .5 and
    -(k + .5), single cells, boxes past every border, the whole map."""
    s = 1.0 / scale
    fw, fh = W * s, H * s
    rows = [
        ("half_pos", [1.5 * s, 2.5 * s, 6.5 * s, 7.5 * s]), ("half_neg", [-1.5 * s, -0.5 * s, 3.5 * s, 4.5 * s]),
        ("neg", [-3. * s, -2. * s, 2. * s, 3. * s]), ("cell", [4. * s, 5. * s, 4. * s, 5. * s]),
        ("cell_last", [(W - 1) * s, (H - 1) * s, (W - 1) * s, (H - 1) * s]), ("whole", [0., 0., fw, fh]),
        ("past_left", [-9. * s, 2. * s, -3. * s, 6. * s]), ("past_right", [fw + 2 * s, 2. * s, fw + 8 * s, 6. * s]),
        ("past_top", [2. * s, -9. * s, 6. * s, -3. * s]), ("past_bottom", [2. * s, fh + 2 * s, 6. * s, fh + 8 * s]),
        ("over_right", [fw - 3 * s, 1. * s, fw + 5 * s, 4. * s]), ("inverted", [7. * s, 7. * s, 2. * s, 2. * s]),
        ("odd", [0.3 * s + 1.7, 0.9 * s + 0.4, 5.2 * s + 0.1, 3.3 * s + 2.2]),
    ]
    return np.array([b for _, b in rows], np.float32), [n for n, _ in rows]
