"""CPU checks of tests/roi_ref.py (the float64 references of the ROI gather kernels) and of the inputs in tests/roi_cases.py.

The references must agree with the oracle's f32 restatements (oracle/ops.py) and with torch's CPU operators inside their own
bounds, integer parts exactly; and every edge-case list the GPU tests feed must contain what its names claim."""
import numpy as np
import torch
import torch.nn.functional as F

import roi_cases as rc
import roi_ref as rr
from oracle import ops


def _maps(dims, seed, n_img=1, C=256):
    rng = np.random.RandomState(seed)
    return [rng.standard_normal((n_img, h, w, C)).astype(np.float32) for h, w in dims]


def _window(maps):
    return lambda lv, img, y0, y1, x0, x1: maps[lv][img, y0:y1, x0:x1]


# ------------------------------------------------------------------------------------------------------ against the oracle
def test_levels_equal_the_oracle():
    boxes = np.concatenate([rc.random_boxes(3, 300, burn=[(1, 256, h, w) for h, w in rc.PYR_A]), rc.align_edge_boxes()[0]])
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    ok = area >= 0                                            # the oracle's cast of a NaN level is undefined
    assert np.array_equal(rr.assign_levels(boxes)[ok], ops.assign_levels(torch.from_numpy(boxes[ok])).numpy())


def test_roi_align_agrees_with_the_oracle():
    """The oracle sums every sample's four taps in f32 (the per-sample form), so its distance from the f64 reference is inside the
    per-sample bound (S + 9) U mag; the tap windows and grids are the integer parts and show as zero / non-zero bins."""
    maps = _maps(rc.PYR_A, 3, C=8)
    feats = [torch.from_numpy(m[0]).permute(2, 0, 1).contiguous() for m in maps]
    boxes = rc.random_boxes(3, 300, burn=[(1, 256, h, w) for h, w in rc.PYR_A])
    for R in (7, 14):
        plan = rr.roi_align_plan(boxes, rc.PYR_A, rr.FPN_SCALES, R)
        res = rr.roi_align_apply(plan, np.zeros(len(boxes), int), _window(maps), R, C=8)
        got = ops.roi_pooler(feats, torch.from_numpy(boxes), R).permute(0, 2, 3, 1).double().numpy()
        n_ops = np.stack([p["ay"]["nvalid"][:, None] * p["ax"]["nvalid"][None, :] + 9 for p in plan])[..., None]
        assert (np.abs(got - res["ref"]) <= n_ops * rr.U * res["mag"]).all()
        # an 84-cell map cannot hold a 17-cell window per bin: the boxes of tests/test_gpu_ops.py all take the separable form (its
        # widest box has windows of 13 cells); the per-sample form is reached through roi_cases.align_edge_boxes
        assert {p["form"] for p in plan} == {"sep"}
        # the same, larger, through the reference's own count
        ok, worst = rr.check(got, dict(res, n_ops=np.maximum(res["n_ops"], n_ops)))
        assert ok, worst


def test_roi_align_integer_parts_equal_the_oracle():
    """The integer parts of ROIAlign against the oracle, exactly.  Grid counts: recomputed the way oracle/ops.py::roi_align_v2
    does (ceil of the f32 roi size over R, in f64; the reference divides in f32).  Tap windows: the oracle pools indicator maps --
    channel c < H is 1 on map row c, channel H + c is 1 on map column c -- so an output element is non-zero exactly where the
    bin puts weight on that row / column; positive terms cannot cancel, and both sides take the fraction from the same f32
    coordinate, so the zero / non-zero patterns must coincide element for element."""
    import math
    C = 48 + 84
    maps = []
    for h, w in rc.PYR_A:
        m = np.zeros((1, h, w, C), np.float32)
        for c in range(h):
            m[0, c, :, c] = 1
        for c in range(w):
            m[0, :, c, 48 + c] = 1
        maps.append(m)
    feats = [torch.from_numpy(m[0]).permute(2, 0, 1).contiguous() for m in maps]
    boxes = rc.random_boxes(3, 300, burn=[(1, 256, h, w) for h, w in rc.PYR_A])
    for R in (7, 14):
        plan = rr.roi_align_plan(boxes, rc.PYR_A, rr.FPN_SCALES, R)
        for b, p in zip(boxes, plan):
            sc = np.float32(rr.FPN_SCALES[p["level"]])
            rw = np.float32((b[2] * sc - np.float32(0.5)) - (b[0] * sc - np.float32(0.5)))
            rh = np.float32((b[3] * sc - np.float32(0.5)) - (b[1] * sc - np.float32(0.5)))
            assert (p["gh"], p["gw"]) == (int(math.ceil(float(rh) / R)), int(math.ceil(float(rw) / R)))
        res = rr.roi_align_apply(plan, np.zeros(len(boxes), int), _window(maps), R, C=C)
        got = ops.roi_pooler(feats, torch.from_numpy(boxes), R).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(got > 0, res["ref"] > 0)
        # and the windows the plan reports are the extents of those patterns (a window may end on a zero-weight tap)
        for i, p in enumerate(plan):
            h = rc.PYR_A[p["level"]][0]
            rows = (got[i, :, :, :h] > 0).any(axis=1)                 # [ph][map row]
            for ph in range(R):
                nz = np.nonzero(rows[ph])[0]
                if nz.size:
                    assert p["ay"]["base"][ph] <= nz[0] and nz[-1] < p["ay"]["base"][ph] + p["ay"]["n"][ph]
                    assert nz[-1] - nz[0] + 1 >= p["ay"]["n"][ph] - 1
                else:
                    assert p["ay"]["n"][ph] == 0 or not (got[i, ph] > 0).any()


def test_roi_pool_equals_the_oracle():
    rng = np.random.RandomState(5)
    feat = rng.standard_normal((2, 48, 84, 16)).astype(np.float32)
    ft = torch.from_numpy(feat).permute(0, 3, 1, 2).contiguous()
    for boxes, scale in ((rc.pool_random_boxes(), 84 / 960.0), (rc.pool_edge_boxes(0.25, 48, 84)[0], 0.25)):
        imgs = np.arange(len(boxes)) % 2
        for R in (1, 7, 10):
            ref, _ = rr.roi_pool(feat, boxes, imgs, scale, R)
            rois5 = torch.cat([torch.from_numpy(imgs).float()[:, None], torch.from_numpy(boxes)], dim=1)
            got = ops.roi_pool(ft, rois5, R, scale).permute(0, 2, 3, 1).double().numpy()
            assert np.array_equal(got, ref)


def test_roi_align_masked_agrees_with_the_oracle():
    rng = np.random.RandomState(7)
    feat = rng.standard_normal((20, 30, 8)).astype(np.float32)
    boxes = np.array([[8., 8., 60., 70.], [10., 10., 10.5, 10.2], [-20., -12., 30., 40.], [90., 50., 140., 95.], [0., 0., 120., 80.],
                      [-40., 20., -8., 60.]], np.float32)
    for SR in (1, 4):
        res = rr.roi_align_masked(feat, np.ones((len(boxes), 20, 30)), boxes, 0.25, 10, SR)
        rois5 = torch.cat([torch.zeros(len(boxes), 1), torch.from_numpy(boxes)], dim=1)
        got = ops.roi_align_legacy(torch.from_numpy(feat).permute(2, 0, 1)[None].contiguous(), rois5, 10, 0.25, SR).double().numpy()
        ok, worst = rr.check(got, res)
        assert ok, worst
        assert res["mag"].max() > 0 and (res["mag"].reshape(len(boxes), -1).max(axis=1) == 0).any()      # one box sees no map


# ------------------------------------------------------------------------------------------------------ against torch
def test_mask_resize_agrees_with_interpolate():
    """Observed: torch's CPU result differs from the two-operation f32 evaluation of the source coordinate
    scale * (dst + .5) - .5 -- it shows a 2^-26 tap at an output whose two-operation coordinate is an integer -- so its
    coordinate is not bit-equal to the reference's.  Why is not established here (a fused multiply-add would do it).  The
    comparison allows any two roundings of that expression: each is within ulp(L) = 2^-23 L of the exact value for a map extent
    L (half an ulp per rounded operation, 1.5 ulp apart at most), and the interpolant of values in [0, 1] has slope <= 1
    along each axis, which adds 1.5 * 2^-23 (H + W) to the reference's bound in this comparison, and in this one only: the GPU
    test keeps the strict bound."""
    rng = np.random.RandomState(11)
    for (H, W), (OH, OW) in (((28, 28), (48, 84)), ((48, 84), (28, 28)), ((17, 23), (5, 40)), ((9, 9), (1, 7)), ((1, 1), (6, 5)),
                             ((30, 40), (30, 40))):
        m = (rng.rand(3, H, W) < 0.5).astype(np.uint8) * rng.randint(1, 255, (3, H, W)).astype(np.uint8)
        res = rr.mask_resize(m, OH, OW)
        got = F.interpolate(torch.from_numpy((m != 0).astype(np.float32))[:, None], size=(OH, OW), mode="bilinear",
                            align_corners=False)[:, 0].double().numpy()
        ok, worst = rr.check(got, res, b=rr.bound(res) + 1.5 * 2.0 ** -23 * (H + W))
        assert ok, ((H, W, OH, OW), worst)


def test_small_operators_agree_with_torch():
    rng = np.random.RandomState(13)
    for D in (64, 100, 128, 256):
        x = rng.standard_normal((9, D)).astype(np.float32)
        x[3] = 0
        res = rr.l2_normalize(x)
        ok, worst = rr.check(F.normalize(torch.from_numpy(x), dim=1).numpy(), res)
        assert ok and not np.isnan(res["ref"]).any() and (res["ref"][3] == 0).all(), worst
        a, b = rng.standard_normal((7, D)).astype(np.float32), rng.standard_normal((5, D)).astype(np.float32)
        res = rr.sqdist(a, b)
        got = (torch.cdist(torch.from_numpy(a).double(), torch.from_numpy(b).double()) ** 2).numpy()
        assert np.abs(got - res["ref"]).max() <= 1e-12 * res["ref"].max()
    for K, N, bias in ((128, 64, True), (1280, 128, False), (2560, 256, True)):
        x, w = rng.standard_normal((5, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
        bv = rng.standard_normal(N).astype(np.float32) if bias else None
        res = rr.assoc_fc(x, w, bv)
        raw = F.linear(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bv) if bias else None)
        ok, worst = rr.check(raw.numpy(), res)
        assert ok, worst
        ok, worst = rr.check(F.normalize(raw, dim=1).numpy(), dict(ref=res["y"]), b=res["y_bound"])
        assert ok, worst


def test_mean_cells_f32_is_inside_its_bound():
    rng = np.random.RandomState(17)
    for cells in (1, 49, 196):
        x = rng.standard_normal((3, cells, 8)).astype(np.float32)
        ok, worst = rr.check(rr.mean_cells_f32(x), rr.mean_cells(x))
        assert ok, worst
    assert np.array_equal(rr.mean_cells_f32(x[:, :1]), x[:, 0])


def test_round16_interval_is_monotone():
    v = np.linspace(-3, 3, 10001)
    for st in (1, 2):
        r = rr.round16(v, st)
        assert (np.diff(r) >= 0).all() and np.abs(r - v).max() <= 2.0 ** (-8 if st == 1 else -11) * 4


# ------------------------------------------------------------------------------------------------------ input coverage
def _edge_plan(R=7):
    boxes, names = rc.align_edge_boxes()
    return boxes, names, rr.roi_align_plan(boxes, rc.PYR_E, rr.FPN_SCALES, R)


def test_edge_list_has_the_16_and_17_cell_windows():
    boxes, names, plan = _edge_plan(7)
    at = {n: p for n, p in zip(names, plan)}
    for ax, (wy, wx) in (("y", (True, False)), ("x", (False, True)), ("yx", (True, True))):
        for cells, form in ((16, "sep"), (17, "direct")):
            p = at["win%d_%s" % (cells, ax)]
            assert p["form"] == form
            assert int(p["win_y"].max()) == (cells if wy else int(p["win_y"].max())) and int(p["win_x"].max()) == (cells if wx else int(p["win_x"].max()))
            if not wy:
                assert p["win_y"].max() < 16
            if not wx:
                assert p["win_x"].max() < 16
    for n in ("big5_a", "big5_b", "big5_thin"):
        assert at[n]["form"] == "direct" and at[n]["level"] == 3
    # R = 14 halves the bins: the same boxes take the separable form there
    assert all(p["form"] == "sep" for n, p in zip(names, rr.roi_align_plan(boxes, rc.PYR_E, rr.FPN_SCALES, 14)) if n.startswith("win"))


def test_edge_list_straddles_every_level_threshold():
    boxes, names = rc.align_edge_boxes()
    lv = rr.assign_levels(boxes) + 2
    k = rr.level_k64(boxes)
    with np.errstate(invalid="ignore"):
        size = np.sqrt((boxes[:, 2].astype(np.float64) - boxes[:, 0]) * (boxes[:, 3].astype(np.float64) - boxes[:, 1]))
    for j, t in enumerate(rc.LEVEL_THRESHOLDS):
        below, above = 2 + j, 3 + j
        for tag, want in (("lo", below), ("hi", above), ("lo_flat", below), ("hi_flat", above)):
            i = names.index("thr%d_%s" % (t, tag))
            assert lv[i] == want and abs(size[i] / t - 1) < 1e-3
            assert abs(k[i] - np.rint(k[i])) >= 1e-5         # a one-ulp difference between log2f implementations cannot decide it
            assert (size[i] < t) == (want == below)
        i = names.index("thr%d_at" % t)
        assert lv[i] == above and size[i] == t and abs(k[i] - above) < 1e-12
    # nothing else in the list sits closer than 1e-5 to a threshold either
    near = np.abs(k - np.rint(k)) < 1e-5
    assert all(names[i].endswith("_at") for i in np.nonzero(near & np.isfinite(k) & (k > 2) & (k < 6))[0])


def test_edge_list_has_empty_rois_and_empty_bins():
    boxes, names, plan = _edge_plan(7)
    at = {n: p for n, p in zip(names, plan)}
    for n in ("zero_w", "zero_h", "zero", "inv_x", "inv_y", "inv_xy", "out_left", "out_right", "out_top", "out_bottom"):
        assert at[n]["empty"], n
    assert at["zero_w"]["gw"] == 0 and at["zero_h"]["gh"] == 0 and at["inv_xy"]["gh"] < 0 and at["inv_xy"]["gw"] < 0
    assert at["out_left"]["gw"] > 0 and at["out_left"]["gh"] > 0          # a sample grid, every sample outside (-1, size)
    for n, axis in (("part_left", "ax"), ("part_top", "ay"), ("part_right", "ax"), ("part_bottom", "ay")):
        cnt = at[n][axis]["n"]
        assert (cnt == 0).any() and (cnt > 0).any(), n
    assert at["frame"]["inside"] is False and at["thr224_at"]["inside"]
    for dims, key in ((rc.PYR_H1, "ay"), (rc.PYR_W1, "ax")):
        p = rr.roi_align_plan(np.array([[0., 0., 512., 512.]], np.float32), dims, rr.FPN_SCALES, 7)[0]
        assert p["level"] == 3 and (p[key]["n"] <= 1).all() and (p[key]["n"] == 1).any()
    for box, lv in rc.FRAME_BOXES:
        p = rr.roi_align_plan(np.array([box], np.float32), rc.PYR_F, rr.FPN_SCALES, 7)[0]
        H, W = rc.PYR_F[lv]
        assert p["level"] == lv and box[2] * rr.FPN_SCALES[lv] == W and box[3] * rr.FPN_SCALES[lv] == H


def test_pool_edge_list_has_half_integer_corners():
    for scale, H, W in ((0.25, 48, 84), (0.0625, 24, 40)):
        boxes, names = rc.pool_edge_boxes(scale, H, W)
        _, _, _, _, scaled = rr.roi_pool_windows(boxes, scale, 7, H, W)
        frac = scaled - np.trunc(scaled)
        assert (frac[names.index("half_pos")] == 0.5).all() and (frac[names.index("half_neg")][:2] == -0.5).all()
        c = rr.round_half_away(scaled)
        assert list(c[names.index("half_pos")]) == [2, 3, 7, 8] and list(c[names.index("half_neg")]) == [-2, -1, 4, 5]
        ref, empty = rr.roi_pool(np.ones((1, H, W, 4), np.float32), boxes, np.zeros(len(boxes), int), scale, 7)
        for n in ("past_left", "past_right", "past_top", "past_bottom"):
            assert empty[names.index(n)].all()
        assert not empty[names.index("whole")].any() and not empty[names.index("cell")].any()


# ------------------------------------------------------------------------------------------------------ the bound has teeth
def test_bound_rejects_a_level_one_off_and_a_shifted_sample():
    """What the frame-level bars absorb: the exact 224 x 224 box pooled one level too fine, and sample coordinates off by 2^-10 of
    a cell, both rounded to f32 as a kernel would return them, fall outside the derived bound on most elements."""
    boxes, names = rc.align_edge_boxes()
    i = names.index("thr224_at")
    maps = _maps(rc.PYR_E, 9, C=8)
    good = rr.roi_align_plan(boxes[i:i + 1], rc.PYR_E, rr.FPN_SCALES, 7)
    res = rr.roi_align_apply(good, [0], _window(maps), 7, C=8)
    ok, worst = rr.check(res["ref"].astype(np.float32), res)
    assert ok and worst < 0.2
    for plan in (rr.roi_align_plan(boxes[i:i + 1], rc.PYR_E, rr.FPN_SCALES, 7, levels=[good[0]["level"] - 1]),
                 rr.roi_align_plan(boxes[i:i + 1] + np.float32(2.0 ** -10 * 16), rc.PYR_E, rr.FPN_SCALES, 7)):
        bad = rr.roi_align_apply(plan, [0], _window(maps), 7, C=8)["ref"].astype(np.float32)
        err = np.abs(bad - res["ref"])
        assert not rr.check(bad, res)[0] and (err > rr.bound(res)).mean() > 0.9
