"""Host only: pins tests/trunk16_ref.py and proves that the inputs of tests/test_gpu_trunk16.py can tell right from wrong.

1. The 4x4 / stride-1 convolution of ``s2d_input`` with ``stem_reindex(w7)``, padded 2 above / left and 1 below / right, IS the
   7x7 / stride-2 / pad-3 convolution of the image (exact in float64 on the lattice), for odd and even image sizes.
2. For every case the GPU file runs, the conditions that make its bit comparison meaningful hold.  They are conditions on the
   inputs, not tolerances: sums of |terms| below 2^24 at every accumulation point, integer pre-rounding values, magnitudes below
   60000 (no f16 overflow), at least 20 % of each of t1 / t2 / y / the stem output positive, the final rounding changing at least
   one value in bf16 AND in f16 (bf16: at all three points of the bottleneck), b1 positive on some channel.
3. Every named wrong variant of the reference gives other bits on every case where it can matter.  This is how the GPU tests
   are shown to be able to fail.
"""
import numpy as np
import pytest
import torch

import trunk16_ref as R

DTYPES = pytest.mark.parametrize("dname", ["bf16", "f16"])
LIMIT = float(2 ** 24)


def _is_int(v):
    return bool(torch.equal(v, v.round()))


# ---------------------------------------------------------------------------------------------- 1. the reference itself
@pytest.mark.parametrize("hw", [(14, 22), (13, 21), (14, 21), (13, 22), (1, 1), (2, 3), (7, 7)], ids=R.case_id)
def test_s2d_reindexed_stem_is_the_7x7_stride2_convolution(hw):
    h, w = hw
    r = np.random.RandomState(h * 100 + w)
    img = torch.from_numpy(r.randint(0, 256, (2, 3, h, w)).astype(np.float64)) - torch.tensor(R.LATTICE_MEAN).view(1, 3, 1, 1)
    w7 = torch.from_numpy(r.randint(-2, 3, (64, 3, 7, 7)).astype(np.float64))
    PH, PW = h + (h & 1), w + (w & 1)
    want = R.stem_conv(img, w7)                                       # [(h + 1) / 2] x [(w + 1) / 2] outputs
    assert want.shape[2:] == (PH // 2, PW // 2)
    xs = R.s2d_input(img, PH, PW, torch.bfloat16)                     # every pixel - mean is a bf16 number
    assert torch.equal(xs[..., 12:], torch.zeros_like(xs[..., 12:]))
    got = R.stem_conv_s2d(xs, R.stem_reindex(w7), (2, 1))
    assert torch.equal(got, want)
    # the named wrong forms of the same computation differ (a 1 x 1 image has one pixel in phase (0, 0): no phase to swap)
    if h > 1 or w > 1:
        assert not torch.equal(R.stem_conv_s2d(R.s2d_input(img, PH, PW, torch.bfloat16, swap_phases=True), R.stem_reindex(w7)), want)
    for pad in ((3, 3), (1, 2)):
        assert not torch.equal(R.stem_conv_s2d(xs, R.stem_reindex(w7), pad), want), pad


def test_s2d_input_layout_padding_and_single_rounding():
    img = torch.arange(2 * 3 * 5 * 7, dtype=torch.float64).view(2, 3, 5, 7) + 0.4140625       # 9 significant bits and more: rounds in bf16
    for dt in R.DT.values():
        out = R.s2d_input(img, 8, 8, dt)
        assert out.shape == (2, 4, 4, 16) and out.dtype == dt
        for y in range(8):
            for x in range(8):
                for c in range(3):
                    v = out[1, y >> 1, x >> 1, (2 * (y & 1) + (x & 1)) * 3 + c]
                    want = img[1, c, y, x].to(torch.float32).to(dt) if (y < 5 and x < 7) else torch.zeros((), dtype=dt)
                    assert v.view(torch.int16) == want.view(torch.int16)
        assert int(R.bits(out[..., 12:]).ne(0).sum()) == 0


def test_identity_fold_has_scale_one():
    fold = R.identity_fold(torch.arange(64, dtype=torch.float64))
    var = fold["running_var"].numpy()
    assert var.dtype == np.float32
    scale = fold["weight"].numpy() * (np.float32(1) / np.sqrt(var + np.float32(1e-5), dtype=np.float32))
    assert scale.dtype == np.float32 and np.all(scale == np.float32(1.0))
    assert np.all(fold["bias"].numpy() - fold["running_mean"].numpy() * scale == fold["bias"].numpy())


# ---------------------------------------------------------------------------------------------- 2. + 3. stem cases
def _stem_conditions(inp, dt):
    x, w7, b = inp
    out, pre, act = R.stem_pool(x, w7, b, dt, parts=True)
    sabs = torch.nn.functional.conv2d(x.abs(), w7.abs(), stride=2, padding=3) + b.abs().view(1, -1, 1, 1)
    assert float(sabs.max()) < LIMIT
    assert _is_int(pre) and _is_int(x)
    assert float(pre.abs().max()) < 60000 and float(out.max()) < 60000
    assert torch.equal(R.round16(x, dt), x)                       # the input values are numbers of the storage type
    assert float((out > 0).double().mean()) >= 0.2
    assert int((act != pre.clamp_min(0)).sum()) >= 1               # the one rounding changes something, in bf16 and in f16
    return out, pre, act


@DTYPES
@pytest.mark.parametrize("case", R.STEM_CASES, ids=R.case_id)
def test_stem_case_conditions_and_sensitivity(case, dname):
    dt = R.DT[dname]
    inp = R.stem_inputs(case)
    out, pre, act = _stem_conditions(inp, dt)
    B, IH, IW = case
    assert out.shape == (B, 64, (IH - 1) // 2 + 1, (IW - 1) // 2 + 1)
    # the kernel's route (s2d input, re-indexed filter, one-sided padding) reaches the same pre-activations ...
    xs = R.s2d_input(inp[0], 2 * IH, 2 * IW, dt)
    w4 = R.stem_reindex(inp[1])
    assert torch.equal(R.stem_conv_s2d(xs, w4) + inp[2].view(1, -1, 1, 1), pre)
    # ... and each wrong form of it does not
    assert not torch.equal(R.stem_conv_s2d(R.s2d_input(inp[0], 2 * IH, 2 * IW, dt, swap_phases=True), w4) + inp[2].view(1, -1, 1, 1), pre)
    for pad in ((3, 3), (1, 2)):
        assert not torch.equal(R.stem_conv_s2d(xs, w4, pad) + inp[2].view(1, -1, 1, 1), pre)
    # a pool that takes the cells one past the map (a tile kernel holds values for them) gives other bits: the row above and the
    # column left of the map are in the first window of every case
    assert not torch.equal(R.stem_pool(*inp, dt, variant="pool_virtual"), out)
    # taking them as 0 can never matter behind the ReLU (every cell is >= 0 and the window centre is always inside)
    assert torch.equal(R.stem_pool(*inp, dt, variant="pool_zero"), out)


@DTYPES
def test_stem_border_case(dname):
    dt = R.DT[dname]
    inp = R.stem_border_inputs()
    out, pre, act = R.stem_pool(*inp, dt, parts=True)
    assert float(inp[2].abs().max()) == 0.0
    border = torch.ones_like(pre, dtype=torch.bool)
    border[:, :, 1:-1, 1:-1] = False
    assert float(pre[border].max()) < 0 and float(pre[~border].min()) > 0         # all-negative border, strictly positive interior
    assert _is_int(pre) and float(pre.abs().max()) < 60000 and torch.equal(R.round16(inp[0], dt), inp[0])
    assert float(act[border].max()) == 0.0
    # every output, the border ones included, is the maximum of the interior cells of its window
    assert torch.equal(out, R.interior_pool(act)) and float(out.min()) > 0
    assert int((act != pre.clamp_min(0)).sum()) >= 1
    # a pool that takes the cells one past the map changes border outputs, and only those
    wrong = R.stem_pool(*inp, dt, variant="pool_virtual")
    diff = wrong != out
    assert int(diff[:, :, 0, :].sum()) > 0 and int(diff[:, :, :, 0].sum()) > 0 and int(diff[:, :, 1:, 1:].sum()) == 0


# ---------------------------------------------------------------------------------------------- 2. + 3. bottleneck cases
@DTYPES
@pytest.mark.parametrize("case", R.BNECK_CASES, ids=R.case_id)
def test_bottleneck_case_conditions_and_sensitivity(case, dname):
    dt = R.DT[dname]
    B, H, W, K1, alias = case
    inp = R.bneck_inputs(case)
    x, res, w1, b1 = inp[:4]
    assert (res is x) == alias and x.shape == (B, K1, H, W) and res.shape == (B, 256, H, W)
    y, p = R.bottleneck(*inp, dt, parts=True)
    for s in R.abs_sums_bottleneck(*inp, p["t1"], p["t2"]):
        assert s < LIMIT
    for v in (x, res, p["p1"], p["p2"], p["p3"]):
        assert _is_int(v) and float(v.abs().max()) < 60000
    assert torch.equal(R.round16(x, dt), x) and torch.equal(R.round16(res, dt), res)
    for v in (p["t1"], p["t2"], y):
        assert float((v > 0).double().mean()) >= 0.2
    assert float(b1.max()) > 0
    changed = [int((a != b).sum()) for a, b in ((p["p1"].clamp_min(0), p["t1"]), (p["p2"].clamp_min(0), p["t2"]), (p["p3"], y))]
    if dname == "bf16":
        assert min(changed) >= 1, changed
    else:
        assert changed[2] >= 1, changed
    # ---- wrong variants
    assert not torch.equal(R.bottleneck(*inp, dt, variant="halo_b1"), y)
    assert not torch.equal(R.bottleneck(*inp, dt, variant="res_after_relu"), y)
    if W > 16 or H > 8:                                   # a seam exists
        assert not torch.equal(R.bottleneck(*inp, dt, variant="seam_shift"), y)
    else:
        assert torch.equal(R.bottleneck(*inp, dt, variant="seam_shift"), y)
    if changed[0]:                                        # the t1 rounding is exercised (bf16: always, asserted above)
        assert not torch.equal(R.bottleneck(*inp, dt, variant="t1_round_up"), y)


def test_case_tables_hold_the_tile_edge_shapes():
    assert R.STEM_CASES == [(1, 1, 1), (1, 2, 3), (1, 8, 32), (1, 9, 33), (2, 7, 31), (3, 16, 24), (1, 216, 608)]
    maps = [(1, 1, 1), (1, 8, 16), (1, 9, 17), (2, 13, 21), (3, 7, 50)]
    assert [c[:3] for c in R.BNECK_CASES if c[3:] == (64, False)] == maps + [(1, 216, 304)]
    assert [c[:3] for c in R.BNECK_CASES if c[3:] == (256, True)] == maps
    assert [c[:3] for c in R.BNECK_CASES if c[3:] == (256, False)] == maps
    # tiles: 4 x 16 pooled pixels (stem), 8 x 16 pixels (bottleneck); both grids are capped at 512 blocks
    assert -(-108 // 4) * -(-304 // 16) == 513 and -(-216 // 8) * -(-304 // 16) == 513
    assert 3 * -(-7 // 8) * -(-50 // 16) == 12


@DTYPES
def test_context_inputs_conditions(dname):
    dt = R.DT[dname]
    img, w7, b = R.ctx_inputs()
    h, w = R.CTX_IMAGE
    x = torch.zeros((2, 3, 160, 256), dtype=torch.float64)
    x[:, :, :h, :w] = img - torch.tensor(R.LATTICE_MEAN).view(1, 3, 1, 1)
    out, pre, act = _stem_conditions((x, w7, b), dt)
    assert not torch.equal(img[0], img[1])
    # the padded region convolves zeros: relu(bias) there
    assert torch.equal(pre[:, :, 79, 127], b.view(1, -1).expand(2, -1))
    xs = R.s2d_input(x[:, :, :h, :w], 160, 256, dt)
    assert torch.equal(R.stem_conv_s2d(xs, R.stem_reindex(w7)) + b.view(1, -1, 1, 1), pre)
    assert not torch.equal(R.stem_conv_s2d(R.s2d_input(x[:, :, :h, :w], 160, 256, dt, swap_phases=True), R.stem_reindex(w7)) + b.view(1, -1, 1, 1), pre)
    for pad in ((3, 3), (1, 2)):
        assert not torch.equal(R.stem_conv_s2d(xs, R.stem_reindex(w7), pad) + b.view(1, -1, 1, 1), pre), pad
    assert not torch.equal(R.stem_pool(x, w7, b, dt, variant="pool_virtual"), out)
