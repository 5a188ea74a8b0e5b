"""CPU: the F(2x2, 3x3) matrices of the f32 Winograd kernel and the f32 emulation of its operation order."""
import numpy as np
import torch
import torch.nn.functional as F

from apse_uav_amd import winograd as wg


def test_transform_matrices_give_the_3x3_correlation():
    rng = np.random.default_rng(0)
    for _ in range(20):
        d, g = rng.standard_normal((4, 4)), rng.standard_normal((3, 3))
        y = wg.AT @ ((wg.G @ g @ wg.G.T) * (wg.BT @ d @ wg.BT.T)) @ wg.AT.T
        ref = np.array([[np.sum(d[r:r + 3, s:s + 3] * g) for s in range(2)] for r in range(2)])
        assert np.allclose(y, ref, rtol=0, atol=1e-12)


def test_filter_transform_layout_and_rounding():
    rng = np.random.default_rng(1)
    w = rng.standard_normal((8, 5, 3, 3)).astype(np.float32)
    u = wg.filter_transform(w)
    assert u.shape == (16, 8, 5) and u.dtype == np.float32
    o, c = 3, 4
    ref = (wg.G @ w[o, c].astype(np.float64) @ wg.G.T).reshape(16)
    assert np.array_equal(u[:, o, c], ref.astype(np.float32))       # float64, rounded once


def _emulation_error(H, W, C, relu, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, C, H, W, generator=g)
    w = torch.randn(32, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(32, generator=g) * 0.01
    y64 = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    y32 = F.conv2d(x, w, b, padding=1)
    if relu:
        y64, y32 = F.relu(y64), F.relu(y32)
    yw = wg.emulate(x[0].permute(1, 2, 0).numpy(), w.numpy(), b.numpy(), relu)
    ref = y64[0].permute(1, 2, 0).numpy()
    scale = np.abs(ref).max()
    return np.abs(yw - ref).max() / scale, np.abs(y32[0].permute(1, 2, 0).numpy() - ref).max() / scale


def test_emulation_matches_float64_at_odd_sizes():
    # odd H / W: the last tile row / column is partial (its missing taps are zeros, its extra outputs are dropped)
    for (H, W), relu in (((7, 9), False), ((12, 5), True), ((1, 1), False)):
        ew, ed = _emulation_error(H, W, 64, relu, H * 100 + W)
        assert ew < 2e-6, (H, W, ew)
        assert ew <= 4 * max(ed, 1e-7), (H, W, ew, ed)
