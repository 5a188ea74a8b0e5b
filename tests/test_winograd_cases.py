"""CPU: the reference side of tests/test_gpu_winograd_edges.py, proved on its own (tests/winograd_cases.py).

The lattice argument -- integer inputs make every partial sum of F(2x2, 3x3) an integer below 2^24, so f32 has to reproduce float64
bit for bit -- is checked here on the numpy statement of the kernel's operation order; the a-priori bound is checked against that
emulation on Gaussian data; and the case list is checked to reach every residue of the kernel's XCD block remap.
"""
import numpy as np
import pytest

import winograd_cases as wc

SMALL = [c for c in wc.CASES if wc.emulation_affordable(c)]


@pytest.fixture(scope="module")
def lattice_ref():
    """float64 convolution of every case's lattice inputs (with bias, no ReLU), computed once."""
    out = {}
    for case in wc.CASES:
        x, w, b = wc.lattice(case)
        out[case[0]] = wc.ref64(x, w, b, False)
    return out


@pytest.mark.parametrize("case", wc.CASES, ids=wc.CASE_IDS)
def test_lattice_values_and_partial_sums_are_f32_integers(case, lattice_ref):
    x, w, b = wc.lattice(case)
    assert set(np.unique(x)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(np.unique(w)) <= {-4.0, 0.0, 4.0}
    assert np.array_equal(b, np.round(b)) and np.abs(b).max() <= 8
    u = wc.wg.filter_transform(w)
    assert np.array_equal(u, np.round(u)) and np.abs(u).max() <= 9            # U = G g G^T is integral for g in 4 Z
    m = wc.magnitude(x, w, b)
    assert m.shape == lattice_ref[case[0]].shape and m.max() < 2.0 ** 24, m.max()
    y = lattice_ref[case[0]]
    assert np.array_equal(y, np.round(y))
    assert np.all(np.abs(y) <= m)                                              # and the cap does cap the result


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_emulation_is_exact_on_the_lattice(case, relu, lattice_ref):
    x, w, b = wc.lattice(case)
    y = wc.emulate(x, w, b, relu)
    ref = np.maximum(lattice_ref[case[0]], 0) if relu else lattice_ref[case[0]]
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), ref)
    assert np.array_equal(wc.emulate(x, w, None, relu).astype(np.float64), wc.ref64(x, w, None, relu))


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_emulation_stays_within_the_bound_on_normal_data(case):
    x, w, b = wc.normal(case)
    y64 = wc.ref64(x, w, b, False)
    bd = wc.bound(x, w, b)
    err = np.abs(wc.emulate(x, w, b, False).astype(np.float64) - y64)
    assert bd.shape == y64.shape and np.all(bd > 0)
    assert int((err > bd).sum()) == 0, float((err / bd).max())
    # behind the ReLU as well, and without a bias
    err = np.abs(wc.emulate(x, w, None, True).astype(np.float64) - wc.ref64(x, w, None, True))
    assert int((err > wc.bound(x, w, None)).sum()) == 0


def test_magnitude_is_the_sum_of_absolute_terms():
    """wc.magnitude (and with it wc.bound) against the formula written out with loops, at a map with partial tiles."""
    case = ("t", 2, 3, 5, 8, 64)
    x, w, b = wc.normal(case)
    m = wc.magnitude(x, w, b)
    u = np.abs(wc.wg.filter_transform(w).astype(np.float64))
    for (img, oy, ox, co) in ((0, 0, 0, 0), (1, 2, 4, 63), (0, 1, 3, 17), (1, 2, 0, 5)):
        ty, tx, p, q = oy // 2, ox // 2, oy % 2, ox % 2
        d = np.zeros((4, 4, 8), np.float32)
        for r in range(4):
            for s in range(4):
                iy, ix = 2 * ty - 1 + r, 2 * tx - 1 + s
                if 0 <= iy < 3 and 0 <= ix < 5:
                    d[r, s] = x[img, iy, ix]
        v = np.abs(wc.wg._input_transform(d).astype(np.float64))              # [16][Cin]
        ref = abs(float(b[co]))
        for i in range(4):
            for j in range(4):
                ref += abs(wc.wg.AT[p, i]) * abs(wc.wg.AT[q, j]) * float(np.sum(v[4 * i + j] * u[4 * i + j, co]))
        assert abs(m[img, oy, ox, co] - ref) <= 1e-12 * ref
    assert np.array_equal(wc.bound(x, w, b), (8 + 16) * 2.0 ** -24 * m)
    assert np.allclose(wc.magnitude(x, w, None) + np.abs(b.astype(np.float64)), m, rtol=1e-14, atol=0)


def test_pack_layout_puts_a_k_slice_of_one_xi_in_one_run():
    u = np.arange(16 * 64 * 16, dtype=np.float32).reshape(16, 64, 16)
    p = wc.pack_layout(u).reshape(2, 16, 64, 8)
    for s, xi, co, c in ((0, 0, 0, 0), (1, 15, 63, 7), (1, 4, 17, 2), (0, 9, 40, 5)):
        assert p[s, xi, co, c] == u[xi, co, 8 * s + c]


def test_ref64_is_the_padded_correlation():
    x, w, b = wc.normal(("t", 1, 3, 4, 8, 64))
    y = wc.ref64(x, w, b, False)
    xp = np.zeros((5, 6, 8))
    xp[1:4, 1:5] = x[0]
    for (oy, ox, co) in ((0, 0, 0), (2, 3, 63), (1, 2, 17)):
        ref = float(np.sum(xp[oy:oy + 3, ox:ox + 3, :] * w[co].astype(np.float64).transpose(1, 2, 0)) + b[co])
        assert abs(y[0, oy, ox, co] - ref) < 1e-12


def test_cases_reach_every_residue_of_the_xcd_remap():
    """conv_winograd_f32 deals its nwg = B * ceil(H / 32) * ceil(W / 8) * (Cout / 64) blocks over 8 XCDs with q = nwg >> 3 and
    r = nwg & 7: every r, a grid below 8 blocks, and a grid with q >= 1 and r != 0 have to be among the cases."""
    nwg = {c[0]: c[1] * ((c[2] + 31) // 32) * ((c[3] + 7) // 8) * (c[5] // 64) for c in wc.CASES}
    assert {n & 7 for n in nwg.values()} == set(range(8))
    assert any(n < 8 for n in nwg.values())
    assert any(n >> 3 >= 1 and n & 7 for n in nwg.values())
    assert nwg["block_edges"] == 8 and nwg["batch_n3"] == 9 and nwg["nwg11"] == 11 and nwg["nwg12"] == 12 and nwg["odd"] == 384
    assert [nwg["nwg%d" % k] for k in (3, 4, 5, 6, 7)] == [3, 4, 5, 6, 7]
    # the remap itself, restated: a bijection of 0 .. nwg - 1 for every grid size of the list
    for n in set(nwg.values()):
        q, r = n >> 3, n & 7
        bid = sorted((x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (wg >> 3) for wg in range(n) for x in [wg & 7])
        assert bid == list(range(n)), n
    for c in wc.CASES:
        assert c[4] >= 8 and c[4] & (c[4] - 1) == 0 and c[5] % 64 == 0
