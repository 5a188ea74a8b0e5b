"""CPU: the reference side of tests/test_gpu_winograd_split.py (tests/winograd_split_cases.py), proved on its own.

winograd.emulate(split=...) -- per-share accumulators and output transforms, the partial Y summed in split order, then bias and
ReLU -- is compared with float64 on the new case list: exactly on the integer lattice, where every intermediate is an integer
below 2^24 (the cap is computed per case), and within the derived bound on Gaussian data.
"""
import numpy as np
import pytest

import winograd_cases as wc
import winograd_split_cases as sc


@pytest.fixture(scope="module")
def lattice_ref():
    """float64 convolution of every case's lattice inputs (with bias, no ReLU), computed once."""
    out = {}
    for case in sc.CASES:
        x, w, b = wc.lattice(sc.shape(case))
        out[case[0]] = wc.ref64(x, w, b, False)
    return out


def test_split_ranges_are_whole_slices_larger_shares_first():
    assert sc.wg.split_ranges(8, 1) == [(0, 8)]
    assert sc.wg.split_ranges(16, 2) == [(0, 8), (8, 16)]
    assert sc.wg.split_ranges(32, 3) == [(0, 16), (16, 24), (24, 32)]
    assert sc.wg.split_ranges(64, 5) == [(0, 16), (16, 32), (32, 48), (48, 56), (56, 64)]
    assert sc.wg.split_ranges(64, 8) == [(8 * z, 8 * z + 8) for z in range(8)]
    assert sc.wg.split_ranges(256, 3) == [(0, 88), (88, 176), (176, 256)]           # res4.c2: 11 11 10 slices
    assert sc.wg.split_ranges(512, 5) == [(0, 104), (104, 208), (208, 312), (312, 416), (416, 512)]     # res5.c2: 13 13 13 13 12
    with pytest.raises(AssertionError):
        sc.wg.split_ranges(16, 3)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_lattice_cap_keeps_every_intermediate_an_integer_below_2_24(case, lattice_ref):
    """wc.magnitude, the sum of the absolute values of all terms of an output, caps every partial sum in any order and any
    split; U is integral for g in 4 Z, so every intermediate is an integer, and below 2^24 an f32 holds it exactly."""
    x, w, b = wc.lattice(sc.shape(case))
    u = wc.wg.filter_transform(w)
    assert np.array_equal(u, np.round(u)) and np.abs(u).max() <= 9
    cap = float(wc.magnitude(x, w, b).max())
    print(case[0], "cap", cap)
    assert cap < 2.0 ** 24
    y = lattice_ref[case[0]]
    assert np.array_equal(y, np.round(y)) and np.all(np.abs(y) <= wc.magnitude(x, w, b))


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_split_emulation_is_exact_on_the_lattice(case, relu, lattice_ref):
    x, w, b = wc.lattice(sc.shape(case))
    y = sc.emulate(x, w, b, relu, case[6])
    ref = np.maximum(lattice_ref[case[0]], 0) if relu else lattice_ref[case[0]]
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), ref)
    assert np.array_equal(sc.emulate(x, w, None, relu, case[6]).astype(np.float64), wc.ref64(x, w, None, relu))


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_split_emulation_stays_within_the_bound_on_normal_data(case):
    x, w, b = wc.normal(sc.shape(case))
    y64 = wc.ref64(x, w, b, False)
    bd = sc.bound(x, w, b, case[6])
    err = np.abs(sc.emulate(x, w, b, False, case[6]).astype(np.float64) - y64)
    assert bd.shape == y64.shape and np.all(bd > 0)
    assert int((err > bd).sum()) == 0, float((err / bd).max())
    assert np.array_equal(bd, (case[4] + 16 + case[6]) * 2.0 ** -24 * wc.magnitude(x, w, b)) and np.all(bd > wc.bound(x, w, b))


def test_split_one_is_the_unsplit_emulation():
    x, w, b = wc.normal(("t", 1, 5, 7, 16, 64))
    assert sc.emulate(x, w, b, True, 1).tobytes() == wc.emulate(x, w, b, True).tobytes()


def test_cases_cover_what_the_kernel_can_get_wrong():
    """Cin 8 unsplit in both geometries; one slice per share; uneven shares; splits 5 and 8 of Cin 64; Cout 64 and 192; B = 3; the
    <8, 8> maps 1x1, 15x17, 16x16, 17x33 and 48x84 with Cin 16; grids of 1..9, 11 and 12 blocks: every residue of the XCD remap."""
    have = {(c[4], c[6], c[7]) for c in sc.CASES}
    assert {(8, 1, 0), (8, 1, 1), (16, 2, 1), (32, 3, 1), (64, 5, 1), (64, 8, 1), (64, 5, 0), (64, 8, 0)} <= have
    assert {c[5] for c in sc.CASES} >= {64, 192} and any(c[1] == 3 for c in sc.CASES)
    maps = {(c[2], c[3]) for c in sc.CASES if c[7] == 1}
    assert {(1, 1), (15, 17), (16, 16), (17, 33), (48, 84)} <= maps and sc.BY_NAME["g1_res4"][4] == 16
    grids = {sc.grid(c)[0] for c in sc.CASES}
    assert set(range(1, 10)) | {11, 12} <= grids and {g & 7 for g in grids} == set(range(8))
    assert sc.grid(sc.BY_NAME["g1_res4"]) == (18, 2)
    for c in sc.CASES:
        assert c[4] >= 8 and c[4] & (c[4] - 1) == 0 and c[5] % 64 == 0 and 1 <= c[6] <= c[4] // 8 and c[7] in (0, 1)
