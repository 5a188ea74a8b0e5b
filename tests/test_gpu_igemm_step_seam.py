"""conv_igemm_f32's k loop at its seams: the rotated step (the barrier in front of the last MFMA group, the next step's first
fragment reads behind it) and the prologue that requests two steps back to back only move loads, LDS reads and one barrier, so
every output keeps its bits.  The shapes are the smallest at which either can go wrong: M = 99 (two 64-row tiles, the second
with 35 live rows; one partly filled 128-row tile), K slices of 1, 2, 9 and 5 steps (the last with a dead second half), columns
past Cout, split K with slices of 3 + 2 and of 2 + 2 + 1 + none, and the fused epilogue.

Per case: (1) the sha256 of the output equals tests/golden/igemm_step_seam_sha256.json, recorded by tools/record_igemm_hashes.py
with the library of the commit BEFORE the loop changed; (2) that output is itself right: against a float64 direct convolution,
|y - y64| <= K * 2^-24 * sum |a| |b| per output, the worst case of a K-term f32 fma chain in any order (K = KH * KW * Cin
products, + 2 terms where bias and residual are added); (3) independently of the file, the unsplit single-k-group tile shapes
(cfg 0, 1, 3, 4) give the same bytes among themselves.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igemm_step_seam_sha256.json")
H, W = 9, 11
WIDE_CFGS, NARROW_CFGS = (0, 1, 3, 4, 6, 7), (2, 5)        # Cout = 72 (columns past Cout in every tile width) / Cout = 16
SAME_BITS_CFGS = (0, 1, 3, 4)                              # unsplit, one k group: one summation order
# (Cin, kernel, stride): one 64-deep step; two steps; nine steps; one live sub-step under KS = 2; nine sub-steps = five steps, the
# last half dead; and one strided 1x1
GEOMS = ((64, 1, 1), (128, 1, 1), (64, 3, 1), (32, 1, 1), (32, 3, 1), (128, 1, 2))


def _cases():
    """name -> dict(cin, k, stride, cfg, cout, splitk, epi)"""
    out = {}
    for cin, k, stride in GEOMS:
        for cfg in WIDE_CFGS + NARROW_CFGS:
            cout = 72 if cfg in WIDE_CFGS else 16
            out["cin%d_k%d_s%d_cfg%d_cout%d" % (cin, k, stride, cfg, cout)] = dict(cin=cin, k=k, stride=stride, cfg=cfg, cout=cout, splitk=0, epi=False)
    # the five-step case through the separate reduce kernel: slices of 3 + 2 steps, and of 2 + 2 + 1 + an EMPTY one (KS = 2 shapes)
    for cfg in (1, 6, 2):
        cout = 72 if cfg in WIDE_CFGS else 16
        for sk in (2, 4):
            out["cin32_k3_s1_cfg%d_cout%d_splitk%d" % (cfg, cout, sk)] = dict(cin=32, k=3, stride=1, cfg=cfg, cout=cout, splitk=sk, epi=False)
    out["cin64_k3_s1_cfg6_cout72_bias_relu_res"] = dict(cin=64, k=3, stride=1, cfg=6, cout=72, splitk=0, epi=True)
    return out


CASES = _cases()


def _inputs(c):
    """Seeded f32 operands of a case: the same x for every case of one geometry, the same w for one (geometry, Cout)."""
    rng = np.random.RandomState(1000 * c["cin"] + 10 * c["k"] + c["stride"])
    x = rng.standard_normal((1, c["cin"], H, W)).astype(np.float32)
    ws = {co: rng.standard_normal((co, c["cin"], c["k"], c["k"])).astype(np.float32) for co in (72, 16)}
    oh = (H + 2 * (c["k"] // 2) - c["k"]) // c["stride"] + 1
    ow = (W + 2 * (c["k"] // 2) - c["k"]) // c["stride"] + 1
    bias = rng.standard_normal(72).astype(np.float32)
    res = rng.standard_normal((1, 72, oh, ow)).astype(np.float32)
    return x, ws[c["cout"]], bias, res


def run_case(c):
    """The case's output, NCHW f32 numpy, from apse_conv2d."""
    from hip_helpers import hip_conv2d
    x, w, bias, res = _inputs(c)
    kw = dict(stride=c["stride"], pad=c["k"] // 2, cfg=c["cfg"], splitk=c["splitk"], fuse=0)
    if c["epi"]:
        kw.update(bias=torch.from_numpy(bias), relu=True, residual=torch.from_numpy(res), res_mode=1)
    return hip_conv2d(torch.from_numpy(x), torch.from_numpy(w), **kw).numpy()


def sha(y):
    return hashlib.sha256(np.ascontiguousarray(y, np.float32).tobytes()).hexdigest()


def reference(c):
    """(y64, bound): the float64 direct convolution and K * 2^-24 * sum |a| |b| per output."""
    x, w, bias, res = _inputs(c)
    k, s, pad = c["k"], c["stride"], c["k"] // 2
    xp = np.zeros((c["cin"], H + 2 * pad, W + 2 * pad), np.float64)
    xp[:, pad:pad + H, pad:pad + W] = x[0]
    oh, ow = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    w64 = w.astype(np.float64)
    y = np.zeros((c["cout"], oh, ow), np.float64)
    mag = np.zeros_like(y)
    for r in range(k):
        for q in range(k):
            patch = xp[:, r:r + (oh - 1) * s + 1:s, q:q + (ow - 1) * s + 1:s]
            y += np.einsum("oc,chw->ohw", w64[:, :, r, q], patch)
            mag += np.einsum("oc,chw->ohw", np.abs(w64[:, :, r, q]), np.abs(patch))
    terms = k * k * c["cin"]
    if c["epi"]:
        y += bias.astype(np.float64)[:, None, None] + res[0].astype(np.float64)
        mag += np.abs(bias.astype(np.float64))[:, None, None] + np.abs(res[0].astype(np.float64))
        terms += 2
        y = np.maximum(y, 0.0)              # 1-Lipschitz: the bound carries over
    return y[None], terms * 2.0 ** -24 * mag[None]


@pytest.fixture(scope="module")
def outputs():
    return {name: run_case(c) for name, c in CASES.items()}


def test_outputs_keep_the_parents_bits(outputs):
    golden = json.load(open(GOLDEN))["cases"]
    bad = []
    for name in sorted(CASES):
        got, want = sha(outputs[name]), golden.get(name)
        print(name, got, "ok" if got == want else "GOLDEN %s" % want)
        if got != want:
            bad.append(name)
    assert not bad, "outputs differ from the recorded ones (or have no entry): %s" % bad


def test_recorded_outputs_are_right(outputs):
    bad = []
    for name in sorted(CASES):
        y64, bound = reference(CASES[name])
        y = outputs[name].astype(np.float64)
        assert y.shape == y64.shape, (name, y.shape, y64.shape)
        ratio = float(np.max(np.abs(y - y64) / bound)) if np.all(np.isfinite(y)) else float("inf")
        print("%s max |y - y64| / bound = %.4f" % (name, ratio))
        if not ratio <= 1.0:
            bad.append((name, ratio))
    assert not bad, bad


def test_single_group_tiles_agree_bit_for_bit(outputs):
    bad = []
    for cin, k, stride in GEOMS:
        names = ["cin%d_k%d_s%d_cfg%d_cout72" % (cin, k, stride, cfg) for cfg in SAME_BITS_CFGS]
        hashes = [sha(outputs[n]) for n in names]
        print(cin, k, stride, hashes)
        if len(set(hashes)) != 1:
            bad.append(dict(zip(names, hashes)))
    assert not bad, bad
