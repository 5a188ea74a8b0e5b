"""CPU: the float64 association reference (tests/assoc_ref64.py) against the reference project's golden output, the f32
restatement (tests/assoc_train_ref.py) and f64 autograd; and the conditions the inputs of tests/test_gpu_assoc_edges.py must
meet (tests/assoc_cases.py) -- asserted here so that the GPU tests can rely on them."""
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import assoc_cases as AC  # noqa: E402
import assoc_ref64 as R64  # noqa: E402
import assoc_train_ref as R32  # noqa: E402

GOLD = ["seed2", "seed7", "seed48", "seed300", "lonely", "one_label", "neg_is_rowmax", "n1", "dups"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "triplet_golden.npz"))


def _grad_ok(got, ref):
    scale = max(float(np.abs(ref).max()), 1e-30)
    return float(np.abs(got - ref).max()) <= 1e-4 * scale + 1e-12


# ------------------------------------------------------------------------------------------------------ against golden
@pytest.mark.parametrize("case", GOLD)
@pytest.mark.parametrize("squared", [0, 1])
def test_reference_against_golden_and_restatement(gold, case, squared):
    lab, e = gold[case + "_labels"], gold[case + "_emb"]
    h = R64.batch_hard(lab, e, 0.2, squared)
    assert h["loss"] == pytest.approx(float(gold["%s_hard_sq%d_loss" % (case, squared)]), rel=1e-5, abs=1e-7)
    assert _grad_ok(h["dE"], gold["%s_hard_sq%d_dE" % (case, squared)])
    rl, rde = R32.batch_hard(lab, e, 0.2, squared)
    assert h["loss"] == pytest.approx(float(rl), rel=1e-5, abs=1e-7) and _grad_ok(h["dE"], rde)
    a = R64.batch_all(lab, e, 0.2, squared)
    assert a["loss"] == pytest.approx(float(gold["%s_all_sq%d_loss" % (case, squared)]), rel=1e-5, abs=1e-7)
    assert float(R64.fraction_f32(a["P"], a["V"])) == pytest.approx(float(gold["%s_all_sq%d_frac" % (case, squared)]), rel=1e-6)
    assert _grad_ok(a["dE"], gold["%s_all_sq%d_dE" % (case, squared)])
    rl, rf, rde = R32.batch_all(lab, e, 0.2, squared)
    assert a["loss"] == pytest.approx(float(rl), rel=1e-5, abs=1e-7) and _grad_ok(a["dE"], rde)
    assert float(R64.fraction_f32(a["P"], a["V"])) == pytest.approx(float(rf), rel=1e-6)


@pytest.mark.parametrize("squared", [0, 1])
def test_triplet_gradients_against_f64_autograd(squared):
    """the hand-written dE against torch autograd of the published expression in f64 (random rows: no ties, no zeros)"""
    lab, e = AC.unit_rows(48, 128)
    x = torch.from_numpy(e.astype(np.float64)).requires_grad_(True)
    l = torch.from_numpy(lab)
    g = x @ x.T
    sq = torch.diag(g)
    d = (sq[None, :] - 2 * g + sq[:, None]).clamp_min(0)
    eye = torch.eye(48, dtype=torch.bool)
    if not squared:
        d = torch.where(eye, torch.zeros_like(d), (d + eye * 1.0).sqrt())
    same = l[None, :] == l[:, None]
    ap = (same & ~eye) * d
    an = d + d.max(1, keepdim=True)[0] * same
    tl = (ap.max(1)[0] - an.min(1)[0] + 0.2).clamp_min(0)
    (3.0 * tl.mean()).backward()
    h = R64.batch_hard(lab, e, 0.2, squared, grad=3.0)
    assert 3.0 * h["loss"] == pytest.approx(float(3.0 * tl.mean().detach()), rel=1e-12)
    assert np.abs(h["dE"] - x.grad.numpy()).max() <= 1e-12 * np.abs(h["dE"]).max()
    x.grad = None
    g = x @ x.T
    sq = torch.diag(g)
    d = (sq[None, :] - 2 * g + sq[:, None]).clamp_min(0)
    if not squared:
        d = torch.where(eye, torch.zeros_like(d), (d + eye * 1.0).sqrt())
    valid = (same & ~eye)[:, :, None] & (~same)[:, None, :]
    t3 = ((d[:, :, None] - d[:, None, :] + 0.2) * valid).clamp_min(0)
    P = int((t3 > 1e-16).sum())
    (t3.sum() / (P + 1e-16)).backward()
    a = R64.batch_all(lab, e, 0.2, squared)
    assert a["P"] == P and a["V"] == int(valid.sum())
    assert a["loss"] == pytest.approx(float((t3.sum() / (P + 1e-16)).detach()), rel=1e-12)
    assert np.abs(a["dE"] - x.grad.numpy()).max() <= 1e-12 * np.abs(a["dE"]).max()


# ------------------------------------------------------------------------------------------------------ family A
@pytest.mark.parametrize("nD", AC.LATTICE_SHAPES, ids=str)
def test_lattice_is_exact_in_f32(nD):
    """every Gram product and d0 an integer below 2^24: the f32 d0 is the f64 d0 whatever the summation order"""
    lab, e = AC.lattice(*nD)
    assert e.dtype == np.float32 and (e == np.round(e)).all() and np.abs(e).max() <= 2
    e64 = e.astype(np.float64)
    assert (np.abs(e64) @ np.abs(e64).T).max() * 4 < 2 ** 24          # the largest partial sum any order can meet
    d0 = R64.batch_hard(lab, e, AC.MARGIN_A, True)["d0"]
    assert (d0 == np.round(d0)).all() and d0.max() < 2 ** 24
    assert R64.batch_hard(lab, e, AC.MARGIN_A, True, exact_d0=True)["tau_max"] == 0


@pytest.mark.parametrize("nD", [s for s in AC.LATTICE_SHAPES if s[0] >= AC.PLANTED], ids=str)
@pytest.mark.parametrize("squared", [0, 1])
def test_lattice_holds_the_edges_and_tells_the_rules_apart(nD, squared):
    lab, e = AC.lattice(*nD)
    n = nD[0]
    h = R64.batch_hard(lab, e, AC.MARGIN_A, squared, exact_d0=True)
    t0 = time.time()
    a = R64.batch_all(lab, e, AC.MARGIN_A, squared, exact_d0=True)
    assert time.time() - t0 < 20                                                       # n = 2048: seconds, no n^3 tensor
    assert (h["pos_gap"] == 0).any() and (h["neg_gap"] == 0).any()                    # tied hardest positives / negatives
    assert h["pos_gap"][5] == 0 and h["neg_gap"][5] == 0 and h["jp"][5] == 3 and h["jn"][5] == 7
    assert (h["tl"] == 0).any() and a["n_zero"] > 0                                    # triplets exactly on the hinge
    assert h["tl"][1 if squared else 6] == 0
    assert ((h["d0"] == 0).sum() - n) >= 4                                             # zero distances off the diagonal
    assert (np.unique(lab, return_counts=True)[1] == 1).any()                          # a label with a single member
    assert (h["tl"] < 0).any()                                                         # an anchor whose hinge is clipped
    # every decision that is not an exact tie is further from its alternative than the f32 error of tl (d0 itself is exact)
    nz = h["tl"] != 0
    assert (np.abs(h["tl"]) > 2 * h["tl_tau"])[nz].all() and (a["tl_margin"] > 0).all()
    # the wrong rules change the result on these inputs
    for rule in ("ties_high", "hinge_nonstrict"):
        w = R64.batch_hard(lab, e, AC.MARGIN_A, squared, wrong_rule=rule)
        assert np.abs(w["dE"] - h["dE"]).max() > 1e-4 * np.abs(h["dE"]).max(), rule
    if n <= 300:                                                                       # the count rule: margin = 1e-16f
        w = R64.batch_all(lab, e, AC.MARGIN_A, squared, wrong_rule="hinge_nonstrict")
        assert np.abs(w["dE"] - a["dE"]).max() > 1e-5 * np.abs(a["dE"]).max()
        c = R64.batch_all(lab, e, AC.MARGIN_CNT, squared, exact_d0=True)
        w = R64.batch_all(lab, e, AC.MARGIN_CNT, squared, wrong_rule="count_ge")
        assert w["P"] > c["P"] and abs(w["loss"] - c["loss"]) > 1e-5 * abs(c["loss"])
        assert R64.fraction_f32(w["P"], w["V"]) != R64.fraction_f32(c["P"], c["V"])


# ------------------------------------------------------------------------------------------------------ family B
@pytest.mark.parametrize("nD", AC.UNIT_SHAPES, ids=str)
def test_unit_rows_decisions_clear_of_the_f32_error(nD):
    """every decision margin > 2 tau (pos / neg / rowmax gaps on d0, |tl| against the error of tl), both losses, both distance
    forms; rows are unit length, labels hold groups and singletons, and both sides of the hinge occur"""
    lab, e = AC.unit_rows(*nD)
    assert e.dtype == np.float32 and np.abs((e.astype(np.float64) ** 2).sum(1) - 1).max() < 1e-6
    assert AC.unit_margins(lab, e).all()
    h = R64.batch_hard(lab, e, AC.MARGIN_B, False)
    assert (h["tl"] < 0).any() and (h["tl"] > 0).any() and np.isfinite(h["pos_gap"]).any()
    a = R64.batch_all(lab, e, AC.MARGIN_B, False)
    assert 0 < a["P"] < a["V"]


# ------------------------------------------------------------------------------------------------------ fc, normalize, sqdist
@pytest.mark.parametrize("nKD", [(5, 75, 100), (3, 16, 1), (70, 300, 65)], ids=str)
def test_fc_reference_against_f64_autograd(nKD):
    n, K, D = nKD
    rng = np.random.RandomState(n + K + D)
    x, w, b = rng.standard_normal((n, K)), rng.standard_normal((D, K)) / np.sqrt(K), rng.standard_normal(D) * 0.1
    ge = rng.standard_normal((n, D))
    wt, bt = torch.from_numpy(w).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    et = torch.nn.functional.normalize(torch.from_numpy(x) @ wt.T + bt, p=2, dim=1)
    (et * torch.from_numpy(ge)).sum().backward()
    f = R64.fc_forward(x, w, b)
    assert np.abs(f["E"] - et.detach().numpy()).max() < 1e-14
    assert np.isfinite(f["E_bound"]).all() and (f["E_bound"] < 1e-3).all() and (f["E_bound"] > 0).all()
    g = R64.fc_backward(x, f["E"], f["inv_norm"], ge)
    scale = n * np.abs(ge).max() * max(np.abs(x).max(), 1.0) * f["inv_norm"].max()      # D = 1: the gradient itself is 0
    assert np.abs(g["dW"] - wt.grad.numpy()).max() <= 1e-12 * scale
    assert np.abs(g["db"] - bt.grad.numpy()).max() <= 1e-12 * scale
    assert (g["dW_bound"] > 0).all() and (g["dW_bound"] < 1e-3 * scale).all()


def test_fc_reference_zero_rows():
    rng = np.random.RandomState(3)
    x, w = rng.standard_normal((4, 32)), rng.standard_normal((8, 32))
    x[2] = 0
    f = R64.fc_forward(x, w, np.zeros(8))
    assert (f["E"][2] == 0).all() and (f["E_bound"][2] == 0).all() and f["inv_norm"][2] == 1.0 / R64.EPS_NORM
    ge = rng.standard_normal((4, 8))
    g = R64.fc_backward(x, f["E"], f["inv_norm"], ge)
    assert np.allclose(g["dZ"][2], ge[2] / R64.EPS_NORM, rtol=1e-15, atol=0)          # dZ = dE / eps
    f = R64.fc_forward(x, w, np.full(8, 0.5))
    assert np.allclose(f["E"][2], 1 / np.sqrt(8)) and np.isfinite(f["E_bound"]).all()


def test_fc_splits_shapes():
    """the shapes the GPU test relies on: a short last chunk and a single chunk"""
    assert R64.fc_splits(37, 25600, 128) == (100, 256)
    assert R64.fc_splits(4, 257, 8) == (2, 144)            # 144 + 113: the smallest K with two chunks has a short last one
    assert R64.fc_splits(4, 256, 8) == (1, 256) and R64.fc_splits(1, 1, 1) == (1, 16)


def test_normalize_and_sqdist_against_roi_ref():
    import roi_ref as rr
    rng = np.random.RandomState(5)
    x = rng.standard_normal((6, 100))
    x[1] = 0
    x[2] *= 1e-15
    res = R64.l2_normalize(x)
    assert np.allclose(res["ref"][[0, 3, 4, 5]], rr.l2_normalize(x)["ref"][[0, 3, 4, 5]], rtol=1e-15, atol=0)
    assert (res["ref"][1] == 0).all() and np.allclose(res["ref"][2], x[2] / R64.EPS_NORM, rtol=1e-15)
    a, b = rng.standard_normal((3, 65)), rng.standard_normal((4, 65))
    b[1] = a[2]
    s = R64.sqdist(a, b)
    assert np.allclose(s["ref"], rr.sqdist(a, b)["ref"], rtol=1e-15) and s["ref"][2, 1] == 0 and s["mag"][2, 1] == 0
