"""-m gpu: the association kernels against the float64 reference (tests/assoc_ref64.py) at their edges: the triplet losses,
the training fc (csrc/assoc_train.hip), apse_l2_normalize / apse_sqdist and the sliced inference FC inside a detector
context (csrc/roi.hip).  The inputs come from tests/assoc_cases.py; tests/test_assoc_ref64.py asserts on the CPU what they
contain (ties, triplets on the hinge, zero distances; decisions clear of the f32 error).

Bounds are derived in assoc_ref64.py / roi_ref.py, not fitted.  The worst err / bound of every case goes to assoc_edges.log."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import assoc_cases as AC  # noqa: E402
import assoc_ref64 as R64  # noqa: E402

BLOCKS = (1, 1, 1, 1)
FRAME = (270, 480)


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "assoc_edges.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


# ====================================================================================================== triplet losses
def _hip_loss(kind, lab, x, margin, squared, up=None):
    """x: a CUDA leaf tensor.  -> (loss f32, fraction f32 or None, x.grad on the host)"""
    from apse_uav_amd.online_triplet_loss import batch_all_triplet_loss, batch_hard_triplet_loss
    labels = torch.from_numpy(np.asarray(lab)).cuda()
    x.grad = None
    if kind == "hard":
        loss, frac = batch_hard_triplet_loss(labels, x, margin, squared=bool(squared), device="cuda:0"), None
    else:
        loss, frac = batch_all_triplet_loss(labels, x, margin, squared=bool(squared))
    (loss if up is None else up * loss).backward()
    torch.cuda.synchronize()
    as32 = lambda t: np.float32(t.detach().cpu().numpy())
    return as32(loss), (None if frac is None else as32(frac)), x.grad.cpu().numpy()


def _leaf(e):
    return torch.from_numpy(np.ascontiguousarray(e)).cuda().requires_grad_(True)


@functools.lru_cache(maxsize=None)
def _ref(family, kind, n, D, squared, margin, grad=1.0):
    if family == "A":
        lab, e = AC.lattice(n, D)
    else:
        lab, e = AC.unit_rows(n, D, full_labels=n > 300, repair=n <= 300)
    fn = R64.batch_hard if kind == "hard" else R64.batch_all
    return fn(lab, e, margin, squared, grad=grad, exact_d0=family == "A")


def _grad_ok(got, ref):
    scale = max(float(np.abs(ref).max()), 1e-30)
    return float(np.abs(got - ref).max()) <= 1e-4 * scale + 1e-12


def _check_lattice(tag, kind, ref, got, logdir):
    loss, frac, de = got
    assert float(loss) == pytest.approx(ref["loss"], rel=1e-5), tag
    if kind == "all":
        want = R64.fraction_f32(ref["P"], ref["V"])
        assert frac.tobytes() == want.tobytes(), (tag, float(frac), float(want), ref["P"], ref["V"])
    res = ref["dE_res"]
    ok, worst = R64.check_res(de, res)
    dead = ~(res["mag"] > 0).any(axis=1)                       # rows whose every coefficient is 0
    _log(logdir, "triplet/" + tag, dict(worst_err_over_bound=worst, zero_rows=int(dead.sum()), loss=float(loss), ref_loss=ref["loss"]))
    assert ok, (tag, worst)
    assert not de[dead].any(), tag


@pytest.mark.parametrize("nD", AC.LATTICE_SHAPES, ids=str)
@pytest.mark.parametrize("squared", [0, 1])
def test_triplet_lattice(nD, squared, logdir):
    """Family A: exact d0, real ties, triplets on the hinge.  The fraction bit for bit from the exact counts, dE inside the
    derived chain bound element by element, dead rows exactly 0."""
    n, D = nD
    lab, e = AC.lattice(n, D)
    x = _leaf(e)
    for kind in ("hard", "all"):
        ref = _ref("A", kind, n, D, squared, AC.MARGIN_A)
        _check_lattice("A/%s/%dx%d/sq%d" % (kind, n, D, squared), kind, ref, _hip_loss(kind, lab, x, AC.MARGIN_A, squared), logdir)
    if AC.PLANTED <= n <= 300:                                  # tl == 1e-16f exactly: counted by >=, not by >
        ref = _ref("A", "all", n, D, squared, AC.MARGIN_CNT)
        _check_lattice("A/all/%dx%d/sq%d/m1e-16" % (n, D, squared), "all", ref, _hip_loss("all", lab, x, AC.MARGIN_CNT, squared), logdir)


@pytest.mark.parametrize("nD", AC.UNIT_SHAPES, ids=str)
@pytest.mark.parametrize("squared", [0, 1])
def test_triplet_unit_rows(nD, squared, logdir):
    """Family B: unit rows whose every decision is clear of the f32 error; the project's loss and gradient tolerances."""
    n, D = nD
    lab, e = AC.unit_rows(n, D)
    x = _leaf(e)
    for kind in ("hard", "all"):
        ref = _ref("B", kind, n, D, squared, AC.MARGIN_B)
        loss, frac, de = _hip_loss(kind, lab, x, AC.MARGIN_B, squared)
        err = float(np.abs(de - ref["dE"]).max() / max(np.abs(ref["dE"]).max(), 1e-30))
        _log(logdir, "triplet/B/%s/%dx%d/sq%d" % (kind, n, D, squared), dict(loss=float(loss), ref_loss=ref["loss"], grad_rel_max=err))
        assert float(loss) == pytest.approx(ref["loss"], rel=1e-5, abs=1e-7)
        assert _grad_ok(de, ref["dE"]), err
        if kind == "all":
            assert float(frac) == pytest.approx(float(R64.fraction_f32(ref["P"], ref["V"])), rel=1e-6)


@pytest.mark.parametrize("nD", AC.UNIT_SHAPES_LOSS_ONLY, ids=str)
def test_triplet_unit_rows_large_loss_only(nD, logdir):
    """n > 300: a near-tie may flip, which moves the loss and the fraction by at most the tied gap: those two only."""
    n, D = nD
    lab, e = AC.unit_rows(n, D, full_labels=True, repair=False)
    x = _leaf(e)
    for kind in ("hard", "all"):
        ref = _ref("B", kind, n, D, 0, AC.MARGIN_B)
        loss, frac, _ = _hip_loss(kind, lab, x, AC.MARGIN_B, 0)
        _log(logdir, "triplet/B/%s/%dx%d/sq0" % (kind, n, D), dict(loss=float(loss), ref_loss=ref["loss"]))
        assert float(loss) == pytest.approx(ref["loss"], rel=1e-5, abs=1e-7)
        if kind == "all":
            assert float(frac) == pytest.approx(float(R64.fraction_f32(ref["P"], ref["V"])), rel=1e-6)


def test_triplet_upstream_gradient(logdir):
    """(3 * loss).backward(): the upstream gradient reaches dE"""
    n, D = 257, 100
    lab, e = AC.lattice(n, D)
    x = _leaf(e)
    for kind in ("hard", "all"):
        ref = _ref("A", kind, n, D, 0, AC.MARGIN_A, 3.0)
        _check_lattice("A/%s/%dx%d/sq0/up3" % (kind, n, D), kind, ref, _hip_loss(kind, lab, x, AC.MARGIN_A, 0, up=3.0), logdir)


def test_triplet_f16_noncontiguous_input():
    """f16 embeddings that are every other column of a wider tensor: the same values (small integers are exact in f16), so
    the same loss and fraction bit for bit and the same gradient, rounded to f16 on its way back and 0 in the unused columns"""
    n, D = 257, 100
    lab, e = AC.lattice(n, D)
    for kind in ("hard", "all"):
        want = _hip_loss(kind, lab, _leaf(e), AC.MARGIN_A, 1)
        wide = torch.zeros((n, 2 * D), dtype=torch.float16)
        wide[:, ::2] = torch.from_numpy(e).half()
        wide[:, 1::2] = 7.0
        base = wide.cuda().requires_grad_(True)
        x = base[:, ::2]
        assert not x.is_contiguous() and x.dtype == torch.float16
        from apse_uav_amd.online_triplet_loss import batch_all_triplet_loss, batch_hard_triplet_loss
        labels = torch.from_numpy(lab).cuda()
        if kind == "hard":
            loss, frac = batch_hard_triplet_loss(labels, x, AC.MARGIN_A, squared=True), None
        else:
            loss, frac = batch_all_triplet_loss(labels, x, AC.MARGIN_A, squared=True)
        loss.backward()
        torch.cuda.synchronize()
        assert np.float32(loss.detach().cpu().numpy()).tobytes() == want[0].tobytes()
        if frac is not None:
            assert np.float32(frac.cpu().numpy()).tobytes() == want[1].tobytes()
        g = base.grad.cpu()
        assert g.dtype == torch.float16 and not g[:, 1::2].any()
        assert torch.equal(g[:, ::2], torch.from_numpy(want[2]).half())


# ====================================================================================================== training fc
FC_SHAPES = [(1, 1, 1, 1), (63, 3, 5, 100), (64, 16, 4, 64), (65, 17, 1, 65), (130, 8, 4, 128), (37, 256, 10, 128), (5, 257, 1, 256),
             (4, 257, 1, 8),       # K = 257: the smallest K with two chunks, 144 + 113 (a short last chunk)
             (3, 16, 4, 8)]        # K = 256: the largest K that stays one chunk (S = 1, the chunk exactly full)


def _fc_abi(x, w, b, ge):
    """apse_assoc_fc_forward / _backward through the C ABI -> (E, inv_norm, dW, db) device tensors"""
    from apse_uav_amd import _lib
    lib = _lib.load()
    n, K = x.shape
    D = w.shape[0]
    e = torch.full((n, D), float("nan"), device="cuda")
    inv = torch.full((n,), float("nan"), device="cuda")
    dw = torch.full((D, K), float("nan"), device="cuda")
    db = torch.full((D,), float("nan"), device="cuda")
    nb = int(lib.apse_assoc_fc_workspace_bytes(n, K, D))
    assert nb >= R64.fc_splits(n, K, D)[0] * n * D * 4
    ws = torch.full((nb // 4,), float("nan"), device="cuda")
    assert lib.apse_assoc_fc_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), n, K, D, _lib.ptr(e), _lib.ptr(inv), _lib.ptr(ws), nb,
                                     _lib.stream_ptr()) == 0
    assert lib.apse_assoc_fc_backward(_lib.ptr(x), _lib.ptr(e), _lib.ptr(inv), _lib.ptr(ge), n, K, D, _lib.ptr(dw), _lib.ptr(db),
                                      _lib.ptr(ws), nb, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return e, inv, dw, db


def _fc_check(tag, x, w, b, ge, logdir, roi=None, depth=None):
    n, K = x.shape
    D = w.shape[0]
    xd, wd, bd, gd = (torch.from_numpy(a).cuda() for a in (x, w, b, ge))
    e, inv, dw, db = _fc_abi(xd, wd, bd, gd)
    again = _fc_abi(xd, wd, bd, gd)
    for p, q in zip((e, inv, dw, db), again):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), tag                    # a second run: the same bits
    S, rchunk = R64.fc_splits(n, K, D)
    f = R64.fc_forward(x, w, b, S, rchunk)
    assert np.isfinite(f["E_bound"]).all() and np.isfinite(f["inv_bound"]).all(), tag
    eh, ih = e.cpu().numpy(), inv.cpu().numpy()
    ok_e, w_e = R64.check(eh, f["E"], f["E_bound"])
    ok_i, w_i = R64.check(ih, f["inv_norm"], f["inv_bound"])
    g = R64.fc_backward(x, eh, ih, ge)                          # from the E and inv_norm the forward kernel produced
    ok_w, w_w = R64.check(dw.cpu().numpy(), g["dW"], g["dW_bound"])
    ok_b, w_b = R64.check(db.cpu().numpy(), g["db"], g["db_bound"])
    _log(logdir, "fc/" + tag, dict(S=S, rchunk=rchunk, worst_E=w_e, worst_inv=w_i, worst_dW=w_w, worst_db=w_b))
    assert ok_e and ok_i and ok_w and ok_b, (tag, w_e, w_i, w_w, w_b)
    if roi is not None:                                          # the same through AssociationHead.train() and autograd
        from apse_uav_amd.networks.association_head import AssociationHead
        head = AssociationHead(roi_size=roi, input_depth=depth, embedding_dim=D)
        head.load_state_dict({"fc.weight": torch.from_numpy(w), "fc.bias": torch.from_numpy(b)})
        head.to("cuda")
        head.train()
        out = head(xd.view(n, depth, roi, roi))
        (out * gd).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(out.detach().view(torch.int32), e.view(torch.int32)), tag
        assert torch.equal(head.fc.weight.grad.view(torch.int32), dw.view(torch.int32)), tag
        assert torch.equal(head.fc.bias.grad.view(torch.int32), db.view(torch.int32)), tag
    return eh, ih, f


def _fc_inputs(n, K, D, seed):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, K)).astype(np.float32)
    w = (rng.standard_normal((D, K)) / np.sqrt(K)).astype(np.float32)
    b = (rng.standard_normal(D) * 0.1).astype(np.float32)
    ge = rng.standard_normal((n, D)).astype(np.float32)
    return x, w, b, ge


@pytest.mark.parametrize("shape", FC_SHAPES, ids=str)
def test_training_fc(shape, logdir):
    n, depth, roi, D = shape
    K = depth * roi * roi
    x, w, b, ge = _fc_inputs(n, K, D, 4000 + n + K + D)
    _fc_check("%dx%dx%dx%d" % shape, x, w, b, ge, logdir, roi, depth)


def test_training_fc_zero_rows(logdir):
    """An all-zero input row: with a zero bias Z = 0, so E is exactly 0, inv_norm = 1 / eps and dZ = dE / eps (the eps branch of
    the normalise); with a bias the row is an ordinary one."""
    n, depth, roi, D = 65, 17, 1, 65
    x, w, b, ge = _fc_inputs(n, depth, D, 4100)
    x[3] = 0
    eh, ih, f = _fc_check("zero_row/zero_bias", x, w, np.zeros_like(b), ge, logdir, roi, depth)
    assert not eh[3].any() and f["E_bound"][3].max() == 0 and ih[3] == np.float32(1.0) / np.float32(1e-12)
    eh, ih, f = _fc_check("zero_row/bias", x, w, b, ge, logdir, roi, depth)
    assert abs(float(np.linalg.norm(eh[3].astype(np.float64))) - 1) < 1e-6


# ====================================================================================================== l2_normalize, sqdist
@pytest.mark.parametrize("D", [1, 63, 64, 65, 128, 200, 256])
def test_l2_normalize_edges(D, logdir):
    """rows: all-zero, norm below eps (divided by eps), ordinary, large and small but above eps; squares stay inside f32"""
    from apse_uav_amd import _lib
    rng = np.random.RandomState(5000 + D)
    x = rng.standard_normal((9, D)).astype(np.float32)
    x[0] = 0
    x[1] *= np.float32(1e-14)
    x[2] *= np.float32(1e3)
    x[3] *= np.float32(1e-6)
    x[4, : D // 2] = 0
    nrm = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    assert nrm[0] == 0 and 0 < nrm[1] < 5e-13 and (nrm[2:] > 1e-9).all()                # no row near the eps threshold (1e-12)
    assert float(np.abs(x[x != 0]).min()) ** 2 > 1e-37
    xd = torch.from_numpy(x).cuda()
    y = torch.full((9, D), float("nan"), device="cuda")
    assert _lib.load().apse_l2_normalize(_lib.ptr(xd), _lib.ptr(y), 9, D, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    ok, worst = R64.check_res(got, R64.l2_normalize(x))
    _log(logdir, "l2_normalize/D%d" % D, dict(worst_err_over_bound=worst))
    assert ok, worst
    assert not got[0].any()


@pytest.mark.parametrize("OND", [(1, 1, 1), (7, 5, 65), (100, 100, 128), (3, 40, 256)], ids=str)
def test_sqdist_edges(OND, logdir):
    from apse_uav_amd import _lib
    O, N, D = OND
    rng = np.random.RandomState(5100 + O + N + D)
    a, b = rng.standard_normal((O, D)).astype(np.float32), rng.standard_normal((N, D)).astype(np.float32)
    same = [(o, (3 * o + 1) % N) for o in range(0, O, 3)] if N > 1 else []
    for o, k in same:
        b[k] = a[o]                                             # identical rows: exactly 0
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.full((O, N), float("nan"), device="cuda")
    assert _lib.load().apse_sqdist(_lib.ptr(ad), _lib.ptr(bd), O, N, D, _lib.ptr(out), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ok, worst = R64.check_res(got, R64.sqdist(a, b))
    _log(logdir, "sqdist/%dx%dx%d" % OND, dict(worst_err_over_bound=worst))
    assert ok, worst
    assert all(got[o, k] == 0 for o, k in same)


# ====================================================================================================== sliced FC in a context
@pytest.fixture(scope="module")
def frames():
    from apse_uav_amd.synthetic import SyntheticSequence
    seq = SyntheticSequence("dynamic", *FRAME)
    return torch.stack([torch.from_numpy(seq.frame(5 * t)) for t in range(2)]).cuda()


@pytest.fixture(scope="module")
def detector_state():
    from apse_uav_amd.weights import synthetic_detector_state
    return synthetic_detector_state(0, BLOCKS)


def _boxes(rng, k):
    """k boxes inside the 252 x 448 resized image, a few pixels to half the frame wide"""
    w, h = rng.uniform(6, 220, k), rng.uniform(6, 120, k)
    x1, y1 = rng.uniform(0, 448 - w), rng.uniform(0, 252 - h)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_sliced_fc_in_context(dim, frames, detector_state, logdir):
    """The per-frame association FC (assoc_fc_slices<1 / 2 / 4> + assoc_fc_finish) as a context runs it on given boxes: the
    float64 FC + normalise of the context's own pooled rows (weights permuted from C,H,W to H,W,C order) inside the derived
    bound, for 40 boxes over two images, then 17, 16 and 1 on one image; rows past the live count keep the bits the run
    before left there."""
    import roi_ref as rr
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks.association_head import AssociationHead
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    from apse_uav_amd.weights import synthetic_association_state
    cfg = setup_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 256, 448
    cfg.APSE.MAX_BATCH = 2
    asd = synthetic_association_state(dim, dim=dim)
    head = AssociationHead(roi_size=10, input_depth=256, embedding_dim=dim)
    head.load_state_dict(asd)
    m = TrackRCNN(cfg)
    m.to("cuda")
    m.load_state_dict(detector_state)
    m.attach_association_head(head)
    w = asd["fc.weight"].view(dim, 256, 10, 10).permute(0, 2, 3, 1).reshape(dim, -1).numpy()
    bias = asd["fc.bias"].numpy()
    rng = np.random.RandomState(6000 + dim)
    prev = None
    worst_raw = worst_y = 0.0
    for counts in ((17, 23), (17,), (16,), (1,)):
        B, live = len(counts), sum(counts)
        boxes = _boxes(rng, live)
        given = (boxes, np.zeros(live, np.int32), np.asarray(counts, np.int32))
        m.inference_frames(frames[:B], given=given, want_masks=False)
        res = m.last_results
        assert res.total == live
        pooled = m.debug_tensor("assoc_pooled").cpu().numpy().reshape(-1, 25600)
        raw = m.debug_tensor("embedding_raw").cpu().numpy().reshape(-1, dim)
        if prev is None:
            assert live == 40
        else:
            assert raw[live:40].tobytes() == prev[live:40].tobytes(), counts           # untouched past the live count
        prev = raw.copy()
        x = pooled[:live]
        assert np.isfinite(x).all() and x.any()
        ref = rr.assoc_fc(x, w, bias)
        assert np.isfinite(ref["y_bound"]).all()
        ok, wr = rr.check(raw[:live], ref)
        assert ok, (counts, wr)
        ok, wy = rr.check(res.embedding[:live], dict(ref=ref["y"]), b=ref["y_bound"])
        assert ok, (counts, wy)
        worst_raw, worst_y = max(worst_raw, wr), max(worst_y, wy)
    _log(logdir, "context_fc/dim%d" % dim, dict(worst_err_over_bound_raw=worst_raw, worst_err_over_bound_y=worst_y))
