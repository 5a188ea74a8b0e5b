"""Box-head training on the GPU (csrc/box_train.hip, networks/box_head.py): the matcher bit for bit against the f32 restatement,
the GEMM entries exactly on a lattice and under the float64 arbiter of tests/mask_train_ref.py on normal data, the loss and its
gradient, the whole head, determinism, the refused limits, and agreement with the inference path.

Observed errors (normalised by max|f64|) are printed per output and logged to box_train.log in the log directory; DESIGN.md
"Box-head training" records them.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import box_train_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def _log(logdir, name, obj):
    print(name, json.dumps(obj))
    with open(os.path.join(logdir, "box_train.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _judge(logdir, tag, outputs, factor=2.0):
    """outputs: {name: (hip, f64, f32)}; logs every pair of errors, then asserts the arbiter rule on each."""
    rows, bad = {}, []
    for name, (hip, f64, f32) in outputs.items():
        eh, ef, bound, ok = R.arbiter(hip, f64, f32, factor)
        rows[name] = {"hip": eh, "torch_f32": ef, "bound": bound}
        if not ok:
            bad.append(name)
    _log(logdir, tag, rows)
    assert not bad, (tag, {k: rows[k] for k in bad})


def _bh():
    from apse_uav_amd.networks import box_head
    return box_head


# ------------------------------------------------------------------------------------------------ matcher
MATCH_K = 5
MATCH_SHAPES = [(1, 1), (63, 1), (65, 3), (1037, 37), (1300, 300), (7, 0)]          # (N, G); N = 1000 + G where G >= 37
MATCH_SEED = {(1, 1): 1, (63, 1): 1, (65, 3): 1, (1037, 37): 1, (1300, 300): 1, (7, 0): 1}


def match_case(N, G, seed):
    """Seeded boxes on a 1/4-pixel lattice: ground truths, proposals of which every second one is a jittered ground truth, the
    ground truths themselves appended when N >= 1000 + G, and the planted cases (as far as N and G allow): proposal 0 has IoU
    exactly 0.5 with ground truth 0, proposal 1 is ground truth 0, proposal 2 touches ground truth 0 (zero-area overlap),
    ground truths 1 and 2 are the same box with different classes and proposal 3 is that box."""
    g = torch.Generator().manual_seed(seed)

    def boxes(n):
        xy = torch.randint(0, 2400, (n, 2), generator=g).float() / 4
        wh = torch.randint(96, 1200, (n, 2), generator=g).float() / 4
        return torch.cat([xy, xy + wh], dim=1)

    gts = boxes(G)
    cls = torch.randint(0, MATCH_K, (G,), generator=g)
    if G >= 3:
        gts[2] = gts[1]
        cls[2] = (cls[1] + 1) % MATCH_K
    props = boxes(N)
    if G:
        for i in range(0, N, 2):
            props[i] = gts[i % G] + torch.randint(-40, 41, (4,), generator=g).float() / 4
        if N >= 1000 + G:
            props[N - G:] = gts
        x1, y1, x2, y2 = gts[0].tolist()
        props[0] = torch.tensor([x1, y1, x1 + 2 * (x2 - x1), y2])
        if N >= 2:
            props[1] = gts[0]
        if N >= 3:
            props[2] = torch.tensor([x2, y1, x2 + (x2 - x1), y2])
        if N >= 4 and G >= 3:
            props[3] = gts[1]
    return props, gts, cls


def match_case_is_clean(props, gts):
    """The condition on the generator: exact ties apart, no IoU within 1e-5 of 0.5 and no proposal whose two best ground truths
    lie within 1e-6 of each other (float64 restatement).  Without it a label flip would be a rounding question."""
    if gts.shape[0] == 0:
        return True
    q = R.pairwise_iou(gts.double(), props.double())               # [G][N]
    near = ((q - 0.5).abs() < 1e-5) & (q != 0.5)
    if bool(near.any()):
        return False
    if gts.shape[0] >= 2:
        top = q.topk(2, dim=0).values
        gap = top[0] - top[1]
        if bool(((gap < 1e-6) & (gap != 0)).any()):
            return False
    return True


@pytest.mark.parametrize("N,G", MATCH_SHAPES)
def test_matcher_bit_exact(N, G):
    bh = _bh()
    props, gts, cls = match_case(N, G, MATCH_SEED[(N, G)])
    assert match_case_is_clean(props, gts)
    idx, iou, lab = R.match(props, gts, cls, MATCH_K)              # f32 restatement
    if G:
        assert float(R.pairwise_iou(gts[:1], props[:1])) == 0.5                        # the planted exact 0.5 ...
        assert int(lab[0]) != MATCH_K and (int(idx[0]) != 0 or int(lab[0]) == int(cls[0]))       # ... is foreground
        i64, _, l64 = R.match(props.double(), gts.double(), cls, MATCH_K)
        assert torch.equal(i64, idx) and torch.equal(l64, lab)                         # the condition above at work
    if N >= 4 and G >= 3:
        assert int(idx[3]) == 1 and float(iou[3]) == 1.0 and int(lab[3]) == int(cls[1])   # identical ground truths: the lower one
    if N >= 3 and G:
        assert float(R.pairwise_iou(gts[:1], props[2:3])) == 0.0
    gi, gv, gl = bh.box_match(props.to(DEV), gts.to(DEV), cls.to(DEV, torch.int32), MATCH_K)
    torch.cuda.synchronize()
    assert np.array_equal(gi.cpu().numpy(), idx.numpy().astype(np.int32))
    assert np.array_equal(gl.cpu().numpy(), lab.numpy().astype(np.int32))
    assert np.array_equal(gv.cpu().numpy(), iou.numpy())


# ------------------------------------------------------------------------------------------------ weight gradient
WGRAD_SHAPES = [(1, 2, 1024), (63, 5, 1024), (65, 81, 1024), (130, 1024, 1024), (1024, 320, 1024), (3, 1024, 12544),
                (512, 1024, 12544)]
PAD_ROWS = 3


def _lattice(shape, g, keep=1.0):
    v = torch.randint(-2, 3, shape, generator=g).float() / 2
    if keep < 1.0:
        v = v * (torch.rand(shape, generator=g) < keep).float()
    return v


def _padded(t):
    """t on the device as the leading rows of a buffer whose PAD_ROWS further rows are NaN: a kernel that reads a row past n shows."""
    buf = torch.full((t.shape[0] + PAD_ROWS,) + tuple(t.shape[1:]), NAN, dtype=torch.float32, device=DEV)
    buf[:t.shape[0]] = t.to(DEV)
    return buf[:t.shape[0]]


def _wgrad_hip(bh, dy, x, kdim):
    """dW through the ABI with NaN behind the inputs and in the output; x is NCHW [n][256][7][7] for fc1, else [n][kdim]."""
    n, O = dy.shape
    dyd = _padded(dy)
    if kdim == 12544:
        xd = bh.permute_features(_padded(R.nhwc(x)))
    else:
        xd = _padded(x)
    dw = torch.full((O, kdim), NAN, dtype=torch.float32, device=DEV)
    bh._check(bh._lib.load().apse_box_fc_wgrad(bh._lib.ptr(dyd), bh._lib.ptr(xd), n, O, kdim, bh._lib.ptr(dw), bh._lib.stream_ptr()),
              "apse_box_fc_wgrad")
    torch.cuda.synchronize()
    return dw.cpu()


def _wgrad_inputs(n, O, kdim, g, lattice):
    if lattice:
        dy = _lattice((n, O), g, keep=1.0 / 8)
        x = _lattice((n, 256, 7, 7) if kdim == 12544 else (n, kdim), g)
    else:
        dy = torch.randn(n, O, generator=g) * (torch.rand(n, O, generator=g) < 0.5).float()
        x = torch.randn((n, 256, 7, 7) if kdim == 12544 else (n, kdim), generator=g)
    return dy, x


@pytest.mark.parametrize("n,O,kdim", WGRAD_SHAPES)
def test_wgrad_exact_on_lattice(n, O, kdim):
    """Every product and partial sum is a multiple of 1/4 far below 2^24: dW must equal the float64 product, whatever the order.
    The fc1 shapes are compared in the checkpoint's (c, h, w) layout."""
    g = torch.Generator().manual_seed(n * 7 + O)
    dy, x = _wgrad_inputs(n, O, kdim, g, True)
    want = dy.double().t() @ x.double().reshape(n, -1)
    got = _wgrad_hip(_bh(), dy, x, kdim)
    assert not bool(torch.isnan(got).any())
    assert np.array_equal(got.numpy().astype(np.float64), want.numpy())


@pytest.mark.parametrize("n,O,kdim", WGRAD_SHAPES)
def test_wgrad_normal_data(logdir, n, O, kdim):
    g = torch.Generator().manual_seed(n * 11 + O)
    dy, x = _wgrad_inputs(n, O, kdim, g, False)
    f64 = dy.double().t() @ x.double().reshape(n, -1)
    f32 = dy.t() @ x.reshape(n, -1)
    got = _wgrad_hip(_bh(), dy, x, kdim)
    _judge(logdir, "wgrad n=%d O=%d K=%d" % (n, O, kdim), {"dW": (got, f64, f32)})


# ------------------------------------------------------------------------------------------------ forward, bias and data gradient
@pytest.mark.parametrize("n", [1, 65, 1024])
def test_bias_and_data_gradient(logdir, n):
    """db and dX = dY W for the three layers that need one: exact on the lattice, under the arbiter on normal data; the two
    predictor layers summed into one dX, cls first."""
    bh = _bh()
    K = 80
    ws = bh._workspace(n, K, DEV)
    for lattice in (True, False):
        g = torch.Generator().manual_seed(n + (1 if lattice else 2))
        rnd = (lambda *s: _lattice(s, g)) if lattice else (lambda *s: torch.randn(*s, generator=g))
        dl, dd, d2 = rnd(n, K + 1), rnd(n, 4 * K), rnd(n, 1024)
        wc, wb, w2 = rnd(K + 1, 1024), rnd(4 * K, 1024), rnd(1024, 1024)
        dld, ddd, d2d = _padded(dl), _padded(dd), _padded(d2)
        dx = torch.full((n, 1024), NAN, dtype=torch.float32, device=DEV)
        wcd, wbd, w2d = wc.to(DEV), wb.to(DEV), w2.to(DEV)
        bh._check(bh._lib.load().apse_box_fc_dgrad(bh._lib.ptr(dld), bh._lib.ptr(wcd), n, K + 1, 1024, 0, bh._lib.ptr(dx),
                                                   bh._lib.stream_ptr()), "apse_box_fc_dgrad")
        dx = bh.fc_dgrad(ddd, wbd, into=dx)
        dx2 = bh.fc_dgrad(d2d, w2d)
        dbs = [bh.bias_grad(t, ws).cpu() for t in (dld, ddd, d2d)]
        torch.cuda.synchronize()
        ref = {}
        for dt in (torch.float64, torch.float32):
            ref[dt] = (dl.to(dt) @ wc.to(dt) + dd.to(dt) @ wb.to(dt), d2.to(dt) @ w2.to(dt), dl.to(dt).sum(0), dd.to(dt).sum(0),
                       d2.to(dt).sum(0))
        got = (dx.cpu(), dx2.cpu()) + tuple(dbs)
        names = ("dX_predictors", "dX_fc2", "db_cls", "db_bbox", "db_fc2")
        if lattice:
            for name, a, b in zip(names, got, ref[torch.float64]):
                assert np.array_equal(a.numpy().astype(np.float64), b.numpy()), name
        else:
            _judge(logdir, "dgrad / bias n=%d" % n, {k: (a, b, c) for k, a, b, c in zip(names, got, ref[torch.float64],
                                                                                        ref[torch.float32])})


@pytest.mark.parametrize("n,O,kdim", [(1, 5, 1024), (65, 81, 1024), (130, 1024, 1024), (3, 1024, 12544)])
def test_fc_forward(logdir, n, O, kdim):
    bh = _bh()
    g = torch.Generator().manual_seed(n + O)
    x = torch.randn(n, kdim, generator=g)
    w = torch.randn(O, kdim, generator=g) * (2.0 / kdim) ** 0.5
    b = torch.randn(O, generator=g) * 0.1
    y = torch.full((n, O), NAN, dtype=torch.float32, device=DEV)
    xd, wd, bd = _padded(x), _padded(w), b.to(DEV)
    ws = torch.full_like(bh._workspace(n, 4, DEV), NAN)
    bh._check(bh._lib.load().apse_box_fc_forward(bh._lib.ptr(xd), bh._lib.ptr(wd), bh._lib.ptr(bd), n, O, kdim, 1, bh._lib.ptr(y),
                                                 bh._lib.ptr(ws), ws.numel() * 4, bh._lib.stream_ptr()), "apse_box_fc_forward")
    lin = bh.fc_forward(x.to(DEV), w.to(DEV), None, False)
    torch.cuda.synchronize()
    f64 = x.double() @ w.double().t()
    f32 = x @ w.t()
    _judge(logdir, "forward n=%d O=%d K=%d" % (n, O, kdim),
           {"relu(xW+b)": (y, torch.relu(f64 + b.double()), torch.relu(f32 + b)), "xW": (lin, f64, f32)})
    # the lattice: exact, and the permutation puts the pooled (h, w, c) features into fc1's (c, h, w) order
    xl, wl = _lattice((n, kdim), g), _lattice((O, kdim), g, keep=1.0 / 8)
    got = bh.fc_forward(xl.to(DEV), wl.to(DEV), None, False)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), (xl.double() @ wl.double().t()).numpy())
    # a row's result does not depend on how many rows share the call
    assert torch.equal(bh.fc_forward(x[:1].to(DEV), w.to(DEV), None, False), lin[:1])
    if kdim == 12544:
        f = torch.randn(n, 256, 7, 7, generator=g)
        assert torch.equal(bh.permute_features(R.nhwc(f).to(DEV)).cpu(), f.reshape(n, -1))


# ------------------------------------------------------------------------------------------------ loss
def loss_case(n, K, seed):
    """Rows of every kind as far as n allows: background, every foreground class (K - 1 included), a row whose prediction equals
    its target (proposal = ground truth, deltas 0: gradient exactly 0), logits of +-80, an all-equal row (argmax tie)."""
    g = torch.Generator().manual_seed(seed)
    labels, props, gts = R.sample_batch(n, K, seed)
    for i in range(min(n, K + 1)):
        labels[i] = (K - 1 + i) % (K + 1) if n > 1 else K - 1          # K - 1, background, 0, 1, ...
    logits = torch.randn(n, K + 1, generator=g) * 2
    deltas = torch.randn(n, 4 * K, generator=g)
    exact_row = None
    if n >= 4:
        r = n - 1
        labels[r] = K - 1
        gts[r] = props[r]
        deltas[r, 4 * (K - 1):] = 0.0
        exact_row = r
        logits[n - 2] = 80.0 * (torch.arange(K + 1) % 2 * 2 - 1).float()
        logits[n - 3] = 0.25
    return logits, deltas, labels, props, gts, exact_row


def loss_case_is_clean(deltas, labels, props, gts, K, beta, exact_row):
    """beta 0: smooth_l1 is |d| and its gradient jumps at d = 0; no compared difference other than the planted zeros may lie
    within 1e-4 of 0 (float64), or the sign would be a rounding question."""
    if beta >= 1e-5:
        return True
    fg = torch.nonzero(labels < K).squeeze(1)
    if fg.numel() == 0:
        return True
    t = R.get_deltas(props.double(), gts.double())
    cols = 4 * labels[fg][:, None] + torch.arange(4)
    d = deltas.double()[fg[:, None], cols] - t[fg]
    if exact_row is not None:
        d = d[fg != exact_row]
    return bool((d.abs() > 1e-4).all())


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("n", [1, 64, 65, 1024])
@pytest.mark.parametrize("K", [1, 4, 80])
def test_loss_and_gradient(logdir, K, n, beta):
    bh = _bh()
    logits, deltas, labels, props, gts, exact_row = loss_case(n, K, 1000 * K + n)
    assert loss_case_is_clean(deltas, labels, props, gts, K, beta, exact_row)
    gcls, gbox = 0.5, 2.0
    ref = {}
    for dt in (torch.float64, torch.float32):
        lg, dl = logits.to(dt).requires_grad_(True), deltas.to(dt).requires_grad_(True)
        lc, lb = R.box_losses(lg, dl, labels, props.to(dt), gts.to(dt), beta)
        (gcls * lc + gbox * lb).backward()
        ref[dt] = (torch.stack([lc.detach(), lb.detach()]), lg.grad, dl.grad)
    ws = bh._workspace(n, K, DEV)
    ld, dd, lab = logits.to(DEV), deltas.to(DEV), labels.to(DEV, torch.int32)
    pd, gd = props.to(DEV), gts.to(DEV)
    out8 = bh.loss_forward(ld, dd, lab, pd, gd, ws, beta=beta)
    dlg, ddl = bh.loss_backward(ld, dd, lab, pd, gd, torch.tensor([gcls], device=DEV), torch.tensor([gbox], device=DEV), beta=beta)
    dlg1, ddl1 = bh.loss_backward(ld, dd, lab, pd, gd, None, None, beta=beta)
    torch.cuda.synchronize()
    out8, dlg, ddl = out8.cpu(), dlg.cpu(), ddl.cpu()
    assert bool(torch.isfinite(out8).all()) and bool(torch.isfinite(dlg).all()) and bool(torch.isfinite(ddl).all())
    a, f = ref[torch.float64], ref[torch.float32]
    _judge(logdir, "loss K=%d n=%d beta=%g" % (K, n, beta),
           {"loss_cls": (out8[0], a[0][0], f[0][0]), "loss_box_reg": (out8[1], a[0][1], f[0][1]), "dlogits": (dlg, a[1], f[1]),
            "ddeltas": (ddl, a[2], f[2])})
    # NULL gradient scalars mean 1
    _judge(logdir, "loss K=%d n=%d beta=%g unit" % (K, n, beta),
           {"dlogits": (dlg1.cpu() * gcls, a[1], f[1]), "ddeltas": (ddl1.cpu() * gbox, a[2], f[2])})
    acc, fg_acc, fn, nfg, nbg = R.box_stats(logits, labels)
    want = np.array([acc, fg_acc, fn, nfg, nbg], np.float64).astype(np.float32)
    assert np.array_equal(out8[2:7].numpy(), want), (out8, want)
    assert float(out8[7]) == 0.0
    # ddeltas: exactly 0 outside the four columns of a foreground row's class, and on the row that equals its target
    mask = torch.zeros(n, 4 * K, dtype=torch.bool)
    fg = torch.nonzero(labels < K).squeeze(1)
    mask[fg[:, None], 4 * labels[fg][:, None] + torch.arange(4)] = True
    assert float(ddl[~mask].abs().max()) == 0.0 if bool((~mask).any()) else True
    if exact_row is not None:
        assert float(ddl[exact_row].abs().max()) == 0.0


def test_zero_rois():
    """n = 0 launches nothing; BoxHead.forward returns zeros whose gradients reach all eight parameters."""
    bh = _bh()
    lib = bh._lib.load()
    w4 = (C.c_float * 4)(10, 10, 5, 5)
    out = torch.full((8,), 7.0, device=DEV)
    assert lib.apse_box_loss_forward(None, None, None, None, None, 0, 4, w4, 0.0, bh._lib.ptr(out), None, 0, bh._lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0] * 8
    head = bh.BoxHead(4, DEV)
    losses = head(torch.zeros(0, 7, 7, 256, device=DEV), torch.zeros(0), torch.zeros(0, 4), torch.zeros(0, 4))
    assert float(losses["loss_cls"].detach()) == 0.0 and float(losses["loss_box_reg"].detach()) == 0.0
    (losses["loss_cls"] + losses["loss_box_reg"]).backward()
    ps = list(head.parameters())
    assert len(ps) == 8 and all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in ps)
    lg, dl = head.predict(torch.zeros(0, 7, 7, 256, device=DEV))
    assert tuple(lg.shape) == (0, 5) and tuple(dl.shape) == (0, 16)


# ------------------------------------------------------------------------------------------------ whole head
def test_whole_head_one_step(logdir):
    """All eight gradients of loss_cls + loss_box_reg, K = 4, n = 130, on an exact-forward state: f32 and f64 see the same ReLU
    masks, so the comparison is not decided by sign flips at rounding distance from 0."""
    bh = _bh()
    K, n = 4, 130
    sd = R.exact_forward_state(K, 5)
    x = R.exact_features(n, 6)
    labels, props, gts = R.sample_batch(n, K, 7)
    l64, g64 = R.head_step(x.double(), sd, labels, props, gts, torch.float64)
    l32, g32 = R.head_step(x, sd, labels, props, gts, torch.float32)
    head = bh.BoxHead(K, DEV)
    head.load_state_dict(sd)
    losses = head(R.nhwc(x).to(DEV), labels, props, gts)
    (losses["loss_cls"] + losses["loss_box_reg"]).backward()
    torch.cuda.synchronize()
    lg, dl = head.predict(R.nhwc(x).to(DEV))
    o64 = R.head_outputs(x.double(), {k: v.double() for k, v in sd.items()})
    o32 = R.head_outputs(x, sd)
    outputs = {"loss_cls": (losses["loss_cls"], l64[0], l32[0]), "loss_box_reg": (losses["loss_box_reg"], l64[1], l32[1]),
               "logits": (lg, o64[0], o32[0]), "deltas": (dl, o64[1], o32[1])}
    for k, p in head.named_parameters():
        outputs[k] = (p.grad, g64[k], g32[k])
    _judge(logdir, "whole head K=4 n=130", outputs)
    stats = head.last_stats.cpu()
    assert float(stats[5]) == float((labels < K).sum()) and float(stats[5] + stats[6]) == n


# ------------------------------------------------------------------------------------------------ determinism
def _three_steps(n, K, opt_kind):
    from apse_uav_amd import optim
    bh = _bh()
    g = torch.Generator().manual_seed(n)
    x = torch.relu(torch.randn(n, 7, 7, 256, generator=g)).to(DEV)
    labels, props, gts = R.sample_batch(n, K, n + 1)
    head = bh.BoxHead(K, DEV)
    head.load_state_dict(R.seeded_state(K, 31))
    params = list(head.parameters())
    opt = (optim.SGD if opt_kind == "apse" else torch.optim.SGD)(params, lr=0.02, momentum=0.9)
    blob = []
    for _ in range(3):
        opt.zero_grad()
        losses = head(x, labels, props, gts)
        loss = losses["loss_cls"] + losses["loss_box_reg"]
        loss.backward()
        blob.append(loss.detach().cpu().numpy().tobytes())
        opt.step()
    torch.cuda.synchronize()
    blob += [p.detach().cpu().numpy().tobytes() for p in params]
    return b"".join(blob), float(loss.detach())


@pytest.mark.parametrize("n,opt_kind", [(130, "apse"), (1024, "apse"), (130, "torch"), (1024, "torch")])
def test_determinism(n, opt_kind):
    a, la = _three_steps(n, 4, opt_kind)
    b, lb = _three_steps(n, 4, opt_kind)
    assert np.isfinite(la) and a == b


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_on_the_device():
    from apse_uav_amd import _lib
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    bh = _bh()
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    ti = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, ip, s = _lib.ptr(t), _lib.ptr(ti), _lib.stream_ptr()
    w4 = (C.c_float * 4)(10, 10, 5, 5)
    assert lib.apse_box_fc_wgrad(p, p, 1025, 4, 4, p, s) == -1 and b"APSE_BOX_TRAIN_MAX_N" in lib.apse_last_error(None)
    assert lib.apse_box_loss_forward(p, p, ip, p, p, 1, 81, w4, 0.0, p, p, 1 << 10, s) == -1
    assert lib.apse_box_loss_forward(p, p, ip, p, p, 1, 0, w4, 0.0, p, p, 1 << 10, s) == -1
    assert lib.apse_box_match(p, 1, p, ip, 4097, 4, 0.5, ip, p, ip, s) == -1
    assert lib.apse_box_loss_forward(p, p, ip, p, p, 2, 1, w4, 0.0, p, p, 95, s) == -1 and b"workspace" in lib.apse_last_error(None)
    assert lib.apse_box_fc_forward(None, p, p, 1, 4, 4, 0, p, p, 256, s) == -1
    assert lib.apse_box_fc_forward(p, p, p, 1, 4, 4096, 0, p, p, 8 * 4 * 4 - 1, s) == -1 and b"workspace" in lib.apse_last_error(None)
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0                               # nothing was launched
    with pytest.raises(_lib.ApseError):
        bh.BoxHead(4, DEV)(torch.zeros(1025, 7, 7, 256, device=DEV), torch.zeros(1025), torch.zeros(1025, 4), torch.zeros(1025, 4))
    c4 = TrackRCNN(setup_cfg(num_classes=4, arch="C4"))
    with pytest.raises(NotImplementedError):
        c4.box_roi_features(np.zeros((1, 4), np.float32))
    with pytest.raises(NotImplementedError):
        c4.rpn_proposals(frames=torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError):
        bh.BoxHead.from_cfg(setup_cfg(num_classes=4, arch="C4"))


# ------------------------------------------------------------------------------------------------ agreement with inference
@pytest.fixture(scope="module")
def predictor():
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg(num_classes=4)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    return TrackPredictor(cfg, state_dict=synthetic_detector_state(0, (1, 1, 1, 1)))


def _detections(insts):
    return (insts[0].pred_boxes.tensor.clone(), insts[0].scores.clone(), insts[0].pred_classes.clone())


def test_agreement_with_inference(predictor, logdir):
    from apse_uav_amd.synthetic import SyntheticSequence
    bh = _bh()
    model = predictor.model
    K = 4
    frames = torch.from_numpy(SyntheticSequence("dynamic", 360, 640).frame(0)[None]).cuda()
    insts, _ = model.inference_frames(frames)
    torch.cuda.synchronize()
    first = _detections(insts)
    count = int(model.last_results.prop_count[0])
    post = int(predictor.cfg.MODEL.RPN.POST_NMS_TOPK_TEST)
    assert 0 < count <= post
    tap_props = model.debug_tensor("proposals").reshape(-1, 4)[:count].clone()
    tap_pooled = model.debug_tensor("box_pooled").reshape(-1, 7, 7, 256)[:count].clone()
    tap_probs = model.debug_tensor("box_probs").reshape(-1, K + 1)[:count].clone()
    props = model.rpn_proposals(frames=frames)
    assert len(props) == 1 and tuple(props[0].shape) == (count, 4)
    assert torch.equal(props[0], tap_props)
    feats = model.box_roi_features(props[0])
    torch.cuda.synchronize()
    assert torch.equal(feats, tap_pooled)
    head = bh.BoxHead(K, DEV)
    head.load_state_dict(model._state)
    logits, _ = head.predict(feats)
    got = torch.softmax(logits, dim=1)
    sd = {k: v.cpu() for k, v in head.state_dict().items()}
    xc = feats.cpu().permute(0, 3, 1, 2).contiguous()
    p64 = torch.softmax(R.head_outputs(xc.double(), {k: v.double() for k, v in sd.items()})[0], dim=1)
    p32 = torch.softmax(R.head_outputs(xc, sd)[0], dim=1)
    rows = {}
    for name, (a, b) in {"train_vs_torch": (got, p32), "train_vs_inference": (got, tap_probs), "inference_vs_torch": (tap_probs, p32)}.items():
        eh, ef, bound, ok = R.arbiter(a, p64, b)
        rows[name] = {"first": eh, "second": ef, "bound": bound, "ok": ok}
    _log(logdir, "train / inference box_probs n=%d" % count, rows)
    assert rows["train_vs_torch"]["ok"] and rows["train_vs_inference"]["ok"], rows
    head.push_into(predictor)
    insts2, _ = model.inference_frames(frames)
    torch.cuda.synchronize()
    second = _detections(insts2)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
