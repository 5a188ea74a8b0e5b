"""-m gpu: conv_winograd_f32 with its Cin split and its <8, 8> block geometry, alone, through apse_winograd_conv2d_split, at the
shapes where they can go wrong (tests/winograd_split_cases.py; the CPU side is tests/test_winograd_split_cases.py).

* integer lattices: the f32 output has to EQUAL the float64 convolution at every element for every split and geometry -- one slice
  per share (the loop's fetches past a share's end land in the next share's range), uneven shares, splits 5 and 8, grids of 1 .. 12
  and 18 blocks, partial blocks, B = 3, ReLU on / off, bias and bias == NULL;
* every element written, nothing else: y and the workspace are NaN-filled between NaN guard bands; afterwards y holds no NaN,
  no guard word changed, and the workspace words behind splitk M Cout are still NaN;
* a result depends on its inputs only: NaN / Inf neighbours in the batch, a second launch, a dirty workspace;
* Gaussian data: inside the derived bound (Cin + 16 + splitk roundings), rms within 1.5 x of winograd.emulate(split=...).
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import winograd_cases as wc
import winograd_split_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 1024                                   # floats: 4 KiB in front of and behind x, y and the workspace
WS_TAIL = 4096                                 # workspace floats behind the slabs, handed to the call, that it must not touch
NAN_BITS = 0x7FC00000                          # what torch.full(nan) writes


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "winograd.log"), "a") as f:
        f.write("split/" + name + " " + json.dumps(obj) + "\n")


def _guarded(n, payload=None):
    """n floats in the middle of a NaN-filled device allocation: (whole buffer, the view)."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    view = buf[GUARD:GUARD + n]
    if payload is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(payload).reshape(-1)))
    return buf, view


def _all_nan_bits(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


def _desc(B, H, W, Cin, Cout, relu, split, over=None):
    from apse_uav_amd import _lib
    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad, d.relu = B, H, W, Cin, Cout, 3, 3, 1, 1, int(relu)
    d.splitk = split
    for k, v in (over or {}).items():
        setattr(d, k, v)
    return d


@functools.lru_cache(maxsize=None)
def _packed(kind, name, seed):
    from apse_uav_amd import _lib
    _, w, _ = getattr(wc, kind)(sc.shape(sc.BY_NAME[name]), seed)
    packed = np.full(16 * w.shape[0] * w.shape[1], np.nan, np.float32)
    assert _lib.load().apse_winograd_pack_filter(_lib.ptr(w), w.shape[0], w.shape[1], _lib.ptr(packed)) == 0
    return torch.from_numpy(packed).cuda()


def run(x, wd, cout, bias, relu, split, geom, ws=None):
    """One launch: x NHWC f32, wd packed filters on the device -> y NHWC f32 (host).  Asserts the call's success, the guard bands of
    x, y and the workspace, and that the workspace behind the slabs is untouched.  ws: a (buffer, view) pair to reuse as it is."""
    from apse_uav_amd import _lib
    B, H, W, Cin = x.shape
    xbuf, xv = _guarded(x.size, x)
    ybuf, yv = _guarded(B * H * W * cout)
    slabs = split * B * H * W * cout if split > 1 else 0
    wsbuf, wsv = ws if ws is not None else _guarded(slabs + WS_TAIL)
    assert wsv.numel() >= slabs + WS_TAIL
    bd = None if bias is None else torch.from_numpy(np.ascontiguousarray(bias, np.float32)).cuda()
    d = _desc(B, H, W, Cin, cout, relu, split)
    rc = _lib.load().apse_winograd_conv2d_split(C.byref(d), _lib.ptr(xv), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(yv), _lib.ptr(wsv),
                                                wsv.numel() * 4, geom, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for buf, v, what in ((ybuf, yv, "y"), (xbuf, xv, "x"), (wsbuf, wsv, "ws")):
        assert _all_nan_bits(buf[:GUARD]) and _all_nan_bits(buf[GUARD + v.numel():]), "write outside " + what
    if ws is None:
        assert _all_nan_bits(wsv[slabs:]), "workspace written behind the slabs"
        if np.isfinite(x).all():                       # (a NaN input legitimately leaves NaN partial sums in its image's slab rows)
            assert not bool(torch.isnan(wsv[:slabs]).any()), "slab words never written"
    return yv.cpu().numpy().reshape(B, H, W, cout)


def run_case(case, kind, bias=True, relu=False, seed=0, x=None, ws=None):
    name, _, _, _, _, Cout, split, geom = case
    xx, _, b = getattr(wc, kind)(sc.shape(case), seed)
    return run(xx if x is None else x, _packed(kind, name, seed), Cout, b if bias else None, relu, split, geom, ws)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _lattice_ref(name, with_bias):
    x, w, b = wc.lattice(sc.shape(sc.BY_NAME[name]))
    return wc.ref64(x, w, b if with_bias else None, False)


# ---------------------------------------------------------------------------------------------- exact on the lattice
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_exact_on_lattice(case, relu, with_bias):
    y = run_case(case, "lattice", with_bias, relu)
    assert not np.isnan(y).any(), "%d elements never written" % int(np.isnan(y).sum())
    ref = _lattice_ref(case[0], with_bias)
    ref = np.maximum(ref, 0) if relu else ref
    bad = np.argwhere(y.astype(np.float64) != ref)
    assert np.array_equal(y.astype(np.float64), ref), (len(bad), [tuple(int(v) for v in i) for i in bad[:6]])


@pytest.mark.parametrize("geom", [0, 1])
@pytest.mark.parametrize("split", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_split_of_cin64_is_exact(split, geom):
    """One shape, every split its 8 slices allow, both geometries: the same float64 values."""
    case = ("g1_17x33", 1, 17, 33, 64, 128)
    x, w, b = wc.lattice(case)
    from apse_uav_amd import _lib
    packed = np.empty(16 * w.shape[0] * w.shape[1], np.float32)
    assert _lib.load().apse_winograd_pack_filter(_lib.ptr(w), w.shape[0], w.shape[1], _lib.ptr(packed)) == 0
    y = run(x, torch.from_numpy(packed).cuda(), 128, b, True, split, geom)
    assert np.array_equal(y.astype(np.float64), wc.ref64(x, w, b, True))


def test_unsplit_geometry0_is_the_existing_entry():
    """split 1 in geometry 0 is apse_winograd_conv2d's launch: the same bits on Gaussian data."""
    from apse_uav_amd import _lib
    case = sc.BY_NAME["g0_batch"]
    x, w, b = wc.normal(sc.shape(case))
    wd = _packed("normal", case[0], 0)
    got = run(x, wd, case[5], b, True, 1, 0)
    xd, bd, y = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda(), torch.full((x.size // case[4] * case[5],), float("nan"), device="cuda")
    d = _desc(*sc.shape(case)[1:], True, 0)
    assert _lib.load().apse_winograd_conv2d(C.byref(d), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got).reshape(-1), _bits(y.cpu().numpy()))


# ---------------------------------------------------------------------------------------------- Gaussian data against float64
@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_normal_data_vs_float64(case, logdir):
    """|y - y64| <= (Cin + 16 + splitk) 2^-24 magnitude at every element; rms(y - y64) <= 1.5 x the rms error of
    winograd.emulate(split=...) on the same inputs (the factor of tests/test_gpu_winograd_edges.py).  Small cases pool seeds until
    the rms stands on >= 10^4 outputs."""
    name, B, H, W, Cin, Cout, split, geom = case
    seeds = -(-10000 // (B * H * W * Cout))
    se_k = se_e = 0.0
    n = 0
    worst = 0.0
    for seed in range(seeds):
        x, w, b = wc.normal(sc.shape(case), seed)
        y = run_case(case, "normal", True, False, seed)
        assert not np.isnan(y).any()
        y64 = wc.ref64(x, w, b, False)
        err = np.abs(y.astype(np.float64) - y64)
        ratio = err / sc.bound(x, w, b, split)
        worst = max(worst, float(ratio.max()))
        assert int((ratio > 1.0).sum()) == 0, (seed, int((ratio > 1.0).sum()), worst)
        emu = sc.emulate(x, w, b, False, split)
        se_k += float((err ** 2).sum())
        se_e += float(((emu.astype(np.float64) - y64) ** 2).sum())
        n += emu.size
    rms_k, rms_e = (se_k / n) ** 0.5, (se_e / n) ** 0.5
    rec = dict(outputs=n, seeds=seeds, max_err_over_bound=worst, rms_kernel=rms_k, rms_emulation=rms_e, rms_ratio=rms_k / rms_e)
    _log(logdir, "normal/" + name, rec)
    print(name, rec)
    assert rms_k <= 1.5 * rms_e, rec


# ---------------------------------------------------------------------------------------------- a result depends only on its inputs
def _hostile(shape, seed):
    r = np.random.default_rng(seed)
    return r.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=shape)


@pytest.mark.parametrize("name", ["g0_batch", "g1_batch"])
@pytest.mark.parametrize("kind", ["lattice", "normal"])
def test_neighbouring_images_do_not_leak(kind, name):
    case = sc.BY_NAME[name]
    x, w, b = getattr(wc, kind)(sc.shape(case))
    alone = run(x[1:2], _packed(kind, name, 0), case[5], b, False, case[6], case[7])
    x = x.copy()
    x[0] = np.nan
    x[2] = _hostile(x[2].shape, 5)
    y = run_case(case, kind, x=x)
    assert not np.isnan(alone).any() and not np.isinf(alone).any()
    assert np.array_equal(_bits(y[1]), _bits(alone[0]))
    if kind == "lattice":
        assert np.array_equal(y[1].astype(np.float64), _lattice_ref(name, True)[1])


@pytest.mark.parametrize("name", ["g1_17x33", "g0_batch", "g1_nwg12", "g1_res4"])
def test_two_launches_and_a_dirty_workspace_same_bits(name):
    """A second launch, and a launch on the NaN-filled workspace a larger launch has used, give the first launch's bits."""
    case = sc.BY_NAME[name]
    a = run_case(case, "normal")
    assert not np.isnan(a).any()
    assert np.array_equal(_bits(a), _bits(run_case(case, "normal")))
    big = ("big", case[1], case[2] + 2, case[3] + 3, case[4], case[5])
    slabs = case[6] * big[1] * big[2] * big[3] * big[5]
    ws = _guarded(slabs + WS_TAIL)
    xb, wb, bb = wc.normal(big)
    run(xb, _packed("normal", name, 0), case[5], bb, False, case[6], case[7], ws=ws)       # the larger launch (same filters)
    ws[1][::3] = float("nan")                                                              # ... and NaN on top of what it left
    assert np.array_equal(_bits(a), _bits(run_case(case, "normal", ws=ws)))


# ---------------------------------------------------------------------------------------------- refusals
REFUSED = [dict(stride=2), dict(pad=0), dict(KH=1), dict(KH=1, KW=1, pad=0), dict(Cout=96), dict(Cin=24), dict(res_mode=1), dict(prec=1),
           dict(x_st=1), dict(y_st=2), dict(splitk=0), dict(splitk=-1), dict(splitk=5), dict(splitk=8)]


def _refusal_buffers():
    """Buffers that hold any of the described shapes (up to 64 input / 128 output channels at 8 x 8, 8 splits), so that a call
    accepted by mistake still stays inside them."""
    r = np.random.default_rng(3)
    x = torch.from_numpy(r.standard_normal(8 * 8 * 64).astype(np.float32)).cuda()
    wu = torch.from_numpy(r.standard_normal(16 * 128 * 64).astype(np.float32)).cuda()
    b = torch.zeros(128, device="cuda")
    ybuf, yv = _guarded(8 * 8 * 128)
    wsbuf, wsv = _guarded(8 * 8 * 8 * 128)
    return x, wu, b, ybuf, yv, wsbuf, wsv


def _call(d, x, wu, b, yv, wsv, ws_bytes, geom):
    from apse_uav_amd import _lib
    rc = _lib.load().apse_winograd_conv2d_split(None if d is None else C.byref(d), _lib.ptr(x), _lib.ptr(wu), _lib.ptr(b), _lib.ptr(yv),
                                                _lib.ptr(wsv), ws_bytes, geom, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_refusal_baseline_is_accepted():
    """The call the refusals below vary in one respect each is itself taken: Cin 32 in 4 shares, geometry 1."""
    x, wu, b, ybuf, yv, wsbuf, wsv = _refusal_buffers()
    n = 8 * 8 * 64
    assert _call(_desc(1, 8, 8, 32, 64, 0, 4), x, wu, b, yv, wsv, 4 * n * 4, 1) == 0
    assert not bool(torch.isnan(yv[:n]).any()) and _all_nan_bits(yv[n:]) and _all_nan_bits(ybuf[:GUARD]) and _all_nan_bits(ybuf[GUARD + yv.numel():])
    assert not bool(torch.isnan(wsv[:4 * n]).any()) and _all_nan_bits(wsv[4 * n:])


@pytest.mark.parametrize("over", REFUSED, ids=["-".join("%s%d" % kv for kv in o.items()) for o in REFUSED])
def test_refuses_descriptor(over):
    x, wu, b, ybuf, yv, wsbuf, wsv = _refusal_buffers()
    d = _desc(1, 8, 8, 32, 64, 0, 4, over)
    assert _call(d, x, wu, b, yv, wsv, wsv.numel() * 4, 1) != 0
    assert _all_nan_bits(ybuf) and _all_nan_bits(wsbuf)


@pytest.mark.parametrize("what", ["ws_one_byte_short", "ws_null", "geometry2", "geometry-1", "desc_null"])
def test_refuses_workspace_and_geometry(what):
    x, wu, b, ybuf, yv, wsbuf, wsv = _refusal_buffers()
    d = _desc(1, 8, 8, 32, 64, 0, 4)
    need = 4 * 8 * 8 * 64 * 4
    if what == "ws_one_byte_short":
        rc = _call(d, x, wu, b, yv, wsv, need - 1, 1)
    elif what == "ws_null":
        rc = _call(d, x, wu, b, yv, None, need, 1)
    elif what == "desc_null":
        rc = _call(None, x, wu, b, yv, wsv, need, 1)
    else:
        rc = _call(d, x, wu, b, yv, wsv, need, int(what[8:]))
    assert rc != 0
    assert _all_nan_bits(ybuf) and _all_nan_bits(wsbuf)
