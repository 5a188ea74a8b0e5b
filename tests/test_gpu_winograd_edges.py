"""-m gpu: conv_winograd_f32 alone, through apse_winograd_pack_filter / apse_winograd_conv2d, at the shapes where it can go wrong
(tests/winograd_cases.py; the CPU side of the argument is tests/test_winograd_cases.py).

* integer lattices: the f32 output has to EQUAL the float64 convolution, every element, every border pixel -- one and two k-slices,
  1 .. 16 N tiles, grids of 1 .. 12 and 384 blocks (every residue of the XCD remap), one-pixel maps, blocks that hold a single row
  or column of pixels, ReLU on / off, bias and bias == NULL; and it equals what the direct kernel gives (plan.hip's alternative);
* Gaussian data: element by element inside the derived bound, and in rms within 1.5 x of the numpy emulation of the kernel's order;
* a result depends on nothing but its inputs: NaN / Inf in the neighbouring images, other N tiles, a second launch.
Every launch reads x from inside a larger allocation whose guard bands are NaN, and writes into a NaN-filled y whose guard bands
must come back untouched; a NaN left inside y is a pixel nobody wrote.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import winograd_cases as wc

pytestmark = pytest.mark.gpu

GUARD = 1024                                   # floats: 4 KiB in front of and behind x and y
NAN_BITS = 0x7FC00000                          # what torch.full(nan) writes


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "winograd.log"), "a") as f:
        f.write("edges/" + name + " " + json.dumps(obj) + "\n")


def _guarded(n, payload=None):
    """n floats in the middle of a NaN-filled device allocation: (whole buffer, the view)."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    view = buf[GUARD:GUARD + n]
    if payload is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(payload).reshape(-1)))
    return buf, view


def _guards_intact(buf, n):
    bits = buf.view(torch.int32)
    return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + n:] == NAN_BITS).all())


def _desc(B, H, W, Cin, Cout, relu, over=None):
    from apse_uav_amd import _lib
    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad, d.relu = B, H, W, Cin, Cout, 3, 3, 1, 1, int(relu)
    for k, v in (over or {}).items():
        setattr(d, k, v)
    return d


def pack(w):
    """apse_winograd_pack_filter of OIHW f32 filters -> host array of 16 * Cout * Cin floats."""
    from apse_uav_amd import _lib
    w = np.ascontiguousarray(w, np.float32)
    packed = np.full(16 * w.shape[0] * w.shape[1], np.nan, np.float32)
    assert _lib.load().apse_winograd_pack_filter(_lib.ptr(w), w.shape[0], w.shape[1], _lib.ptr(packed)) == 0
    return packed


def run(x, w, bias, relu):
    """One launch: x NHWC f32, w OIHW f32, bias f32 or None -> y NHWC f32 (host).  Asserts the call's success and y's guard bands."""
    from apse_uav_amd import _lib
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    xbuf, xv = _guarded(x.size, x)
    ybuf, yv = _guarded(B * H * W * Cout)
    wd = torch.from_numpy(pack(w)).cuda()
    bd = None if bias is None else torch.from_numpy(np.ascontiguousarray(bias, np.float32)).cuda()
    d = _desc(B, H, W, Cin, Cout, relu)
    rc = _lib.load().apse_winograd_conv2d(C.byref(d), _lib.ptr(xv), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(yv), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert _guards_intact(ybuf, yv.numel()), "write outside y"
    assert _guards_intact(xbuf, xv.numel())
    return yv.cpu().numpy().reshape(B, H, W, Cout)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _lattice_ref(name, with_bias):
    x, w, b = wc.lattice(wc.BY_NAME[name])
    return wc.ref64(x, w, b if with_bias else None, False)


# ---------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("cout", [64, 192])
@pytest.mark.parametrize("cin", [8, 64, 512])
def test_pack_filter_bytes(cin, cout):
    _, w, _ = wc.normal(("pack", 1, 1, 1, cin, cout))
    got = pack(w)
    assert got.tobytes() == wc.pack_layout(wc.wg.filter_transform(w)).tobytes()
    _, w, _ = wc.lattice(("pack", 1, 1, 1, cin, cout))
    assert pack(w).tobytes() == wc.pack_layout(wc.wg.filter_transform(w)).tobytes()


def test_pack_filter_refusals():
    from apse_uav_amd import _lib
    lib = _lib.load()
    w = np.ones((64, 32, 3, 3), np.float32)
    out = np.full(16 * 64 * 32, np.nan, np.float32)
    for cout, cin in ((64, 4), (64, 24), (0, 32)):
        assert lib.apse_winograd_pack_filter(_lib.ptr(w), cout, cin, _lib.ptr(out)) != 0, (cout, cin)
    assert lib.apse_winograd_pack_filter(None, 64, 32, _lib.ptr(out)) != 0
    assert lib.apse_winograd_pack_filter(_lib.ptr(w), 64, 32, None) != 0
    assert np.isnan(out).all()
    assert lib.apse_winograd_pack_filter(_lib.ptr(w), 64, 32, _lib.ptr(out)) == 0 and not np.isnan(out).any()


# ---------------------------------------------------------------------------------------------- exact on the lattice
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("case", wc.CASES, ids=wc.CASE_IDS)
def test_exact_on_lattice(case, relu, with_bias):
    x, w, b = wc.lattice(case)
    y = run(x, w, b if with_bias else None, relu)
    assert not np.isnan(y).any(), "%d elements never written" % int(np.isnan(y).sum())
    ref = _lattice_ref(case[0], with_bias)
    ref = np.maximum(ref, 0) if relu else ref
    bad = np.argwhere(y.astype(np.float64) != ref)
    assert np.array_equal(y.astype(np.float64), ref), (len(bad), [tuple(int(v) for v in i) for i in bad[:6]])


@pytest.mark.parametrize("case", wc.CASES, ids=wc.CASE_IDS)
def test_lattice_equals_direct_kernel(case):
    """The two kernels plan.hip chooses between for these layers give the same values where both are exact."""
    from hip_helpers import hip_conv2d
    x, w, b = wc.lattice(case)
    y = run(x, w, b, True)
    direct = hip_conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(w), torch.from_numpy(b), 1, 1, True, cfg=-1)
    assert np.array_equal(y, direct.permute(0, 2, 3, 1).numpy())


# ---------------------------------------------------------------------------------------------- Gaussian data against float64
@pytest.mark.parametrize("case", wc.CASES, ids=wc.CASE_IDS)
def test_normal_data_vs_float64(case, logdir):
    """|y - y64| <= bound at every element; rms(y - y64) <= 1.5 x the rms error of winograd.emulate on the same inputs, where the
    emulation is affordable (the whole case, or image 0 of the 256-channel one).  The emulation is the reference of that ratio, not
    the kernel: the MFMA takes a slice's channels as 0, 4, 1, 5, .. and adds its two products in an order of its own, which changes
    which roundings occur, not how many.  Small cases pool seeds until the rms stands on >= 10^4 outputs.  The fraction of outputs
    bit-equal to the emulation is logged for whoever touches the k loop next; nothing is asserted of it."""
    name, B, H, W, Cin, Cout = case
    n_img = B if wc.emulation_affordable(case) else 1                 # images that go through the emulation
    seeds = -(-10000 // (n_img * H * W * Cout))
    se_k = se_e = 0.0
    n = same = 0
    worst = 0.0
    for seed in range(seeds):
        x, w, b = wc.normal(case, seed)
        y = run(x, w, b, False)
        assert not np.isnan(y).any()
        y64 = wc.ref64(x, w, b, False)
        err = np.abs(y.astype(np.float64) - y64)
        ratio = err / wc.bound(x, w, b)
        worst = max(worst, float(ratio.max()))
        assert int((ratio > 1.0).sum()) == 0, (seed, int((ratio > 1.0).sum()), worst)
        emu = wc.emulate(x[:n_img], w, b, False)
        se_k += float((err[:n_img] ** 2).sum())
        se_e += float(((emu.astype(np.float64) - y64[:n_img]) ** 2).sum())
        same += int((_bits(emu) == _bits(y[:n_img])).sum())
        n += emu.size
    rms_k, rms_e = (se_k / n) ** 0.5, (se_e / n) ** 0.5
    rec = dict(outputs=n, seeds=seeds, max_err_over_bound=worst, rms_kernel=rms_k, rms_emulation=rms_e, rms_ratio=rms_k / rms_e,
               bit_equal_to_emulation=same / n)
    _log(logdir, "normal/" + name, rec)
    print(name, rec)
    assert rms_k <= 1.5 * rms_e, rec


# ---------------------------------------------------------------------------------------------- a result depends only on its inputs
def _hostile(shape, seed):
    r = np.random.default_rng(seed)
    return r.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=shape)


@pytest.mark.parametrize("kind", ["lattice", "normal"])
def test_neighbouring_images_do_not_leak(kind):
    case = wc.BY_NAME["batch_n3"]
    x, w, b = getattr(wc, kind)(case)
    alone = run(x[1:2], w, b, False)
    x = x.copy()
    x[0] = np.nan
    x[2] = _hostile(x[2].shape, 5)
    y = run(x, w, b, False)
    assert not np.isnan(alone).any() and not np.isinf(alone).any()
    assert np.array_equal(_bits(y[1]), _bits(alone[0]))
    if kind == "lattice":
        assert np.array_equal(y[1].astype(np.float64), _lattice_ref("batch_n3", True)[1])


def test_n_tiles_are_independent():
    case = wc.BY_NAME["batch_n3"]
    x, w, b = wc.normal(case)
    full = run(x, w, b, True)
    mid = run(x, w[64:128], b[64:128], True)
    assert not np.isnan(full).any() and float(np.abs(mid).max()) > 0
    assert np.array_equal(_bits(mid), _bits(full[..., 64:128]))


@pytest.mark.parametrize("name", ["block_edges", "batch_n3", "odd"])
def test_two_launches_same_bits(name):
    x, w, b = wc.normal(wc.BY_NAME[name])
    a = run(x, w, b, False)
    assert not np.isnan(a).any()
    assert np.array_equal(_bits(a), _bits(run(x, w, b, False)))


# ---------------------------------------------------------------------------------------------- refusals
REFUSED = [dict(stride=2), dict(pad=0), dict(KH=1), dict(KH=1, KW=1, pad=0), dict(Cout=96), dict(Cin=24), dict(res_mode=1), dict(prec=1),
           dict(x_st=1), dict(y_st=2)]


def _refusal_buffers():
    """Buffers that hold any of the described shapes (up to 64 input / 128 output channels at 8 x 8), so that a call accepted by
    mistake still stays inside them."""
    r = np.random.default_rng(3)
    x = torch.from_numpy(r.standard_normal(8 * 8 * 64).astype(np.float32)).cuda()
    wu = torch.from_numpy(r.standard_normal(16 * 128 * 64).astype(np.float32)).cuda()
    b = torch.zeros(128, device="cuda")
    ybuf, yv = _guarded(8 * 8 * 128)
    return x, wu, b, ybuf, yv


def test_refusal_baseline_is_accepted():
    """The descriptor the refusals below vary in one field each is itself taken."""
    from apse_uav_amd import _lib
    x, wu, b, ybuf, yv = _refusal_buffers()
    d = _desc(1, 8, 8, 32, 64, 0)
    assert _lib.load().apse_winograd_conv2d(C.byref(d), _lib.ptr(x), _lib.ptr(wu), _lib.ptr(b), _lib.ptr(yv), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(yv[:8 * 8 * 64]).any()) and bool(torch.isnan(yv[8 * 8 * 64:]).all()) and _guards_intact(ybuf, yv.numel())


@pytest.mark.parametrize("over", REFUSED, ids=["-".join("%s%d" % kv for kv in o.items()) for o in REFUSED])
def test_refuses_descriptor(over):
    from apse_uav_amd import _lib
    x, wu, b, ybuf, yv = _refusal_buffers()
    d = _desc(1, 8, 8, 32, 64, 0, over)
    rc = _lib.load().apse_winograd_conv2d(C.byref(d), _lib.ptr(x), _lib.ptr(wu), _lib.ptr(b), _lib.ptr(yv), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((ybuf.view(torch.int32) == NAN_BITS).all())


@pytest.mark.parametrize("null", ["x", "wu", "y", "desc"])
def test_refuses_null_pointer(null):
    from apse_uav_amd import _lib
    x, wu, b, ybuf, yv = _refusal_buffers()
    d = _desc(1, 8, 8, 32, 64, 0)
    args = dict(desc=C.byref(d), x=_lib.ptr(x), wu=_lib.ptr(wu), y=_lib.ptr(yv))
    args[null] = None
    rc = _lib.load().apse_winograd_conv2d(args["desc"], args["x"], args["wu"], _lib.ptr(b), args["y"], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((ybuf.view(torch.int32) == NAN_BITS).all())
