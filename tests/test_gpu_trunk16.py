"""-m gpu: the 16-bit trunk front -- input writer, stem_s2d_pool16, bottleneck64_fused16 -- and the small kernels beside it
(round16, subsample2, nhwc_to_nchw) against the float64 references of tests/trunk16_ref.py, called directly through ctypes
(tests/hip_helpers.py: TRUNK_KERNEL_SIG) and, for the input writer and plan.hip's stem re-indexing, through a context.

Every comparison is BIT EQUALITY: the inputs are integer lattices on which the f32 accumulators hold exact sums, so the float64
result rounded once where the kernel rounds is the only correct pattern (tests/test_trunk16_ref.py asserts the conditions for
exactly these case tables and shows that each named wrong variant gives other bits).  There are no tolerances.  Outputs are
allocated exactly sized with a 4 KiB guard behind them, both prefilled with a NaN pattern no kernel writes: every element must
be written, the guard must be untouched.  Each test appends one line to trunk16.log (case, precision, live share, share changed
by the rounding, mismatches).

Wall time per test on an MI355X (seconds, CPU reference included; 71 tests, 6.2 s in all): the 513-tile cases 0.74 / 0.51
(bottleneck 1x216x304, bf16 / f16) and 0.15 / 0.13 (stem 1x216x608); the context tests 0.11 .. 0.43 (each builds a context);
the first test of the file 0.38 (it loads the library); round16 0.06 / 0.02; every other test 0.09 or less, most below 0.005.
The 513-tile cases are not far above the rest, so they keep their channels.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import trunk16_ref as R

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dname", ["bf16", "f16"])
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
SENT = 0x7fee                 # a NaN in bf16 and in f16: "this element was not written"
GUARD = 2048                  # 16-bit elements: 4 KiB
E_INVALID = -1
BLOCKS = (1, 1, 1, 1)


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "trunk16.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _lib():
    from hip_helpers import trunk_kernels
    return trunk_kernels()


def _p(t):
    from apse_uav_amd import _lib as L
    return L.ptr(t)


def _s():
    from apse_uav_amd import _lib as L
    return L.stream_ptr()


def _guarded(n):
    return torch.full((n + GUARD,), SENT, dtype=torch.int16, device="cuda")


def _check(buf, n, want_bits):
    """(mismatches, unwritten) of the first n words against ``want_bits``; the guard behind them must be untouched"""
    got = buf[:n].cpu()
    assert bool((buf[n:] == SENT).all()), "the guard behind the output was written"
    return int((got != want_bits.reshape(-1)).sum()), int((got == SENT).sum())


def _bias(b, n):
    out = torch.zeros(n, dtype=torch.float32)
    out[:b.numel()] = b.to(torch.float32)
    return out.cuda()


def _share(mask):
    return round(float(mask.double().mean()), 4)


# ---------------------------------------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=None)
def _stem_ref(case, dname, border=False):
    inp = R.stem_border_inputs() if border else R.stem_inputs(case)
    out, pre, act = R.stem_pool(*inp, R.DT[dname], parts=True)
    return dict(inp=inp, act=act if border else None, bits=R.bits(R.to_nhwc(out, R.DT[dname])), live=_share(out > 0),
                changed=_share(act != pre.clamp_min(0)))


@functools.lru_cache(maxsize=None)
def _bneck_ref(case, dname):
    inp = R.bneck_inputs(case)
    y, p = R.bottleneck(*inp, R.DT[dname], parts=True)
    return dict(inp=inp, bits=R.bits(R.to_nhwc(y, R.DT[dname])), live=_share(y > 0), changed=_share(y != p["p3"]))


# ---------------------------------------------------------------------------------------------- 3. stem_s2d_pool16 alone
def _run_stem(case, dname, inp):
    from hip_helpers import pack_filter16
    lib = _lib()
    dt = R.DT[dname]
    B, IH, IW = case
    x, w7, b = inp
    xs = R.s2d_input(x, 2 * IH, 2 * IW, dt).cuda().contiguous()
    w16 = pack_filter16(R.stem_reindex(w7), dt)                    # [128][4][64]
    assert w16.numel() >= 64 * 4 * 64 and xs.shape == (B, IH, IW, 16)
    bias = _bias(b, 128)
    n = B * ((IH - 1) // 2 + 1) * ((IW - 1) // 2 + 1) * 64
    buf = _guarded(n)
    rc = lib.apse_k_stem_pool16(_p(xs), _p(w16), _p(bias), _p(buf), B, IH, IW, R.PREC[dname], _s(), None, None)
    torch.cuda.synchronize()
    assert rc == 0
    return buf, n


@DTYPES
@pytest.mark.parametrize("case", R.STEM_CASES, ids=R.case_id)
def test_stem_pool16_exact_on_lattice(case, dname, logdir):
    ref = _stem_ref(case, dname)
    buf, n = _run_stem(case, dname, ref["inp"])
    assert n == ref["bits"].numel()
    bad, unwritten = _check(buf, n, ref["bits"])
    _log(logdir, "stem_pool16/" + R.case_id(case), dict(prec=dname, live=ref["live"], changed_by_rounding=ref["changed"],
                                                        unwritten=unwritten, mismatches=bad, of=n))
    assert unwritten == 0 and bad == 0


@DTYPES
def test_stem_pool16_skips_cells_outside_the_map(dname, logdir):
    """All-negative pre-activation border, bias 0, strictly positive interior (trunk16_ref.stem_border_inputs): every pooled
    output, the border ones included, is the maximum of the interior cells of its window.  The cells one past the map, which
    the tile holds values for (+2600 .. 3315 above and left of this map), must not enter."""
    case = R.STEM_BORDER_CASE
    ref = _stem_ref(case, dname, True)
    buf, n = _run_stem(case, dname, ref["inp"])
    bad, unwritten = _check(buf, n, ref["bits"])
    want = R.bits(R.to_nhwc(R.interior_pool(ref["act"]), R.DT[dname]))
    bad_interior = int((buf[:n].cpu() != want.reshape(-1)).sum())
    _log(logdir, "stem_pool16/border_" + R.case_id(case), dict(prec=dname, live=ref["live"], changed_by_rounding=ref["changed"],
                                                               unwritten=unwritten, mismatches=bad, vs_interior_max=bad_interior, of=n))
    assert unwritten == 0 and bad == 0 and bad_interior == 0


# ---------------------------------------------------------------------------------------------- 4. bottleneck64_fused16 alone
def _bneck_args(case, dname, inp):
    from hip_helpers import pack_filter16
    dt = R.DT[dname]
    B, H, W, K1, alias = case
    x, res, w1, b1, w2, b2, w3, b3 = inp
    xd = R.to_nhwc(x, dt).cuda().contiguous()
    rd = xd if alias else R.to_nhwc(res, dt).cuda().contiguous()
    w1d = pack_filter16(w1.view(64, K1, 1, 1), dt)                 # [128][K1]
    w2d = pack_filter16(w2, dt)                                    # [128][3][192]
    w3d = pack_filter16(w3.view(256, 64, 1, 1), dt)                # [256][64]
    assert w1d.numel() >= 64 * K1 and w2d.numel() >= 64 * 576 and w3d.numel() >= 256 * 64
    return [xd, rd, w1d, _bias(b1, 128), w2d, _bias(b2, 128), w3d, _bias(b3, 256)]


def _launch_bneck(t, buf, B, H, W, K1, prec):
    xd, rd, w1d, b1d, w2d, b2d, w3d, b3d = t
    rc = _lib().apse_k_bottleneck64_fused16(_p(xd), _p(rd), _p(buf), _p(w1d), _p(b1d), _p(w2d), _p(b2d), _p(w3d), _p(b3d), B, H, W, K1,
                                           prec, _s(), None, None)
    torch.cuda.synchronize()
    return rc


@DTYPES
@pytest.mark.parametrize("case", R.BNECK_CASES, ids=R.case_id)
def test_bottleneck64_fused16_exact_on_lattice(case, dname, logdir):
    """K1 = 64 with a separate residual (block 0), K1 = 256 with the residual being x itself (the same pointer) and with a
    separate tensor."""
    B, H, W, K1, alias = case
    ref = _bneck_ref(case, dname)
    t = _bneck_args(case, dname, ref["inp"])
    assert (t[0].data_ptr() == t[1].data_ptr()) == alias
    n = B * H * W * 256
    buf = _guarded(n)
    assert _launch_bneck(t, buf, B, H, W, K1, R.PREC[dname]) == 0
    bad, unwritten = _check(buf, n, ref["bits"])
    _log(logdir, "bottleneck64_fused16/" + R.case_id(case), dict(prec=dname, live=ref["live"], changed_by_rounding=ref["changed"],
                                                                 unwritten=unwritten, mismatches=bad, of=n))
    assert unwritten == 0 and bad == 0


def test_bottleneck64_fused16_refusals_launch_nothing(logdir):
    case = (1, 8, 16, 256, False)
    t = _bneck_args(case, "bf16", R.bneck_inputs(case))
    n = 8 * 16 * 256
    buf = _guarded(n)
    got = {}
    for name, (B, K1, prec) in dict(prec0=(1, 256, 0), k128=(1, 128, 1), b0=(0, 256, 1)).items():
        got[name] = _launch_bneck(t, buf, B, 8, 16, K1, prec)
    untouched = bool((buf == SENT).all())
    _log(logdir, "bottleneck64_fused16/refusals", dict(prec="bf16", rc=got, untouched=untouched, mismatches=0))
    assert all(rc == E_INVALID for rc in got.values()), got
    assert untouched


# ---------------------------------------------------------------------------------------------- 5. the front through a context
@functools.lru_cache(maxsize=None)
def _lattice_state():
    from apse_uav_amd.weights import synthetic_detector_state
    sd = dict(synthetic_detector_state(0, BLOCKS))
    _, w7, b = R.ctx_inputs()
    key = "backbone.bottom_up.stem.conv1"
    sd[key + ".weight"] = w7.to(torch.float32)
    for k, v in R.identity_fold(b).items():
        sd[key + ".norm." + k] = v
    return sd


def _model(dname, mean=None, min_size=None):
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.networks.track_rcnn import TrackRCNN
    cfg = setup_cfg()
    cfg.APSE.DTYPE = dname
    cfg.APSE.MAX_BATCH = 2
    if mean is not None:
        cfg.MODEL.PIXEL_MEAN = tuple(mean)
    if min_size is not None:
        cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = min_size, 1000
    model = TrackRCNN(cfg).to(torch.device(cfg.MODEL.DEVICE)).eval()
    model.load_state_dict(_lattice_state())
    return model


@functools.lru_cache(maxsize=None)
def _ctx_ref(dname):
    dt = R.DT[dname]
    img, w7, b = R.ctx_inputs()
    h, w = R.CTX_IMAGE
    xm = img - torch.tensor(R.LATTICE_MEAN).view(1, 3, 1, 1)
    x = torch.zeros((2, 3, 160, 256), dtype=torch.float64)         # the zero-padded image: the padding convolves zeros -> relu(bias)
    x[:, :, :h, :w] = xm
    out, pre, act = R.stem_pool(x, w7, b, dt, parts=True)
    return dict(input=R.bits(R.s2d_input(xm, 160, 256, dt)), stem=R.bits(R.to_nhwc(out, dt)), live=_share(out > 0),
                changed=_share(act != pre.clamp_min(0)))


@DTYPES
@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "two_kernel"])
def test_context_input_and_stem_match_the_reference(dname, unfused, monkeypatch, logdir):
    """preprocess_images writes the space-to-depth input (padding and channels 12..15 included) and apse_backbone's stem -- plan.hip's
    7x7 -> 4x4 re-indexing, its one-sided padding, and either form of the stem + pool -- gives stem_pool of the zero-padded image:
    the first check of that route against something that does not share it.  APSE_NO_STEM_FUSE is read when the context is built."""
    if unfused:
        monkeypatch.setenv("APSE_NO_STEM_FUSE", "1")
    else:
        monkeypatch.delenv("APSE_NO_STEM_FUSE", raising=False)
    ref = _ctx_ref(dname)
    img = R.ctx_inputs()[0]
    assert img.shape == (2, 3) + R.CTX_IMAGE
    model = _model(dname, mean=R.LATTICE_MEAN)
    model.backbone_images(img.to(torch.float32).cuda().contiguous(), R.CTX_IMAGE)
    torch.cuda.synchronize()
    # which form ran: the fused plan has no stem.conv1 tensor (the convolution output never leaves the kernel), the two-kernel one does
    from apse_uav_amd._lib import ApseError
    if unfused:
        assert model.debug_tensor("stem.conv1", torch.int16).numel() == 2 * 80 * 128 * 64
    else:
        with pytest.raises(ApseError):
            model.debug_tensor("stem.conv1", torch.int16)
    got_in = model.debug_tensor("input", torch.int16).cpu()
    got_stem = model.debug_tensor("stem", torch.int16).cpu()
    assert got_in.numel() == ref["input"].numel() and got_stem.numel() == ref["stem"].numel()
    bad_in = int((got_in != ref["input"].reshape(-1)).sum())
    bad_stem = int((got_stem != ref["stem"].reshape(-1)).sum())
    _log(logdir, "context/images_151x237/" + ("two_kernel" if unfused else "fused"),
         dict(prec=dname, live=ref["live"], changed_by_rounding=ref["changed"], input_mismatches=bad_in, mismatches=bad_stem,
              of=got_stem.numel()))
    assert bad_in == 0 and bad_stem == 0


@DTYPES
@pytest.mark.parametrize("frame_hw,taps", [((100, 150), 3), ((200, 300), 5)], ids=["up_3taps", "down_5taps"])
def test_context_frames_input_is_pillow_minus_mean_in_s2d_layout(frame_hw, taps, dname, logdir):
    """preprocess_frames with the real pixel mean: uint8 frames whose resized size (151 x 227) is odd on both sides, through the
    context (its dword vertical pass).  The input tensor is Pillow's bytes minus the mean -- one f32 subtraction -- rounded once,
    in space-to-depth layout, zeros outside."""
    from PIL import Image
    from apse_uav_amd.utils import resample
    H, W = frame_hw
    ih, iw = resample.resize_shortest_edge(H, W, 151, 1000)
    assert (ih, iw) == (151, 227)
    assert resample.precompute_coeffs(H, ih)[2] == taps and resample.precompute_coeffs(W, iw)[2] == taps
    model = _model(dname, min_size=151)
    mean = np.array([np.float32(v) for v in model.cfg.MODEL.PIXEL_MEAN], np.float32)
    assert not np.all(mean == np.round(mean))                      # the real, fractional mean
    r = np.random.RandomState(H)
    frames = r.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    model.preprocess_frames(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    got = model.debug_tensor("input", torch.int16).cpu()
    res = np.stack([np.asarray(Image.fromarray(f).resize((iw, ih), Image.BILINEAR)) for f in frames])       # [2, ih, iw, 3] u8
    xm = res.astype(np.float32) - mean.reshape(1, 1, 1, 3)         # f32, as the kernel subtracts
    assert xm.dtype == np.float32
    want = R.bits(R.s2d_input(torch.from_numpy(xm).permute(0, 3, 1, 2), 160, 256, R.DT[dname]))
    assert got.numel() == want.numel()
    bad = int((got != want.reshape(-1)).sum())
    changed = _share(torch.from_numpy(xm).to(R.DT[dname]).to(torch.float32) != torch.from_numpy(xm))
    _log(logdir, "context/frames_%dx%d" % frame_hw, dict(prec=dname, live=_share(want != 0), changed_by_rounding=changed, mismatches=bad,
                                                         of=got.numel()))
    assert bad == 0


# ---------------------------------------------------------------------------------------------- 6. small kernels
def _f32(words):
    return torch.from_numpy(np.array(words, np.uint32).view(np.float32).copy())


def _round16_edges(st):
    """f32 bit patterns at the edges of the conversion to bf16 (st 1) / f16 (st 2), both signs"""
    if st == 1:
        w = [0x3f808000, 0x3f818000,                         # ties: to even downwards / upwards
             0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,  # one f32 ulp either side of each
             0x7f7f7fff, 0x7f7f8000, 0x7f7fffff,              # just below f32 max: the last stays finite, the tie and above -> inf
             0x40490fdb, 0x3f800000]
    else:
        w = [0x3f801000, 0x3f803000,                         # ties: to even downwards / upwards
             0x3f800fff, 0x3f801001, 0x3f802fff, 0x3f803001,  # one f32 ulp either side of each
             0x477fe000, 0x477fefff, 0x477ff000, 0x477ff001, 0x47800000,      # 65504, 65519.996 (-> 65504), 65520 (tie -> inf), above
             0x33800000, 0x33000000, 0x33000001, 0x33c00000,  # 2^-24, 2^-25 (tie -> 0), one ulp above (-> 2^-24), 3 x 2^-25 (tie -> 2^-23)
             0x33bfffff, 0x33c00001, 0x32800000,              # one ulp either side of that tie, 2^-26 (-> 0)
             0x38800000, 0x387fe000, 0x387ff000,              # 2^-14 (smallest normal) and the largest subnormals below it
             0x40490fdb, 0x3f800000]
        assert np.array([0x477ff000], np.uint32).view(np.float32)[0] == 65520.0
        assert np.array([0x33c00000], np.uint32).view(np.float32)[0] == 3 * 2.0 ** -25
    w = w + [0x00000000, 0x7f800000]
    w = w + [v | 0x80000000 for v in w]
    nan = [0x7fc00000, 0x7f800001, 0x7f80ffff, 0xffc12345, 0x7fffffff, 0xff800100, 0x7fa00000]
    return w, nan


@pytest.mark.parametrize("st", [1, 2], ids=["bf16", "f16"])
def test_round16_edges_and_sizes(st, logdir):
    """apse_k_round16 -- the kernel behind every 16-bit filter of the stateless operators -- equals torch's cast bit for bit:
    ties to even in both directions, one ulp either side, +-0, +-inf, overflow to inf, f16 subnormal ties; a NaN stays a NaN
    whatever its payload (sign and payload are free); n = 0 launches nothing; n = 4096 * 256 + 3 takes the grid-stride loop."""
    lib = _lib()
    dt = TDT[st]
    words, nan = _round16_edges(st)
    edges = _f32(words + nan)
    n_fin = len(words)
    stats = {}
    r = np.random.RandomState(st)
    for n in (0, len(words) + len(nan), 257, 4096 * 256 + 3):
        x = torch.from_numpy((r.standard_normal(n) * np.exp(r.uniform(-12, 12, n))).astype(np.float32))
        k = min(n, edges.numel())
        x[:k] = edges[:k]
        if n > 2 * edges.numel():
            x[-edges.numel():] = edges                       # and at the far end of the grid-stride loop
        xd = x.cuda()
        buf = _guarded(n)
        rc = lib.apse_k_round16(_p(xd), _p(buf), n, st, _s())
        torch.cuda.synchronize()
        assert rc == 0
        assert bool((buf[n:] == SENT).all())
        got = buf[:n].cpu()
        want = x.to(dt)
        isnan = torch.isnan(x)
        bad = int((got[~isnan] != R.bits(want)[~isnan]).sum())
        bad_nan = int((~torch.isnan(got.view(dt)[isnan])).sum())
        stats[n] = dict(mismatches=bad, nan_not_kept=bad_nan, nans=int(isnan.sum()))
        assert bad == 0 and bad_nan == 0, stats
    # the edge list does what its comments say (so the comparison above is about these edges and not about typos)
    e = edges[:n_fin].to(dt)
    if st == 1:
        assert R.bits(e)[:3].tolist() == [0x3f80, 0x3f82, 0x3f80] and torch.isinf(e[7]) and torch.isinf(e[8]) and torch.isfinite(e[6])
    else:
        assert R.bits(e)[:3].tolist() == [0x3c00, 0x3c02, 0x3c00] and float(e[6]) == 65504 and float(e[7]) == 65504 and torch.isinf(e[8])
        assert R.bits(e)[11:15].tolist() == [1, 0, 1, 2]
    _log(logdir, "round16", dict(prec={1: "bf16", 2: "f16"}[st], live=1.0, changed_by_rounding=None, mismatches=0, sizes=stats))


def _typed(shape, st, seed):
    r = np.random.RandomState(seed)
    return torch.from_numpy(r.standard_normal(shape).astype(np.float32) * 37).to(TDT[st]).cuda().contiguous()


def _guarded_like(n, st):
    if st == 0:
        return torch.full((n + GUARD // 2,), float("nan"), dtype=torch.float32, device="cuda").view(torch.int32)
    return _guarded(n)


@pytest.mark.parametrize("st", [0, 1, 2], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", [(2, 7, 9, 256), (1, 1, 1, 8)], ids=R.case_id)
def test_subsample2_is_strided_indexing(shape, st, logdir):
    B, H, W, Cn = shape
    x = _typed(shape, st, 5)
    want = x[:, ::2, ::2, :].contiguous().cpu()
    n = want.numel()
    buf = _guarded_like(n, st)
    fill = buf.clone()
    rc = _lib().apse_k_subsample2(_p(x), _p(buf), B, H, W, Cn, st, _s())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(buf[n:], fill[n:])
    iv = torch.int32 if st == 0 else torch.int16
    bad = int((buf[:n].cpu() != want.view(iv).reshape(-1)).sum())
    _log(logdir, "subsample2/" + R.case_id(shape), dict(prec=st, live=1.0, changed_by_rounding=0.0, mismatches=bad, of=n))
    assert bad == 0


@pytest.mark.parametrize("st", [0, 1, 2], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", [(2, 111, 40), (1, 32, 32)], ids=R.case_id)
def test_nhwc_to_nchw_is_a_widening_transpose(shape, st, logdir):
    B, HW, Cn = shape
    x = _typed(shape, st, 6)
    want = x.to(torch.float32).permute(0, 2, 1).contiguous().cpu()
    n = want.numel()
    buf = _guarded_like(n, 0)
    fill = buf.clone()
    rc = _lib().apse_k_nhwc_to_nchw(_p(x), _p(buf), B, HW, Cn, st, _s())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(buf[n:], fill[n:])
    bad = int((buf[:n].cpu() != want.view(torch.int32).reshape(-1)).sum())
    _log(logdir, "nhwc_to_nchw/" + R.case_id(shape), dict(prec=st, live=1.0, changed_by_rounding=0.0, mismatches=bad, of=n))
    assert bad == 0
