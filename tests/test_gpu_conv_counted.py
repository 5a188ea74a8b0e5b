"""-m gpu: the convolution kernels in the forms the ROI heads launch them in (apse_conv2d_ex): count-limited persistent launches
(ConvParams::m_count / m_per_item / m_hint), output rows wider than Cout (y_ld > Cout) and the 2x2 deconvolution scatter.

y (with a tile of rows behind the capacity) and the workspace are filled with a NaN pattern no kernel produces in front of every
launch; "untouched" and "equal" compare integers.  Counted against uncounted is equality (the tile decomposition and the split-K
order do not depend on the grid); values are checked on an integer lattice against float64 (test_conv2d_exact_on_lattice's)."""
import json
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
STN = ("f32", "bf16", "f16")
# rows x columns of a block's tile per cfg (conv_igemm.hip apse_launch_conv; the 16-bit kernels keep the tile of 0, 1, 3, 6)
TILE = {0: (128, 128), 1: (64, 64), 2: (128, 32), 3: (128, 64), 4: (64, 64), 5: (128, 32), 6: (64, 64), 7: (64, 64)}
SKINNY = 13
GRID_HINT1 = 64        # blocks of a counted launch whose hint is one item of at most a tile (launch_cfg_x: never below 64)


def _log(logdir, name, obj):
    with open(os.path.join(logdir, "conv_counted.log"), "a") as f:
        f.write(name + " " + json.dumps(obj) + "\n")


def _form(name, st, Cin, H, Cout, K, stride, pad, relu, res_mode, cfg, splitk, B, strided, x_st=None):
    """st: operand and storage type of x / residual / y (the skinny kernel: x_st only, f32 arithmetic and output)"""
    return dict(name=name, st=st, Cin=Cin, H=H, Cout=Cout, K=K, stride=stride, pad=pad, relu=relu, res_mode=res_mode, cfg=cfg,
                splitk=splitk, B=B, strided=strided, x_st=st if x_st is None else x_st)


def _forms():
    f = [
        # f32: one form per tile config, then the layers of the plan with one row per item, then the scalar reduce with a residual
        _form("f32-cfg0-mask3x3", 0, 256, 14, 256, 3, 1, 1, True, 0, 0, 0, 34, True),
        _form("f32-cfg1-mask3x3", 0, 256, 14, 256, 3, 1, 1, True, 0, 1, 0, 18, True),
        _form("f32-cfg2-k1024-n21", 0, 1024, 1, 21, 1, 1, 0, False, 0, 2, 0, 8400, True),
        _form("f32-cfg3-1x1-n1024", 0, 256, 14, 1024, 1, 1, 0, True, 0, 3, 0, 34, True),
        _form("f32-cfg4-small", 0, 64, 9, 64, 3, 1, 1, True, 0, 4, 0, 66, False),
        _form("f32-cfg5-small", 0, 64, 5, 40, 1, 1, 0, False, 0, 5, 0, 130, False),
        _form("f32-cfg6-res5-3x3-res-sk2", 0, 512, 7, 512, 3, 1, 1, True, 1, 6, 2, 66, True),       # conv_splitk_reduce4 + residual
        _form("f32-cfg7-1x1-s2", 0, 256, 14, 512, 1, 2, 0, False, 0, 7, 0, 66, True),
        _form("f32-cfg0-assoc-fc-sk8", 0, 256, 10, 128, 10, 1, 0, False, 0, 0, 8, 140, False),
        _form("f32-cfg0-fc1-sk16", 0, 256, 7, 1024, 7, 1, 0, True, 0, 0, 16, 140, False),
        _form("f32-cfg1-upres-sk3", 0, 64, 6, 64, 3, 1, 1, True, 2, 1, 3, 18, False),                 # conv_splitk_reduce + residual
    ]
    for st in (1, 2):
        for res in (0, 1):
            tag = "%s-%s" % (STN[st], "res" if res else "nores")
            f += [_form("%s-cfg0-mask3x3" % tag, st, 256, 14, 256, 3, 1, 1, True, res, 0, 0, 34, True),
                  _form("%s-cfg1-mask3x3" % tag, st, 256, 14, 256, 3, 1, 1, True, res, 1, 0, 18, True),
                  _form("%s-cfg3-1x1-n1024" % tag, st, 256, 14, 1024, 1, 1, 0, True, res, 3, 0, 34, True),
                  _form("%s-cfg6-res5-3x3" % tag, st, 512, 7, 512, 3, 1, 1, True, res, 6, 0, 66, True)]
    for xst in (0, 1, 2):
        f += [_form("skinny-masklogits-x_%s" % STN[xst], 0, 256, 28, 4, 1, 1, 0, False, 0, SKINNY, 0, 6, False, x_st=xst),
              _form("skinny-n15-x_%s" % STN[xst], 0, 256, 28, 15, 1, 1, 0, True, 0, SKINNY, 0, 6, False, x_st=xst)]
    return f


FORMS = _forms()


def _tile(fm):
    if fm["cfg"] == SKINNY:
        return (64 if fm["x_st"] else 32), 16          # rows a wave walks per step (conv_skinny16: NT tiles of 16 rows)
    return TILE[fm["cfg"]]


def _out_hw(fm):
    return (fm["H"] + 2 * fm["pad"] - fm["K"]) // fm["stride"] + 1


def _counts(B, ohw, bm):
    """0, 1, a count that ends mid-tile, one that ends exactly on a tile boundary, the capacity, and past it"""
    mid = next(c for c in range(5, B) if (c * ohw) % bm)
    edge = next(c for c in range(2, B) if (c * ohw) % bm == 0)
    return [0, 1, mid, edge, B, B + 5]


def _tiles(rows, Cout, bm, bn):
    return ((rows + bm - 1) // bm) * ((Cout + bn - 1) // bn)


def _layer(fm, B, lattice, bias_pad=0.0):
    """(ConvExLayer, x, w, b, res) of `B` items: seeded normal data (rounded to the storage type), or the integer lattice"""
    from hip_helpers import ConvExLayer
    st, xst = fm["st"], fm["x_st"]
    g = torch.Generator().manual_seed(zlib.crc32(fm["name"].encode()) % 10000 + (7 if lattice else 0))
    Cin, H, Cout, K = fm["Cin"], fm["H"], fm["Cout"], fm["K"]
    oh = _out_hw(fm)
    if lattice:
        x = torch.randint(-2, 3, (B, Cin, H, H), generator=g).float()
        w = torch.randint(-2, 3, (Cout, Cin, K, K), generator=g).float()
        b = torch.randint(-8, 9, (Cout,), generator=g).float()
        mk = lambda shape: torch.randint(-8, 9, shape, generator=g).float()
    else:
        x = torch.randn(B, Cin, H, H, generator=g).to(TDT[xst]).float()
        w = torch.randn(Cout, Cin, K, K, generator=g) / (Cin * K * K) ** 0.5
        b = torch.randn(Cout, generator=g)
        mk = lambda shape: torch.randn(shape, generator=g).to(TDT[st]).float()
    res = None
    if fm["res_mode"] == 1:
        res = mk((B, Cout, oh, oh))
    elif fm["res_mode"] == 2:
        res = mk((B, Cout, oh // 2, oh // 2))
    L = ConvExLayer(x, w, b, fm["stride"], fm["pad"], fm["relu"], res, fm["res_mode"], prec=st, x_st=xst,
                    res_st=st if res is not None else 0, y_st=st, bias_pad=bias_pad)
    return L, x, w, b, res


def _lattice_ref(fm, x, w, b, res):
    """float64 result of the layer on lattice inputs (NHWC rows [M][Cout]); asserts that every partial sum fits 24 bits"""
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=fm["stride"], padding=fm["pad"])
    cap = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=fm["stride"], padding=fm["pad"])     # sum of |terms|
    if fm["res_mode"] == 1:
        ref, cap = ref + res.double(), cap + res.double().abs()
    elif fm["res_mode"] == 2:
        up = F.interpolate(res.double(), scale_factor=2, mode="nearest")
        ref, cap = ref + up, cap + up.abs()
    if fm["relu"]:
        ref = F.relu(ref)
    assert float(cap.max()) < 2.0 ** 24 and float(ref.abs().max()) < 60000 and torch.equal(ref, ref.round())
    return ref.permute(0, 2, 3, 1).reshape(-1, ref.shape[1])


def _fits_asked_tile(fm, B):
    """16-bit 128x128 layers move to 256x128 from 250 such tiles on (fast16_shape): the forms stay below"""
    ohw = _out_hw(fm) ** 2
    assert fm["st"] == 0 or fm["cfg"] != 0 or _tiles(B * ohw, fm["Cout"], 256, 128) < 250


# ------------------------------------------------------------------------------------------------ a. counted == uncounted
@pytest.mark.parametrize("fm", FORMS, ids=[f["name"] for f in FORMS])
def test_counted_equals_uncounted(fm, logdir):
    """A launch limited to c of B items writes rows [0, min(c, B) OH OW) with the bytes of an uncounted launch of min(c, B) items
    (same cfg and split) and nothing else, whatever hint sized its grid.  With hint = 1 the grid is 64 blocks: the forms marked
    `strided` have more live tiles than that at c = B, so the persistent loop really strides."""
    from hip_helpers import conv_untouched
    B, cfg, sk, st = fm["B"], fm["cfg"], fm["splitk"], fm["st"]
    ohw = _out_hw(fm) ** 2
    bm, bn = _tile(fm)
    _fits_asked_tile(fm, B)
    counts = _counts(B, ohw, bm)
    assert (counts[2] * ohw) % bm != 0 and (counts[3] * ohw) % bm == 0 and 1 < counts[3] <= B
    live_tiles = {c: _tiles(min(c, B) * ohw, fm["Cout"], bm, bn) for c in counts}
    if fm["strided"]:
        assert live_tiles[B] > GRID_HINT1, live_tiles
    L = _layer(fm, B, lattice=False)[0]
    _log(logdir, "counted/" + fm["name"], dict(counts=counts, live_tiles=live_tiles, tile=[bm, bn]))
    for c in counts:
        live = min(c, B) * ohw
        want = None
        if live:
            rc, want, _ = L.run(min(c, B), cfg, sk)
            assert rc == 0 and conv_untouched(want[live:], st)
            assert not bool((want[:live] == want[live]).any()), "an uncounted launch left live elements unwritten"
        first = None
        for hint in sorted({0, 1, c, B}):
            rc, y, _ = L.run(B, cfg, sk, count=c, hint=hint)
            assert rc == 0, (c, hint, rc)
            assert conv_untouched(y[live:], st), ("rows past the count written", c, hint,
                                                  (y[live:] != y[-1, -1]).nonzero()[:4].tolist())
            if live:
                assert torch.equal(y[:live], want[:live]), ("counted != uncounted", c, hint,
                                                            (y[:live] != want[:live]).nonzero()[:4].tolist())
            if first is None:
                first = y
            assert torch.equal(y, first), ("result depends on the hint", c, hint)


# ------------------------------------------------------------------------------------------------ b. counted against float64
@pytest.mark.parametrize("fm", FORMS, ids=[f["name"] for f in FORMS])
def test_counted_exact_on_lattice(fm):
    """One mid-tile count of each form on the integer lattice: live rows equal float64 (16-bit outputs: float64 rounded once to
    the storage type), the rest of y keeps the fill."""
    from hip_helpers import conv_untouched
    ohw = _out_hw(fm) ** 2
    bm, _ = _tile(fm)
    B, c = 8, 5
    assert (c * ohw) % bm != 0
    L, x, w, b, res = _layer(fm, B, lattice=True)
    ref = _lattice_ref(fm, x[:c], w, b, None if res is None else res[:c])
    rc, y, _ = L.run(B, fm["cfg"], fm["splitk"], count=c, hint=1)
    assert rc == 0
    live = c * ohw
    assert conv_untouched(y[live:], fm["st"])
    out = L.values(y[:live])
    want = ref if fm["st"] == 0 else ref.to(TDT[fm["st"]]).double()
    bad = (out != want).nonzero()
    assert torch.equal(out, want), (int(bad.shape[0]), bad[:6].tolist())


# ------------------------------------------------------------------------------------------------ c. wide rows
def _wide(name, Cin, Cout, y_ld, cfg, splitk, x_st=0, reduce=None):
    fm = _form(name, 0, Cin, 1, Cout, 1, 1, 0, True, 0, cfg, splitk, 300, False, x_st=x_st)
    fm.update(y_ld=y_ld, reduce=reduce)
    return fm


WIDE = [
    _wide("n21-ld32-cfg2", 1024, 21, 32, 2, 0),
    _wide("n21-ld27-cfg2-scalar-tail", 1024, 21, 27, 2, 0),        # y_ld no multiple of 4: the n + k < Cout scalar stores
    _wide("n21-ld32-cfg2-sk8", 1024, 21, 32, 2, 8, reduce="scalar"),
    _wide("n401-ld416-cfg0-sk8", 1024, 401, 416, 0, 8, reduce="scalar"),
    _wide("n15-ld16-skinny-x_f32", 256, 15, 16, SKINNY, 0, x_st=0),
    _wide("n15-ld16-skinny-x_bf16", 256, 15, 16, SKINNY, 0, x_st=1),
    _wide("n15-ld16-skinny-x_f16", 256, 15, 16, SKINNY, 0, x_st=2),
    _wide("n15-ld16-cfg2", 256, 15, 16, 2, 0),
    _wide("n64-ld80-cfg1", 256, 64, 80, 1, 0),
    _wide("n64-ld80-cfg3", 256, 64, 80, 3, 0),
    _wide("n128-ld160-cfg1-sk3", 256, 128, 160, 1, 3, reduce="vec4"),
]
BIAS_PAD = 3.0       # bias entries behind Cout in these tests (a plan pads with zeros): what a written pad column must hold


@pytest.mark.parametrize("fm", WIDE, ids=[f["name"] for f in WIDE])
def test_wide_rows(fm):
    """y_ld > Cout, counted and uncounted, on the lattice.  Columns < Cout equal float64; columns >= roundup(Cout, 4) keep the
    fill in every row; columns Cout .. roundup(Cout, 4) - 1 of a live row follow the contract of DESIGN.md: written only by the
    whole-float4 stores of the direct epilogue (an unsplit tiled launch with y_ld a multiple of 4), and then with the epilogue of
    an all-zero filter row (the padded bias entry, ReLU applied); left alone by the scalar tail, both reduce kernels and
    conv_skinny16.  Rows past the count keep the fill in every column."""
    from hip_helpers import CONV_FILL
    B, Cout, ld = fm["B"], fm["Cout"], fm["y_ld"]
    if fm["reduce"]:       # which reduce kernel launch_cfg_x takes: the four-column one needs Cout, y_ld (and y_coff) multiples of 4
        assert ("vec4" if ((Cout | ld) & 3) == 0 else "scalar") == fm["reduce"]
    L, x, w, b, _ = _layer(fm, B, lattice=True, bias_pad=BIAS_PAD)
    ref = _lattice_ref(fm, x, w, b, None)
    ru4 = (Cout + 3) // 4 * 4
    fill = CONV_FILL[0][1]
    for count in (None, 200):
        rc, y, _ = L.run(B, fm["cfg"], fm["splitk"], count=count, hint=0 if count is None else 1, y_ld=ld)
        assert rc == 0 and y.shape[1] == ld
        live = B if count is None else count
        assert bool((y[live:] == fill).all()), "rows past the count written"
        assert bool((y[:, ru4:] == fill).all()), "columns behind roundup(Cout, 4) written"
        out = L.values(y[:live, :Cout])
        bad = (out != ref[:live]).nonzero()
        assert torch.equal(out, ref[:live]), (count, int(bad.shape[0]), bad[:6].tolist())
        if ru4 > Cout:
            padc = y[:live, Cout:ru4]
            vec_store = fm["cfg"] != SKINNY and fm["splitk"] <= 1 and ld % 4 == 0
            expect = torch.tensor(BIAS_PAD).view(torch.int32).item() if vec_store else fill      # relu(0 + BIAS_PAD), as f32 bits
            assert bool((padc == expect).all()), (count, vec_store, padc[:2].tolist())


# ------------------------------------------------------------------------------------------------ d. deconvolution scatter
DECONV_B = 34
_deconv_cache = {}


def _deconv_case(ch, lattice):
    """ConvTranspose2d(256 -> ch, 2, stride 2) over DECONV_B maps of 14x14: inputs and the float64 reference [B][28][28][ch]
    (before ReLU), computed once"""
    key = (ch, lattice)
    if key not in _deconv_cache:
        g = torch.Generator().manual_seed(4242 + ch + (1 if lattice else 0))
        if lattice:
            x = torch.randint(-2, 3, (DECONV_B, 256, 14, 14), generator=g).float()
            w = torch.randint(-2, 3, (256, ch, 2, 2), generator=g).float()
            b = torch.randint(-8, 9, (ch,), generator=g).float()
        else:
            x = torch.randn(DECONV_B, 256, 14, 14, generator=g)
            w = torch.randn(256, ch, 2, 2, generator=g) / 16.0
            b = torch.randn(ch, generator=g)
        _deconv_cache[key] = (x, w, b, {})
    return _deconv_cache[key]


def _deconv_ref(ch, lattice, st):
    """float64 F.conv_transpose2d of the case with x and w as the storage type st holds them, NHWC, before ReLU"""
    x, w, b, refs = _deconv_case(ch, lattice)
    st = 0 if lattice else st                      # lattice values are exact in every storage type
    if st not in refs:
        r16 = (lambda t: t) if st == 0 else (lambda t: t.to(TDT[st]).float())
        ref = F.conv_transpose2d(r16(x).double(), r16(w).double(), b.double(), stride=2)
        if lattice:
            cap = F.conv_transpose2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2)
            assert float(cap.max()) < 2.0 ** 24 and torch.equal(ref, ref.round())
        refs[st] = ref.permute(0, 2, 3, 1).contiguous()
    return refs[st]


def _deconv_layer(ch, lattice, st, relu):
    """the layer as the plan runs it: 1x1, Cout = 4 ch, the filter packed by mask_head.pack_weight(kind 2)"""
    from hip_helpers import ConvExLayer
    from apse_uav_amd.networks import mask_head
    x, w, b, _ = _deconv_case(ch, lattice)
    dev = torch.device("cuda:0")
    packed, bias_p = mask_head.pack_weight(w.to(dev).contiguous(), b.to(dev), 2, 4 * ch, 256, 1, 1)
    torch.cuda.synchronize()
    return ConvExLayer(x.to(TDT[st]).float(), relu=relu, prec=st, x_st=st, y_st=st, packed=packed, bias_p=bias_p, geom=(4 * ch, 1, 1))


DECONV = [(0, 0, 0), (0, 1, 0), (0, 3, 0), (0, 6, 0), (0, 1, 2), (0, 6, 2), (1, 0, 0), (1, 1, 0), (1, 3, 0), (2, 0, 0), (2, 1, 0), (2, 3, 0)]


@pytest.mark.parametrize("st,cfg,splitk", DECONV, ids=["%s-cfg%d-sk%d" % (STN[s], c, k) for s, c, k in DECONV])
@pytest.mark.parametrize("ch", [256, 64])
def test_deconv_scatter(ch, st, cfg, splitk):
    """out_mode 1, counted, in the storage type of the mode: live items equal float64 conv_transpose2d on the lattice (16-bit:
    rounded once), ReLU on and off; items past the count keep the fill in all 2 OH x 2 OW x cdec elements."""
    from hip_helpers import conv_untouched
    B, bm = DECONV_B, TILE[cfg][0]
    counts = _counts(B, 196, bm)
    assert (counts[2] * 196) % bm != 0 and (counts[3] * 196) % bm == 0 and counts[3] <= B
    ref = _deconv_ref(ch, True, st)
    for relu in (False, True):
        L = _deconv_layer(ch, True, st, relu)
        want = F.relu(ref) if relu else ref
        want = (want.reshape(-1, ch) + 0.0).to(TDT[st]).cuda()          # rounded once to the storage type
        for c in counts:
            live = min(c, B) * 4 * 196
            for hint in (0, 1):
                rc, y, _ = L.run(B, cfg, splitk, count=c, hint=hint, deconv=1)
                assert rc == 0 and y.shape[1] == ch
                assert conv_untouched(y[live:], st), ("items past the count written", relu, c, hint)
                out = y[:live].view(TDT[st])                               # NaN (fill) != anything: value equality on the device
                assert torch.equal(out, want[:live]), (relu, c, hint, (out != want[:live]).nonzero()[:6].tolist())


@pytest.mark.parametrize("st", [0, 1, 2], ids=STN)
def test_deconv_scatter_normal_data(st, logdir):
    """Normal data through the counted scatter (cfg 1): f32 within test_conv2d_parity's bound, 16-bit within
    test_conv2d_16bit_storage's one-ulp-plus-summation-noise rule."""
    from hip_helpers import conv_untouched, err_stats, storage16_tolerance
    ch, B, c = 256, DECONV_B, 7
    ref = F.relu(_deconv_ref(ch, False, st)).reshape(-1, ch)
    L = _deconv_layer(ch, False, st, True)
    rc, y, _ = L.run(B, 1, 0, count=c, hint=1, deconv=1)
    live = c * 4 * 196
    assert rc == 0 and conv_untouched(y[live:], st)
    out, ref = L.values(y[:live]), ref[:live]
    if st == 0:
        stats = err_stats(out, ref)
        _log(logdir, "deconv_normal/f32", stats)
        assert stats["nan"] == 0 and stats["rel_to_max"] < 2e-5, stats
    else:
        diff = (out - ref.to(TDT[st]).double()).abs()
        tol = storage16_tolerance(ref, st)
        frac = float((diff > 1e-6 * ref.abs().clamp_min(1.0)).float().mean())
        info = dict(max=float(diff.max()), frac_differs=frac, violations=int((diff > tol).sum()))
        _log(logdir, "deconv_normal/" + STN[st], info)
        assert bool((diff <= tol).all()) and frac < 0.02, info


# ------------------------------------------------------------------------------------------------ e. refusals
def _small(st=0, Cout=64, res=False, Cin=64):
    fm = _form("refuse", st, Cin, 6, Cout, 1, 1, 0, False, 1 if res else 0, 1, 0, 4, False)
    return _layer(fm, 4, lattice=True)[0]


REFUSALS = [
    ("y_ld-below-cout", dict(), dict(y_ld=60)),
    ("y_ld-with-deconv", dict(), dict(y_ld=64, deconv=1)),
    ("bf16-y_ld-not-8", dict(st=1), dict(y_ld=68)),
    ("f16-y_ld-not-8", dict(st=2), dict(y_ld=68)),
    ("f16-deconv-cdec-not-8", dict(st=2, Cout=48), dict(deconv=1)),
    ("fuse-reduce-with-count", dict(Cin=256), dict(splitk=2, fuse=1, count=2)),
    ("residual-cout-not-4", dict(Cout=62, res=True), dict()),
    ("residual-cout-not-4-bf16", dict(st=1, Cout=62, res=True), dict()),
    ("stream-with-count", dict(Cout=128), dict(cfg=9, count=2)),
    ("glds-with-count", dict(st=1, Cout=128), dict(cfg=11, count=2)),
]


@pytest.mark.parametrize("name,layer,call", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(name, layer, call):
    from hip_helpers import conv_untouched
    L = _small(**layer)
    kw = dict(cfg=1, splitk=0)
    kw.update(call)
    rc, y, ws = L.run(4, ws_slabs=4, **kw)
    assert rc != 0
    assert conv_untouched(y, L.y_st) and conv_untouched(ws, 0)


AUTO = [
    # 1x1 64 -> 128 in f32: uncounted, the auto rule takes conv1x1_stream; its tiled choice for 18 x 196 rows is 64x64, unsplit
    ("f32-stream-shape", 0, 64, 128, 1, 0, 18, 1),
    # 3x3 256 -> 256 in bf16 over 75 x 196 rows (230 tiles of 128x128): uncounted, the LDS-DMA kernel; tiled choice 128x64
    ("bf16-glds-shape", 1, 256, 256, 3, 1, 75, 3),
]


@pytest.mark.parametrize("name,st,Cin,Cout,K,pad,B,tiled", AUTO, ids=[a[0] for a in AUTO])
def test_auto_cfg_with_count_stays_tiled(name, st, Cin, Cout, K, pad, B, tiled):
    """cfg = -1 with a count: the stream / LDS-DMA kernels ignore counts, so the launch must be the tiled kernel apse_conv_pick_cfg
    names -- the bytes of that cfg asked for explicitly, and nothing behind the count."""
    from hip_helpers import conv_untouched
    fm = _form(name, st, Cin, 14, Cout, K, 1, pad, True, 0, -1, 0, B, False)
    L = _layer(fm, B, lattice=False)[0]
    for c in (B - 3, B):
        rc, y, _ = L.run(B, -1, 0, count=c, hint=0, ws_slabs=1)
        rc2, want, _ = L.run(B, tiled, 0, count=c, hint=0)
        assert rc == 0 and rc2 == 0
        assert conv_untouched(y[c * 196:], st)
        assert not bool((y[:c * 196] == y[-1, -1]).any())
        assert torch.equal(y, want), (c, (y != want).nonzero()[:4].tolist())
