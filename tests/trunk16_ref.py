"""Float64 CPU reference of the 16-bit trunk front -- the space-to-depth(2) input writer, the stem re-indexed as a 4x4 / stride-1
convolution, stem + max-pool, and a res2 bottleneck -- with the case tables and seeded lattice generators that
tests/test_trunk16_ref.py (host) and tests/test_gpu_trunk16.py (GPU) share.  Plain torch / numpy: nothing here imports the library.

Lattice.  Every input is a small integer, so every product and every partial sum is an integer below 2^24: an f32 accumulator
holds the exact sum in ANY order, and the float64 sum rounded once at each point where the kernel rounds (t1, t2, y; the stem
output) is the only correct bit pattern, whatever the tile, wave split or k order.  test_trunk16_ref.py asserts the conditions
that make this true for every case below, and that each named wrong variant of the reference gives other bits.

Ranges (case generators below).  Stem: image bytes 0..255 minus the integer mean (104, 116, 124) (|v| <= 151: exact in bf16),
w7 in [-2, 2], bias 16 x [-64, 64] -- except bias[0], set so that the first cell of channel 0 is 2049: below 2048 every integer is an
f16 number, and on the 1 x 1 map (|pre-activation| <= ~1200) the f16 rounding would otherwise change nothing.  Bottleneck: x in [-2, 2], w1 / w2 / w3 in {-1, 0, 1}, b2 = 4 x [-8, 8], b3 and a separate
residual 16 x [-8, 8], b1 in [-8, 8] -- except b1[0]: with |conv1| <= ~100 and |b1| <= 8 no t1 value reaches 256, below which
every integer is a bf16 number, and the t1 rounding would never be exercised.  b1[0] is therefore set so that channel 0 of t1 is
301 at the first pixel (a bf16 tie) and 301 +- ~30 elsewhere: odd integers in (256, 512), which bf16 rounds, in every case down
to the 1 x 1 map.  Sums of |terms| stay below 1e5 at every point.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
PREC = {"bf16": 1, "f16": 2}                     # the library's precision / storage codes
LATTICE_MEAN = (104.0, 116.0, 124.0)

# ---------------------------------------------------------------------------------------------- case tables
# stem_s2d_pool16: (B, IH, IW), the space-to-depth map (image = 2 IH x 2 IW); 4 x 16 pooled pixels per tile
STEM_CASES = [
    (1, 1, 1), (1, 2, 3),        # maps smaller than a tile
    (1, 8, 32),                  # exactly one 4 x 16 pooled tile
    (1, 9, 33),                  # one row and one column past a tile
    (2, 7, 31),                  # odd sizes, batch 2
    (3, 16, 24),                 # the network's multiples of 8
    (1, 216, 608),               # 27 x 19 = 513 tiles over the 512-block grid: prefetch + second pass of the persistent loop
]
STEM_BORDER_CASE = (1, 9, 21)    # all-negative pre-activation border, bias 0 (stem_border_inputs)
# bottleneck64_fused16: (B, H, W, K1, alias) -- alias: the residual IS x (the identity blocks; K1 = 256 only); 8 x 16 pixels per tile
_BNECK_MAPS = [
    (1, 1, 1),                   # map smaller than a tile
    (1, 8, 16),                  # one exact tile
    (1, 9, 17),                  # four tiles, three of them almost empty
    (2, 13, 21),                 # ragged tiles, batch 2
    (3, 7, 50),                  # 12 tiles: not a multiple of 8 (remainder branch of the XCD remap), batch stride in the tile decode
]
BNECK_CASES = ([(b, h, w, 64, False) for b, h, w in _BNECK_MAPS] + [(b, h, w, 256, True) for b, h, w in _BNECK_MAPS] +
               [(b, h, w, 256, False) for b, h, w in _BNECK_MAPS] +
               [(1, 216, 304, 64, False)])       # 513 tiles over the 512-block cap: the weight stream across a tile seam, the g + 1 < G tail
# the front through a context: image h x w (padded to 160 x 256: odd on both sides), batch 2
CTX_IMAGE = (151, 237)


def case_id(c):
    return "x".join(str(int(v)) for v in c)


# ---------------------------------------------------------------------------------------------- rounding
def round16(v, dtype):
    """float64 -> ``dtype`` (round to nearest even) -> float64.  torch converts through f32; every value rounded here is an f32
    number (asserted), so this is ONE rounding."""
    f = v.to(torch.float32)
    assert torch.equal(f.to(torch.float64), v), "value is not an f32 number: the f32 step would round a second time"
    return f.to(dtype).to(torch.float64)


def to_nhwc(v, dtype):
    """[B, C, H, W] float64 holding ``dtype`` numbers -> [B, H, W, C] in ``dtype`` (the kernels' layout, for bit comparison)"""
    return v.permute(0, 2, 3, 1).contiguous().to(torch.float32).to(dtype)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------- input writer
def s2d_input(img_minus_mean, PH, PW, dtype, swap_phases=False):
    """[B, 3, h, w] (pixel - mean) -> [B, PH/2, PW/2, 16] in ``dtype``: channel (2 (y & 1) + (x & 1)) 3 + c, each value rounded
    once, zeros outside h x w and in channels 12..15.  ``swap_phases``: the wrong layout (2 (x & 1) + (y & 1))."""
    B, _, h, w = img_minus_mean.shape
    assert PH % 2 == 0 and PW % 2 == 0 and h <= PH and w <= PW
    full = torch.zeros((B, 3, PH, PW), dtype=torch.float64)
    full[:, :, :h, :w] = img_minus_mean.to(torch.float64)
    out = torch.zeros((B, PH // 2, PW // 2, 16), dtype=torch.float64)
    for dy in range(2):
        for dx in range(2):
            ph = 2 * dx + dy if swap_phases else 2 * dy + dx
            out[..., 3 * ph:3 * ph + 3] = full[:, :, dy::2, dx::2].permute(0, 2, 3, 1)
    return out.to(torch.float32).to(dtype)


# ---------------------------------------------------------------------------------------------- stem
def stem_reindex(w7):
    """[64, 3, 7, 7] -> [64, 12, 4, 4]: the 7x7 / stride-2 filter on the space-to-depth input.  Tap (r, s) of phase (dy, dx)
    is w7[ky = 2 r + dy - 1][kx = 2 s + dx - 1]; taps outside 0..6 are absent (zero)."""
    w4 = torch.zeros((w7.shape[0], 12, 4, 4), dtype=torch.float64)
    for dy in range(2):
        for dx in range(2):
            for r in range(4):
                for s in range(4):
                    ky, kx = 2 * r + dy - 1, 2 * s + dx - 1
                    if 0 <= ky <= 6 and 0 <= kx <= 6:
                        w4[:, 3 * (2 * dy + dx):3 * (2 * dy + dx) + 3, r, s] = w7[:, :, ky, kx].to(torch.float64)
    return w4


def stem_conv_s2d(xs, w4, pad=(2, 1)):
    """4x4 / stride-1 convolution of the space-to-depth input [B, IH, IW, 16] (any float type) with [64, 12, 4, 4], padded
    pad[0] above / left and pad[1] below / right, the first IH x IW outputs: [B, 64, IH, IW] float64."""
    x = xs.to(torch.float64).permute(0, 3, 1, 2)[:, :12]
    IH, IW = x.shape[2], x.shape[3]
    y = F.conv2d(F.pad(x, (pad[0], pad[1], pad[0], pad[1])), w4)
    return y[:, :, :IH, :IW]


def stem_conv(x, w7):
    """7x7 / stride-2 / pad-3 convolution, float64: [B, 3, H, W] -> [B, 64, ., .]"""
    return F.conv2d(x.to(torch.float64), w7.to(torch.float64), stride=2, padding=3)


def stem_pool(x, w7, b, dtype, variant=None, parts=False):
    """conv 7x7 / 2 / 3 + bias, ReLU, ONE rounding to ``dtype``, max-pool 3x3 / 2 / 1 (cells outside the map do not exist).
    [B, 3, H, W] -> [B, 64, PHo, PWo] float64.  ``variant`` "pool_virtual": the window also takes the cells one past the map, with
    the value the convolution of the zero-extended image has there (what a tile kernel holds for them); "pool_zero": it takes
    them as 0."""
    pre = stem_conv(x, w7) + b.to(torch.float64).view(1, -1, 1, 1)
    act = round16(pre.clamp_min(0.0), dtype)
    if variant == "pool_virtual":
        ext = F.conv2d(F.pad(x.to(torch.float64), (5, 5, 5, 5)), w7.to(torch.float64), stride=2) + b.to(torch.float64).view(1, -1, 1, 1)
        ext = round16(ext.clamp_min(0.0), dtype)                    # outputs -1 .. H/2: one cell past the map on each side
        assert torch.equal(ext[:, :, 1:1 + act.shape[2], 1:1 + act.shape[3]], act)
        out = F.max_pool2d(ext, 3, 2, 0)[:, :, :(act.shape[2] - 1) // 2 + 1, :(act.shape[3] - 1) // 2 + 1]
    elif variant == "pool_zero":
        out = F.max_pool2d(F.pad(act, (1, 1, 1, 1)), 3, 2, 0)
    else:
        assert variant is None
        out = F.max_pool2d(act, 3, 2, 1)
    return (out, pre, act) if parts else out


# ---------------------------------------------------------------------------------------------- bottleneck
BNECK_VARIANTS = ("halo_b1", "res_after_relu", "seam_shift", "t1_round_up")


def _ulp_up(v, dtype):
    """the next ``dtype`` number above each (positive, ``dtype``-valued) element"""
    t = v.to(torch.float32).to(dtype).view(torch.int16)
    return (t + 1).view(dtype).to(torch.float64)


def bottleneck(x, res, w1, b1, w2, b2, w3, b3, dtype, variant=None, parts=False):
    """t1 = round(relu(conv1 1x1 + b1)); t2 = round(relu(conv2 3x3 of t1, ZERO padded, + b2)); y = round(relu(conv3 1x1 + b3 + res)).
    x [B, K1, H, W], res [B, 256, H, W], w1 [64, K1], w2 [64, 64, 3, 3], w3 [256, 64]; float64 throughout, [B, 256, H, W] out.
    Wrong variants (test_trunk16_ref.py): "halo_b1" pads t1 with round(relu(b1)) -- conv1 of a zero pixel -- instead of zeros;
    "res_after_relu" adds the residual behind the ReLU; "seam_shift" reads x one pixel to the left from column 16 on and one
    pixel up from row 8 on (a tile seam off by one); "t1_round_up" gives every t1 value the rounding changed the next number
    above the correctly rounded one (a second, wrong rounding step)."""
    assert variant is None or variant in BNECK_VARIANTS
    d = torch.float64
    x, res = x.to(d), res.to(d)
    B, K1, H, W = x.shape
    if variant == "seam_shift":
        xs = x.clone()
        if W > 16:
            xs[:, :, :, 16:] = x[:, :, :, 15:W - 1]
        if H > 8:
            xs[:, :, 8:, :] = xs.clone()[:, :, 7:H - 1, :]
        x = xs
    p1 = F.conv2d(x, w1.to(d).view(64, K1, 1, 1)) + b1.to(d).view(1, -1, 1, 1)
    t1 = round16(p1.clamp_min(0.0), dtype)
    if variant == "t1_round_up":
        ch = t1 != p1.clamp_min(0.0)
        t1 = torch.where(ch, _ulp_up(t1, dtype), t1)
    if variant == "halo_b1":
        halo = round16(b1.to(d).clamp_min(0.0), dtype).view(1, -1, 1, 1).expand(B, 64, H + 2, W + 2).clone()
        halo[:, :, 1:-1, 1:-1] = t1
        p2 = F.conv2d(halo, w2.to(d)) + b2.to(d).view(1, -1, 1, 1)
    else:
        p2 = F.conv2d(t1, w2.to(d), padding=1) + b2.to(d).view(1, -1, 1, 1)
    t2 = round16(p2.clamp_min(0.0), dtype)
    c3 = F.conv2d(t2, w3.to(d).view(256, 64, 1, 1)) + b3.to(d).view(1, -1, 1, 1)
    p3 = c3.clamp_min(0.0) + res if variant == "res_after_relu" else (c3 + res).clamp_min(0.0)
    y = round16(p3, dtype)
    return (y, dict(p1=p1, t1=t1, p2=p2, t2=t2, p3=p3)) if parts else y


def abs_sums_bottleneck(x, res, w1, b1, w2, b2, w3, b3, t1, t2):
    """largest sum of |terms| at the three accumulation points (bias and residual included)"""
    d = torch.float64
    K1 = x.shape[1]
    s1 = F.conv2d(x.abs().to(d), w1.abs().to(d).view(64, K1, 1, 1)) + b1.abs().to(d).view(1, -1, 1, 1)
    s2 = F.conv2d(t1.abs(), w2.abs().to(d), padding=1) + b2.abs().to(d).view(1, -1, 1, 1)
    s3 = F.conv2d(t2.abs(), w3.abs().to(d).view(256, 64, 1, 1)) + b3.abs().to(d).view(1, -1, 1, 1) + res.abs().to(d)
    return float(s1.max()), float(s2.max()), float(s3.max())


# ---------------------------------------------------------------------------------------------- seeded lattice generators
def _rng(tag, case):
    return np.random.RandomState([20240611, tag] + [int(v) for v in case])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


@functools.lru_cache(maxsize=None)
def stem_inputs(case):
    """(image minus mean [B, 3, 2 IH, 2 IW], w7 [64, 3, 7, 7], bias [64]) as float64 tensors.  Treat as read-only."""
    B, IH, IW = case
    r = _rng(1, case)
    img = r.randint(0, 256, (B, 3, 2 * IH, 2 * IW)).astype(np.float64) - np.array(LATTICE_MEAN).reshape(1, 3, 1, 1)
    w7 = r.randint(-2, 3, (64, 3, 7, 7))
    bias = 16 * r.randint(-64, 65, (64,))
    # bias[0] puts channel 0 of the first convolution cell at 2049, an f16 tie (and a bf16 inexact): below 2048 every integer is
    # an f16 number, and on the smallest maps (|pre-activation| <= ~1200) the f16 rounding would otherwise change nothing
    n, m = min(4, 2 * IH), min(4, 2 * IW)                 # cell (0, 0) reads image rows / columns 0..3 through taps 3..6
    bias[0] = 2049 - int((img[0, :, :n, :m] * w7[0, :, 3:3 + n, 3:3 + m]).sum())
    return _t(img), _t(w7), _t(bias)


@functools.lru_cache(maxsize=None)
def stem_border_inputs(case=STEM_BORDER_CASE):
    """The pool's border rule on its own.  Bias 0; every filter has two taps on one colour: +g (g = 49 or 51) at the centre
    (ky = kx = 3) and -13 at (5, 5), so cell (oy, ox) = g pixel(2 oy, 2 ox) - 13 pixel(2 oy + 2, 2 ox + 2).  The pixels the border
    cells read at their centre are -255 .. -200, every other pixel is 60 .. 70: the pre-activation border is all negative (0 behind
    the ReLU), the interior is strictly positive (2030 and up, odd values among them: rounded in bf16 and in f16), and a pooled
    border output is the maximum of the INTERIOR cells of its window.  The cells one past the map above / left would hold
    -13 pixel(0, .) = +2600 .. 3315 (a tile kernel computes them): a pool that does not skip them gives other bits."""
    B, IH, IW = case
    r = _rng(2, case)
    img = r.randint(60, 71, (B, 3, 2 * IH, 2 * IW)).astype(np.float64)
    neg = -r.randint(200, 256, (B, 3, 2 * IH, 2 * IW)).astype(np.float64)
    for rows in (0, 2 * (IH - 1)):
        img[:, :, rows, :] = neg[:, :, rows, :]
    for cols in (0, 2 * (IW - 1)):
        img[:, :, :, cols] = neg[:, :, :, cols]
    w7 = np.zeros((64, 3, 7, 7))
    for o in range(64):
        w7[o, o % 3, 3, 3] = 49 + 2 * (o % 2)
        w7[o, o % 3, 5, 5] = -13
    return _t(img), _t(w7), _t(np.zeros(64))


def interior_pool(act):
    """max-pool 3x3 / 2 / 1 over the interior cells only (the border ring of ``act`` and everything outside do not exist)"""
    inner = F.pad(act[:, :, 1:-1, 1:-1], (1, 1, 1, 1), value=float("-inf"))
    return F.max_pool2d(inner, 3, 2, 1)


@functools.lru_cache(maxsize=None)
def bneck_inputs(case):
    """(x, res, w1, b1, w2, b2, w3, b3) as float64 tensors; ``res is x`` for an alias case.  Treat as read-only.
    b1[0] is set so that t1 of channel 0 at pixel (0, 0, 0) is 301 (module docstring)."""
    B, H, W, K1, alias = case
    r = _rng(3, (B, H, W, K1, int(alias)))
    x = r.randint(-2, 3, (B, K1, H, W))
    w1 = r.randint(-1, 2, (64, K1))
    w2 = r.randint(-1, 2, (64, 64, 3, 3))
    w3 = r.randint(-1, 2, (256, 64))
    b1 = r.randint(-8, 9, (64,))
    b2 = 4 * r.randint(-8, 9, (64,))
    b3 = 16 * r.randint(-8, 9, (256,))
    res = 16 * r.randint(-8, 9, (B, 256, H, W))
    c0 = int((x[0, :, 0, 0] * w1[0]).sum())
    b1[0] = 301 - c0                                      # t1[0, 0, 0, 0] = 301: a bf16 tie between 300 and 302; b1[0] > 0, so zero
                                                          # padding of t1 differs from conv1 of a zero pixel
    x = _t(x)
    return x, (x if alias else _t(res)), _t(w1), _t(b1), _t(w2), _t(b2), _t(w3), _t(b3)


@functools.lru_cache(maxsize=None)
def ctx_inputs():
    """(two integer-valued images [2, 3, 151, 237] with bytes 0..255, w7, bias) for the context tests"""
    h, w = CTX_IMAGE
    r = _rng(4, (2, h, w))
    img = r.randint(0, 256, (2, 3, h, w))
    w7 = r.randint(-2, 3, (64, 3, 7, 7))
    bias = 16 * r.randint(-64, 65, (64,))
    return _t(img), _t(w7), _t(bias)


def identity_fold(bias):
    """FrozenBN parameters whose fold is the identity: scale = gamma / sqrtf(var + 1e-5f) == 1.0f in f32, bias' = beta."""
    var = np.float32(1) - np.float32(1e-5)
    scale = np.float32(1) * (np.float32(1) / np.sqrt(np.float32(var + np.float32(1e-5)), dtype=np.float32))
    assert scale.dtype == np.float32 and scale == np.float32(1.0)
    n = bias.numel()
    return {"weight": torch.ones(n), "bias": bias.to(torch.float32).clone(), "running_mean": torch.zeros(n),
            "running_var": torch.full((n,), float(var), dtype=torch.float32)}
