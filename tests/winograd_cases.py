"""Shapes, inputs and float64 references for conv_winograd_f32 taken alone (apse_winograd_pack_filter / apse_winograd_conv2d).

CPU only, and of the project only ``apse_uav_amd.winograd`` (the numpy statement of the kernel's operation order):
tests/test_winograd_cases.py proves this side by itself, tests/test_gpu_winograd_edges.py holds the kernel to it.

Two kinds of input per case:
* ``lattice``: small integers.  Every product and every partial sum of F(2x2, 3x3) is then an integer far below 2^24 (U = G g G^T
  is integral for g in 4 Z), so an f32 result has to equal the float64 convolution bit for bit, whatever the order of the sums;
* ``normal``: Gaussian data, held element by element to ``bound`` (derived, below) and in rms to ``winograd.emulate``.
"""
import numpy as np
import torch
import torch.nn.functional as F

from apse_uav_amd import winograd as wg

# (name, B, H, W, Cin, Cout); a block of the kernel is 32 x 8 output pixels x 64 output channels, a k-slice 8 input channels
CASES = [
    ("pixel", 1, 1, 1, 8, 64),               # one pixel, one k-slice, one block
    ("two_slices", 1, 2, 3, 16, 64),         # the prologue's second fetch is the last real one
    ("full_block", 1, 32, 8, 8, 64),         # exactly one full block
    ("block_edges", 1, 33, 9, 32, 128),      # 8 blocks, three of them holding one row or one column of pixels
    ("batch_n3", 3, 31, 7, 64, 192),         # batch, three N tiles, 9 blocks (q = 1, r = 1)
    ("column", 1, 64, 1, 8, 64),             # one-pixel-wide maps
    ("row", 1, 1, 64, 8, 64),
    ("nwg3", 1, 3, 24, 8, 64),               # grids below the 8 XCDs
    ("nwg4", 1, 3, 25, 8, 64),
    ("nwg5", 1, 3, 40, 8, 64),
    ("nwg6", 2, 5, 17, 16, 64),
    ("nwg7", 1, 3, 56, 8, 64),
    ("nwg11", 1, 3, 88, 8, 64),              # q = 1, r = 3
    ("nwg12", 1, 40, 10, 8, 192),            # r = 4
    ("k512", 1, 9, 10, 512, 64),             # 64 k-slices
    ("n1024", 1, 5, 6, 8, 1024),             # 16 N tiles
    ("odd", 2, 75, 125, 256, 256),           # the probe's "odd" shape, 384 blocks
]
CASE_IDS = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
EMULATION_LIMIT = 1e6                        # B H W Cin up to which winograd.emulate (a Python loop over Cin) is run on the whole case

AAT = np.abs(wg.AT)


def emulation_affordable(case):
    _, B, H, W, Cin, _ = case
    return B * H * W * Cin <= EMULATION_LIMIT


def _rng(case, seed, kind):
    name, B, H, W, Cin, Cout = case
    return np.random.default_rng([seed, kind, B, H, W, Cin, Cout])


def lattice(case, seed=0):
    """x NHWC in {-2..2}, w OIHW in 4 {-1, 0, 1}, bias in {-8..8}; all f32."""
    _, B, H, W, Cin, Cout = case
    r = _rng(case, seed, 0)
    x = r.integers(-2, 3, (B, H, W, Cin)).astype(np.float32)
    w = (4 * r.integers(-1, 2, (Cout, Cin, 3, 3))).astype(np.float32)
    b = r.integers(-8, 9, (Cout,)).astype(np.float32)
    return x, w, b


def normal(case, seed=0):
    """x NHWC ~ N(0, 1), w OIHW ~ N(0, 1 / (9 Cin)), bias ~ N(0, 1); all f32."""
    _, B, H, W, Cin, Cout = case
    r = _rng(case, seed, 1)
    x = r.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9.0 * Cin)).astype(np.float32)
    b = r.standard_normal((Cout,)).astype(np.float32)
    return x, w, b


def ref64(x, w, bias, relu):
    """3x3 / stride 1 / pad 1 convolution in float64 (torch CPU): x NHWC, w OIHW, bias or None -> NHWC float64."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).double().permute(0, 3, 1, 2)
    bt = None if bias is None else torch.from_numpy(np.ascontiguousarray(bias)).double()
    y = F.conv2d(xt, torch.from_numpy(np.ascontiguousarray(w)).double(), bt, padding=1)
    if relu:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def emulate(x, w, bias, relu):
    """winograd.emulate over a batch: NHWC f32."""
    b = np.zeros(w.shape[0], np.float32) if bias is None else bias
    return np.stack([wg.emulate(x[i], w, b, relu) for i in range(x.shape[0])])


def pack_layout(u):
    """winograd.filter_transform's [16][Cout][Cin] -> the layout the kernel reads, [Cin / 8][16][Cout][8] (flat)."""
    xi, cout, cin = u.shape
    assert xi == 16 and cin % 8 == 0
    return np.ascontiguousarray(u.reshape(16, cout, cin // 8, 8).transpose(2, 0, 1, 3)).reshape(-1)


def _tiles(x_hwc):
    """The 4x4 input tiles (stride 2, one pixel of zero padding) of one HWC image: [th][tw][4][4][C]."""
    H, W, C = x_hwc.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((2 * th + 2, 2 * tw + 2, C), x_hwc.dtype)
    xp[1:H + 1, 1:W + 1] = x_hwc
    iy = (2 * np.arange(th))[:, None] + np.arange(4)[None, :]
    ix = (2 * np.arange(tw))[:, None] + np.arange(4)[None, :]
    return xp[iy[:, None, :, None], ix[None, :, None, :]]


def magnitude(x, w, bias):
    """|A^T| (sum_c |V| |U|) |A| + |bias| per output element, float64 NHWC: what the absolute values of the terms of one output
    add up to.  Every partial sum of the algorithm, in any order, is at most this."""
    B, H, W, C = x.shape
    u = np.abs(wg.filter_transform(w).astype(np.float64)).transpose(0, 2, 1)           # [16][Cin][Cout]
    ab = 0.0 if bias is None else np.abs(np.asarray(bias, np.float64))
    out = np.empty((B, H, W, w.shape[0]), np.float64)
    for b in range(B):
        v = np.abs(wg._input_transform(_tiles(np.asarray(x[b], np.float32))).astype(np.float64))      # [th][tw][16][Cin]
        th, tw = v.shape[:2]
        m = np.matmul(v.reshape(th * tw, 16, C).transpose(1, 0, 2), u).reshape(4, 4, th, tw, -1)      # [i][j][th][tw][Cout]
        y = np.stack([(AAT[p][:, None, None, None, None] * m).sum(0) for p in range(2)])           # rows: [p][j][th][tw][Cout]
        y = np.stack([(AAT[q][None, :, None, None, None] * y).sum(1) for q in range(2)])           # columns: [q][p][th][tw][Cout]
        out[b] = y.transpose(2, 1, 3, 0, 4).reshape(2 * th, 2 * tw, -1)[:H, :W] + ab
    return out


def bound(x, w, bias):
    """A-priori cap on |y_f32 - y_float64| per output element, float64 NHWC:

        (Cin + 16) 2^-24 (|A^T| (sum_c |V| |U|) |A| + |bias|)

    Each of the Cin products entering an accumulator carries the roundings of U (one: float64 -> f32) and V (two: row and column
    combination) and that of its own accumulation step; the sum over Cin terms adds at most Cin roundings of the running sum; the
    output transform adds four (two per pass) and the bias one.  Cin + 8 unit roundoffs of 2^-24, each relative to a partial sum that
    ``magnitude`` caps; + 16 leaves the second-order terms room.  ReLU is 1-Lipschitz: the cap holds behind it.  Derived, not
    measured: no kernel that computes F(2x2, 3x3) in f32 can exceed it, whatever its summation order."""
    return (x.shape[3] + 16) * 2.0 ** -24 * magnitude(x, w, bias)
