"""Shapes for conv_winograd_f32 with its Cin split and its second block geometry (apse_winograd_conv2d_split), on top of
tests/winograd_cases.py, whose inputs, float64 reference and derived bound are used unchanged.

A case adds the split and the geometry to the shape: geometry 0 = blocks of 16 x 4 Winograd tiles (32 x 8 output pixels), geometry
1 = 8 x 8 (16 x 16 output pixels); a block holds 64 output channels; a split multiplies whole 8-channel k-slices, larger shares
first.  tests/test_winograd_split_cases.py proves this side on the CPU, tests/test_gpu_winograd_split.py holds the kernel to it.
"""
import numpy as np

import winograd_cases as wc
from apse_uav_amd import winograd as wg

# (name, B, H, W, Cin, Cout, split, geometry)
CASES = [
    ("g0_c8", 1, 1, 1, 8, 64, 1, 0),              # Cin 8, split 1, today's geometry: grid 1
    ("g1_c8", 1, 1, 1, 8, 64, 1, 1),              # ... and <8, 8>, a 1 x 1 map
    ("g1_15x17", 1, 15, 17, 16, 64, 2, 1),        # one slice per share: both fetches past s_end of split 0 land in split 1's range; grid 2
    ("g1_nwg3", 1, 10, 33, 8, 64, 1, 1),          # grid 3, a block of one pixel column
    ("g1_16x16", 1, 16, 16, 64, 64, 5, 1),        # exactly one full <8, 8> block; shares 2 2 2 1 1
    ("g1_nwg4", 1, 17, 17, 64, 64, 8, 1),         # grid 4, three blocks with one row or column; one slice per share at Cin 64
    ("g0_nwg5", 1, 3, 40, 16, 64, 2, 0),          # grid 5
    ("g1_17x33", 1, 17, 33, 32, 64, 3, 1),        # shares 2 1 1; grid 6
    ("g0_nwg7", 1, 3, 56, 64, 64, 8, 0),          # grid 7
    ("g0_nwg8", 1, 33, 9, 32, 128, 3, 0),         # grid 8, two N tiles
    ("g0_batch", 3, 31, 7, 64, 192, 5, 0),        # B = 3, three N tiles: grid 9
    ("g1_batch", 3, 16, 16, 16, 192, 2, 1),       # the same in <8, 8>
    ("g0_nwg11", 1, 3, 88, 16, 64, 2, 0),         # grid 11
    ("g1_nwg12", 1, 17, 33, 64, 128, 8, 1),       # grid 12
    ("g1_res4", 1, 48, 84, 16, 64, 2, 1),         # the res4 map of a 4K frame: 3 x 6 blocks
]
CASE_IDS = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}


def shape(case):
    """The tests/winograd_cases.py case (name, B, H, W, Cin, Cout) of a split case: its inputs and references."""
    return case[:6]


def grid(case):
    """(spatial x N blocks, splits) of the launch."""
    _, B, H, W, _, Cout, split, geom = case
    bh, bw = (16, 16) if geom else (32, 8)
    return B * ((H + bh - 1) // bh) * ((W + bw - 1) // bw) * (Cout // 64), split


def emulate(x, w, bias, relu, split):
    """winograd.emulate with the Cin split over a batch: NHWC f32."""
    b = np.zeros(w.shape[0], np.float32) if bias is None else bias
    return np.stack([wg.emulate(x[i], w, b, relu, split=split) for i in range(x.shape[0])])


def bound(x, w, bias, split):
    """wc.bound with Cin + 16 replaced by Cin + 16 + split: each partial sum the reduce adds is one more rounding of a running sum
    that wc.magnitude caps."""
    return (x.shape[3] + 16 + split) * 2.0 ** -24 * wc.magnitude(x, w, bias)
