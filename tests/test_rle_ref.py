"""tests/rle_ref.py (the window-only run ends the GPU tests use for frames too large to make dense) against the host codec
utils/rle.counts_from_mask on small dense frames: seams, corners, edges.  No GPU."""
import os
import re

import numpy as np
import pytest

import rle_ref
from apse_uav_amd.utils import rle


def _check(win, rect, h, w):
    want = np.cumsum(np.asarray(rle.counts_from_mask(rle_ref.dense(win, rect, h, w)), np.int64))
    got = rle_ref.ends_from_window(win, rect, h, w)
    assert got.tolist() == want.tolist(), (rect, h, w)


@pytest.mark.parametrize("hw", [(1, 1), (1, 9), (9, 1), (7, 5), (30, 150)])
def test_corners_and_full_frame(hw):
    h, w = hw
    one = np.ones((1, 1), bool)
    for x, y in ((0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0)):
        _check(one, (x, y, x + 1, y + 1), h, w)
    _check(np.ones((h, w), bool), (0, 0, w, h), h, w)
    _check(np.zeros((h, w), bool), (0, 0, w, h), h, w)
    _check(None, (0, 0, 0, 0), h, w)
    _check(None, (0, 0, w, h), h, w)


def test_column_seam():
    h, w = 6, 8
    for bottom, top in ((1, 1), (1, 0), (0, 1)):
        win = np.zeros((h, 3), bool)
        win[h - 1, 0] = bottom
        win[0, 1] = top
        win[2:4, 2] = True
        _check(win, (4, 0, 7, h), h, w)
        _check(win[:, :2], (6, 0, 8, h), h, w)               # the seam pair in the last two columns


def test_random_windows():
    g = np.random.default_rng(5)
    for h, w in ((5, 7), (30, 150), (64, 70)):
        for _ in range(60):
            x0, y0 = int(g.integers(0, w)), int(g.integers(0, h))
            x1, y1 = int(g.integers(x0 + 1, w + 1)), int(g.integers(y0 + 1, h + 1))
            win = g.random((y1 - y0, x1 - x0)) < g.choice([0.1, 0.5, 0.9, 1.0])
            _check(win, (x0, y0, x1, y1), h, w)
    yy, xx = np.mgrid[0:64, 0:70]
    _check((yy + xx) % 2 == 0, (0, 0, 70, 64), 64, 70)       # checkerboard: every pixel is a run


def test_pack_words_round_trip():
    g = np.random.default_rng(6)
    for x0, wd in ((0, 1), (1, 63), (63, 65), (64, 64), (127, 129)):
        win = g.random((5, wd)) < 0.5
        rect = (x0, 2, x0 + wd, 7)
        for garbage, extra in ((None, 0), (g, 0), (g, 2)):
            words = rle_ref.pack_words(win, rect, garbage, extra)
            assert words.shape == (5, ((x0 + wd + 63) >> 6) - (x0 >> 6) + extra)
            assert np.array_equal(rle_ref.unpack_words(words, rect), win)


def test_python_limits_equal_the_header():
    """structures/device_windows.py copies three header constants by hand, the GPU tests size their cases from them, and the
    modules that used to hold copies of their own re-export the same objects."""
    from apse_uav_amd.structures import device_windows as dw
    from apse_uav_amd.utils import mask_utils, mots_eval, rle_device
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "apse_hip.h")) as fh:
        text = fh.read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))      # noqa: E731
    assert dw.MAX_OBJECTS == value("APSE_MOTS_MAX_OBJECTS")
    assert dw.SEG_ROWS == value("APSE_MOTS_RLE_SEG_ROWS")
    assert dw.MAX_PAIRS == value("APSE_MOTS_MAX_PAIRS")
    assert rle_device.MAX_OBJECTS is dw.MAX_OBJECTS and mots_eval.MAX_OBJECTS is dw.MAX_OBJECTS
    assert rle_device.SEG_ROWS is dw.SEG_ROWS
    assert mask_utils.MAX_PAIRS is dw.MAX_PAIRS and mots_eval.MAX_PAIRS is dw.MAX_PAIRS
