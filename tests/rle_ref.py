"""Run ends of a mask window without the dense frame (test infrastructure, numpy only).

``ends_from_window`` derives the running sums of pycocotools' counts (column-major, first run = zeros) from the window's
pixels alone, for frames too large to make dense; tests/test_rle_ref.py proves it equal to utils/rle.counts_from_mask on small
dense frames.  ``pack_words`` / ``unpack_words`` convert a bool window to and from the WindowMask word layout.
"""
import numpy as np


def ends_from_window(win, rect, h, w):
    """win: bool [y1 - y0, x1 - x0] (or None: no pixels), rect (x0, y0, x1, y1) inside an h x w frame -> int64 run ends."""
    x0, y0, x1, y1 = rect
    total = h * w
    if win is None or x1 <= x0 or y1 <= y0:
        return np.asarray([total], np.int64)
    assert 0 <= x0 and 0 <= y0 and x1 <= w and y1 <= h
    xs, ys = np.nonzero(np.asarray(win, bool).T)             # column-major order of the set pixels
    p = (xs.astype(np.int64) + x0) * h + ys + y0
    if p.size == 0:
        return np.asarray([total], np.int64)
    first = np.concatenate(([True], np.diff(p) != 1))       # a run starts where the pixel before is not set
    last = np.concatenate((np.diff(p) != 1, [True]))
    ends = np.sort(np.concatenate((p[first], p[last] + 1)))
    if ends[-1] == total:                                    # the last pixel is set: its run ends with the image
        ends = ends[:-1]
    return np.concatenate((ends, [total])).astype(np.int64)


def pack_words(win, rect, garbage=None, extra_words=0):
    """bool window -> uint64 [rows, words] in the WindowMask layout.  ``garbage``: a numpy Generator that sets random bits
    outside the rect's columns; ``extra_words``: unused words at the end of every row (a row stride)."""
    x0, y0, x1, y1 = rect
    rows = y1 - y0
    base = (x0 >> 6) << 6
    words = ((x1 + 63) >> 6) - (x0 >> 6) + extra_words
    px = np.zeros((rows, words * 64), bool)
    if garbage is not None:
        px[:] = garbage.random(px.shape) < 0.5
    px[:, x0 - base:x1 - base] = win
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (px.reshape(rows, words, 64).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64)


def unpack_words(words, rect):
    """uint64 [rows, words] -> the bool window of ``rect``."""
    x0, y0, x1, y1 = rect
    base = (x0 >> 6) << 6
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(words.shape[0], -1)
    return bits[:, x0 - base:x1 - base]


def dense(win, rect, h, w):
    out = np.zeros((h, w), bool)
    if win is not None and rect[2] > rect[0] and rect[3] > rect[1]:
        out[rect[1]:rect[3], rect[0]:rect[2]] = win
    return out
