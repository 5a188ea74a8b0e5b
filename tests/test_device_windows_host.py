"""structures/device_windows.py on the host: the struct bytes against ctypes' own layout of _lib.MotsWindow / _lib.MotsObject,
the pool layout against the scalar loop it replaced, the score ranks and ``mask_words`` on CPU tensors.  No GPU, no library
call."""
import ctypes as C

import numpy as np
import pytest
import torch

from apse_uav_amd import _lib
from apse_uav_amd.structures import device_windows as dw
from apse_uav_amd.structures.window_mask import WindowMask

FRAME = (300, 400)
CPU = torch.device("cpu")


def edge_rects():
    """x0 in {0, 1, 63, 64, 127} x widths in {1, 63, 64, 65, 129}, an empty rect of each kind, seeded random rects."""
    rects = [(x0, 3, x0 + w, 8) for x0 in (0, 1, 63, 64, 127) for w in (1, 63, 64, 65, 129)]
    rects += [(70, 5, 70, 9), (10, 6, 90, 6)]
    g = np.random.default_rng(11)
    for _ in range(40):
        x0, y0 = int(g.integers(0, FRAME[1])), int(g.integers(0, FRAME[0]))
        rects.append((x0, y0, int(g.integers(x0, FRAME[1] + 1)), int(g.integers(y0, FRAME[0] + 1))))
    return rects


def struct_case():
    """rects, words per row (one larger than its rect needs: a row stride), pointers (one NULL), scores."""
    rects = edge_rects()
    g = np.random.default_rng(12)
    wprs = [dw.words_per_row(r) for r in rects]
    wprs[3] += 2
    ptrs = [int(v) for v in g.integers(1, 2 ** 47, len(rects))]
    ptrs[5] = 0
    scores = [float(v) for v in g.integers(0, 9, len(rects))]
    return rects, wprs, ptrs, scores


def ctypes_bytes(struct, rects, wprs, ptrs, scores=None):
    arr = (struct * len(rects))()
    for k, r in enumerate(rects):
        arr[k].rect[:] = list(r)
        arr[k].words_per_row = wprs[k]
        if scores is None:
            arr[k].area = 0
        else:
            arr[k].score = scores[k]
        arr[k].bits = ptrs[k] or None
    return bytes(arr)


def test_layouts_are_the_ctypes_layouts():
    for dtype, struct in ((dw.WIN_DTYPE, _lib.MotsWindow), (dw.OBJ_DTYPE, _lib.MotsObject)):
        assert dtype.itemsize == C.sizeof(struct) == dw.STRUCT_BYTES
        assert [(n, dtype.fields[n][1]) for n in dtype.names] == [(n, getattr(struct, n).offset) for n, _ in struct._fields_]


def test_fill_windows_bytes():
    rects, wprs, ptrs, _ = struct_case()
    got = dw.fill_windows(rects, wprs, ptrs)
    assert got.dtype == dw.WIN_DTYPE and got.shape == (len(rects),)
    assert got.tobytes() == ctypes_bytes(_lib.MotsWindow, rects, wprs, ptrs)
    assert got["words_per_row"][3] == dw.words_per_row(rects[3]) + 2 and got["bits"][5] == 0
    assert got.flags["C_CONTIGUOUS"] and _lib.ptr(got).value == got.ctypes.data


def test_fill_objects_bytes():
    rects, wprs, ptrs, scores = struct_case()
    got = dw.fill_objects(rects, wprs, ptrs, scores)
    assert got.dtype == dw.OBJ_DTYPE
    assert got.tobytes() == ctypes_bytes(_lib.MotsObject, rects, wprs, ptrs, scores)


def test_no_structs():
    assert dw.fill_windows((), (), ()).shape == (0,) and dw.fill_windows([], [], []).tobytes() == b""
    assert dw.fill_objects((), (), (), ()).shape == (0,)
    up = dw.upload(dw.fill_windows((), (), ()), CPU)
    assert up.dtype == torch.uint8 and tuple(up.shape) == (0, dw.STRUCT_BYTES)
    assert dw.read_back(up).shape == (0,)


def test_upload_and_read_back_keep_the_bytes():
    rects, wprs, ptrs, _ = struct_case()
    arr = dw.fill_windows(rects, wprs, ptrs)
    up = dw.upload(arr, CPU)
    assert up.dtype == torch.uint8 and tuple(up.shape) == (len(rects), dw.STRUCT_BYTES)
    assert up.numpy().tobytes() == arr.tobytes()
    back = dw.read_back(up)
    assert back.dtype == dw.WIN_DTYPE and np.array_equal(back, arr)


def test_pool_layout_against_the_scalar_loop():
    rects = edge_rects()
    wpr, off, total = dw.pool_layout(rects)
    want_off, words = [], 0
    for k, r in enumerate(rects):                            # the loop of mots_eval.rle_masks before this module
        w = (((r[2] + 63) >> 6) - (r[0] >> 6)) if r[2] > r[0] else 0
        want_off.append(words)
        words += (r[3] - r[1]) * w
        assert wpr[k] == (w if r[3] > r[1] else 0) == dw.words_per_row(r)
    assert off.tolist() == want_off + [words] and total == words and total > 0
    wpr0, off0, total0 = dw.pool_layout([])
    assert len(wpr0) == 0 and off0.tolist() == [0] and total0 == 0
    # row strides given: a stride of 0 reserves nothing, an empty rect reserves nothing whatever its stride
    stride, off2, total2 = dw.pool_layout([(0, 0, 65, 2), (0, 0, 65, 2), (5, 5, 5, 9)], [4, 0, 3])
    assert stride.tolist() == [4, 0, 0] and off2.tolist() == [0, 8, 8, 8] and total2 == 8


def test_pooled_windows_point_into_the_pool():
    rects = [(0, 0, 65, 2), (5, 5, 5, 9), (64, 1, 128, 4)]
    arr, pool = dw.pooled_windows(rects, CPU)
    assert pool.dtype == torch.int64 and pool.numel() == 4 + 3
    assert arr["rect"].tolist() == [list(r) for r in rects] and arr["words_per_row"].tolist() == [2, 0, 1]
    assert arr["bits"].tolist() == [pool.data_ptr(), 0, pool.data_ptr() + 8 * 4]


def test_score_ranks():
    scores = [0.5, -1.0, 0.5, float("inf"), 0.25, -1.0, float("-inf")]
    rank = dw.score_ranks(scores)
    assert set(rank) == set(scores) and all(isinstance(v, float) for v in rank.values())
    assert sorted(rank, key=rank.get) == sorted(set(scores))
    assert sorted(rank.values()) == [float(r) for r in range(len(set(scores)))]
    for a in scores:
        for b in scores:
            assert (rank[a] < rank[b]) == (a < b) and (rank[a] == rank[b]) == (a == b)
    assert dw.score_ranks([0.3]) == {0.3: 0.0}
    assert dw.score_ranks([]) == {}


def test_mask_words_window_masks():
    words = torch.arange(5 * 3, dtype=torch.int64).reshape(5, 3)
    m = WindowMask(words, (63, 2, 129, 7), FRAME, (70, 4), 9)
    rect, wpr, bits, keep = dw.mask_words(m, 0, FRAME, CPU)
    assert rect == (63, 2, 129, 7) and wpr == 3 and keep is None
    assert bits.data_ptr() == words.data_ptr()              # used in place
    wide = WindowMask(torch.zeros((5, 5), dtype=torch.int64), (63, 2, 129, 7), FRAME, (-1, -1), 0)
    assert dw.mask_words(wide, 0, FRAME, CPU)[1] == 5       # a row stride larger than the rect needs
    strided = WindowMask(torch.zeros((5, 6), dtype=torch.int64)[:, ::2], (63, 2, 129, 7), FRAME, (-1, -1), 0)
    rect, wpr, bits, _ = dw.mask_words(strided, 0, FRAME, CPU)
    assert wpr == 3 and bits.is_contiguous()
    # no bits: the rect stays, with the words per row it needs and no pointer
    none = WindowMask(None, (63, 2, 129, 7), FRAME, (-1, -1), 0)
    assert dw.mask_words(none, 1, FRAME, CPU) == ((63, 2, 129, 7), 3, None, None)
    for r in ((70, 5, 70, 9), (10, 6, 90, 6)):               # an empty rect
        empty = WindowMask(torch.zeros((4, 1), dtype=torch.int64), r, FRAME, (-1, -1), 0)
        assert dw.mask_words(empty, 2, FRAME, CPU) == (r, 0, None, None)
    # the list form: one entry per mask, the addresses 0 where there are no words
    rects, wprs, ptrs, bits, packed = dw.masks_words([m, none, wide], FRAME, CPU, first=4)
    assert rects == [m.rect, none.rect, wide.rect] and wprs == [3, 3, 5] and packed == []
    assert ptrs == [words.data_ptr(), 0, wide.bits.data_ptr()] and bits[1] is None and bits[2] is wide.bits
    assert dw.masks_words([], FRAME, CPU) == ([], [], [], [], [])
    with pytest.raises(ValueError, match="mask 5: "):       # numbered from ``first``
        dw.masks_words([m, WindowMask(words[:2], m.rect, FRAME, (-1, -1), 0)], FRAME, CPU, first=4)


def test_mask_words_refusals():
    short = WindowMask(torch.zeros((3, 3), dtype=torch.int64), (63, 2, 129, 7), FRAME, (-1, -1), 0)
    with pytest.raises(ValueError) as e:
        dw.mask_words(short, 4, FRAME, CPU)
    assert str(e.value) == "mask 4: (3, 3) bit words for a window of 5 rows"
    with pytest.raises(ValueError) as e:
        dw.mask_words(short, 4, FRAME, CPU, windows_only=True)
    assert str(e.value) == "mask 4: (3, 3) torch.int64 bit words for a window of 5 rows"
    flat = WindowMask(torch.zeros(10, dtype=torch.int64), (63, 2, 129, 7), FRAME, (-1, -1), 0)
    with pytest.raises(ValueError):
        dw.mask_words(flat, 0, FRAME, CPU)
    i32 = WindowMask(torch.zeros((5, 3), dtype=torch.int32), (63, 2, 129, 7), FRAME, (-1, -1), 0)
    with pytest.raises(ValueError) as e:
        dw.mask_words(i32, 7, FRAME, CPU, windows_only=True)
    assert str(e.value) == "mask 7: (5, 3) torch.int32 bit words for a window of 5 rows"
    with pytest.raises(TypeError) as e:
        dw.mask_words(torch.zeros(FRAME, dtype=torch.bool), 3, FRAME, CPU, windows_only=True)
    assert str(e.value) == "mask 3 is Tensor: the device writers take WindowMask only"
    with pytest.raises(ValueError) as e:
        dw.mask_words(torch.zeros((2, 2), dtype=torch.bool), 3, FRAME, CPU, dense_hw_only=True)
    assert str(e.value) == "pred_masks entries must be WindowMask or dense [H, W] bool tensors"
    host = WindowMask(torch.zeros((5, 3), dtype=torch.int64), (63, 2, 129, 7), FRAME, (-1, -1), 0)
    with pytest.raises(_lib.ApseError) as e:
        dw.mask_words(host, 0, FRAME, CPU, host_bits="refuse")
    assert str(e.value) == "mask_utils needs the mask on the GPU (no CPU fallback)"
    with pytest.raises(_lib.ApseError):
        dw.mask_words(torch.zeros(FRAME, dtype=torch.bool), 0, FRAME, CPU, host_bits="refuse")
