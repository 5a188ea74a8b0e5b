"""-m gpu: apse_k_roi_align_windows (csrc/roi.hip) alone -- roi_align(aligned=False, sampling_ratio=SR) of feat * m_r with m_r
evaluated from mask BITS -- against the two-kernel path it replaces: the same masks expanded to dense u8 on the host, through
apse_k_mask_resize and apse_k_roi_align_masked (both pinned to float64 by tests/roi_ref.py / test_gpu_roi_ops.py).  The contract
is bit equality (``torch.equal``), for every storage type, R, SR, output layout and mask source:

  windows   one apse_mots_window per row, image from img0, a host row count
  planes    the mask tail's form: full-frame planes + rects + valid, image from an index array, the row count from a device
            ``total`` below n_max (the rows past it stay untouched)

The launcher's ctypes signature is declared here (apse_kernels.h is the source of truth).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
H, W = 48, 84                                    # the feature map: two images, features on image 1
SENT = 0x7fc0beef                                # a NaN payload no kernel writes
FRAMES = [(96, 168), (123, 211), (540, 960), (20, 30)]
# the twelve boxes of test_gpu_roi_ops.py::test_roi_align_masked, in pixels of a 336-wide frame
BOXES = np.array([[8., 8., 60., 70.], [10., 10., 10.5, 10.2], [100.3, 40.7, 101.1, 44.], [-20., -12., 30., 40.], [300., 150., 400., 260.],
                  [0., 0., 336., 192.], [-60., 20., -8., 60.], [340., 20., 420., 90.], [33.3, 171.9, 290.1, 191.9], [50., 50., 50., 50.],
                  [120., -30., 200., -6.], [64., 64., 32., 32.]], np.float32)

_vp, _i, _f = C.c_void_p, C.c_int, C.c_float


def _lib():
    from hip_helpers import roi_kernels
    lib = roi_kernels()
    fn = lib.apse_k_roi_align_windows
    # feat, st, H, W, rois, roi_img, img0, total, n_max, windows, planes, rects, valid, plane_wpr, frame_h, frame_w, R, SR, scale,
    # out, nchw, stream
    fn.argtypes = [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _i, _vp]
    fn.restype = _i
    return lib


def _p(t):
    from apse_uav_amd import _lib as L
    return L.ptr(t)


def _s():
    from apse_uav_amd import _lib as L
    return L.stream_ptr()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()


def _rect_of_kind(kind, FH, FW):
    """(rect x0, y0, x1, y1; extra row stride in words) of window kind 1..7"""
    if kind == 1:                                # the whole frame
        return (0, 0, FW, FH), 0
    if kind == 2:                                # inner rect, x0 % 64 == 6, across a word boundary where the frame has one, long rows
        x0 = 70 if FW >= 150 else 6
        return (x0, FH // 5, min(x0 + 70, FW - 2), FH - FH // 4), 2
    if kind == 3:                                # one pixel
        return (FW // 3, FH // 2, FW // 3 + 1, FH // 2 + 1), 0
    if kind == 4:                                # NULL bits (planes: valid = 0) under a rect that is not empty
        return (0, 0, FW, FH), 0
    if kind == 5:                                # an empty rect with a pointer
        return (FW // 2, FH // 4, FW // 2, FH // 2), 0
    if kind == 6:                                # touches the right and the bottom edge
        return (FW - min(40, FW // 2), FH - min(30, FH // 2), FW, FH), 1
    return (FW - FW // 3, FH - FH // 3, FW - 2, FH - 1), 0      # 7: row 6's box lies left of the frame, its mask bottom right


def _masks(FH, FW, n, seed):
    """Per row: kind, rect, row stride, the stored words [rows][stride] (random everywhere, also outside the rect), and the dense
    u8 [n][FH][FW] expansion: bit inside the rect, else 0."""
    rng = np.random.RandomState(seed)
    rows, dense = [], np.zeros((n, FH, FW), np.uint8)
    for r in range(n):
        kind = r % 7 + 1
        (x0, y0, x1, y1), extra = _rect_of_kind(kind, FH, FW)
        empty = x1 <= x0 or y1 <= y0
        need = 1 if empty else ((x1 + 63) >> 6) - (x0 >> 6)
        stride = need + extra
        words = rng.randint(0, 1 << 63, size=(max(y1 - y0, 1), stride), dtype=np.int64).astype(np.uint64)
        words ^= rng.randint(0, 2, size=words.shape).astype(np.uint64) << np.uint64(63)
        if kind == 3:
            words[0, 0] |= np.uint64(1) << np.uint64(x0 & 63)
        if not empty and kind != 4:
            xs = np.arange(x0, x1)
            dense[r, y0:y1, x0:x1] = (words[:, (xs >> 6) - (x0 >> 6)] >> (xs & 63).astype(np.uint64)) & np.uint64(1)
        rows.append((kind, (x0, y0, x1, y1), stride, words))
    return rows, dense


def _windows(rows):
    """The device apse_mots_window [n] of the rows and the word pool they point into"""
    from apse_uav_amd.structures import device_windows as dw
    pool = torch.from_numpy(np.concatenate([w.reshape(-1) for _, _, _, w in rows]).view(np.int64)).cuda()
    off, ptrs = 0, []
    for kind, _, _, w in rows:
        ptrs.append(0 if kind == 4 else pool.data_ptr() + 8 * off)
        off += w.size
    arr = dw.fill_windows([r for _, r, _, _ in rows], [s for _, _, s, _ in rows], ptrs)
    return dw.upload(arr, pool.device), pool


def _planes(rows, dense, FH, FW, n_max, seed):
    """The mask tail's form: planes [n_max][FH][wpr] holding the dense bits inside each rect and random bits everywhere else,
    rects [n_max][4], valid [n_max] (0 for the NULL-bits rows)"""
    rng = np.random.RandomState(seed)
    wpr = ((FW + 63) >> 6) + 1                   # a row stride larger than the frame needs
    full = (rng.rand(n_max, FH, wpr * 64) < 0.5).astype(np.uint8)
    rects = np.zeros((n_max, 4), np.int32)
    valid = np.ones(n_max, np.int32)
    for r, (kind, (x0, y0, x1, y1), _, _) in enumerate(rows):
        rects[r] = x0, y0, x1, y1
        valid[r] = kind != 4
        if x1 > x0 and y1 > y0 and kind != 4:
            full[r, y0:y1, x0:x1] = dense[r, y0:y1, x0:x1]
    planes = np.packbits(full, axis=-1, bitorder="little").view("<u8").view(np.int64).reshape(n_max, FH, wpr)
    return _dev(planes), _dev(rects), _dev(valid), wpr


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("st", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_roi_align_windows_equals_the_dense_pair(st, frame):
    lib = _lib()
    FH, FW = frame
    n, n_max = len(BOXES), len(BOXES) + 3
    rng = np.random.RandomState(4000 + st)
    fd = torch.from_numpy(rng.standard_normal((2, H, W, 256)).astype(np.float32)).to(TDT[st]).cuda().contiguous()
    boxes = (BOXES * np.float32(FW / 336.0)).astype(np.float32)
    scale = W / float(FW)
    rows, dense = _masks(FH, FW, n, 4100 + FH)
    assert {k for k, _, _, _ in rows} == set(range(1, 8))
    win, pool = _windows(rows)
    planes, rects, valid, wpr = _planes(rows, dense, FH, FW, n_max, 4200 + FH)
    bd = _dev(np.concatenate([boxes, np.full((3, 4), 7.0, np.float32)]))
    md = _dev(dense)
    mk = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    assert lib.apse_k_mask_resize(_p(md), n, FH, FW, H, W, _p(mk), _s()) == 0
    img = torch.ones(n_max, dtype=torch.int32, device="cuda")
    total = torch.tensor([n], dtype=torch.int32, device="cuda")
    for R in (7, 10):
        for SR in (1, 4):
            ref = torch.full((n, 256, R, R), float("nan"), device="cuda")
            assert lib.apse_k_roi_align_masked(_p(fd), st, H, W, 1, _p(bd), _p(mk), n, R, SR, scale, _p(ref), _s()) == 0
            torch.cuda.synchronize()
            assert not torch.isnan(ref).any()
            flat = ref.reshape(n, -1)
            zero = (flat == 0).all(dim=1)
            assert bool(zero.any()) and bool((~zero).any())
            for source in ("windows", "planes"):
                for nchw in (1, 0):
                    out = torch.full((n_max, 256, R, R) if nchw else (n_max, R, R, 256), float("nan"), device="cuda")
                    out.view(torch.int32)[n:] = SENT
                    if source == "windows":
                        rc = lib.apse_k_roi_align_windows(_p(fd), st, H, W, _p(bd), None, 1, None, n, _p(win), None, None, None, 0,
                                                          FH, FW, R, SR, scale, _p(out), nchw, _s())
                    else:
                        rc = lib.apse_k_roi_align_windows(_p(fd), st, H, W, _p(bd), _p(img), 0, _p(total), n_max, None, _p(planes),
                                                          _p(rects), _p(valid), wpr, FH, FW, R, SR, scale, _p(out), nchw, _s())
                    assert rc == 0
                    torch.cuda.synchronize()
                    got = out[:n] if nchw else out[:n].permute(0, 3, 1, 2)
                    assert torch.equal(got, ref), (source, nchw, R, SR, float((got - ref).abs().max()))
                    assert bool((out.view(torch.int32)[n:] == SENT).all()), "rows past the live ones were written"
    del pool


def test_roi_align_windows_refuses_bad_arguments():
    lib = _lib()
    out = torch.full((1, 256, 7, 7), float("nan"), device="cuda")
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    for R, SR, wpr in ((33, 4, 1), (7, 3, 1), (0, 4, 1)):
        assert lib.apse_k_roi_align_windows(_p(z), 0, 4, 4, _p(z), None, 0, None, 1, _p(z), None, None, None, wpr, 8, 8, R, SR, 0.5,
                                            _p(out), 1, _s()) == -1
    # the planes form needs planes, rects, valid and a row stride that covers the frame
    assert lib.apse_k_roi_align_windows(_p(z), 0, 4, 4, _p(z), None, 0, None, 1, None, _p(z), _p(z), _p(z), 0, 8, 70, 7, 4, 0.5,
                                        _p(out), 1, _s()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
