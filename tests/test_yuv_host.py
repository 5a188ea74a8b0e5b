"""Host checks of the YUV input path (no GPU): the coefficient table against its defining expressions, the numpy oracle at
its corner values, YuvFrame geometry, what is refused, and FrameUploader's slot shape and row bands."""
import ctypes as C

import numpy as np
import pytest

import yuv_ref

KRKB = {"bt601": (0.299, 0.114, False), "bt709": (0.2126, 0.0722, False),
        "bt601-full": (0.299, 0.114, True), "bt709-full": (0.2126, 0.0722, True)}


def test_table_equals_expressions():
    for name, (kr, kb, full) in KRKB.items():
        assert yuv_ref.exact_matrix(kr, kb, full) == yuv_ref.MATRICES[name], name
    # cv601: OpenCV's ITUR_BT_601_* integers (CY, CVR, CVG, CUG, CUB at shift 20), not derived from an expression
    assert yuv_ref.MATRICES["cv601"] == (16, 1220542, 1673527, -852492, -409993, 2116026)


def test_library_table_equals_oracle_table():
    from apse_uav_amd import _lib
    from apse_uav_amd.structures.yuv_frame import MATRICES
    lib = _lib.load()
    out = (C.c_int * 6)()
    assert list(MATRICES) == yuv_ref.ORDER and list(MATRICES.values()) == list(range(5))
    for i, name in enumerate(yuv_ref.ORDER):
        assert lib.apse_yuv_matrix_host(i, C.byref(out)) == 0
        assert tuple(out) == yuv_ref.MATRICES[name], name
    assert lib.apse_yuv_matrix_host(5, C.byref(out)) == -1 and lib.apse_yuv_matrix_host(-1, C.byref(out)) == -1


@pytest.mark.parametrize("matrix", yuv_ref.ORDER)
def test_oracle_spot_values(matrix):
    full = matrix.endswith("-full")
    px = lambda y, u, v: tuple(int(c[0]) for c in yuv_ref.convert([y], [u], [v], matrix))
    assert px(0 if full else 16, 128, 128) == (0, 0, 0)
    assert px(255 if full else 235, 128, 128) == (255, 255, 255)
    assert px(0, 128, 128) == (0, 0, 0)                        # below black: max(0, Y - yoff)
    # saturation at both ends: strongest chroma at white and at black
    assert px(255, 255, 255)[0] == 255 and px(255, 255, 255)[2] == 255
    assert px(0, 0, 0)[0] == 0 and px(0, 0, 0)[2] == 0 and px(0, 255, 255)[1] == 0
    # a negative sum through the floor shift: Y at black, V = 127 -> (CVR (-1) + 2^19) >> 20 = -2 or -1 before the clip; the
    # unclipped value must be the floor, not the truncation towards zero
    yoff, cy, cvr, cvg, cug, cub = yuv_ref.MATRICES[matrix]
    for v in (127, 100, 1):
        s = cvr * (v - 128) + (1 << 19)
        assert s < 0 and int(np.int32(s) >> np.int32(20)) == s // (1 << 20) == -(-s >> 20) - (1 if -s & ((1 << 20) - 1) else 0)
    # ... and one whose clipped result shows it: R of (Y, 128, V) with yy + CVR v + 2^19 in (-2^20, 0) is -1 -> 0, and the
    # next luma step up gives 0 or 1 exactly as floor says
    v = 127
    for y in range(yoff, yoff + 4):
        s = (y - yoff) * cy + cvr * (v - 128) + (1 << 19)
        assert px(y, 128, v)[2] == min(255, max(0, s // (1 << 20)))


def test_oracle_matches_float_model():
    """The integer conversion is the rounded float one to within 1 (shift-20 coefficients, one rounding)."""
    rng = np.random.default_rng(3)
    Y, U, V = (rng.integers(0, 256, 4096) for _ in range(3))
    for name, (kr, kb, full) in KRKB.items():
        yoff, cy, cvr, cvg, cug, cub = (c / float(1 << 20) for c in yuv_ref.exact_matrix(kr, kb, full))
        yy = np.maximum(0, Y - (0 if full else 16)) * cy
        ref = [np.clip(np.rint(yy + cub * (U - 128.0)), 0, 255), np.clip(np.rint(yy + cvg * (V - 128.0) + cug * (U - 128.0)), 0, 255),
               np.clip(np.rint(yy + cvr * (V - 128.0)), 0, 255)]
        for got, want in zip(yuv_ref.convert(Y, U, V, name), ref):
            assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1, name


def test_yuvframe_geometry():
    from apse_uav_amd.structures.yuv_frame import YuvFrame
    for H, W, pitch in ((4, 6, 6), (375, 1242, 1280), (375, 1241, 1242), (5, 3, 17), (1, 1, 2), (2160, 3840, 3840)):
        CH = (H + 1) // 2
        f = YuvFrame(np.zeros((H + CH, pitch), np.uint8), W)
        assert f.shape == (H, W, 3) and (f.height, f.width, f.pitch, f.format) == (H, W, pitch, "NV12")
        assert f.rows == H + CH and not f.is_cuda
    f = YuvFrame(np.zeros((6, 8), np.uint8))                   # width defaults to the pitch
    assert f.shape == (4, 8, 3)
    f = YuvFrame(np.zeros((27, 18), np.uint8), format="I420")
    assert f.shape == (18, 18, 3) and f.format == "I420" and f.pitch == 18


def test_refusals():
    from apse_uav_amd import _lib
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.track_predictor import FrameUploader, TrackPredictor
    from apse_uav_amd.structures.yuv_frame import YuvFrame, matrix_index
    with pytest.raises(ValueError, match="even"):
        YuvFrame(np.zeros((9, 5), np.uint8), format="I420")               # odd width
    with pytest.raises(ValueError, match="even"):
        YuvFrame(np.zeros((5, 4), np.uint8), format="I420")               # 5 rows: H = 3, odd
    with pytest.raises(ValueError, match="pitch"):
        YuvFrame(np.zeros((6, 5), np.uint8), width=5)                     # odd width: 2 CW = 6 > pitch 5
    with pytest.raises(ValueError, match="pitch"):
        YuvFrame(np.zeros((6, 4), np.uint8), width=6)
    with pytest.raises(ValueError):
        YuvFrame(np.zeros((4, 6, 3), np.uint8))
    with pytest.raises(ValueError):
        YuvFrame(np.zeros((6, 8), np.float32))
    with pytest.raises(ValueError, match="unknown YUV matrix"):
        matrix_index("bt2020")
    up = FrameUploader("cuda", "NV12")
    with pytest.raises(ValueError, match="2-D"):
        up.slot_shape([np.zeros((4, 6, 3), np.uint8)])                    # a BGR frame under FORMAT = NV12
    with pytest.raises(ValueError):
        FrameUploader("cuda", "BGR").slot_shape([YuvFrame(np.zeros((6, 8), np.uint8))])
    cfg = setup_cfg()
    cfg.INPUT.FORMAT = "NV12"
    cfg.APSE.YUV_MATRIX = "bt2020"
    with pytest.raises(ValueError, match="unknown YUV matrix"):
        TrackPredictor(cfg)
    # the C ABI refuses the same before anything is launched (the pointers are only compared with NULL)
    lib = _lib.load()
    p = C.c_void_p(64)
    for H, W, pitch, fmt, mat in ((4, 5, 5, 1, 0), (5, 4, 4, 1, 0), (4, 6, 8, 1, 0), (4, 5, 5, 0, 0), (4, 6, 5, 0, 0), (4, 6, 6, 0, 5),
                                  (4, 6, 6, 2, 0), (0, 6, 6, 0, 0), (4, 49154, 49154, 0, 0), (32770, 4, 4, 0, 0)):
        assert lib.apse_yuv_to_bgr(p, p, 1, H, W, pitch, fmt, mat, None) == -1, (H, W, pitch, fmt, mat)
        assert len(lib.apse_last_error(None)) > 0
    assert lib.apse_yuv_to_bgr(None, p, 1, 4, 6, 6, 0, 0, None) == -1


def test_uploader_slot_shape_and_bands():
    from apse_uav_amd.engines.track_predictor import FrameUploader
    from apse_uav_amd.structures.yuv_frame import YuvFrame
    up = FrameUploader("cuda", "NV12")
    f = YuvFrame(np.zeros((3240, 3840), np.uint8))
    shape, yuv = up.slot_shape([f, np.zeros((3240, 3840), np.uint8)])      # a bare 2-D array is wrapped
    assert shape == (2, 3240, 3840) and [y.shape for y in yuv] == [(2160, 3840, 3)] * 2
    with pytest.raises(ValueError, match="same size"):
        up.slot_shape([f, YuvFrame(np.zeros((3240, 4096), np.uint8), 3840)])
    shape, yuv = FrameUploader("cuda", "BGR").slot_shape([np.zeros((270, 480, 3), np.uint8)])
    assert shape == (1, 270, 480, 3) and yuv is None
    # the bands tile the rows -- luma, then chroma -- without a gap; a short frame goes in one piece
    for rows in (3240, 563, 33, 32, 31, 2):
        bands = FrameUploader.band_rows(rows, 4)
        assert bands[0][0] == 0 and bands[-1][1] == rows and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        assert len(bands) == (4 if rows >= 32 else 1) or rows == 33
    assert FrameUploader.band_rows(3240, 4) == [(0, 810), (810, 1620), (1620, 2430), (2430, 3240)]


def test_synthetic_encoders_round_trip():
    """bgr_to_nv12 / bgr_to_i420 are float encoders for test input; the oracle brings a flat colour back to within 2."""
    from apse_uav_amd.synthetic import bgr_to_i420, bgr_to_nv12
    f = np.empty((6, 10, 3), np.uint8)
    f[...] = (40, 120, 200)
    for m in yuv_ref.ORDER:
        y = bgr_to_nv12(f, m, pitch=16)
        assert y.shape == (6, 10, 3) and y.pitch == 16
        assert np.abs(yuv_ref.yuv_to_bgr(y.data, 6, 10, "NV12", m).astype(int) - f).max() <= 2
        y = bgr_to_i420(f, m)
        assert y.format == "I420" and np.abs(yuv_ref.yuv_to_bgr(y.data, 6, 10, "I420", m).astype(int) - f).max() <= 2
    assert bgr_to_nv12(f[:5, :9]).shape == (5, 9, 3)
    with pytest.raises(ValueError):
        bgr_to_i420(f[:5])
