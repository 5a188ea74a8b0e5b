"""The numpy oracle of the YUV 4:2:0 -> BGR conversion (include/apse_hip.h, "YUV 4:2:0 frames"): int32 arithmetic, ``>>`` (numpy's
arithmetic shift floors) and ``np.clip``.  Nothing here reads the library; test_yuv_host.py compares the library's table with
``MATRICES`` and ``MATRICES`` with the Kr / Kb expressions."""
import numpy as np

SHIFT = 20
# name -> (yoff, CY, CVR, CVG, CUG, CUB), integers at shift 20
MATRICES = {
    "cv601": (16, 1220542, 1673527, -852492, -409993, 2116026),
    "bt601": (16, 1220945, 1673555, -852458, -410793, 2115221),
    "bt709": (16, 1220945, 1879825, -558796, -223607, 2215014),
    "bt601-full": (0, 1048576, 1470104, -748826, -360853, 1858077),
    "bt709-full": (0, 1048576, 1651297, -490864, -196424, 1945738),
}
ORDER = ["cv601", "bt601", "bt709", "bt601-full", "bt709-full"]          # APSE_YUV_* values


def exact_matrix(kr, kb, full):
    """(yoff, CY, CVR, CVG, CUG, CUB) as rint(2^20 x) of the exact expressions: R = y' + 2 (1 - Kr) v', B = y' + 2 (1 - Kb) u',
    G from Kr R + Kg G + Kb B = y', with y' = (Y - 16) 255 / 219 and u', v' = (U, V - 128) 255 / 224 in limited range."""
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    vals = (sy, 2.0 * (1.0 - kr) * sc, -2.0 * kr * (1.0 - kr) / kg * sc, -2.0 * kb * (1.0 - kb) / kg * sc, 2.0 * (1.0 - kb) * sc)
    return (0 if full else 16,) + tuple(int(np.rint(v * (1 << SHIFT))) for v in vals)


def convert(Y, U, V, matrix="cv601"):
    """Arrays of equal shape (any integer dtype, values 0..255) -> (B, G, R) uint8 arrays."""
    yoff, cy, cvr, cvg, cug, cub = (np.int32(v) for v in MATRICES[matrix])
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    u, v = U - np.int32(128), V - np.int32(128)
    yy = np.maximum(np.int32(0), Y - yoff) * cy
    half = np.int32(1 << (SHIFT - 1))
    r = np.clip((yy + cvr * v + half) >> SHIFT, 0, 255)
    g = np.clip((yy + cvg * v + cug * u + half) >> SHIFT, 0, 255)
    b = np.clip((yy + cub * u + half) >> SHIFT, 0, 255)
    assert r.dtype == np.int32
    return b.astype(np.uint8), g.astype(np.uint8), r.astype(np.uint8)


def planes(data, H, W, fmt="NV12"):
    """(Y [H][W], U [CH][CW], V [CH][CW]) views / copies of one frame: ``data`` is (H + CH, pitch) for NV12, (3 H / 2, W) for I420."""
    CH, CW = (H + 1) // 2, (W + 1) // 2
    data = np.asarray(data)
    if fmt == "NV12":
        assert data.shape[0] == H + CH and data.shape[1] >= max(W, 2 * CW)
        c = data[H:H + CH, :2 * CW]
        return data[:H, :W], c[:, 0::2], c[:, 1::2]
    assert fmt == "I420" and H % 2 == 0 and W % 2 == 0 and data.shape == (3 * H // 2, W)
    flat = data.reshape(-1)
    return (flat[:H * W].reshape(H, W), flat[H * W:H * W + CH * CW].reshape(CH, CW),
            flat[H * W + CH * CW:H * W + 2 * CH * CW].reshape(CH, CW))


def yuv_to_bgr(data, H, W, fmt="NV12", matrix="cv601"):
    """One frame -> BGR uint8 [H][W][3]; pixel (x, y) takes the chroma sample (x >> 1, y >> 1)."""
    Y, U, V = planes(data, H, W, fmt)
    yi, xi = np.arange(H) >> 1, np.arange(W) >> 1
    b, g, r = convert(Y, U[yi][:, xi], V[yi][:, xi], matrix)
    return np.ascontiguousarray(np.stack([b, g, r], axis=-1))
