"""Winograd F(2x2, 3x3) as the f32 HIP kernel computes it (apse_uav_amd/csrc/conv_winograd.hip).

The transforms are written out here once, in the kernel's operation order, so that the CPU tests can check the
matrices and the numerics of the f32 Winograd path without a GPU:

    U = G g G^T        (filter, 4x4 per (cout, cin): computed in float64, rounded to f32 once; plan.hip does the same)
    V = B^T d B        (input tile 4x4: row combinations first, then column combinations, every step in f32)
    M = sum_cin U * V  (per transform component xi = 4 i + j, channels ascending)
    Y = A^T M A        (output 2x2: row combinations first, then column combinations), + bias, optional ReLU
"""
import numpy as np

BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def filter_transform(w):
    """OIHW 3x3 filters -> U[16][Cout][Cin] f32 (xi = 4 i + j), computed in float64 and rounded once."""
    w = np.asarray(w, dtype=np.float64)
    u = np.einsum("ir,ocrs,js->ijoc", G, w, G)
    return u.reshape(16, w.shape[0], w.shape[1]).astype(np.float32)


def _input_transform(d):
    """d: [..., 4, 4, C] f32 input tiles -> V [..., 16, C] in the kernel's order (rows, then columns)."""
    d0, d1, d2, d3 = d[..., 0, :, :], d[..., 1, :, :], d[..., 2, :, :], d[..., 3, :, :]
    rows = [d0 - d2, d1 + d2, d2 - d1, d1 - d3]               # B^T d
    v = []
    for x in rows:
        x0, x1, x2, x3 = x[..., 0, :], x[..., 1, :], x[..., 2, :], x[..., 3, :]
        v += [x0 - x2, x1 + x2, x2 - x1, x1 - x3]             # (B^T d) B
    return np.stack(v, axis=-2)


def _output_transform(m):
    """m: [..., 16, Cout] -> Y [..., 2, 2, Cout] in the kernel's order (A^T M, then (A^T M) A)."""
    q = [m[..., k, :] for k in range(16)]
    s0 = [q[0 + j] + q[4 + j] + q[8 + j] for j in range(4)]      # row 0 of A^T M
    s1 = [q[4 + j] - q[8 + j] - q[12 + j] for j in range(4)]     # row 1
    y00 = s0[0] + s0[1] + s0[2]
    y01 = s0[1] - s0[2] - s0[3]
    y10 = s1[0] + s1[1] + s1[2]
    y11 = s1[1] - s1[2] - s1[3]
    return np.stack([np.stack([y00, y01], -2), np.stack([y10, y11], -2)], -3)


def split_ranges(cin, split):
    """The channel ranges [c0, c1) of a Cin split: whole 8-channel slices divided as evenly as possible, larger shares first."""
    slices = cin // 8
    assert cin % 8 == 0 and 1 <= split <= slices
    share, extra = divmod(slices, split)
    out, s = [], 0
    for z in range(split):
        n = share + (1 if z < extra else 0)
        out.append((8 * s, 8 * (s + n)))
        s += n
    return out


def emulate(x_hwc, w_oihw, bias, relu, split=1):
    """3x3 / stride 1 / pad 1 convolution of one HWC f32 image by F(2x2, 3x3), every step in f32 -> HWC f32.

    split > 1: the Cin split of the kernel.  Every share of the channels (split_ranges) goes through its own accumulators and its
    own output transform; the partial Y are then summed from zero in split order, and bias and ReLU follow, as the split-K reduce
    kernel does."""
    x = np.asarray(x_hwc, dtype=np.float32)
    H, W, C = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((2 * th + 2, 2 * tw + 2, C), np.float32)
    xp[1:H + 1, 1:W + 1] = x
    iy = (2 * np.arange(th))[:, None] + np.arange(4)[None, :]
    ix = (2 * np.arange(tw))[:, None] + np.arange(4)[None, :]
    d = xp[iy[:, None, :, None], ix[None, :, None, :]]            # [th][tw][4][4][C]
    v = _input_transform(d)                                       # [th][tw][16][C]
    u = filter_transform(w_oihw)                                  # [16][Cout][C]
    m = np.zeros((th, tw, 16, u.shape[1]), np.float32)
    uc = np.ascontiguousarray(u.transpose(2, 0, 1))               # [C][16][Cout]
    rows = max(1, (1 << 18) // (tw * 16 * u.shape[1]))            # tile rows per pass: about 1 MiB of m, so the channel loop stays in cache
    if split == 1:
        for r0 in range(0, th, rows):                             # (tiles are independent: the same arithmetic as one pass over the image)
            vr, mr = v[r0:r0 + rows], m[r0:r0 + rows]
            for c in range(C):                                    # channels ascending, one f32 rounding per product and per add
                mr += vr[..., c:c + 1] * uc[c]
        y = _output_transform(m) + np.asarray(bias, np.float32)  # [th][tw][2][2][Cout]
    else:
        y = np.zeros((th, tw, 2, 2, u.shape[1]), np.float32)
        for c0, c1 in split_ranges(C, split):
            m[...] = 0
            for r0 in range(0, th, rows):
                vr, mr = v[r0:r0 + rows], m[r0:r0 + rows]
                for c in range(c0, c1):
                    mr += vr[..., c:c + 1] * uc[c]
            y += _output_transform(m)                             # the reduce: partial Y summed from zero, z ascending
        y = y + np.asarray(bias, np.float32)
    if relu:
        y = np.maximum(y, 0)
    y = y.transpose(0, 2, 1, 3, 4).reshape(2 * th, 2 * tw, -1)
    return y[:H, :W]
