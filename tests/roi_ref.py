"""float64 references of the ROI gather kernels (csrc/roi.hip), the yardstick of tests/test_gpu_roi_ops.py.  Pinned to
oracle/ops.py and to torch's CPU operators by tests/test_roi_ref.py.

Written from the published algorithms: detectron2 ROIAlign (aligned, sampling_ratio = 0) and assign_boxes_to_levels,
torchvision roi_pool and roi_align (aligned = False), F.interpolate (bilinear, align_corners = False), F.normalize, Linear and
the squared distance.

What is f32 and what is f64:
  * f32, one numpy float32 operation at a time, in the published order (the library is built with -ffp-contract=off and
    correctly rounded division / sqrt, so these are reproducible bit for bit): every DISCRETE decision -- the pyramid level,
    the grid counts ceil(roi / R), the sample coordinates, the (-1, size) validity window, the low / high cell, roundf of the
    pool corners, the bins' floor / ceil.
  * f64: everything continuous -- the bilinear weights taken from the f32 coordinates, products, sums, divisions, norms.

Every reference returns, per output element, ``ref`` (f64), ``mag`` (the sum of the absolute values of the terms) and
``n_ops`` (the number of rounded f32 operations any one term passes through in the documented evaluation order); the f32
bound is ``n_ops * U * mag`` with U = 2^-24, the unit roundoff of f32.  Each rounded operation multiplies the terms it
touches by (1 + d), |d| <= U; k of them give (1 + U)^k - 1 <= (k + 1) U while k (k + 1) U <= 1, so every count below ends with
"+ 1" for the second-order terms.  The f64 reference itself is off by at most n_ops * 2^-53 * mag, 2^-29 of the bound.
"""
import numpy as np

_F = np.float32
U = 2.0 ** -24
RA_CAP = 16              # tap windows of at most this many cells per axis take the separable form (csrc/roi.hip)
FPN_SCALES = (0.25, 0.125, 0.0625, 0.03125)


def bound(res):
    return res["n_ops"] * U * res["mag"]


# ------------------------------------------------------------------------------------------------------ pyramid level
def level_k64(boxes):
    """4 + log2(sqrt(area) / 224 + eps) in float64 (NaN for a negative area): how far a box is from a level threshold."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return 4.0 + np.log2(np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / 224.0 + np.finfo(np.float64).eps)


def assign_levels(boxes):
    """detectron2 assign_boxes_to_levels on f32 boxes, every step in f32: floor(4 + log2(sqrt(area) / 224 + eps)) clamped to
    [2, 5], returned as level - 2.  A negative area (a box inverted on one axis) has a NaN size, for which the published cast to
    int64 is undefined; the contract here is the finest level (fmax / fmin drop the NaN)."""
    b = np.asarray(boxes, _F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        q = np.sqrt(area) / _F(224) + _F(np.finfo(np.float64).eps)
        k = np.floor(_F(4) + np.log2(q))
    assert k.dtype == _F
    k = np.where(np.isnan(k), _F(2), np.clip(k, 2, 5))
    return k.astype(np.int64) - 2


# ------------------------------------------------------------------------------------------------------ ROIAlign
def _axis(s0, bsz, g, L, R):
    """The taps of one axis of one roi: R bins, g samples each, on a map of extent L.  s0 / bsz: f32 roi start and bin size.
    Sample i of bin p sits at (s0 + p * bsz) + ((i + .5) * bsz) / g in f32; it is skipped outside [-1, L], clamped at 0, its low
    cell is the truncation (the last cell takes both taps with the fraction set to 0); the fraction is f64.
    Returns W [R][L] (f64 weight every map cell gets from the bin's samples), base / n [R] (the tap window, n = 0: no valid
    sample), m [R] (most tap contributions any one cell receives), nvalid [R], inside (every sample valid and within [0, L-1])."""
    W = np.zeros((R, L))
    cn = np.zeros((R, L), np.int64)
    z = np.zeros(R, np.int64)
    if g <= 0:
        return dict(W=W, base=z, n=z.copy(), m=z.copy(), nvalid=z.copy(), inside=False)
    p = np.arange(R, dtype=_F)[:, None]
    i = np.arange(g, dtype=_F)[None, :]
    v = (s0 + p * bsz) + ((i + _F(0.5)) * bsz) / _F(g)
    assert v.dtype == _F
    valid = ~((v < _F(-1.0)) | (v > _F(L)))
    inside = bool(valid.all() and (v >= 0).all() and (v <= _F(L - 1)).all())
    vv = np.where(valid, v, _F(0))
    vv = np.where(vv <= 0, _F(0), vv)
    lo = vv.astype(np.int64)
    top = lo >= L - 1
    hi = np.where(top, L - 1, lo + 1)
    lo = np.where(top, L - 1, lo)
    frac = np.where(top, 0.0, vv.astype(np.float64) - lo)
    rows = np.broadcast_to(np.arange(R)[:, None], lo.shape)[valid]
    np.add.at(W, (rows, lo[valid]), 1.0 - frac[valid])
    np.add.at(W, (rows, hi[valid]), frac[valid])
    np.add.at(cn, (rows, lo[valid]), 1)
    np.add.at(cn, (rows, hi[valid]), 1)
    first = np.where(valid, lo, L).min(axis=1)
    last = np.where(valid, hi, -1).max(axis=1)
    n = np.where(last < 0, 0, last - first + 1)
    return dict(W=W, base=np.where(n > 0, first, 0), n=n, m=cn.max(axis=1), nvalid=valid.sum(axis=1), inside=inside)


def roi_align_plan(boxes, dims, scales, R, levels=None):
    """detectron2 ROIPooler + ROIAlign(aligned = True, sampling_ratio = 0): everything that does not depend on the map values.

    boxes [n][4] frame pixels; dims [(H, W)] and scales per level; levels: None = assign_levels.  Per roi a dict:
      level, gh, gw, cnt = max(gh * gw, 1), ay / ax (``_axis``), form ("sep": every bin's tap window has at most RA_CAP cells on
      both axes, else "direct", the per-sample loop), win_y / win_x [R] (the tap-window extent per bin and axis), n_ops [R][R].
    f32: start = x1 * scale - 0.5, end likewise, roi = end - start, bin = roi / R, g = ceil(roi / R).

    n_ops, separable form (out = sum_Y sum_X (wy[Y] wx[X]) F[Y][X] / cnt, wy[Y] the f32 sum of the taps 1 - l or l that land on
    row Y): forming 1 - l and adding my taps: my; likewise mx; wy * wx: 1; times F: 1; the running sum over the ny * nx window
    cells: ny * nx; joining the two half-waves of the 16-bit form: 1; the division: 1; second order: 1
        = my + mx + ny * nx + 5.
    Per-sample form (out = sum_samples (hy hx F1 + hy lx F2 + ly hx F3 + ly lx F4) / cnt): the two factors and their product: 3;
    times F: 1; the 4-term sum: 3; the running sum over the S valid samples: S; division: 1; second order: 1  = S + 9.
    l itself (coordinate minus its truncation) is exact in f32."""
    b = np.asarray(boxes, _F).reshape(-1, 4)
    lv = assign_levels(b) if levels is None else np.asarray(levels, np.int64)
    plan = []
    for r in range(b.shape[0]):
        k = int(lv[r])
        H, W = dims[k]
        sc = _F(scales[k])
        sw, sh = b[r, 0] * sc - _F(0.5), b[r, 1] * sc - _F(0.5)
        ew, eh = b[r, 2] * sc - _F(0.5), b[r, 3] * sc - _F(0.5)
        rw, rh = ew - sw, eh - sh
        bw, bh = rw / _F(R), rh / _F(R)
        gh, gw = int(np.ceil(rh / _F(R))), int(np.ceil(rw / _F(R)))
        ay, ax = _axis(sh, bh, gh, H, R), _axis(sw, bw, gw, W, R)
        sep = bool((ay["n"] <= RA_CAP).all() and (ax["n"] <= RA_CAP).all())
        if sep:
            n_ops = (ay["m"][:, None] + ax["m"][None, :]) + ay["n"][:, None] * ax["n"][None, :] + 5
        else:
            n_ops = ay["nvalid"][:, None] * ax["nvalid"][None, :] + 9
        plan.append(dict(level=k, gh=gh, gw=gw, cnt=max(gh * gw, 1), ay=ay, ax=ax, form="sep" if sep else "direct",
                         win_y=ay["n"], win_x=ax["n"], n_ops=n_ops, inside=ay["inside"] and ax["inside"],
                         empty=not (ay["n"].any() and ax["n"].any())))
    return plan


def _span(a):
    live = a["n"] > 0
    if not live.any():
        return 0, 0
    return int(a["base"][live].min()), int((a["base"][live] + a["n"][live]).max())


def roi_align_apply(plan, imgs, window, R, C=256):
    """The map-dependent half: window(level, img, y0, y1, x0, x1) -> [y1-y0][x1-x0][C] map cells (any float type, widened to
    f64 here).  Returns dict(ref, mag, n_ops), each [n][R][R][C] (n_ops broadcast over C)."""
    n = len(plan)
    ref = np.zeros((n, R, R, C))
    mag = np.zeros((n, R, R, C))
    n_ops = np.zeros((n, R, R, 1))
    for r, p in enumerate(plan):
        n_ops[r, :, :, 0] = p["n_ops"]
        (y0, y1), (x0, x1) = _span(p["ay"]), _span(p["ax"])
        if y1 <= y0 or x1 <= x0:
            continue
        f = np.asarray(window(p["level"], int(imgs[r]), y0, y1, x0, x1), np.float64)
        wy, wx = p["ay"]["W"][:, y0:y1], p["ax"]["W"][:, x0:x1]
        for dst, src in ((ref, f), (mag, np.abs(f))):
            t = (wy @ src.reshape(y1 - y0, -1)).reshape(R, x1 - x0, C)
            dst[r] = np.einsum("qx,pxc->pqc", wx, t) / p["cnt"]
    return dict(ref=ref, mag=mag, n_ops=n_ops)


def roi_align_used_cells(plan, imgs, dims, n_img):
    """used[level][img][y][x]: the union of the tap windows -- the only map cells a roi's output may depend on."""
    used = [np.zeros((n_img,) + tuple(d), bool) for d in dims]
    for r, p in enumerate(plan):
        ry, rx = np.zeros(dims[p["level"]][0], bool), np.zeros(dims[p["level"]][1], bool)
        for a, m in ((p["ay"], ry), (p["ax"], rx)):
            for base, cnt in zip(a["base"], a["n"]):
                m[base:base + cnt] = True
        used[p["level"]][int(imgs[r])][np.ix_(ry, rx)] = True
    return used


# ------------------------------------------------------------------------------------------------------ roi_pool
def round_half_away(v):
    """C roundf of f32 values: halves go away from zero."""
    v = np.asarray(v, _F).astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def roi_pool_windows(boxes, scale, R, H, W):
    """torchvision roi_pool's integer bin windows: corners = roundf(f32(box * scale)), roi = max(end - start + 1, 1),
    bin = f32(roi) / f32(R), rows [floor(p * bin), ceil((p + 1) * bin)) + start clamped to [0, H].  Returns (hs, he [n][R],
    ws, we [n][R], scaled [n][4] the f32 products that were rounded)."""
    b = np.asarray(boxes, _F).reshape(-1, 4)
    scaled = b * _F(scale)
    assert scaled.dtype == _F
    c = round_half_away(scaled)
    p = np.arange(R, dtype=_F)[None, :]

    def axis(s, e, L):
        roi = np.maximum(e - s + 1, 1)
        bsz = (roi.astype(_F) / _F(R))[:, None]
        a = np.floor(p * bsz).astype(np.int64) + s[:, None]
        z = np.ceil((p + _F(1)) * bsz).astype(np.int64) + s[:, None]
        return np.clip(a, 0, L), np.clip(z, 0, L)
    hs, he = axis(c[:, 1], c[:, 3], H)
    ws, we = axis(c[:, 0], c[:, 2], W)
    return hs, he, ws, we, scaled


def roi_pool(feat, boxes, imgs, scale, R):
    """feat [B][H][W][C] (values as stored, widened exactly); the max of the same cells, an empty bin gives 0.  Exact: a max
    rounds nothing.  Returns (out [n][R][R][C] float64, empty [n][R][R])."""
    B, H, W, C = feat.shape
    hs, he, ws, we, _ = roi_pool_windows(boxes, scale, R, H, W)
    n = hs.shape[0]
    out = np.zeros((n, R, R, C))
    empty = np.zeros((n, R, R), bool)
    for r in range(n):
        f = feat[int(imgs[r])]
        for ph in range(R):
            for pw in range(R):
                a, z, c, d = hs[r, ph], he[r, ph], ws[r, pw], we[r, pw]
                if z <= a or d <= c:
                    empty[r, ph, pw] = True
                else:
                    out[r, ph, pw] = f[a:z, c:d].reshape(-1, C).max(axis=0)
    return out, empty


# ------------------------------------------------------------------------------------------------------ small operators
def mean_cells(x):
    """x [n][cells][C] -> the mean over cells.  f32 order: a running sum in ascending cell order, then one division:
    cells - 1 rounded adds (the first lands on 0) + 1 division + 1 second order = cells + 1."""
    x64 = np.asarray(x, np.float64)
    cells = x.shape[1]
    return dict(ref=x64.sum(axis=1) / cells, mag=np.abs(x64).sum(axis=1) / cells, n_ops=float(cells + 1))


def mean_cells_f32(x):
    """The same mean, one float32 operation at a time in ascending cell order: what an f32 implementation must give bit for bit."""
    x = np.asarray(x, _F)
    acc = np.zeros((x.shape[0], x.shape[2]), _F)
    for k in range(x.shape[1]):
        acc = acc + x[:, k]
    assert acc.dtype == _F
    return acc / _F(x.shape[1])


def mask_resize(masks, OH, OW):
    """F.interpolate(mask != 0, (OH, OW), mode="bilinear", align_corners=False).  f32: scale = in / out, source =
    max(scale * (dst + .5) - .5, 0), its truncation, the neighbour (clamped at the last cell).  f64: the fraction l and
    (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11).  Rounded f32 operations on the way of one term: 1 - lx: 1,
    its product with v: 1, the row sum: 1, 1 - ly: 1, its product: 1, the final sum: 1, second order: 1 = 7.  mag = ref (every
    term is non-negative)."""
    m = (np.asarray(masks) != 0).astype(np.float64)
    n, H, W = m.shape

    def axis(L, O):
        s = _F(L) / _F(O)
        f = s * (np.arange(O, dtype=_F) + _F(0.5)) - _F(0.5)
        assert f.dtype == _F
        f = np.where(f < 0, _F(0), f)
        i0 = f.astype(np.int64)
        i1 = i0 + (i0 < L - 1)
        return i0, i1, f.astype(np.float64) - i0
    y0, y1, ly = axis(H, OH)
    x0, x1, lx = axis(W, OW)
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = (1 - lx) * m[:, y0][:, :, x0] + lx * m[:, y0][:, :, x1]
    bot = (1 - lx) * m[:, y1][:, :, x0] + lx * m[:, y1][:, :, x1]
    ref = (1 - ly) * top + ly * bot
    return dict(ref=ref, mag=ref.copy(), n_ops=7.0)


def roi_align_masked(feat, mask, boxes, scale, R, SR):
    """torchvision roi_align(aligned = False, sampling_ratio = SR) of feat * mask[roi] on one image.  feat [H][W][C],
    mask [n][H][W].  f32: corner = box * scale, roi = max(end - start, 1), bin = roi / R, sample =
    (start + p * bin) + ((i + .5) * bin) / SR, the validity window (a sample is dropped when EITHER coordinate is outside
    [-1, size]) and the cells as in ROIAlign; the mean is over all SR * SR samples.
    n_ops: the two weight factors and their product: 3; feat * mask: 1; times the weight: 1; the 4-term sum: 3; the running
    sum over SR * SR samples: SR * SR; the division: 1; second order: 1 = SR * SR + 10."""
    feat = np.asarray(feat, np.float64)
    mask = np.asarray(mask, np.float64)
    H, W, C = feat.shape
    b = np.asarray(boxes, _F).reshape(-1, 4) * _F(scale)
    assert b.dtype == _F
    n = b.shape[0]
    ref = np.zeros((n, C, R, R))
    mag = np.zeros((n, C, R, R))
    p = np.arange(R, dtype=_F)[:, None]
    i = np.arange(SR, dtype=_F)[None, :]

    def axis(start, end, L):
        roi = np.maximum(end - start, _F(1))
        bsz = roi / _F(R)
        v = (start + p * bsz) + ((i + _F(0.5)) * bsz) / _F(SR)
        assert v.dtype == _F
        ok = ~((v < _F(-1)) | (v > _F(L)))
        v = np.where(v <= 0, _F(0), v)
        v = np.where(ok, v, _F(0))
        lo = v.astype(np.int64)
        top = lo >= L - 1
        hi = np.where(top, L - 1, lo + 1)
        lo = np.where(top, L - 1, lo)
        fr = np.where(top, 0.0, v.astype(np.float64) - lo)
        return ok, lo, hi, fr
    for r in range(n):
        oy, yl, yh, ly = axis(b[r, 1], b[r, 3], H)           # [R][SR]
        ox, xl, xh, lx = axis(b[r, 0], b[r, 2], W)
        fm = feat * mask[r][:, :, None]
        for dst, src in ((ref, fm), (mag, np.abs(fm))):
            acc = np.zeros((R, R, C))
            for ya, wy in ((yl, (1 - ly) * oy), (yh, ly * oy)):
                for xa, wx in ((xl, (1 - lx) * ox), (xh, lx * ox)):
                    # [R][SR][R][SR][C] taps, weighted and summed over the two sample axes
                    acc += np.einsum("ai,bj,aibjc->abc", wy, wx, src[ya][:, :, xa])
            dst[r] = (acc / (SR * SR)).transpose(2, 0, 1)
    return dict(ref=ref, mag=mag, n_ops=float(SR * SR + 10))


def l2_normalize(x):
    """F.normalize(x, dim = 1, eps = 1e-12): x / max(||x||, 1e-12).  One 64-lane wave per row: every lane squares (1) and adds
    ceil(D / 64) values, the lanes meet in a 6-step tree (6), sqrt (1; it does not amplify the error of its argument), the
    division (1), second order (1) = ceil(D / 64) + 10.  mag = |ref|."""
    x = np.asarray(x, np.float64)
    nrm = np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)
    ref = x / nrm
    return dict(ref=ref, mag=np.abs(ref), n_ops=float(-(-x.shape[1] // 64) + 10))


def sqdist(a, b):
    """D[o][n] = sum_k (a[o][k] - b[n][k])^2.  The difference (1) enters the square twice and the square rounds (1): 3; the lane
    sum ceil(D / 64) and the 6-step tree; second order 1 = ceil(D / 64) + 10.  mag = ref (a sum of squares)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = a[:, None, :] - b[None, :, :]
    ref = (d * d).sum(axis=2)
    return dict(ref=ref, mag=ref.copy(), n_ops=float(-(-a.shape[1] // 64) + 10))


def assoc_fc(x, w, bias):
    """AssociationHead: raw = Linear(x) (x [n][K], w [N][K], bias [N] or None), y = F.normalize(raw).

    raw, f32 order: K is cut into slices of 128; inside a slice the products are accumulated by 4-wide f32 matrix instructions
    (each product and each accumulation rounds at most once; any term sees at most 128 accumulations); the slices are added in
    1024 / N groups of per = ceil(slices / groups) consecutive slices, sequentially, then the groups sequentially, then the
    bias: product 1 + 128 + per + groups + bias 1 + second order 1.  mag = sum |x w| + |bias|.

    y: with e = raw_got - raw, |e[n]| <= b[n] = bound(raw)[n], the computed norm differs from ||raw|| by at most ||b||_2
    (triangle inequality) before its own rounding, so
        |y_got - y| <= b[n] / nrm' + |raw[n]| ||b||_2 / (nrm nrm') + n_norm U |raw[n]| / nrm',   nrm' = nrm - ||b||_2,
    n_norm = square (1, entering twice: 2) + the 6-step wave tree + 3 adds of the four wave sums + sqrt 1 + division 1 +
    second order 1 = 14.  Returned as ``y_bound``; rows whose norm is within 2 ||b||_2 of 0 have no finite bound."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, K = w.shape
    raw = x @ w.T
    mag = np.abs(x) @ np.abs(w).T
    if bias is not None:
        raw = raw + np.asarray(bias, np.float64)[None, :]
        mag = mag + np.abs(np.asarray(bias, np.float64))[None, :]
    slices, groups = K // 128, 1024 // N
    per = -(-slices // groups)
    n_ops = float(1 + 128 + per + groups + 1 + 1)
    b = n_ops * U * mag
    nrm = np.sqrt((raw * raw).sum(axis=1, keepdims=True))
    bn = np.sqrt((b * b).sum(axis=1, keepdims=True))
    nrm_c = np.maximum(nrm, 1e-12)
    y = raw / nrm_c
    with np.errstate(all="ignore"):
        lo = nrm_c - bn
        y_bound = np.where(lo > bn, b / lo + np.abs(raw) * bn / (nrm_c * lo) + 14 * U * np.abs(raw) / lo, np.inf)
    return dict(ref=raw, mag=mag, n_ops=n_ops, y=y, y_bound=y_bound)


# ------------------------------------------------------------------------------------------------------ 16-bit rounding
def round16(v, st):
    """Round f64 values to the storage type (1 bf16, 2 f16), through f32 as a kernel's store does, back to f64.  Monotone, which
    is all the interval check round16(ref - b) <= got <= round16(ref + b) needs."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(torch.float32)
    return t.to(torch.bfloat16 if st == 1 else torch.float16).to(torch.float64).numpy()


def check(got, res, st=0, b=None):
    """Worst err / bound of ``got`` against a reference result (f32 outputs), or for 16-bit outputs the interval check
    round16(ref - b) <= got <= round16(ref + b).  Returns (ok, worst ratio); an element whose bound is 0 must be equal."""
    got = np.asarray(got, np.float64)
    ref = res["ref"]
    b = bound(res) if b is None else b
    if st == 0:
        err = np.abs(got - ref)
        with np.errstate(all="ignore"):
            ratio = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isnan(got), np.inf, ratio)
        return bool((ratio <= 1).all()), float(ratio.max()) if ratio.size else 0.0
    lo, hi = round16(ref - b, st), round16(ref + b, st)
    ok = (got >= lo) & (got <= hi)                       # NaN fails both
    # the ratio reported: 0 where got is the rounding of ref itself; otherwise how far ref had to move to round to got -- to
    # the midpoint between the two stored values -- as a fraction of b
    near = round16(ref, st)
    with np.errstate(all="ignore"):
        ratio = np.where(got == near, 0.0, np.abs((got + near) / 2 - ref) / b)
    ratio = np.where(ok, ratio, np.inf)
    return bool(ok.all()), float(ratio.max()) if ratio.size else 0.0
