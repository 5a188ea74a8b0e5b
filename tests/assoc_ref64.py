"""float64 references of the association kernels: the two online triplet losses with their gradients, the training fc +
F.normalize forward and backward (csrc/assoc_train.hip), and l2_normalize / sqdist (csrc/roi.hip).  numpy only, no autograd,
written from the published operations (online_triplet_loss/losses.py, F.normalize, Linear) and independent of the f32
restatement tests/assoc_train_ref.py.  tests/test_assoc_ref64.py pins it to the reference project's golden output.

Everything continuous is f64.  The discrete rules are the published ones: max / min ties go to the lowest index, the hinge is
strict (``tl[tl < 0] = 0``: a triplet with tl == 0 keeps its gradient), a triplet counts as positive when tl > 1e-16.
``wrong_rule`` switches one of them to a plausible mistake ("ties_high", "hinge_nonstrict", "count_ge"), so a test can prove
that its inputs tell the rules apart.

Error bounds are derived, never fitted.  U = 2^-24 is the unit roundoff of f32.  A chain of m rounded operations multiplies
a term by (1 + d)^m, |d| <= U, and (1 + U)^m - 1 <= (m + 1) U while m (m + 1) U <= 1; so a sum of terms that each pass at
most m rounded operations is off by at most (m + 2) U sum |terms| (one more for the reference's own 2^-53).  fmaf rounds
once per step, so a D-term fmaf chain is m = D.

tau, the worst f32 error of one Gram-form distance d0[i][j] = (sq[j] - 2 G[i][j]) + sq[i]: sq and G are D-step fmaf chains,
|error(G)| <= (D + 1) U sum_d |e_id e_jd| <= (D + 1) U |e_i| |e_j| (Cauchy-Schwarz), likewise sq[i] with |e_i|^2; 2 G is
exact; the two additions round once each, every term passing at most both: D + 2 operations, + 1 second order:
    tau[i][j] = (D + 3) U (|e_i|^2 + 2 |e_i| |e_j| + |e_j|^2).
Two decisions taken on d0 values further apart than 2 tau come out the same in f32 and in f64.
"""
import numpy as np

U = 2.0 ** -24
EPS_NORM = float(np.float32(1e-12))          # F.normalize's eps as an f32 kernel holds it
CNT_EPS = float(np.float32(1e-16))           # the positive-triplet threshold, likewise
WRONG_RULES = ("ties_high", "hinge_nonstrict", "count_ge")


# ------------------------------------------------------------------------------------------------------ triplet losses
def _distances(e, squared, exact_d0=False):
    """-> d0 (f64 Gram form; exactly 0 between identical rows, as equal fmaf chains give), d, tau, dd (d d / d d0).
    exact_d0: the caller knows every f32 product and sum is exact (integer rows), so tau = 0."""
    e = np.asarray(e, np.float64)
    n, D = e.shape
    G = e @ e.T
    sq = np.einsum("id,id->i", e, e)
    d0 = (sq[None, :] - 2.0 * G) + sq[:, None]
    _, inv = np.unique(e, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    d0[inv[:, None] == inv[None, :]] = 0.0
    nrm = np.sqrt(sq)
    tau = (0.0 if exact_d0 else (D + 3) * U) * (nrm[:, None] + nrm[None, :]) ** 2
    dc = np.maximum(d0, 0.0)
    if squared:
        return d0, dc, tau, (d0 >= 0).astype(np.float64)
    with np.errstate(divide="ignore"):
        d = np.sqrt(dc)                                  # eq(0) mask: (1 - m) sqrt(d + m 1e-16) is 0 at 0, sqrt elsewhere
        dd = np.where(dc > 0, 0.5 / np.where(dc > 0, d, 1.0), 0.0)      # zero gradient at zero distance and under the clamp
    return d0, d, tau, dd


def _arg(v, want_max, high):
    """argmax / argmin along axis 1 with ties to the lowest (published) or highest index."""
    if not high:
        return v.argmax(1) if want_max else v.argmin(1)
    r = v[:, ::-1]
    return v.shape[1] - 1 - (r.argmax(1) if want_max else r.argmin(1))


def _gap(vals, want_max):
    """|best - runner-up| of a 1-d array (inf with fewer than two entries)."""
    if vals.size < 2:
        return np.inf
    s = np.sort(vals)
    return float(s[-1] - s[-2]) if want_max else float(s[1] - s[0])


def _grad(e, gd, dd, scale):
    """dE and its f32 bound from the coefficients gd of the loss in each distance.  The kernel forms, per anchor a,
    w[a][j] = c(gd[a][j]) + c(gd[j][a]) (squared: exact small integers; otherwise sqrt, the division and the sum: 3 rounded
    operations), then acc = fma(w, e_a - e_j, acc) over the m_a entries with w != 0 (the difference 1, the fma 1 per step:
    m_a + 1), 2 acc (exact), times g = grad / divisor (the divisor's conversion, the division, the product: 3), second order 1:
    n_ops = m_a + 8.  mag >= sum_j |w| |e_a - e_j| by the triangle inequality."""
    w = gd * dd
    W = w + w.T
    e = np.asarray(e, np.float64)
    de = 2.0 * scale * (W.sum(1, keepdims=True) * e - W @ e)
    A = np.abs(W)
    mag = 2.0 * abs(scale) * (A.sum(1, keepdims=True) * np.abs(e) + A @ np.abs(e))
    n_ops = (W != 0).sum(1, keepdims=True) + 8.0
    return de, dict(ref=de, mag=mag, n_ops=n_ops)


def batch_hard(labels, e, margin, squared=False, wrong_rule=None, grad=1.0, exact_d0=False):
    """batch_hard_triplet_loss: per anchor the hardest positive max_j mask_ap d, the row maximum, the hardest negative
    min_j d + rowmax (1 - mask_an), tl = hp - hn + margin hinged, the mean over anchors.

    Returns a dict: loss, dE, dE_res (ref / mag / n_ops for ``check``), tau_max, and per anchor the decision margins
      pos_gap   d0 gap between the hardest positive and its runner-up (inf with fewer than two positives)
      neg_gap   the same for the hardest negative among the negatives (inf with fewer than two negatives)
      max_gap   the same for the row maximum, where it enters the result (no negative: the minimum falls on a masked entry)
      row_tau   the largest tau of the anchor's row
      tl, tl_tau   the triplet value before the hinge and its worst f32 error (tau of both distances through the sqrt, + 3
                   rounded operations on |hp| + |hn| + |margin|)
    """
    assert wrong_rule in (None,) + WRONG_RULES
    e = np.asarray(e, np.float64)
    labels = np.asarray(labels, np.float64)
    n = e.shape[0]
    high = wrong_rule == "ties_high"
    d0, d, tau, dd = _distances(e, squared, exact_d0)
    same = labels[None, :] == labels[:, None]
    m_ap = same & ~np.eye(n, dtype=bool)
    m_an = ~same
    r = np.arange(n)
    ap = m_ap * d
    jp = _arg(ap, True, high)
    jm = _arg(d, True, high)
    rowmax = d[r, jm]
    an = d + rowmax[:, None] * (~m_an)
    jn = _arg(an, False, high)
    hp, hn = ap[r, jp], an[r, jn]
    tl = (hp - hn) + margin
    active = (tl > 0) if wrong_rule == "hinge_nonstrict" else ~(tl < 0)
    loss = float(np.where(active, tl, 0.0).sum() / n)
    gd = np.zeros((n, n))
    act = active.astype(np.float64)
    np.add.at(gd, (r, jp), act * m_ap[r, jp])
    np.add.at(gd, (r, jn), -act)
    np.add.at(gd, (r, jm), -act * (~m_an[r, jn]))
    de, res = _grad(e, gd, dd, grad / n)
    pos_gap, neg_gap, max_gap = np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf)
    for a in range(n):
        pos_gap[a] = _gap(d0[a, m_ap[a]], True)
        neg_gap[a] = _gap(d0[a, m_an[a]], False)
        if not m_an[a, jn[a]]:
            max_gap[a] = _gap(d0[a], True)
    slope = np.where(dd > 0, dd, 0.0) if not squared else np.ones_like(dd)
    tl_tau = tau[r, jp] * slope[r, jp] + tau[r, jn] * slope[r, jn] + 3 * U * (np.abs(hp) + np.abs(hn) + abs(margin))
    return dict(loss=loss, dE=de, dE_res=res, tau_max=float(tau.max()), pos_gap=pos_gap, neg_gap=neg_gap, max_gap=max_gap,
                row_tau=tau.max(1), tl=tl, tl_tau=tl_tau, d0=d0, jp=jp, jn=jn, jm=jm)


def batch_all(labels, e, margin, squared=False, wrong_rule=None, grad=1.0, exact_d0=False):
    """batch_all_triplet_loss: over the valid triplets (a, p, k) -- p != a, label p == label a, label k != label a --
    tl = d[a][p] - d[a][k] + margin hinged; loss = sum / (P + 1e-16), fraction = P / (V + 1e-16), P = #(tl > 1e-16), V = #valid.
    One anchor at a time over (positives x negatives); no n^3 tensor.

    Returns a dict: loss, P, V (exact integers), dE, dE_res, tau_max, and the hinge margin
      tl_min      min |tl| over the valid triplets with tl != 0 (inf if none), n_zero = #(tl == 0)
      tl_margin   per anchor, min over its valid triplets with tl != 0 of |tl| - 2 tl_tau (tl_tau as in batch_hard; inf without
                  triplets): all > 0 means every hinge and every count decision not exactly on the hinge is the same in f32
    """
    assert wrong_rule in (None,) + WRONG_RULES
    e = np.asarray(e, np.float64)
    labels = np.asarray(labels, np.float64)
    n = e.shape[0]
    d0, d, tau, dd = _distances(e, squared, exact_d0)
    slope = np.ones_like(dd) if squared else dd
    terr = tau * slope + 3 * U * d                          # per distance: tau through the sqrt + its share of the 3 operations
    gd = np.zeros((n, n))
    total, P, V, n_zero = 0.0, 0, 0, 0
    tl_min, tl_margin = np.inf, np.full(n, np.inf)
    for a in range(n):
        same = labels == labels[a]
        pos = np.nonzero(same & (np.arange(n) != a))[0]
        neg = np.nonzero(~same)[0]
        if pos.size == 0 or neg.size == 0:
            continue
        tl = (d[a, pos][:, None] - d[a, neg][None, :]) + margin
        keep = (tl > 0) if wrong_rule == "hinge_nonstrict" else ~(tl < 0)
        total += float(tl[keep].sum())
        P += int((tl >= CNT_EPS).sum() if wrong_rule == "count_ge" else (tl > CNT_EPS).sum())
        V += tl.size
        gd[a, pos] += keep.sum(1)
        gd[a, neg] -= keep.sum(0)
        at = np.abs(tl)
        n_zero += int((tl == 0).sum())
        tt = (terr[a, pos][:, None] + terr[a, neg][None, :]) + 3 * U * abs(margin)
        if (tl != 0).any():
            tl_min = min(tl_min, float(at[tl != 0].min()))
            tl_margin[a] = float((at - 2 * tt)[tl != 0].min())
    div = P + 1e-16
    de, res = _grad(e, gd, dd, grad / div)
    return dict(loss=total / div, P=P, V=V, dE=de, dE_res=res, tau_max=float(tau.max()), tl_min=tl_min, n_zero=n_zero,
                tl_margin=tl_margin)


def fraction_f32(P, V):
    """the fraction as the kernel must give it bit for bit: f32(P) / (f32(V) + 1e-16f)"""
    return np.float32(P) / (np.float32(V) + np.float32(1e-16))


# ------------------------------------------------------------------------------------------------------ training fc
def fc_splits(n, K, D):
    """(S, rchunk) of the training forward: K is cut into S chunks of rchunk (a multiple of 16; the last may be short) so that
    about 1024 blocks of 64 x 64 outputs run, at most one chunk per 256 of K (DESIGN.md "Association-head training")."""
    tiles = -(-n // 64) * -(-D // 64)
    s = max(min(-(-1024 // tiles), -(-K // 256)), 1)
    rc = -(-(-(-K // s)) // 16) * 16
    return -(-K // rc), rc


def _normalize_bounds(z, bz, n_norm):
    """E = z / max(|z|, eps) and inv = 1 / max(|z|, eps) with bounds, given |z_got - z| <= bz element by element.  The computed
    norm differs from |z| by at most |bz|_2 (triangle inequality) before its own n_norm rounded operations, so with
    den' >= den - |bz|_2 =: lo
        |E_got - E| <= bz / lo + |z| |bz|_2 / (den lo) + n_norm U |z| / lo
        |inv_got - inv| <= |bz|_2 / (den lo) + n_norm U / lo.
    A row that is exactly 0 (bz = 0) gives E = 0 and inv = 1 / eps up to the division's rounding; a row whose norm is within
    2 |bz|_2 of eps has no finite bound (the max() may go either way)."""
    nrm = np.sqrt((z * z).sum(1, keepdims=True))
    bn = np.sqrt((bz * bz).sum(1, keepdims=True))
    den = np.maximum(nrm, EPS_NORM)
    lo = den - bn
    with np.errstate(all="ignore"):
        ok = (lo > bn) & ((np.abs(nrm - EPS_NORM) > 2 * bn) | (bn == 0))
        eb = np.where(ok, bz / lo + np.abs(z) * bn / (den * lo) + n_norm * U * np.abs(z) / lo, np.inf)
        ib = np.where(ok, bn / (den * lo) + n_norm * U / lo, np.inf)
    return z / den, eb, (1.0 / den)[:, 0], ib[:, 0]


def fc_forward(x, w, b, S=None, rchunk=None):
    """E = F.normalize(x w^T + b), inv_norm = 1 / max(|Z|, eps).  x [n][K], w [D][K], b [D].

    f32 order: S partial sums over chunks of rchunk, each one fmaf chain (rchunk operations), added in s order onto 0 (S), then
    the bias (1): m = rchunk + S + 1, bound_z = (m + 2) U (|x| |w|^T + |b|).  The normalise: the square (entering twice: 2), the
    8-step tree over 256 threads, sqrt, the division, second order: n_norm = 13."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    n, K = x.shape
    if S is None:
        S, rchunk = fc_splits(n, K, w.shape[0])
    z = x @ w.T + b[None, :]
    mag = np.abs(x) @ np.abs(w).T + np.abs(b)[None, :]
    bz = (min(rchunk, K) + S + 1 + 2) * U * mag
    E, eb, inv, ib = _normalize_bounds(z, bz, 13)
    return dict(Z=z, Z_bound=bz, E=E, E_bound=eb, inv_norm=inv, inv_bound=ib)


def fc_backward(x, E, inv_norm, dE):
    """dZ = (dE - E (E . dE)) inv_norm, db = sum_i dZ, dW = dZ^T x from the f32 E and inv_norm the forward kernel produced.

    dot = E . dE: product 1 + the 8-step tree: |error| <= 10 U sum |E dE|.  dZ: E dot (1), the difference (1), times inv (1):
    |dZ_got - dZ| <= bdz = inv U (3 |dE| + 13 |E| sum |E dE|) + second order (x 1.001).  db and dW are chains of length n over
    i: (n + 2) U sum_i |terms| plus the terms' own error sum_i bdz |x|."""
    x, E, dE = np.asarray(x, np.float64), np.asarray(E, np.float64), np.asarray(dE, np.float64)
    inv = np.asarray(inv_norm, np.float64)[:, None]
    n = x.shape[0]
    dot = (E * dE).sum(1, keepdims=True)
    adot = (np.abs(E) * np.abs(dE)).sum(1, keepdims=True)
    dz = (dE - E * dot) * inv
    bdz = 1.001 * inv * U * (3 * np.abs(dE) + 13 * np.abs(E) * adot)
    db = dz.sum(0)
    db_b = bdz.sum(0) * 1.001 + (n + 2) * U * np.abs(dz).sum(0)
    dw = dz.T @ x
    dw_b = (bdz.T @ np.abs(x)) * 1.001 + (n + 2) * U * (np.abs(dz).T @ np.abs(x))
    return dict(dZ=dz, dW=dw, dW_bound=dw_b, db=db, db_bound=db_b)


# ------------------------------------------------------------------------------------------------------ inference
def l2_normalize(x):
    """x / max(|x|, eps), one 64-lane wave per row: every lane squares (entering twice: 2) and adds ceil(D / 64) values, the
    6-step tree, sqrt, the division, second order: n_ops = ceil(D / 64) + 11 on mag = |ref|.  Rows with a norm below eps divide
    by eps exactly: the same count covers them."""
    x = np.asarray(x, np.float64)
    den = np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), EPS_NORM)
    ref = x / den
    return dict(ref=ref, mag=np.abs(ref), n_ops=float(-(-x.shape[1] // 64) + 11))


def sqdist(a, b):
    """out[o][n] = sum_k (a[o][k] - b[n][k])^2: the difference (entering the square twice: 2), the square (1), ceil(D / 64) lane
    adds, the 6-step tree, second order: n_ops = ceil(D / 64) + 10 on mag = ref.  Identical rows give exactly 0 (mag = 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = a[:, None, :] - b[None, :, :]
    ref = (d * d).sum(2)
    return dict(ref=ref, mag=ref.copy(), n_ops=float(-(-a.shape[1] // 64) + 10))


def check(got, ref, bound):
    """(ok, worst err / bound) element by element; an element whose bound is 0 must be equal; NaN fails."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(got), np.inf, ratio)
    return bool((ratio <= 1).all()), float(ratio.max()) if ratio.size else 0.0


def check_res(got, res):
    return check(got, res["ref"], res["n_ops"] * U * res["mag"])
