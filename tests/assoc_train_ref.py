"""numpy restatement of association-head training (dcnn/online_triplet_loss/losses.py, dcnn/networks/association_head.py,
torch.optim.SGD): the two triplet losses with their gradients in the embeddings written out by hand (no autograd), the
head's fc + F.normalize forward and backward, and the SGD step.  f32 throughout, following the reference's expression
order; ties of max / min go to the lowest index.  The GPU tests compare the HIP kernels with it, the CPU tests compare it
with the golden the reference itself produced."""
import numpy as np

F = np.float32


def _dist0(e):
    g = e @ e.T
    sq = np.diag(g).copy()
    return (sq[None, :] - F(2.0) * g) + sq[:, None]          # losses.py:27, before the clamp


def _dist(d0, squared):
    d = np.where(d0 < 0, F(0), d0).astype(F)
    if squared:
        return d
    m = (d == 0).astype(F)
    return ((F(1) - m) * np.sqrt(d + m * F(1e-16))).astype(F)


def _chain(g, d0, squared):
    """coefficient on the distance -> coefficient on d0 (clamp, eq(0) mask, sqrt)."""
    out = np.where(d0 < 0, F(0), g).astype(F)
    if squared:
        return out
    s = np.sqrt(np.maximum(d0, F(0)))
    return np.where(d0 > 0, out / (F(2) * np.where(s > 0, s, F(1))), F(0)).astype(F)


def _grad_from_coeffs(e, d0, gd, squared, scale):
    w = _chain(gd, d0, squared)
    w = w + w.T                                              # d0[i][j] depends on e_i and e_j
    de = F(2) * (w.sum(1, keepdims=True) * e - w @ e)
    return (de * F(scale)).astype(F)


def batch_hard(labels, e, margin, squared=False):
    """-> (loss, dE) of batch_hard_triplet_loss (losses.py:102-146)."""
    e = np.asarray(e, F)
    labels = np.asarray(labels, np.float64)
    n = e.shape[0]
    if n == 0:
        return F(np.nan), np.zeros_like(e)
    d0 = _dist0(e)
    d = _dist(d0, squared)
    same = labels[None, :] == labels[:, None]
    m_ap = (same & ~np.eye(n, dtype=bool)).astype(F)
    m_an = (~same).astype(F)
    ap = m_ap * d
    jp = ap.argmax(1)                       # numpy argmax / argmin: first index on ties
    jm = d.argmax(1)
    rowmax = d[np.arange(n), jm]
    an = d + rowmax[:, None] * (F(1) - m_an)
    jn = an.argmin(1)
    r = np.arange(n)
    tl = (ap[r, jp] - an[r, jn]) + F(margin)
    active = ~(tl < 0)
    loss = F(np.where(active, tl, F(0)).astype(np.float64).sum() / n)
    gd = np.zeros((n, n), F)
    for a in range(n):
        if active[a]:
            gd[a, jp[a]] += m_ap[a, jp[a]]
            gd[a, jn[a]] += F(-1)
            gd[a, jm[a]] += -(F(1) - m_an[a, jn[a]])
    return loss, _grad_from_coeffs(e, d0, gd, squared, F(1) / F(n))


def batch_all(labels, e, margin, squared=False):
    """-> (loss, fraction_positive_triplets, dE) of batch_all_triplet_loss (losses.py:149-197)."""
    e = np.asarray(e, F)
    labels = np.asarray(labels, np.float64)
    n = e.shape[0]
    if n == 0:
        return F(0), F(0), np.zeros_like(e)
    d0 = _dist0(e)
    d = _dist(d0, squared)
    same = labels[None, :] == labels[:, None]
    eye = np.eye(n, dtype=bool)
    valid = (same & ~eye)[:, :, None] & (~same)[:, None, :]            # [a, p, k]
    tl = (d[:, :, None] - d[:, None, :]) + F(margin)
    tl = np.where(valid, tl, F(0)).astype(F)
    keep = valid & ~(tl < 0)
    hinged = np.where(keep, tl, F(0))
    P = int((hinged > F(1e-16)).sum())
    V = int(valid.sum())
    div = F(P + 1e-16)
    loss = F(F(hinged.astype(np.float64).sum()) / div)
    frac = F(F(P) / (F(V) + F(1e-16)))
    gd = keep.sum(2).astype(F) - keep.sum(1).astype(F)               # +count at each p, -count at each k
    return loss, frac, _grad_from_coeffs(e, d0, gd, squared, F(1) / div)


def fc_forward(x, w, b):
    """x [n, C, H, W] -> (E, inv_norm): x.view(n, -1) @ w.T + b, then F.normalize (association_head.py:27-31)."""
    xf = np.asarray(x, F).reshape(x.shape[0], -1)
    z = (xf.astype(np.float64) @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)).astype(F)
    den = np.maximum(np.sqrt((z.astype(np.float64) ** 2).sum(1)), 1e-12).astype(F)
    return (z / den[:, None]).astype(F), (F(1) / den).astype(F)


def fc_backward(x, e, inv_norm, de):
    """-> (dW, db): dZ = (dE - E (E . dE)) inv_norm, dW = dZ^T X, db = sum_i dZ."""
    xf = np.asarray(x, F).reshape(x.shape[0], -1)
    dz = (de - e * (e * de).sum(1, keepdims=True)) * inv_norm[:, None]
    return (dz.astype(np.float64).T @ xf.astype(np.float64)).astype(F), dz.astype(np.float64).sum(0).astype(F)


def sgd_step(p, grad, state, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """torch.optim.SGD on one parameter; ``state`` holds the momentum buffer.  Returns the new p."""
    d = np.asarray(grad, F)
    if weight_decay != 0:
        d = d + F(weight_decay) * p
    if momentum != 0:
        buf = state.get("buf")
        buf = d.copy() if buf is None else buf * F(momentum) + F(1 - dampening) * d
        state["buf"] = buf
        d = d + F(momentum) * buf if nesterov else buf
    return (p + F(-lr) * d).astype(F)
