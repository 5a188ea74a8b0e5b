"""Inputs of the association edge tests, shared by tests/test_assoc_ref64.py (which asserts on the CPU that they contain what
they claim) and tests/test_gpu_assoc_edges.py.

Family A, ``lattice``: integer embeddings in [-2, 2], not normalised.  In f32 every product, every partial sum of a Gram chain
and every d0 is an exact integer far below 2^24, so a kernel's d0 equals the f64 reference's bit for bit whatever its
summation order, ties are real ties, and with squared distances and an integer margin every tl is an exact integer.  From
n >= 16 and D >= 16 the rows below are planted (indices fixed; everything else is random):
    5  anchor A: all entries +-2       3, 9  = -A, label of A: the two farthest rows there can be -> tied hardest positives
    7, 11  = A with one entry moved by 1, another label -> tied hardest negatives (and a zero distance between two labels)
    1  Z = 0      2  = e1, label of Z      4  = e1 + e2, another label:  tl(Z) = 1 - 2 + 1 = 0 with squared distances,
                                                                          and tl(2, Z, 4) = 1 - 1 + m = m for the count rule
    6  C = (0, 0, 0, 2, 2, ...)   8  = C + 2 e1, label of C   10  = C + 2 e1 + 2 e2 + e3, another label:
                                                                          tl(C) = 2 - 3 + 1 = 0 with plain distances
    12 a label of its own (no positive)
Family B, ``unit_rows``: seeded random unit rows with a few small label groups; rows whose decisions are closer than the f32
error allows are redrawn from the same generator until none is left (n <= 300), so the result is a function of the seed."""
import numpy as np

import assoc_ref64 as R64

LATTICE_SHAPES = [(1, 1), (2, 5), (16, 16), (17, 33), (255, 64), (256, 128), (257, 100), (1024, 128), (1025, 32), (2048, 256)]
UNIT_SHAPES = [(48, 128), (257, 33), (300, 256)]
UNIT_SHAPES_LOSS_ONLY = [(1025, 128), (2048, 128)]
MARGIN_A = 1.0
MARGIN_CNT = float(np.float32(1e-16))       # tl == 1e-16f exactly where a positive and a negative are equally far
MARGIN_B = 0.2
PLANTED = 16                                # lattice cases from this n on (and D >= 4) hold the planted rows


def lattice(n, D):
    rng = np.random.RandomState(7000 + 13 * n + D)
    e = rng.randint(-2, 3, (n, D)).astype(np.float32)
    n_lab = int(min(64, max(2, n // 8)))
    lab = 1000.0 + rng.randint(0, n_lab, n).astype(np.float64) * 0.5        # labels are compared as values, not as integers
    if n < PLANTED or D < 16:
        return lab, e
    for k in range(n // 50):                                                  # a few duplicated rows, labels left as drawn
        i, j = rng.randint(13, n, 2)
        e[i] = e[j]
    A = (rng.randint(0, 2, D) * 4 - 2).astype(np.float32)
    near = A.copy()
    near[0] -= np.sign(A[0])
    C = np.full(D, 2, np.float32)
    C[:3] = 0
    unit = np.eye(D, dtype=np.float32)
    e[5], e[3], e[9], e[7], e[11] = A, -A, -A, near, near
    e[1], e[2], e[4] = 0, unit[0], unit[0] + unit[1]
    e[6], e[8], e[10] = C, C + 2 * unit[0], C + 2 * unit[0] + 2 * unit[1] + unit[2]
    lab[[5, 3, 9]] = 2001.0
    lab[[7, 11]] = 2002.0
    lab[[1, 2]] = 2003.0
    lab[[4, 10]] = 2004.0
    lab[[6, 8]] = 2005.0
    lab[12] = 2006.0
    return lab, e


def _unit(rng, k, D):
    x = rng.standard_normal((k, D)).astype(np.float32)
    return (x / np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(np.float32)


def _labels_b(rng, n, full):
    if full:
        return 300.0 + rng.randint(0, max(2, n // 32), n).astype(np.float64)
    lab = 5000.0 + np.arange(n, dtype=np.float64)             # singletons ...
    k = 0
    for g in range(n // 8):                                    # ... and n / 8 groups of 2 to 4 rows
        size = 2 + g % 3
        lab[k:k + size] = 300.0 + g
        k += size
    return lab[rng.permutation(n)]


def unit_margins(lab, e, margin=MARGIN_B):
    """Per anchor, whether every decision the two losses take there (both distance forms) is further from its alternative
    than twice the worst f32 error: -> bool [n], True = safe."""
    ok = np.ones(e.shape[0], bool)
    for squared in (False, True):
        h = R64.batch_hard(lab, e, margin, squared)
        ok &= (h["pos_gap"] > 2 * h["row_tau"]) & (h["neg_gap"] > 2 * h["row_tau"]) & (h["max_gap"] > 2 * h["row_tau"])
        ok &= np.abs(h["tl"]) > 2 * h["tl_tau"]
        a = R64.batch_all(lab, e, margin, squared)
        ok &= (a["tl_margin"] > 0) & (a["n_zero"] == 0)
    return ok


def unit_rows(n, D, seed=0, full_labels=False, repair=True):
    rng = np.random.RandomState(9000 + 17 * n + D + 1009 * seed)
    e = _unit(rng, n, D)
    lab = _labels_b(rng, n, full_labels)
    if not repair:
        return lab, e
    for _ in range(200):
        bad = np.nonzero(~unit_margins(lab, e))[0]
        if bad.size == 0:
            return lab, e
        e[bad] = _unit(rng, bad.size, D)
    raise AssertionError("unit_rows(%d, %d): decisions still inside the f32 error after 200 redraws" % (n, D))
