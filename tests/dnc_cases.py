"""Case builder and numpy fp64 reference for DnC (byzantine_aircomp_amd dnc, csrc/dnc.hip),
shared by tests/test_dnc_cpu.py and tests/test_gpu_dnc.py.  Importing it needs no GPU.

case(K, f, d, seed): rows 0.05 N(0,1) + 0.001 j + t_k p with p ~ N(0,1)^d; t_k of the K - f honest
rows a grid on [0, 0.2], of the last f rows minus a grid on [0.5, 1.0]; the rows then permuted.
The colluding rows line up along p, which is what the top singular vector of the centred sample
finds.

reference(X, cols, q): the definition of include/gmagg.h in numpy fp64: per round the column
means summed in row order, the SVD of the centred sub-matrix, the scores (c_k . v)^2, the K - q
rows first in the (score, index) order with NaN last; the intersection of the rounds; the
sequential fp64 mean of the good rows in increasing row index, rounded once (one good row: the
row itself).  A sub-matrix that is not finite scores NaN everywhere, as the definition's
non-finite norm does.

Preconditions, asserted by reference(..., check=True) for every round (they are conditions on the
inputs, computed from the reference alone):
  * sigma_2 / sigma_1 <= 0.5: the power iteration contracts by at least 4 per application of
    C^T C, so the 1e-10 stop on the iterate's movement leaves the scores some 1e-10 of the
    largest, against the 1e-9 bar of the GPU tests;
  * the score gap across the cut (between the last kept and the first dropped row) is at least
    1e-6 of the largest score, three orders above that bar: the selection is decided.
"""
import functools

import numpy as np

F32 = np.float32
SCORE_TOL = 1e-9           # of the largest reference score
GAP_MIN = 1e-6             # of the largest reference score
SIGMA_RATIO_MAX = 0.5

# (K, f, d, b): a partial wave, the 64 / 65 and 1024 wave boundaries, n not a multiple of 4, all
# columns (b == d), d below and across a panel width
GPU_SHAPES = [(7, 1, 40, 8), (50, 10, 300, 64), (64, 13, 517, 100), (65, 16, 517, 517),
              (257, 60, 333, 128), (513, 100, 700, 200), (1000, 200, 2051, 256),
              (1024, 255, 1030, 300)]
CS = (0.5, 1.0, 1.5)
ITERS = (1, 3)
GPU_CASES = [(K, f, d, b, c, it) for (K, f, d, b) in GPU_SHAPES for c in CS for it in ITERS]


def removed(K, f, c, iters):
    """q = int(c f), or None where the definition refuses the call (q * iters >= K)."""
    q = int(c * f)
    return None if q * iters >= K else q


def case(K, f, d, seed):
    rng = np.random.RandomState(seed)
    p = rng.randn(d)
    t = np.empty(K)
    t[:K - f] = np.linspace(0.0, 0.2, K - f)
    t[K - f:] = -np.linspace(0.5, 1.0, f)
    X = 0.05 * rng.randn(K, d) + 0.001 * np.arange(d) + t[:, None] * p
    return np.ascontiguousarray(X[rng.permutation(K)].astype(F32))


def seed_of(K, f, d, b):
    return 1000 * K + 7 * f + d + b


@functools.lru_cache(maxsize=None)
def shape_input(K, f, d, b):
    X = case(K, f, d, seed_of(K, f, d, b))
    X.setflags(write=False)
    return X


def draw(d, b, iters, seed):
    """The library's own draw (torch CPU only): dnc.columns from a generator seeded `seed`."""
    import torch
    import byzantine_aircomp_amd as bz
    return bz.dnc.columns(d, b, iters, generator=torch.Generator().manual_seed(seed)).numpy()


def score_order(s):
    """Row indices in the order (score ascending, NaN last, ties to the lower index)."""
    nan = np.isnan(s)
    return np.lexsort((np.arange(s.size), np.where(nan, 0.0, s), nan))


def round_scores(X, J):
    """(scores, sigma) of one round: fp64 throughout on the fp32 values widened exactly."""
    S = X[:, J].astype(np.float64)
    K = S.shape[0]
    mu = np.zeros(S.shape[1])
    for k in range(K):                                   # row order
        mu += S[k]
    mu /= K
    with np.errstate(invalid="ignore"):
        Cm = S - mu
    if not np.isfinite(Cm).all():
        return np.full(K, np.nan), None
    _, sig, Vt = np.linalg.svd(Cm, full_matrices=False)
    return (Cm @ Vt[0]) ** 2, sig


def mean_rows(X, rows):
    if len(rows) == 1:
        return X[rows[0]].copy()
    acc = X[rows[0]].astype(np.float64)
    for k in rows[1:]:
        acc = acc + X[k].astype(np.float64)
    return (acc / len(rows)).astype(F32)


def reference(X, cols, q, check=False):
    """{"scores" [iters, K], "good" (increasing), "out" fp32 [d], "gap", "sigma_ratio"}; q == 0:
    no round is run (scores zero, every row good)."""
    K = X.shape[0]
    cols = np.asarray(cols)
    iters = cols.shape[0]
    scores = np.zeros((iters, K))
    good = np.ones(K, dtype=bool)
    gaps, ratios = [], []
    for t in range(iters if q > 0 else 0):
        s, sig = round_scores(X, cols[t])
        scores[t] = s
        order = score_order(s)
        kept = np.zeros(K, dtype=bool)
        kept[order[:K - q]] = True
        good &= kept
        if sig is not None and np.nanmax(s) > 0:
            gaps.append((s[order[K - q]] - s[order[K - q - 1]]) / s.max())
            ratios.append(sig[1] / sig[0] if sig.size > 1 else 0.0)
    if check:
        assert gaps and min(gaps) >= GAP_MIN, gaps
        assert max(ratios) <= SIGMA_RATIO_MAX, ratios
    rows = np.flatnonzero(good)
    return {"scores": scores, "good": rows, "out": mean_rows(X, rows),
            "gap": min(gaps) if gaps else None, "sigma_ratio": max(ratios) if ratios else None}


@functools.lru_cache(maxsize=None)
def gpu_case(K, f, d, b, c, iters):
    """(X, cols, q, reference) of one case of the GPU matrix, computed once; q None: refused."""
    X = shape_input(K, f, d, b)
    q = removed(K, f, c, iters)
    if q is None:
        return X, None, None, None
    if q == 0:
        return X, np.empty((iters, 0), dtype=np.int64), 0, reference(X, np.empty((iters, 0)), 0)
    cols = draw(d, b, iters, seed_of(K, f, d, b) + iters)
    return X, cols, q, reference(X, cols, q, check=True)
