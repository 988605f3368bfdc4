"""Inputs, numpy references and checks of nearest-neighbor mixing (byzantine_aircomp_amd nnm /
mixed, csrc/nnm.hip), shared by tests/test_nnm_cpu.py and tests/test_gpu_nnm.py.  Importing it
needs no GPU and nothing of the library.

Notation: K rows, f Byzantine rows to mix against, m = K - f.  The definition (include/gmagg.h):
D[i][j] the squared distance with D[i][i] = 0; N(i) the m rows first in the order of
(D[i][j], j), NaN last; Y[i] = the sum of the rows of N(i) / m, rounded to fp32 once.

Neighbours (check_neighbors).  The kernel's distances are pair_dist's: per term one fp32
subtraction (relative 2^-24 on the difference, hence 2^-23 on its square), 32 fp32 fma roundings
per 32-column stage, fp64 across stages (negligible): at most 34 * 2^-24 ~ 2.03e-6 relative,
below EPS_D = 2^-18 ~ 3.8e-6.  With b the m-th smallest reference distance of row i, the kernel's
list must hold every j with D[i][j] < b (1 - EPS_D) and no j with D[i][j] > b (1 + EPS_D); what
lies in the band may go either way.  A row whose (m + 1)-th distance lies in the band of its
m-th is ambiguous; a shape is usable when at most 5 % of its rows are (asserted).

Values (mix_mismatch).  The reference is the exact sum of the kernel's OWN neighbour list,
correctly rounded to fp64 (what math.fsum returns), divided by m, rounded to fp32.  The bar on
finite reference entries:
    |got - ref| <= 2^-24 |ref| + 2^-41 mean|x_kept| + 2^-149
one fp32 rounding, plus an fp64 accumulation of n <= 4096 terms in another order
(n 2^-53 sum|x| / n), as robust_cases.meamed_mismatch.  Non-finite entries must match exactly.
"""
import functools
import math

import numpy as np

import robust_cases as rc

F32 = np.float32
EPS_D = 2.0 ** -18
MAX_AMBIGUOUS = 0.05

# (K, d, fo, f): robust_cases.spread(K, d, fo) mixed against f.  f != fo puts the boundary inside
# the honest cluster (f > fo) or inside the Byzantine one (f < fo).
NNM_CASES = [(17, 1000, 3, 3), (50, 7850, 10, 10), (65, 333, 13, 1), (65, 333, 13, 13),
             (256, 2051, 50, 50), (256, 2051, 50, 100), (600, 1030, 100, 100),
             (600, 1030, 100, 250), (1000, 520, 100, 100), (1000, 520, 100, 400),
             (1024, 70, 200, 60), (1024, 70, 200, 200)]
BIG_CASES = [(1100, 40, 220, 220), (2049, 24, 409, 409)]
# 8 < K <= 16, the one rows-per-wave regime of the mixing kernel (1, 2, 4, 8 rows at K <= 8, 16,
# 32, above) that the shapes above and the K = 8 / K = 1 tests leave out
SMALL_CASES = [(12, 70, 2, 3)]
LAYOUT_CASE = (257, 333, 50, 50)


def ref_dist(X):
    """fp64 squared distances from the differences themselves, zero diagonal (an inf entry
    makes its row's own difference NaN: the definition says 0)."""
    x = np.asarray(X, dtype=np.float64)
    K = x.shape[0]
    D = np.empty((K, K))
    with np.errstate(all="ignore"):
        for i in range(K):
            t = x - x[i]
            D[i] = (t * t).sum(axis=1)
    np.fill_diagonal(D, 0.0)
    return D


def ref_neighbors(X, f, D=None):
    """int64 [K, m]: per row the m first of np.lexsort((j, D[i])) (NaN last), increasing."""
    D = ref_dist(X) if D is None else D
    K = D.shape[0]
    m = K - f
    j = np.arange(K)
    return np.stack([np.sort(np.lexsort((j, D[i]))[:m]) for i in range(K)])


def _membership(N, K):
    W = np.zeros((N.shape[0], K))
    np.put_along_axis(W, np.asarray(N, dtype=np.int64), 1.0, axis=1)
    return W


def ref_mix(X, N, with_scale=False):
    """fp32 [K, d]: per entry math.fsum over the rows N[i] (the exact sum, correctly rounded to
    fp64), divided by m, rounded to fp32; IEEE for non-finite terms (a NaN, or both infinities,
    gives NaN).  with_scale: also mean|x_kept| per entry (fp64).

    The exact sums come from exact partial sums instead of K d Python loops: the finite values
    are split into pieces on grids 2^41 apart, each piece at most 2^40 grid units, so that a sum
    of up to 4096 of them is an integer below 2^53 units and the fp64 matrix product W @ piece
    is exact in any order; math.fsum then adds the few piece sums of an entry."""
    x = np.asarray(X, dtype=F32).astype(np.float64)
    K = x.shape[0]
    N = np.asarray(N, dtype=np.int64)
    m = N.shape[1]
    assert m <= 4096
    W = _membership(N, K)
    fin = np.isfinite(x)
    r = np.where(fin, x, 0.0)
    top = np.abs(r).max() if r.size else 0.0
    sums = []
    if top > 0.0:
        u = 2.0 ** (math.frexp(top)[1] - 40)               # |r| <= 2^40 u
        while np.any(r != 0.0):
            p = np.round(r / u) * u
            sums.append(W @ p)
            r = r - p                                      # exact; |r| <= u / 2
            u *= 2.0 ** -41
    if not sums:
        S = W @ r                                          # signed zeros only
    elif len(sums) == 1:
        S = sums[0]
    else:
        flat = [s.ravel().tolist() for s in sums]
        S = np.array(list(map(math.fsum, zip(*flat)))).reshape(sums[0].shape)
    with np.errstate(all="ignore"):
        if not fin.all():
            nan = (W @ np.isnan(x).astype(np.float64)) > 0
            pinf = (W @ (x == np.inf).astype(np.float64)) > 0
            ninf = (W @ (x == -np.inf).astype(np.float64)) > 0
            S = np.where(pinf, np.inf, S)
            S = np.where(ninf, -np.inf, S)
            S = np.where(nan | (pinf & ninf), np.nan, S)
        out = (S / m).astype(F32)
        if not with_scale:
            return out
        # (of the finite terms: an entry with a non-finite term is compared exactly, and
        # 0 * inf in the product would make the whole column's scale NaN)
        return out, (W @ np.where(fin, np.abs(x), 0.0)) / m


def brute_neighbors(X, f):
    """The definition, row by row in Python: sort by (is NaN, D, j), take m, sort the indices."""
    x = np.asarray(X, dtype=np.float64)
    K = x.shape[0]
    out = []
    for i in range(K):
        keys = []
        for j in range(K):
            with np.errstate(all="ignore"):
                dij = 0.0 if i == j else float(((x[i] - x[j]) ** 2).sum())
            keys.append((math.isnan(dij), dij, j))
        out.append(sorted(k[2] for k in sorted(keys)[:K - f]))
    return np.array(out, dtype=np.int64)


def brute_mix(X, N):
    """math.fsum over N[i], entry by entry (finite inputs)."""
    x = np.asarray(X, dtype=F32).astype(np.float64)
    m = len(N[0])
    return np.array([[math.fsum(x[k, j] for k in N[i]) / m for j in range(x.shape[1])]
                     for i in range(len(N))]).astype(F32)


def check_neighbors(N_got, X, f, D=None, rows=None):
    """Asserts the module docstring's conditions on the kernel's lists; returns the number of
    ambiguous rows (asserted to be at most MAX_AMBIGUOUS of the rows checked).  rows: the rows
    whose band and ambiguity are checked (all by default; the shape of the lists is always
    checked on every row)."""
    D = ref_dist(X) if D is None else D
    K = D.shape[0]
    m = K - f
    N_got = np.asarray(N_got, dtype=np.int64)
    assert N_got.shape == (K, m), (N_got.shape, (K, m))
    assert N_got.min() >= 0 and N_got.max() < K
    assert (np.diff(N_got, axis=1) > 0).all(), "rows of N must be strictly increasing"
    assert (N_got == np.arange(K)[:, None]).any(axis=1).all(), "row i must be in N(i)"
    rows = np.arange(K) if rows is None else np.asarray(rows)
    member = (_membership(N_got, K) > 0)[rows]
    Dr = D[rows]
    srt = np.sort(Dr, axis=1)                              # NaN last
    b = srt[:, m - 1:m]
    with np.errstate(all="ignore"):
        must = Dr < b * (1.0 - EPS_D)
        never = Dr > b * (1.0 + EPS_D)
        bad = (must & ~member) | (never & member)
        assert not bad.any(), f"rows {rows[bad.any(axis=1)][:8]} miss the distance band"
        ambiguous = int((srt[:, m] <= b[:, 0] * (1.0 + EPS_D)).sum()) if m < K else 0
    assert ambiguous <= MAX_AMBIGUOUS * rows.size, f"{ambiguous} ambiguous rows of {rows.size}"
    return ambiguous


def mix_mismatch(got, ref, scale):
    """Flat indices where `got` misses the bar of the module docstring."""
    got = np.asarray(got, dtype=F32)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        tol = 2.0 ** -24 * np.abs(ref.astype(np.float64)) + 2.0 ** -41 * scale + 2.0 ** -149
        bad_fin = fin & ~(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= tol)
    bad_non = ~fin & ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    return np.flatnonzero(bad_fin | bad_non)


@functools.lru_cache(maxsize=None)
def case(K, d, fo):
    """(X fp32 numpy [K, d], D fp64 [K, K]) of robust_cases.spread(K, d, fo); computed once,
    never modified."""
    X = rc.spread(K, d, fo).numpy()
    D = ref_dist(X)
    X.setflags(write=False)
    D.setflags(write=False)
    return X, D


@functools.lru_cache(maxsize=None)
def copies_input():
    """K = 65, d = 40: robust_cases.spread with rows 5, 9, 12, 20, 21, 33, 40, 47, 58, 64 all
    copies of row 5 (ten rows at distance exactly 0 of each other)."""
    X = rc.spread(65, 40, 13).numpy().copy()
    X[[9, 12, 20, 21, 33, 40, 47, 58, 64]] = X[5]
    X.setflags(write=False)
    return X
