"""Inputs and numpy references of meamed / multi_krum / bulyan (byzantine_aircomp_amd,
csrc/robust.hip), shared by tests/test_robust_cpu.py and tests/test_gpu_robust.py.  Importing it
needs no GPU and nothing of the library.

Notation: K rows, honest = options['honestSize'], f = K - honest.

meamed (ref_meamed), per column over the rows used: values read as x + 0.0f; med = the lower
median (rank (n - 1) // 2); dev = |x - med| as ONE fp32 subtraction; the `keep` smallest dev by
stable argsort (ties to the lower row index, numpy sorts NaN after +inf); the fp64 sum of the
kept values / keep, rounded to fp32 once; a NaN among the rows used gives NaN.
  Bar (meamed_mismatch) on finite reference entries:
      |got - ref| <= 2^-24 |ref| + 2^-42 mean|x_kept| + 2^-149
  one fp32 rounding (2^-24 |ref|, plus half the smallest subnormal) and the fp64 accumulation
  bound for n <= 1024 terms summed in another order: n * 2^-53 * sum|x| / keep <= 2^-43
  mean|x_kept| for each of the two sums.  Non-finite reference entries must match exactly.

Krum scores (krum_scores): score_i = the sum of the kk smallest entries of row i of D, D[i][i] = 0
included; D in fp64 from fp64 differences' Gram form.

multi_krum (ref_multi_krum): kk = honest - 1; the m rows of smallest score by stable argsort;
out[j] = the fp64 sum of the selected rows in increasing row index (acc = x[r0]; acc += x[r]),
/ m, rounded once: the kernel adds the same terms in the same order, so the test asks for the
same bits.  `gap`: the relative score gap at the m boundary.

bulyan (ref_bulyan): theta = K - 2f rounds on the remaining set S; kk_t = max(1, |S| - f - 1);
score = the sum of the kk_t smallest D[i][j], j in S, self included; the smallest score (first
minimum) is selected and leaves S.  Stage 2 = ref_meamed(X[sorted(selected)], theta - 2f).
`gap`: the smallest relative gap between the best and the second-best score over the rounds.
"""
import functools

import numpy as np

F32 = np.float32

# meamed: (K, d) — every register regime (K <= 64, 128, 256, 512, 1024) at and around its
# edges, d ragged against the 16-column tile and the float4 groups
MEAMED_CASES = [(3, 70), (17, 333), (64, 1000), (65, 70), (129, 2051), (256, 333), (257, 1000),
                (513, 2051), (600, 70), (1000, 333), (1024, 2051)]
QUANT_CASES = [(64, 70), (257, 333), (1000, 70)]
SPECIAL_CASE = (65, 40)
ROWS_CASES = [(65, 70, 17), (600, 333, 401), (1024, 70, 300)]      # (K, d, n_rows)
# (K, d, f), the spread recipe
MULTI_KRUM_CASES = [(17, 1000, 3), (50, 7850, 10), (256, 2051, 50), (600, 1030, 100),
                    (1000, 520, 100)]
BULYAN_CASES = [(17, 1000, 3), (50, 7850, 10), (256, 2051, 50), (600, 1030, 100)]
MULTI_KRUM_MIN_GAP = 1e-5
BULYAN_MIN_GAP = 1e-6


def keeps(K):
    return sorted({1, K - K // 5, K})


def ms(K, f):
    H = K - f
    return sorted({H, max(1, H // 2), 1}, reverse=True)


@functools.lru_cache(maxsize=None)
def spread(K, d, f):
    """The selection tests' input: honest row i = 0.05 * 4**(i/(H-1)) * z_i, H = K - f, with z
    ONE draw randn(H, d); then f rows 1.0 + 0.5 * randn(f, d) (one draw); then shuffled by
    randperm(K); all from torch.Generator().manual_seed(3000 + K).  (Drawn row by row the
    generator gives other values and other gaps: 1.5e-6 instead of 1.4e-5 for Bulyan at K = 600.)
    The graded scales make the selection well posed (on iid honest rows adjacent Krum scores are
    closer than fp32 distances resolve)."""
    import torch
    g = torch.Generator().manual_seed(3000 + K)
    H = K - f
    scale = torch.tensor([0.05 * 4.0 ** (i / max(H - 1, 1)) for i in range(H)],
                         dtype=torch.float32)
    X = torch.cat([scale[:, None] * torch.randn(H, d, generator=g),       # one draw of [H, d]
                   1.0 + 0.5 * torch.randn(f, d, generator=g)])
    return X[torch.randperm(K, generator=g)].contiguous()


@functools.lru_cache(maxsize=None)
def meamed_input(K, d):
    """Honest rows N(0, 0.05^2), K // 5 rows 0.25 + N(0, 0.5^2), shuffled;
    torch.Generator().manual_seed(2000 + K)."""
    import torch
    g = torch.Generator().manual_seed(2000 + K)
    nb = K // 5
    X = torch.randn(K, d, generator=g) * 0.05
    if nb:
        X[K - nb:] = torch.randn(nb, d, generator=g) * 0.5 + 0.25
    return X[torch.randperm(K, generator=g)].contiguous()


@functools.lru_cache(maxsize=None)
def quantised_input(K, d):
    """meamed_input rounded to multiples of 1/8 scaled so that the honest values fall on a few
    grid points: real ties on both sides of the median."""
    import torch
    return (torch.round(8 * 20 * meamed_input(K, d)) / 8).contiguous()


@functools.lru_cache(maxsize=None)
def special_input():
    """A minority of +-inf rows, a NaN column, -0 entries, a column holding both infinities."""
    import torch
    K, d = SPECIAL_CASE
    X = meamed_input(K, d).clone()
    X[3, 0:20] = float("inf")
    X[7, 10:30] = float("-inf")
    X[11, 5] = float("nan")
    X[20:40, 31] = -0.0
    X[40:60, 31] = 0.0
    X[:, 33] = -0.0
    return X


@functools.lru_cache(maxsize=None)
def tie_matrix():
    """K = 8, d = 40, small integers (|x| <= 8): four distinct rows, each present twice, so
    every D is exact in fp32 and fp64 and duplicate rows tie in every score."""
    rng = np.random.RandomState(8)
    base = rng.randint(-8, 9, size=(4, 40)).astype(F32)
    base[1] = base[0] + rng.randint(-1, 2, size=40)            # two nearby pairs, two far ones
    base = np.clip(base, -8, 8)
    return np.ascontiguousarray(base[[0, 1, 0, 2, 1, 3, 2, 3]])


def ref_meamed(X, keep, with_scale=False):
    """fp32 [d] (and mean|x_kept| per column, fp64) of the fp32 matrix X [n, d]."""
    x = np.asarray(X, dtype=F32) + F32(0.0)
    n = x.shape[0]
    with np.errstate(all="ignore"):
        med = np.sort(x, axis=0)[(n - 1) // 2]
        dev = np.abs(x - med[None, :])
        assert dev.dtype == F32
        kept = np.argsort(dev, axis=0, kind="stable")[:keep]
        vals = np.take_along_axis(x, kept, axis=0).astype(np.float64)
        out = (vals.sum(axis=0) / keep).astype(F32)
        scale = np.abs(vals).sum(axis=0) / keep
    out[np.isnan(x).any(axis=0)] = np.nan
    return (out, scale) if with_scale else out


def threshold_ties(X, keep):
    """Columns in which the keep-th and the (keep + 1)-th smallest deviation are equal."""
    x = np.asarray(X, dtype=F32) + F32(0.0)
    n = x.shape[0]
    if keep >= n:
        return np.zeros(x.shape[1], dtype=bool)
    dev = np.sort(np.abs(x - np.sort(x, axis=0)[(n - 1) // 2][None, :]), axis=0)
    return dev[keep - 1] == dev[keep]


def meamed_mismatch(got, ref, scale):
    """Indices where `got` misses the bar of the module docstring."""
    got = np.asarray(got, dtype=F32)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        tol = 2.0 ** -24 * np.abs(ref.astype(np.float64)) + 2.0 ** -42 * scale + 2.0 ** -149
        bad_fin = fin & ~(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= tol)
    bad_non = ~fin & ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    return np.flatnonzero(bad_fin | bad_non)


def dist64(X):
    """fp64 squared distances of the rows of X, zero diagonal."""
    x = np.asarray(X, dtype=np.float64)
    n = (x * x).sum(axis=1)
    D = np.maximum(n[:, None] + n[None, :] - 2.0 * (x @ x.T), 0.0)
    np.fill_diagonal(D, 0.0)
    return D


def dist64_direct(X):
    """The same from the differences themselves (small inputs)."""
    x = np.asarray(X, dtype=np.float64)
    return ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)


def krum_scores(D, kk):
    return np.sort(D, axis=1)[:, :kk].sum(axis=1)


def ref_multi_krum(X, honest, m, D=None):
    """(out fp32 [d], selected rows increasing, relative score gap at the m boundary, whether
    the boundary is an exact tie)."""
    X = np.asarray(X, dtype=F32)
    K = X.shape[0]
    s = krum_scores(dist64(X) if D is None else D, honest - 1)
    order = np.argsort(s, kind="stable")
    sel = sorted(int(i) for i in order[:m])
    if m < K:
        lo, hi = s[order[m - 1]], s[order[m]]
        gap = (hi - lo) / lo if lo > 0 else (np.inf if hi > lo else 0.0)
        tie = bool(hi == lo)
    else:
        gap, tie = np.inf, False
    acc = X[sel[0]].astype(np.float64)
    for r in sel[1:]:
        acc = acc + X[r].astype(np.float64)
    out = X[sel[0]].copy() if m == 1 else (acc / m).astype(F32)
    return out, sel, float(gap), tie


def ref_bulyan_select(D, f):
    """(selected rows in selection order, smallest relative best / second-best gap over the
    rounds, whether some round's best two scores tie exactly)."""
    K = D.shape[0]
    theta = K - 2 * f
    idx = np.argsort(D, axis=1, kind="stable")
    Ds = np.take_along_axis(D, idx, axis=1)
    alive = np.ones(K, dtype=bool)
    sel, gap, tie = [], np.inf, False
    for t in range(theta):
        nS = K - t
        kk = max(1, nS - f - 1)
        A = alive[idx]
        mask = A & (np.cumsum(A, axis=1) <= kk)
        score = np.where(mask, Ds, 0.0).sum(axis=1)
        score[~alive] = np.inf
        best = int(np.argmin(score))
        if nS > 1:
            second = np.partition(score, 1)[1]
            b = score[best]
            tie = tie or bool(second == b)
            g = (second - b) / b if b > 0 else (np.inf if second > b else 0.0)
            gap = min(gap, g)
        sel.append(best)
        alive[best] = False
    return sel, float(gap), tie


def ref_bulyan(X, honest, D=None):
    """(out fp32 [d], mean|x_kept| per column, selected rows in selection order, gap, tie)."""
    X = np.asarray(X, dtype=F32)
    K = X.shape[0]
    f = K - honest
    assert K >= 4 * f + 3
    sel, gap, tie = ref_bulyan_select(dist64(X) if D is None else D, f)
    theta = K - 2 * f
    out, scale = ref_meamed(X[sorted(sel)], theta - 2 * f, with_scale=True)
    return out, scale, sel, gap, tie


@functools.lru_cache(maxsize=None)
def multi_krum_case(K, d, f, m):
    return ref_multi_krum(spread(K, d, f).numpy(), K - f, m, D=_spread_D(K, d, f))


@functools.lru_cache(maxsize=None)
def bulyan_case(K, d, f):
    return ref_bulyan(spread(K, d, f).numpy(), K - f, D=_spread_D(K, d, f))


@functools.lru_cache(maxsize=None)
def _spread_D(K, d, f):
    return dist64(spread(K, d, f).numpy())


# ---- brute-force restatements of the definitions (tiny sizes; tests/test_robust_cpu.py) ----

def brute_meamed(X, keep):
    X = np.asarray(X, dtype=F32)
    n, d = X.shape
    out = np.empty(d, dtype=F32)
    for j in range(d):
        col = [F32(v) + F32(0.0) for v in X[:, j]]
        if any(np.isnan(v) for v in col):
            out[j] = np.nan
            continue
        med = sorted(col)[(n - 1) // 2]
        with np.errstate(all="ignore"):
            dev = [abs(F32(v - med)) for v in col]
        # a NaN deviation ranks after +inf; ties to the lower row index
        order = sorted(range(n), key=lambda k: (np.isnan(dev[k]), dev[k] if not np.isnan(dev[k])
                                                else 0.0, k))
        with np.errstate(all="ignore"):
            out[j] = F32(sum(float(col[k]) for k in order[:keep]) / keep)
    return out


def brute_scores(D, kk, members):
    """score_i for i in members: the kk smallest D[i][j], j in members, self included."""
    return {i: sum(sorted(D[i][j] for j in members)[:kk]) for i in members}


def brute_multi_krum_select(X, honest, m):
    D = dist64_direct(X)
    K = D.shape[0]
    s = brute_scores(D, honest - 1, list(range(K)))
    return sorted(sorted(range(K), key=lambda i: (s[i], i))[:m])


def brute_bulyan_select(X, honest):
    D = dist64_direct(X)
    K = D.shape[0]
    f = K - honest
    S, sel = list(range(K)), []
    for _ in range(K - 2 * f):
        s = brute_scores(D, max(1, len(S) - f - 1), S)
        best = min(S, key=lambda i: (s[i], i))
        sel.append(best)
        S.remove(best)
    return sel
