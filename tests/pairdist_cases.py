"""Inputs, fp64 references and checks of the distance family on bf16 client updates (Krum,
multi_krum, nnm, pair_distances with ``bf16=True``; csrc/pairdist_bf16.hip), shared by
tests/test_pairdist_cpu.py and tests/test_gpu_pairdist_bf16.py.  Importing it needs no GPU and
nothing of the library.

Two tiers.  "exact" is the fp32 kernels on widened elements: its results are compared bit for bit
with the fp32 call on ``X.float()``.  "mfma" forms D~ = max(0, G_ii + G_jj - 2 G_ij) from
G = X X^T on the bf16 matrix cores and states

    |D~_ij - D_ij| <= beta (rho_i + rho_j),   rho_i = ||x_i||^2,   beta <= 2^-13,

with D and rho in exact arithmetic on the widened values (here: fp64 from the differences, whose
own error, about d 2^-53 relative, is far below any beta).  Everything a consumer decides from
D~ is checked against that band and nothing tighter:

  neighbours (check_neighbors_band)   with e_ij = beta (rho_i + rho_j), e_ii = 0, row i's true
      rank of j lies between #{k != j : D_ik + e_ik < D_ij - e_ij} and #{k != j : D_ik - e_ik <=
      D_ij + e_ij}.  j is surely inside N(i) when the upper count is < m, surely outside when the
      lower count is >= m; every surely-inside j must be listed and no surely-outside j may be.
      A row with an undecided j is ambiguous; at most 5 % of the rows may be (asserted).
  selection (selection_determined)    a Krum score is monotone in every distance, so
      LB_i = score(max(0, D - e)) <= score~_i <= UB_i = score(D + e); the m rows of smallest
      reference score are THE selection when their largest UB is below the smallest LB of the rest.

Inputs.  graded(K, d): x_k = 1.02^k z_k, z = torch.randn(K, d) from a CPU generator seeded 0,
rounded to bf16: norms spread over 1.02^K, so the neighbourhoods are nested and well separated
relative to the band.  (robust_cases.spread rounded to bf16 is used for the exact tier and the
bound; its honest rows are too close to each other for the band rule at K >= 129.)
integers(K, d, B): entries uniform in [-15, 15] as bf16, the last B rows copies of row K - B:
every product, partial sum and distance is an integer below 2^24 for d <= 4120 (d 30^2 <= 3.8e6),
so both tiers are exact in any summation order and must agree bit for bit.
"""
import functools

import numpy as np

import nnm_cases as nc
import robust_cases as rc

C_FLUSH = 256                     # the MFMA tier's flush width in columns
BETA_MAX = 2.0 ** -13             # the condition on the library's beta
BETA_CHECKED = 2.0 ** -12         # the band at which the inputs below are checked on the CPU
MAX_AMBIGUOUS = nc.MAX_AMBIGUOUS

KS = (1, 2, 17, 128, 129, 257, 300)
DS = (1, 7, 8, 264, 333, C_FLUSH, C_FLUSH + 8, 4120)
# one more d, from the launcher's slicing rule (S = ceil(d / C) while the tile pairs times S stay
# within two blocks per CU): more than one slice at K = 300, the last one a tail of 8 columns
D_TWO_SLICES = 2 * C_FLUSH + 8
LAYOUTS = ("rows", "offset", "panels")

# (K, d, layout) of the bound test and (K, d, f) of the neighbour test on graded inputs
BOUND_CASES = [(129, 264, "rows"), (257, 333, "panels"), (300, 4120, "rows")]
NEIGHBOR_CASES = [(129, 264, 26), (257, 333, 50), (300, 4120, 60)]
# (K, d, honestSize, ms)
SELECT_CASES = [(129, 264, 103, (1, 40, 103)), (257, 333, 207, (207,)), (300, 4120, 240, (240,))]
# spread inputs: (K, d, f)
SPREAD_CASES = [(17, 264, 3), (129, 333, 26), (300, 520, 60)]


@functools.lru_cache(maxsize=None)
def graded(K, d):
    """bf16 torch tensor [K, d]; never modified."""
    import torch
    g = torch.Generator().manual_seed(0)
    z = torch.randn(K, d, generator=g)
    s = torch.tensor(1.02, dtype=torch.float64) ** torch.arange(K, dtype=torch.float64)
    return (z.double() * s[:, None]).float().to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def spread_bf16(K, d, f):
    import torch
    return rc.spread(K, d, f).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def integers(K, d, B=0):
    import torch
    g = torch.Generator().manual_seed(77 + K)
    X = torch.randint(-15, 16, (K, d), generator=g).float()
    if B:
        X[K - B:] = X[K - B]
    return X.to(torch.bfloat16)


def widened(X):
    """fp64 numpy of a bf16 (or fp32) torch tensor."""
    return X.float().numpy().astype(np.float64)


def dist_rho(X):
    """(D fp64 [K, K] from the differences, zero diagonal; rho fp64 [K]) of a torch tensor."""
    x = widened(X)
    return nc.ref_dist(x), (x * x).sum(axis=1)


def band(rho, beta):
    e = beta * (rho[:, None] + rho[None, :])
    np.fill_diagonal(e, 0.0)
    return e


def bound_ratio(Dt, D, rho):
    """max over pairs of |D~ - D| / (rho_i + rho_j) (0 where both rows are zero)."""
    den = rho[:, None] + rho[None, :]
    with np.errstate(all="ignore"):
        r = np.where(den > 0, np.abs(Dt - D) / den, np.where(Dt == D, 0.0, np.inf))
    return float(r.max())


def neighbor_sets(D, e, m):
    """(surely inside, surely outside) boolean [K, K] under the band e."""
    K = D.shape[0]
    lo, hi = D - e, D + e
    inside = np.zeros((K, K), dtype=bool)
    outside = np.zeros((K, K), dtype=bool)
    for i in range(K):
        slo, shi = np.sort(lo[i]), np.sort(hi[i])
        # others that may precede j: lo_ik <= hi_ij (j itself always counts once: lo <= hi)
        may = np.searchsorted(slo, hi[i], side="right") - 1
        # others that surely precede j: hi_ik < lo_ij (never j itself)
        surely = np.searchsorted(shi, lo[i], side="left")
        inside[i] = may < m
        outside[i] = surely >= m
    return inside, outside


def ambiguous_rows(D, rho, f, beta):
    K = D.shape[0]
    inside, outside = neighbor_sets(D, band(rho, beta), K - f)
    return int((~(inside | outside)).any(axis=1).sum())


def check_neighbors_band(N_got, D, rho, f, beta):
    """Asserts the module docstring's conditions on the kernel's lists under the band
    beta (rho_i + rho_j); returns the number of ambiguous rows (asserted <= 5 %)."""
    K = D.shape[0]
    m = K - f
    N_got = np.asarray(N_got, dtype=np.int64)
    assert N_got.shape == (K, m), (N_got.shape, (K, m))
    assert N_got.min() >= 0 and N_got.max() < K
    assert (np.diff(N_got, axis=1) > 0).all(), "rows of N must be strictly increasing"
    assert (N_got == np.arange(K)[:, None]).any(axis=1).all(), "row i must be in N(i)"
    member = np.zeros((K, K), dtype=bool)
    np.put_along_axis(member, N_got, True, axis=1)
    inside, outside = neighbor_sets(D, band(rho, beta), m)
    bad = (inside & ~member) | (outside & member)
    assert not bad.any(), f"rows {np.flatnonzero(bad.any(axis=1))[:8]} miss the distance band"
    amb = int((~(inside | outside)).any(axis=1).sum())
    assert amb <= MAX_AMBIGUOUS * K, f"{amb} ambiguous rows of {K}"
    return amb


def score_bounds(D, e, kk):
    lb = rc.krum_scores(np.maximum(D - e, 0.0), kk)
    ub = rc.krum_scores(D + e, kk)
    return lb, ub


def selection_determined(D, rho, honest, m, beta):
    """(the m rows of smallest reference score, increasing; whether no other selection is
    possible under the band)."""
    K = D.shape[0]
    s = rc.krum_scores(D, honest - 1)
    order = np.lexsort((np.arange(K), s))
    sel, rest = order[:m], order[m:]
    lb, ub = score_bounds(D, band(rho, beta), honest - 1)
    ok = rest.size == 0 or ub[sel].max() < lb[rest].min()
    return np.sort(sel), bool(ok)


def eligible(X, layout):
    """Whether the MFMA tier takes a torch operand handed over as `layout`: panels always, rows
    when 16-byte aligned with a row stride that is a multiple of 8."""
    if layout == "panels":
        return True
    return X.data_ptr() % 16 == 0 and X.stride(0) % 8 == 0
