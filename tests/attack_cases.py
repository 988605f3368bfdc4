"""Cases and numpy fp64 references of the omniscient attacks (byzantine_aircomp_amd.attacks,
csrc/attack.hip), shared by tests/test_attacks_cpu.py and tests/test_gpu_attacks.py.
Importing it needs no GPU.

Definitions (include/gmagg.h).  H = K - B >= 2 honest rows 0 .. H-1, Byzantine rows H .. K-1;
bf16 inputs widened exactly.  Per column j in fp64
    mu_j    = (sum_{k<H} x_kj) / H, summed in increasing k
    sigma_j = sqrt(sum_{k<H} (x_kj - mu_j)^2 / (H - 1))
affine:    y = a mu + b sigma (b == 0: no sigma term), rounded once to the storage type
min-max:   m = mu - gamma p,  gamma = min_i (b_i + sqrt(b_i^2 + c (D* - a_i))) / c
min-sum:   m = mu - gamma p,  gamma = sqrt((S* - sum_i a_i) / (H c))
with a_i = ||mu - x_i||^2, b_i = p . (mu - x_i), c = ||p||^2, D* = max_ij ||x_i - x_j||^2,
S* = max_i sum_j ||x_i - x_j||^2 over the honest rows, p = sigma / mu/||mu|| / sign(mu).

Tolerances (derived, not measured):
  fp32   |got - fp32(ref)| <= spacing(fp32(ref)) + 2^-40 (|a mu_j| + |b sigma_j|): fp64 sums
         of <= 2^12 terms err by <= 2^-41 relative on each of mu and sigma, one fp32 rounding
         on each side adds at most one spacing.
  bf16   |got - ref| <= half a bf16 spacing of ref + the same 2^-40 term, got a bf16 value.
  gamma  relative 1e-5: the exact Krum path's distances sum 32-column stages in fp32
         (<= 64 * 2^-24 ~ 4e-6 relative on a sum of squares), which reaches gamma amplified by
         at most D* / (D* - max a_i) resp. S* / (S* - sum a_i) (asserted <= 2 on the reference)
         and halved by the square root.
"""
import functools
from statistics import NormalDist

import numpy as np

from bucket_cases import normal_matrix

F32 = np.float32
F64 = np.float64

# (K, B, d): every panel width, ragged tails against 4 and the panel widths, one row group and
# many, B = 1, K = 3000 beyond the panel layout (row-major only)
CASES = [(7, 2, 37), (50, 10, 70), (17, 4, 1000), (513, 100, 333), (1000, 200, 2051),
         (1024, 1, 4096), (3000, 600, 64)]
NO_PANELS = {3000}
MINMAX_CASES = [c for c in CASES if c[0] <= 1024] + [(3000, 600, 64)]
DEVS = ("std", "unit", "sign")
GAMMA_RTOL = 1e-5
EPS40 = 2.0 ** -40


def ref_z_max(K, B):
    s = K // 2 + 1 - B
    return NormalDist().inv_cdf((K - B - s) / (K - B))


def ref_stats(X, B):
    """(mu, sigma) fp64 of the honest rows of X (any float dtype, widened to fp64)."""
    X = np.asarray(X)
    H = X.shape[0] - B
    with np.errstate(all="ignore"):
        acc = np.zeros(X.shape[1], dtype=F64)
        for k in range(H):
            acc = acc + X[k].astype(F64)
        mu = acc / H
        sq = np.zeros(X.shape[1], dtype=F64)
        for k in range(H):
            t = X[k].astype(F64) - mu
            sq = sq + t * t
        sigma = np.sqrt(sq / (H - 1))
    return mu, sigma


def ref_affine(X, B, a, b):
    """(y fp64, the 2^-40 tolerance term) of the affine attack."""
    mu, sigma = ref_stats(X, B)
    with np.errstate(all="ignore"):
        y = a * mu
        slack = np.abs(a * mu)
        if b != 0:
            y = y + b * sigma
            slack = slack + np.abs(b * sigma)
    return y, EPS40 * slack


def deviation(mu, sigma, dev):
    if dev == "std":
        return sigma
    if dev == "unit":
        n = np.sqrt(np.sum(mu * mu))
        return mu / n if n > 0 else np.zeros_like(mu)
    if dev == "sign":
        return np.sign(mu)
    raise ValueError(dev)


@functools.lru_cache(maxsize=None)
def honest_geometry(K, B, d):
    """What the closed forms need of normal_matrix(K, d)'s honest rows, in fp64: mu, sigma, the
    centred rows, a_i, D* and S*."""
    X = normal_matrix(K, d)
    H = K - B
    mu, sigma = ref_stats(X, B)
    Xc = X[:H].astype(F64) - mu
    a = np.sum(Xc * Xc, axis=1)
    G = Xc @ Xc.T
    D = np.maximum(a[:, None] + a[None, :] - 2.0 * G, 0.0)
    np.fill_diagonal(D, 0.0)
    return {"mu": mu, "sigma": sigma, "Xc": Xc, "a": a, "Dstar": float(D.max()),
            "Sstar": float(D.sum(axis=1).max())}


def bound_of(geo, rule):
    return geo["Dstar"] if rule == "max" else geo["Sstar"]


def amplification(geo, rule):
    """The factor by which a relative error of the distances reaches the radicand of gamma."""
    if rule == "max":
        return geo["Dstar"] / (geo["Dstar"] - float(geo["a"].max()))
    return geo["Sstar"] / (geo["Sstar"] - float(geo["a"].sum()))


def ref_gamma(geo, rule, dev):
    """(gamma, p) of the closed forms."""
    p = deviation(geo["mu"], geo["sigma"], dev)
    a, H = geo["a"], len(geo["a"])
    b = -(geo["Xc"] @ p)                      # p . (mu - x_i)
    c = float(p @ p)
    if c == 0:
        return 0.0, p
    if rule == "max":
        g = np.min((b + np.sqrt(b * b + c * (geo["Dstar"] - a))) / c)
    else:
        g = np.sqrt((geo["Sstar"] - a.sum()) / (H * c))
    return float(g), p


def constraint_value(geo, rule, m):
    """The constraint's left side for the malicious row m (fp64): max_i or sum_i ||m - x_i||^2."""
    t = (np.asarray(m, dtype=F64) - geo["mu"])[None, :] - geo["Xc"]
    r = np.sum(t * t, axis=1)
    return float(r.max() if rule == "max" else r.sum())


def bisect_gamma(geo, rule, dev, steps=200):
    """The largest gamma meeting the constraint, by bisection (the closed forms' check)."""
    p = deviation(geo["mu"], geo["sigma"], dev)
    bound = bound_of(geo, rule)
    ok = lambda g: constraint_value(geo, rule, geo["mu"] - g * p) <= bound     # noqa: E731
    lo, hi = 0.0, 1.0
    while ok(hi):
        hi *= 2.0
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


# ---------------------------------------------------------------------------------- tolerances

def mismatch_f32(got, ref, slack):
    """Elements of the fp32 vector `got` outside |got - fp32(ref)| <= spacing(fp32(ref)) + slack
    (NaN and infinities must match exactly)."""
    got = np.asarray(got, dtype=F32)
    with np.errstate(all="ignore"):
        r32 = ref.astype(F32)
        fin = np.isfinite(r32)
        bad = np.where(fin, np.abs(got.astype(F64) - r32.astype(F64)) >
                       np.spacing(np.abs(r32)).astype(F64) + slack, False)
        bad |= ~fin & ~((np.isnan(r32) & np.isnan(got)) | (got == r32))
    return int(bad.sum())


def bf16_spacing(ref):
    """The spacing of bf16 (8 significant bits) at |ref| (normal range)."""
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    return np.where(np.isfinite(e), 2.0 ** (e - 7), 0.0)


def mismatch_bf16(got, ref, slack):
    """Elements of `got` (bf16 values widened to fp32) outside |got - ref| <= half a bf16 spacing
    + slack, or that are no bf16 values."""
    got = np.asarray(got, dtype=F32)
    assert not np.any(got.view(np.uint32) & 0xFFFF), "not bf16 values"
    with np.errstate(all="ignore"):
        fin = np.isfinite(ref)
        bad = np.where(fin, np.abs(got.astype(F64) - ref) > 0.5 * bf16_spacing(ref) + slack, False)
        bad |= ~fin & ~((np.isnan(ref) & np.isnan(got)) | (got.astype(F64) == ref))
    return int(bad.sum())
