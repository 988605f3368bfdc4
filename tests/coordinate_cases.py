"""Case builders and CPU references for the coordinate-wise aggregators and Krum
(byzantine_aircomp_amd/csrc/coordinate.hip), shared by tests/test_gpu_coordinate_paths.py and
by the child processes it starts: run as a script, this file checks a compact matrix of the
same cases under whatever GMAGG_SELECT_* settings its environment carries (they are read once
per process, so each setting needs a process of its own).  Importing it needs no GPU.

References (numpy / Python floats, nothing from the library under test):
  median        NaN if the column holds one, else sorted[(K-1)//2]; compared with ==
                (-0 equals +0) plus an equal NaN mask.
  trimmed mean  sort with NaN last (torch's topk order, which the kernel documents), keep
                s[b:K-b]; NaN if the kept values hold a NaN or both infinities, +-inf if
                they hold one infinity sign, else math.fsum(kept) / (K - 2b) rounded to fp32.
  mean          the trimmed mean with b = 0.
  Krum          fp64 distances in the Gram form, score = the sum of the honestSize - 1
                smallest per row, first argmin.

Tolerance of the mean and the trimmed mean: per element, within 1 ulp of the fp32-rounded
reference (np.nextafter either way), the NaN / inf pattern identical.  The kernels sum at
most K fp64 terms, a relative error <= K 2^-53 kappa with kappa = sum|x| / |sum x| over the
kept values; for kappa <= 1e4 and K <= 8192 that is below 1e-8, far under half an fp32 ulp
(6e-8), so only the final rounding can differ.  kappa <= 1e4 is a precondition on the inputs
(assert_kappa); the builders shift a column that would break it by a constant.
"""
import functools
import math
import os
import sys

import numpy as np

KAPPA_MAX = 1e4
F32 = np.float32


# ---------------------------------------------------------------------------- references

def ref_median(X):
    K = X.shape[0]
    out = np.sort(X, axis=0)[(K - 1) // 2].astype(F32)
    out[np.isnan(X).any(axis=0)] = np.nan
    return out


def ref_trimmed_mean(X, b):
    K, d = X.shape
    S = np.sort(X, axis=0)[b:K - b]                    # NaN sorts last
    n = K - 2 * b
    nan = np.isnan(S).any(axis=0)
    pinf = (S == np.inf).any(axis=0)
    ninf = (S == -np.inf).any(axis=0)
    cols = S.astype(np.float64).T.tolist()
    out = np.empty(d, dtype=F32)
    for j in range(d):
        if nan[j] or (pinf[j] and ninf[j]):
            out[j] = np.nan
        elif pinf[j]:
            out[j] = np.inf
        elif ninf[j]:
            out[j] = -np.inf
        else:
            out[j] = F32(math.fsum(cols[j]) / n)
    return out


def ref_mean(X):
    return ref_trimmed_mean(X, 0)


def default_trim(K):
    return int(K * 0.1)                                # the reference's int(0.1 K)


def kappa(X, b):
    """sum|x| / |sum x| over the kept values of every column; NaN where they are not all
    finite (those columns' results are decided by the NaN / inf rules, not by a sum)."""
    K = X.shape[0]
    S = np.sort(X, axis=0)[b:K - b].astype(np.float64)
    fin = np.isfinite(S).all(axis=0)
    with np.errstate(all="ignore"):
        a = np.abs(S).sum(axis=0)
        s = np.abs(S.sum(axis=0))
        k = np.where(s > 0, a / np.where(s > 0, s, 1.0), np.where(a == 0, 1.0, np.inf))
    return np.where(fin, k, np.nan)


def assert_kappa(X, trims):
    for b in trims:
        k = np.nan_to_num(kappa(X, b), nan=0.0)
        assert k.max() <= KAPPA_MAX, (b, int(k.argmax()), float(k.max()))


def condition(X, trims):
    """Shift (never drop) the columns whose kappa at one of `trims` is near the bound.  A
    constant added in fp32 keeps equal values equal, so ties survive."""
    for _ in range(64):
        bad = np.zeros(X.shape[1], dtype=bool)
        for b in trims:
            bad |= np.nan_to_num(kappa(X, b), nan=0.0) > KAPPA_MAX / 4
        if not bad.any():
            return X
        with np.errstate(invalid="ignore"):
            scale = np.nanmedian(np.where(np.isfinite(X[:, bad]), np.abs(X[:, bad]), np.nan),
                                 axis=0)
        X[:, bad] += (0.5 * (1.0 + scale)).astype(F32)
    raise AssertionError("a column could not be conditioned")


# ---------------------------------------------------------------------------- comparisons

def mismatch_ulp(got, ref, what):
    """None, or a description of the first element of `got` that is not within 1 fp32 ulp
    of `ref` (NaN where ref is NaN, the same infinity where ref is infinite)."""
    got, ref = np.asarray(got, dtype=F32), np.asarray(ref, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = np.nextafter(ref, F32(-np.inf))
        hi = np.nextafter(ref, F32(np.inf))
        near = (got >= lo) & (got <= hi) & np.isfinite(got)
        ok = np.where(np.isnan(ref), np.isnan(got), np.where(np.isinf(ref), got == ref, near))
    if ok.all():
        return None
    j = int(np.flatnonzero(~ok)[0])
    return f"{what}: column {j}: got {got[j]!r}, want {ref[j]!r} +- 1 ulp ({int((~ok).sum())} wrong)"


def mismatch_exact(got, ref, what):
    got, ref = np.asarray(got, dtype=F32), np.asarray(ref, dtype=F32)
    with np.errstate(invalid="ignore"):
        ok = (got == ref) | (np.isnan(got) & np.isnan(ref))
    if ok.all():
        return None
    j = int(np.flatnonzero(~ok)[0])
    return f"{what}: column {j}: got {got[j]!r}, want {ref[j]!r} ({int((~ok).sum())} wrong)"


# ---------------------------------------------------------------------------- case builders

def _normal(rng, K, d):
    """N(0,1), every fifth column rounded to quarters (ties), every column its own draw,
    + 0.001 j per column so that a permuted or duplicated tile cannot go unnoticed."""
    X = rng.standard_normal((K, d), dtype=F32)
    X[:, ::5] = np.round(4 * X[:, ::5]) / 4
    X += (0.001 * np.arange(d)).astype(F32)
    return X


def full_tile_d(K):
    """33 column tiles of the kernel that owns K: 16 columns per tile to K = 1024 (two
    permuted groups of 16 tiles + a ragged last one), 8 above."""
    return 517 if K <= 1024 else 261


@functools.lru_cache(maxsize=None)
def normal_case(K, d, trims=None):
    """(X, refs) of the plain case; refs: median, trimmed (default trim), mean, and
    ("trim", b) for every b in `trims`."""
    rng = np.random.default_rng(1000 * K + d)
    tr = (0, default_trim(K)) + tuple(trims or ())
    X = condition(_normal(rng, K, d), tr)
    X.setflags(write=False)
    return X, _refs(X, tr)


ADVERSARIAL_D = 40


@functools.lru_cache(maxsize=None)
def adversarial_case(K):
    """The columns where a selection kernel goes wrong, padded with plain ones to 40."""
    assert K >= 60
    rng = np.random.default_rng(77 * K + 1)
    d, b = ADVERSARIAL_D, default_trim(K)
    X = _normal(rng, K, d)
    N = lambda: rng.standard_normal(K, dtype=F32)      # noqa: E731
    half = K // 2 + 5
    X[:5, 0] = 1e30                                    # five huge outliers
    X[:, 1] = 0.03 + 1e-3 * N()                        # a cluster
    X[:, 2] = 1.0 + np.arange(K, dtype=F32) * F32(1e-7)   # > 128 keys share 16 leading bits
    X[:, 3] = F32(1e-40) * rng.integers(0, 3, K).astype(F32)   # subnormals
    X[:, 4] = 2.5                                      # all equal
    X[:, 5] = 0.0
    X[::2, 5] = -0.0                                   # +-0 alternating
    X[:, 6] = np.round(2 * N())                        # heavy ties
    X[:, 7] = -np.abs(N()) - F32(0.01)                 # all negative
    X[:, 8] = N()
    X[K // 2:, 8] *= 1e4                               # half the rows scaled
    X[0, 9] = np.inf
    X[1, 10] = -np.inf
    X[:half, 11] = np.inf                              # +inf in more than half the rows
    X[:half, 12] = 3e38                                # ... a huge finite value
    X[K // 2, 13] = np.nan                             # one NaN (trimmed away)
    X[:K // 3, 14] = np.nan                            # NaN reaches the kept middle
    X[:b + 2, 15] = np.inf                             # both infinities inside the kept middle
    X[b + 2:2 * b + 4, 15] = -np.inf
    X[:, 16] = np.clip(N(), -2.5, 2.5)                 # b+1 copies of the smallest and of the
    X[:b + 1, 16] = -3.0                               # largest value: one of each is kept,
    X[b + 1:2 * b + 2, 16] = 3.0                       # counted from the boundary ties
    X[:, 17] = np.clip(N(), -2.5, 2.5)                 # exactly b copies: none is kept
    X[:b, 17] = -3.0
    X[b:2 * b, 17] = 3.0
    X[:, 18] = 1.0 + np.arange(K, dtype=F32) * F32(1e-7)  # column 2 with its ends tied too
    X[:b + 3, 18] = 1.0
    X[K - b - 3:, 18] = X[K - 1, 18]
    X = X[rng.permutation(K)]                          # the special rows anywhere in the wave
    tr = (0, b)
    X = condition(np.ascontiguousarray(X), tr)
    X.setflags(write=False)
    return X, _refs(X, tr)


def _refs(X, trims):
    refs = {"median": ref_median(X)}
    for b in set(trims):
        refs[("trim", b)] = ref_trimmed_mean(X, b)
    refs["mean"] = refs[("trim", 0)]
    refs["trimmed"] = refs[("trim", default_trim(X.shape[0]))]
    return refs


def layouts(torch, X):
    """X on the GPU as the two layouts the launchers tell apart: "vec4", a view of a
    16-byte-aligned buffer whose row stride is a multiple of 4 (the float4 loads), and
    "scalar", a view one element into its buffer (base pointer off by 4 bytes).  The
    buffers' other columns are NaN: a read past column d shows in the result."""
    K, d = X.shape
    Xt = torch.from_numpy(np.array(X))
    pad = (-d) % 4 or 4
    a = torch.full((K, d + pad), float("nan"), dtype=torch.float32, device="cuda")
    a[:, :d] = Xt.cuda()
    b = torch.full((K, d + 4), float("nan"), dtype=torch.float32, device="cuda")
    b[:, 1:1 + d] = Xt.cuda()
    va, vb = a[:, :d], b[:, 1:1 + d]
    assert va.stride(0) % 4 == 0 and va.data_ptr() % 16 == 0 and vb.data_ptr() % 16 == 4
    return [("vec4", va), ("scalar", vb)]


def check_select(bz, torch, X, refs, what, funcs=("median", "trimmed", "mean")):
    """The first mismatch of the aggregators in `funcs` on both layouts of X, or None."""
    for lname, V in layouts(torch, X):
        for f in funcs:
            if f == "median":
                bad = mismatch_exact(bz.median(V).cpu().numpy(), refs["median"],
                                     f"{what} {lname} median")
            elif f == "trimmed":
                bad = mismatch_ulp(bz.trimmed_mean(V).cpu().numpy(), refs["trimmed"],
                                   f"{what} {lname} trimmed_mean")
            else:
                bad = mismatch_ulp(bz.mean(V).cpu().numpy(), refs["mean"], f"{what} {lname} mean")
            if bad:
                return bad
    return None


# ---------------------------------------------------------------------------- Krum

KRUM_MIN_GAP = 1e-3
KRUM_SHAPES = [(1100, 40, 880), (2049, 24, 1640), (4096, 8, 3277), (1100, 40, 1101)]


def krum_case(K, d, honest):
    """0.05 N(0,1) rows, the last max(K - honest, K/5) shifted by 0.5 N(0,1), rows permuted
    (a torch CPU tensor)."""
    import torch
    g = torch.Generator().manual_seed(K + d + honest)
    X = 0.05 * torch.randn(K, d, generator=g)
    nb = max(K - honest, K // 5)
    X[K - nb:] += 0.5 * torch.randn(nb, d, generator=g)
    return X[torch.randperm(K, generator=g)].contiguous()


def ref_krum_scores(X, honest):
    """fp64 Krum scores of a torch / numpy [K, d] matrix."""
    A = np.asarray(X, dtype=np.float64)
    n = (A * A).sum(axis=1)
    D = n[:, None] + n[None, :] - 2.0 * (A @ A.T)
    np.maximum(D, 0.0, out=D)
    np.fill_diagonal(D, 0.0)
    kk = honest - 1
    K = A.shape[0]
    if kk >= K:
        return D.sum(axis=1)
    return np.partition(D, kk - 1, axis=1)[:, :kk].sum(axis=1)


def ref_krum(X, honest, tied=None):
    """(index, relative gap): the first argmin of the fp64 scores and the gap between the
    best score and the best of the other rows.  `tied`: rows that are copies of one another
    and expected to share the best score (they tie to ~1e-16 in fp64 and exactly in the
    kernel, whose first index wins); the gap is then to the best row outside them."""
    s = ref_krum_scores(X, honest)
    best = int(np.argmin(s))
    group = np.flatnonzero(s <= s[best] * (1 + 1e-9))
    if tied is None:
        assert list(group) == [best], group
    else:
        assert sorted(group) == sorted(tied), (group, tied)
    rest = np.delete(s, group)
    gap = float((rest.min() - s[best]) / s[best])
    return int(group.min()), gap


# ---------------------------------------------------------------------------- child process

CHILD_KS = (200, 256, 400, 513, 1000, 2048)
WIDE = (513, 12309)    # 770 tiles of 16 columns: three per CU where two blocks fit, so
#                        blocks of the persistent form walk more than one tile


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import byzantine_aircomp_amd as bz
    knobs = {k: v for k, v in os.environ.items() if k.startswith("GMAGG_SELECT_")}
    cases = []
    for K in CHILD_KS:
        cases.append((f"full tiles K={K}",) + normal_case(K, full_tile_d(K)))
        cases.append((f"adversarial K={K}",) + adversarial_case(K))
    if "--wide" in argv:
        cases.append((f"wide K={WIDE[0]} d={WIDE[1]}",) + normal_case(*WIDE))
    for what, X, refs in cases:
        assert_kappa(X, (default_trim(X.shape[0]),))
        bad = check_select(bz, torch, X, refs, what, funcs=("median", "trimmed"))
        if bad:
            print(f"MISMATCH under {knobs}: {bad}", flush=True)
            return 1
    torch.cuda.synchronize()
    print(f"ok: {len(cases)} cases under {knobs}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
