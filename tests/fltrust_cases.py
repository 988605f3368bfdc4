"""Inputs, references and bars of the FLTrust tests (test_fltrust_cpu.py, test_gpu_fltrust.py).
Importable without a GPU and without the library.

The recipe (K, d), drawn from torch.Generator().manual_seed(4000 + K):
  c = 0.07 N(0, 1), a true direction t = 0.01 N, the server update g = t + 0.005 N, honest
  updates u_k = t + 0.02 N; the last K // 5 rows cycle through the kinds KINDS (sign-flipped
  -3 u, scaled 100 u, zero: x_k = c exactly, slightly negative cosine: projected off g, then
  - 1e-3 ||v|| / ||g|| g (1e-2 in bf16 cases with d < 4096: negcos_margin), one NaN entry, one
  +inf entry); the rows are then permuted and X = c + U in fp32.  bf16 cases round X with
  .to(torch.bfloat16) and every reference is computed on the widened values; their c is
  rounded to bf16-representable values first, so that the zero rows keep x_k = c exactly
  (otherwise the kind would turn into rows of pure rounding noise, whose cosine is as likely
  as not within 1e-4 of the threshold).  With the server as a row, the first honest row is
  replaced by c + g before the permutation; without a centre c = 0 and the rows are the
  updates.

The reference is the definition of include/gmagg.h in np.longdouble, at every shape (case()).

Bars, with eps_d = max(2^-36, d 2^-50):
  out    |got - ref32| <= 2^-24 |ref| + eps_d scale_j + 2^-149,
         scale_j = sum over the counted rows of sqrt(n_g / n_k) |u_kj| / T
  cos    |got - ref| <= d 2^-52, the fp64 accumulation bound for another summation order
  n_k    relative d 2^-52;  TS as cos;  n_g as n_k;  T within K d 2^-52 (K terms, each within
         the cos bar)
  non-finite reference entries must match as NaN / the same infinity.
The builder asserts that every finite |cos| >= 1e-4, so the set {k : TS_k > 0} is determined and
the tests compare it exactly."""
import functools
import math

import numpy as np
import torch

KINDS = ("flip", "scaled", "zero", "negcos", "nan", "inf")
SHAPES = [(1, 70), (3, 70), (17, 2051), (50, 7850), (64, 1000), (65, 333), (257, 1000),
          (600, 8200), (1000, 2051), (1024, 4096), (2048, 520)]
LARGE = (5, 4_300_009)
MIN_COS = 1e-4


def negcos_margin(dtype, d=0):
    """The cosine of the slightly-negative kind is minus this.  fp32: 1e-3.  bf16: 1e-2, because
    rounding x = c + u to bf16 moves each element by up to 2^-9 |x|, about 2e-4 rms at |x| ~ 0.1,
    whose component along g / ||g|| is of that size too, while ||u|| is only 0.022 sqrt(d): the
    cosine moves by about 2e-4 / (0.022 sqrt(d)), 5e-4 at d = 333.  A cosine of -1e-3 then
    lands within 1e-4 of zero, or across it, in some of the 68 such rows of the 2048 x 520
    case, and the trusted set is no longer determined; -1e-2 is 20 of those deviations away.
    From d = 4096 on the deviation is at most 1.4e-4, 1e-3 is more than six of them from the
    1e-4 condition, and the bf16 cases keep the fp32 margin (50 x 7850, 600 x 8200, 1024 x 4096)."""
    return 1e-2 if dtype == "bf16" and d < 4096 else 1e-3


def eps_d(d):
    return max(2.0 ** -36, d * 2.0 ** -50)


def inputs(K, d, dtype="fp32", server="vector", centre=True):
    """(X [K, d] fp32 or bf16 tensor, s [d] fp32 tensor or None, server_row or None, c [d] fp32
    tensor or None, kinds: list of K strings, "honest" / "server" / one of KINDS)."""
    gen = torch.Generator().manual_seed(4000 + K)
    N = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    c = 0.07 * N(d)
    t = 0.01 * N(d)
    g = t + 0.005 * N(d)
    U = t + 0.02 * N(K, d)
    kinds = ["honest"] * K
    nb = K // 5
    where = torch.randint(0, d, (max(nb, 1),), generator=gen)
    for i in range(nb):
        k = K - nb + i
        kind = KINDS[i % len(KINDS)]
        kinds[k] = kind
        if kind == "flip":
            U[k] = -3.0 * U[k]
        elif kind == "scaled":
            U[k] = 100.0 * U[k]
        elif kind == "zero":
            U[k] = 0.0
        elif kind == "negcos":
            v = U[k] - (U[k] @ g) / (g @ g) * g
            U[k] = v - negcos_margin(dtype, d) * v.norm() / g.norm() * g
        elif kind == "nan":
            U[k, where[i]] = float("nan")
        else:
            U[k, where[i]] = float("inf")
    if server == "row":
        U[0] = g
        kinds[0] = "server"
    perm = torch.randperm(K, generator=gen)
    U = U[perm]
    kinds = [kinds[int(p)] for p in perm]
    if not centre:
        c = torch.zeros(d, dtype=torch.float64)
    c32 = c.to(torch.float32)
    if dtype == "bf16":
        c32 = c32.to(torch.bfloat16).to(torch.float32)   # the zero rows stay x_k = c exactly
    X = (c32.to(torch.float64) + U).to(torch.float32)
    for k, kind in enumerate(kinds):
        if kind == "zero":
            X[k] = c32                                # exactly
    if dtype == "bf16":
        X = X.to(torch.bfloat16)
    s = (c32.to(torch.float64) + g).to(torch.float32) if server == "vector" else None
    row = kinds.index("server") if server == "row" else None
    return X, s, row, (c32 if centre else None), kinds


def reference(X, s, row, c, real=np.longdouble):
    """The definition on numpy arrays (X fp32 [K, d], the widened values): a dict with cos, n,
    ts (real [K]), ng, T, out (real [d]), out32, scale [d], trusted (the k with TS_k > 0)."""
    K, d = X.shape
    Xr = X.astype(real)
    cr = np.zeros(d, dtype=real) if c is None else c.astype(real)
    sr = Xr[row] if s is None else s.astype(real)
    with np.errstate(all="ignore"):
        U = Xr - cr
        g = sr - cr
        a = (U * g).sum(axis=1)
        n = (U * U).sum(axis=1)
        ng = (g * g).sum()
        cos = a / np.sqrt(n * ng)
        counted = (np.isfinite(ng) & (ng > 0) & np.isfinite(n) & (n > 0) & np.isfinite(a)
                   & (np.arange(K) != (-1 if row is None else row)))
        ts = np.where(counted & (cos > 0), cos, real(0))
    T = real(0)
    for k in range(K):
        T = T + ts[k]
    trusted = [k for k in range(K) if ts[k] > 0]
    out = cr.copy()
    scale = np.zeros(d, dtype=real)
    if T > 0:
        acc = np.zeros(d, dtype=real)
        for k in trusted:
            acc = acc + (ts[k] * np.sqrt(ng / n[k]) / T) * U[k]
        out = cr + acc
        for k in np.nonzero(counted)[0]:
            scale = scale + np.sqrt(ng / n[k]) * np.abs(U[k]) / T
    return {"cos": cos, "n": n, "ts": ts, "ng": ng, "T": T, "out": out,
            "out32": out.astype(np.float32), "scale": scale, "trusted": trusted,
            "counted": counted}


def check_well_posed(ref):
    """The recipe's condition: no finite cosine within MIN_COS of the threshold."""
    cos = np.asarray(ref["cos"], dtype=np.float64)
    fin = np.isfinite(cos)
    assert (np.abs(cos[fin]) >= MIN_COS).all(), float(np.abs(cos[fin]).min())


@functools.lru_cache(maxsize=None)
def case(K, d, dtype="fp32", server="vector", centre=True):
    """(inputs, reference) of one recipe case, built once and shared; the tensors are not to be
    modified.  np.longdouble at every shape, the large-d one included: a plain fp64 reference
    is within 4e-17 of it there, but that is enough to put element 4,062,002 of the 5 x
    4,300,009 fp32 case exactly on an fp32 rounding midpoint, and the fp64 reference then rounds
    it the other way (one fp32 ulp, 1.68 of the bar, with the kernel on longdouble's side)."""
    inp = inputs(K, d, dtype, server, centre)
    X, s, row, c, _ = inp
    ref = reference(X.to(torch.float32).numpy(), None if s is None else s.numpy(), row,
                    None if c is None else c.numpy())
    check_well_posed(ref)
    return inp, ref


def out_bar(ref, d):
    return (2.0 ** -24 * np.abs(ref["out"]) + eps_d(d) * ref["scale"]
            + 2.0 ** -149).astype(np.float64)


def _match_nonfinite(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), what
    return ~(nan | inf)


def worst_out(got, ref, d):
    """max over j of |got - ref32| / bar (<= 1 passes)."""
    err = np.abs(got.astype(np.float64) - ref["out32"].astype(np.float64))
    return float((err / out_bar(ref, d)).max()) if d else 0.0


def check_out(got, ref, d, what=""):
    w = worst_out(np.asarray(got), ref, d)
    print(f"fltrust out {what}: worst error / bar = {w:.3e}")
    assert np.isfinite(np.asarray(got)).all() and w <= 1.0, (what, w)


def check_stats(stats, ref, K, d, what=""):
    """stats: the 3K + 2 doubles of the call."""
    stats = np.asarray(stats, dtype=np.float64)
    cos, n, ts = stats[:K], stats[K:2 * K], stats[2 * K:3 * K]
    tol = d * 2.0 ** -52
    fin = _match_nonfinite(cos, ref["cos"], f"{what} cos")
    e_cos = np.abs(cos[fin] - np.asarray(ref["cos"], dtype=np.float64)[fin]).max(initial=0.0)
    fin = _match_nonfinite(n, ref["n"], f"{what} n")
    rn = np.asarray(ref["n"], dtype=np.float64)[fin]
    e_n = (np.abs(n[fin] - rn) / np.where(rn > 0, rn, 1.0)).max(initial=0.0)
    e_ts = np.abs(ts - np.asarray(ref["ts"], dtype=np.float64)).max(initial=0.0)
    ng, T = float(ref["ng"]), float(ref["T"])
    e_ng = abs(stats[3 * K] - ng) / ng if math.isfinite(ng) and ng > 0 else 0.0
    e_T = abs(stats[3 * K + 1] - T)
    print(f"fltrust stats {what}: cos {e_cos:.2e} n {e_n:.2e} ts {e_ts:.2e} ng {e_ng:.2e} "
          f"T {e_T:.2e} (bar {tol:.2e})")
    assert e_cos <= tol and e_n <= tol and e_ts <= tol and e_ng <= tol and e_T <= K * tol, what
    assert [k for k in range(K) if ts[k] > 0] == ref["trusted"], what


# ---- restatements for the bar's discrimination (test_fltrust_cpu.py) ------------------------

def restate(X, s, row, c, acc_dtype, chunks=64):
    """The definition with every sum taken in `chunks` interleaved parts (columns j = l mod
    chunks first, then the parts in order) in `acc_dtype`: fp64 models a GPU summation order,
    fp32 a kernel that accumulates in fp32."""
    K, d = X.shape
    f = acc_dtype
    Xr = X.astype(f)
    cr = np.zeros(d, dtype=f) if c is None else c.astype(f)
    sr = Xr[row] if s is None else s.astype(f)

    def csum(M):
        parts = [M[..., l::chunks].sum(axis=-1, dtype=f) for l in range(chunks)]
        tot = parts[0]
        for p in parts[1:]:
            tot = (tot + p).astype(f)
        return tot
    with np.errstate(all="ignore"):
        U = (Xr - cr).astype(f)
        g = (sr - cr).astype(f)
        a, n, ng = csum(U * g), csum(U * U), csum(g * g)
        cos = a / np.sqrt(n * ng)
        counted = (np.isfinite(n) & (n > 0) & np.isfinite(a)
                   & (np.arange(K) != (-1 if row is None else row)))
        ts = np.where(counted & (cos > 0), cos, f(0)).astype(f)
    T = f(0)
    for k in range(K):
        T = f(T + ts[k])
    acc = np.zeros(d, dtype=f)
    for k in range(K):
        if ts[k] > 0:
            acc = (acc + f(ts[k] * np.sqrt(ng / n[k]) / T) * U[k]).astype(f)
    return (cr + acc).astype(np.float32)
