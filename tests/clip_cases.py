"""Inputs, references and bars of the norm-clipping tests (test_clip_cpu.py, test_gpu_clip.py).
Importable without a GPU and without the library.

The recipe (K, d), drawn from torch.Generator().manual_seed(5000 + K), starts from
fltrust_cases': c = 0.07 N(0, 1), a true direction t = 0.01 N, honest updates u_k = t + 0.02 N.
f = K // 5, and the last f rows cycle through KINDS: sign-flipped -3 u, scaled 100 u, zero
(x_k = c exactly), tiny 1e-3 u, one NaN entry, one +inf entry, and an exact copy of an honest
row (copied after rounding, so the two rows hold the same bits).  The rows are then permuted and
X = c + U in fp32.  bf16 cases round c to bf16-representable values first (the zero rows stay
x_k = c exactly), then X with .to(torch.bfloat16); every reference is computed on the widened
values.

The reference is the definition of include/gmagg.h in np.longdouble, at every shape (case()).
ARC takes f = K // 5; the static cases take tau = sqrt(T) of the ARC reference, rounded to fp64.

Bars, with eps_d = max(2^-36, d 2^-50) as in fltrust_cases:
  n_k, T  relative d 2^-52: positive terms, and the order of the sum is free
  s_k     relative (d + 4) 2^-52: T and n_k within d 2^-52 each, halved by the root, plus the
          roundings of the quotient and the root
  rows with s_k = 1 are the widened input bit for bit, rows with s_k = 0 are c bit for bit
  the others  |got - ref32| <= 2^-24 |ref| + eps_d (|c_j| + s_k |u_kj|) + 2^-149
  non-finite reference entries must match as NaN / the same infinity.

The builder asserts that no finite n_k other than T itself lies within 1e-8 (relative) of T:
six orders above the d 2^-52 accumulation bound, so which rows lie beyond the threshold does not
depend on the order of the sums, and the tests compare the set {k : s_k != 1} exactly.  The rows
AT the threshold (the threshold row and its exact copies, n_k == T) are ARC's ties: the device
takes T from its own n_k, equal rows have equal n_k bits, and the tests require s_k == 1 there.
For the static rule the same rows sit within an ulp of tau^2 = sqrt(T)^2, on either side
depending on the last bit of the device's n_k, so s_k is 1 or 1 - 1e-16 there: both are within
the s_k bar and give the same fp32 row, and those rows alone are left out of the set comparison."""
import functools

import numpy as np
import torch

KINDS = ("flip", "scaled", "zero", "tiny", "nan", "inf", "copy")
SHAPES = [(2, 70), (3, 70), (17, 2051), (50, 7850), (64, 1000), (65, 333), (257, 1000),
          (600, 8200), (1000, 2051), (1024, 4096), (2048, 520), (4096, 130)]
LARGE = (5, 4_300_009)
MIN_GAP = 1e-8
ARC, STATIC = "arc", "static"


def eps_d(d):
    return max(2.0 ** -36, d * 2.0 ** -50)


def arc_k(K, f):
    """The number of rows ARC clips: (2 f (K - f)) div K, in integers."""
    return (2 * f * (K - f)) // K


def arc_k_float(K, f):
    """The floating-point evaluation found elsewhere; differs from arc_k (test_clip_cpu.py)."""
    return int(2 * (f / K) * (K - f))


def inputs(K, d, dtype="fp32"):
    """(X [K, d] fp32 or bf16 tensor, c [d] fp32 tensor, kinds: list of K strings, "honest" or
    one of KINDS)."""
    gen = torch.Generator().manual_seed(5000 + K)
    N = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    c = 0.07 * N(d)
    t = 0.01 * N(d)
    U = t + 0.02 * N(K, d)
    kinds = ["honest"] * K
    nb = K // 5
    where = torch.randint(0, d, (max(nb, 1),), generator=gen)
    source = {}
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
        elif kind == "tiny":
            U[k] = 1e-3 * U[k]
        elif kind == "nan":
            U[k, where[i]] = float("nan")
        elif kind == "inf":
            U[k, where[i]] = float("inf")
        else:
            source[k] = i % (K - nb)                  # an honest row
    c32 = c.to(torch.float32)
    if dtype == "bf16":
        c32 = c32.to(torch.bfloat16).to(torch.float32)
    X = (c32.to(torch.float64) + U).to(torch.float32)
    if dtype == "bf16":
        X = X.to(torch.bfloat16)
    for k, kind in enumerate(kinds):
        if kind == "zero":
            X[k] = c32.to(X.dtype)                    # exactly
        elif kind == "copy":
            X[k] = X[source[k]]                       # the same bits
    perm = torch.randperm(K, generator=gen)
    return X[perm].contiguous(), c32, [kinds[int(p)] for p in perm]


def row_norms(X, c, real=np.longdouble):
    """n_k of the definition (X fp32 [K, d] numpy, the widened values; c fp32 [d] or None)."""
    K, d = X.shape
    cr = np.zeros(d, dtype=real) if c is None else c.astype(real)
    n = np.empty(K, dtype=real)
    with np.errstate(all="ignore"):
        for k in range(K):                            # (a row at a time: the large case)
            u = X[k].astype(real) - cr
            n[k] = (u * u).sum()
    return n


def order_of(n):
    """The rows in score_before's order: ascending, NaN last, ties to the lower index."""
    K = len(n)
    return sorted(range(K), key=lambda k: (bool(np.isnan(n[k])), n[k] if not np.isnan(n[k]) else 0,
                                           k))


def reference(X, c, rule, f=None, tau=None, real=np.longdouble, n=None, k_of=arc_k):
    """The definition on numpy arrays: a dict with n, s (real [K]), T, out32 (fp32 [K, d]),
    scale [K, d] (|c_j| + s_k |u_kj| of the rows with 0 < s_k < 1, else 0), clipped (the k with
    s_k != 1)."""
    K, d = X.shape
    cr = np.zeros(d, dtype=real) if c is None else c.astype(real)
    c32 = np.zeros(d, dtype=np.float32) if c is None else c.astype(np.float32)
    if n is None:
        n = row_norms(X, c, real)
    if rule == ARC:
        T = n[order_of(n)[K - 1 - k_of(K, f)]]
    else:
        T = real(np.float64(tau) * np.float64(tau))   # (double)tau * (double)tau
    s = np.empty(K, dtype=real)
    out32 = np.empty((K, d), dtype=np.float32)
    scale = np.zeros((K, d), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(K):
            if np.isnan(n[k]) or n[k] == np.inf:
                s[k] = 0
                out32[k] = c32
            elif np.isnan(T) or n[k] <= T:
                s[k] = 1
                out32[k] = X[k]
            else:
                s[k] = np.sqrt(T / n[k])
                if s[k] == 1:
                    out32[k] = X[k]
                elif s[k] == 0:
                    out32[k] = c32
                else:
                    u = X[k].astype(real) - cr
                    out32[k] = (cr + s[k] * u).astype(np.float32)
                    scale[k] = (np.abs(cr) + s[k] * np.abs(u)).astype(np.float64)
    return {"n": n, "s": s, "T": T, "out32": out32, "scale": scale,
            "clipped": [k for k in range(K) if s[k] != 1]}


def check_well_posed(ref):
    """The recipe's condition: no finite n other than T itself within MIN_GAP (relative) of T."""
    T = ref["T"]
    if not np.isfinite(T) or T == 0:
        return
    n = ref["n"]
    other = np.isfinite(n) & (n != T)
    gap = np.abs(n[other] - T) / T
    assert (gap > MIN_GAP).all(), float(gap.min())


@functools.lru_cache(maxsize=None)
def case(K, d, dtype="fp32", rule=ARC):
    """(inputs, reference, f, tau) of one recipe case, built once and shared; the tensors are not
    to be modified.  f = K // 5; tau (static only) is the ARC reference's sqrt(T) in fp64."""
    inp = inputs(K, d, dtype)
    f = K // 5
    if rule == ARC:
        X, c, _ = inp
        ref = reference(X.to(torch.float32).numpy(), c.numpy(), ARC, f=f)
        check_well_posed(ref)
        return inp, ref, f, None
    inp, arc_ref, f, _ = case(K, d, dtype, ARC)
    X, c, _ = inp
    tau = float(np.sqrt(arc_ref["T"]))
    ref = reference(X.to(torch.float32).numpy(), c.numpy(), STATIC, tau=tau, n=arc_ref["n"])
    ref["T_arc"] = arc_ref["T"]                      # (well posed with it: the same n_k)
    return inp, ref, f, tau


def at_threshold(ref):
    """The rows whose n_k is T (ARC) or within MIN_GAP of it (static: tau^2 is sqrt(T)^2)."""
    T, n = ref.get("T_arc", ref["T"]), ref["n"]
    if not np.isfinite(T):
        return np.zeros(len(n), dtype=bool)
    with np.errstate(all="ignore"):
        return np.isfinite(n) & (np.abs(n - T) <= MIN_GAP * T)


def _match_nonfinite(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), what
    return ~(nan | inf)


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.where(want != 0, np.abs(want), 1.0)


def worst_n(n, ref, what=""):
    """max relative error of the finite n_k (non-finite ones must match)."""
    fin = _match_nonfinite(n, ref["n"], f"{what} n")
    return float(_rel(np.asarray(n)[fin], np.asarray(ref["n"], dtype=np.float64)[fin]).max(
        initial=0.0))


def check_stats(stats, ref, K, d, rule, what=""):
    """stats: the 2K + 2 doubles of the call."""
    stats = np.asarray(stats, dtype=np.float64)
    n, s, T, m = stats[:K], stats[K:2 * K], stats[2 * K], stats[2 * K + 1]
    tol = d * 2.0 ** -52
    e_n = worst_n(n, ref, what)
    _match_nonfinite([T], [ref["T"]], f"{what} T")
    e_T = float(_rel([T], [ref["T"]])[0]) if np.isfinite(ref["T"]) else 0.0
    rs = np.asarray(ref["s"], dtype=np.float64)
    e_s = float(_rel(s, rs).max(initial=0.0))
    print(f"clip stats {what}: n {e_n:.2e} T {e_T:.2e} (bar {tol:.2e}) s {e_s:.2e} "
          f"(bar {(d + 4) * 2.0 ** -52:.2e})")
    assert e_n <= tol and e_T <= tol and e_s <= (d + 4) * 2.0 ** -52, what
    assert np.array_equal(s == 0, rs == 0), what      # the rows mapped to the centre
    tie = at_threshold(ref)
    if rule == ARC:
        assert (s[tie] == 1).all(), what              # ties at the threshold stay unclipped
        free = np.zeros(K, dtype=bool)
    else:
        free = tie
    assert np.array_equal((s != 1)[~free], (rs != 1)[~free]), what
    assert m == float((s != 1).sum()), what


def out_bar(ref):
    return (2.0 ** -24 * np.abs(ref["out32"].astype(np.float64))
            + eps_d(ref["out32"].shape[1]) * ref["scale"] + 2.0 ** -149)


def worst_out(got, ref):
    """max over the finite reference entries of |got - ref32| / bar (<= 1 passes); non-finite
    entries must match."""
    fin = _match_nonfinite(got, ref["out32"], "out")
    err = np.abs(np.asarray(got, dtype=np.float64) - ref["out32"].astype(np.float64))
    return float((err[fin] / out_bar(ref)[fin]).max(initial=0.0))


def check_out(got, X, c, ref, s_got=None, what=""):
    """got: fp32 [K, d]; X: the widened input, c: fp32 [d] or None (numpy).  s_got: the call's
    own s_k, which decide the rows that must be copies (default: the reference's)."""
    got = np.asarray(got)
    K, d = got.shape
    w = worst_out(got, ref)
    print(f"clip out {what}: worst error / bar = {w:.3e}")
    assert w <= 1.0, (what, w)
    s = np.asarray(ref["s"] if s_got is None else s_got, dtype=np.float64)
    c32 = np.zeros(d, dtype=np.float32) if c is None else c
    for k in range(K):
        if s[k] == 1:
            assert np.array_equal(got[k].view(np.int32), X[k].view(np.int32)), (what, k)
        elif s[k] == 0:
            assert np.array_equal(got[k].view(np.int32), c32.view(np.int32)), (what, k)


# ---- restatements for the bars' discrimination (test_clip_cpu.py) ---------------------------

def restate(X, c, f, acc_dtype=np.float64, k_of=arc_k, skip=True, chunks=64):
    """ARC with every n_k taken in `chunks` interleaved parts in `acc_dtype` (fp64 models a GPU
    summation order, fp32 a kernel that accumulates in fp32), k from `k_of`, and with
    skip=False the non-finite rows multiplied by s = 0 instead of replaced by c.  Returns
    (n [K] fp64, s [K] fp64, out32 [K, d])."""
    K, d = X.shape
    a = acc_dtype
    with np.errstate(all="ignore"):
        U = (X.astype(np.float64) - c.astype(np.float64))
        Ua = U.astype(a)
        parts = [(Ua[:, l::chunks] * Ua[:, l::chunks]).sum(axis=1, dtype=a) for l in range(chunks)]
        n = parts[0]
        for p in parts[1:]:
            n = (n + p).astype(a)
        n = n.astype(np.float64)
        T = n[order_of(n)[K - 1 - k_of(K, f)]]
        s = np.where(np.isnan(n) | (n == np.inf), 0.0,
                     np.where(np.isnan(T) | (n <= T), 1.0, np.sqrt(T / n)))
        out = (c.astype(np.float64) + s[:, None] * U).astype(np.float32)
        out[s == 1] = X[s == 1]
        if skip:
            out[s == 0] = c
    return n, s, out
