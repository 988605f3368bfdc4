"""Case builder and numpy fp64 references for CAF (byzantine_aircomp_amd caf, csrc/caf.hip),
shared by tests/test_caf_cpu.py and tests/test_gpu_caf.py.  Importing it needs no GPU.

case(K, f, d): a centre p ~ 0.05 N(0, I), honest rows p + 0.01 N, the last f rows
p + 0.25 + 0.1 N (`scale` multiplies the planted rows' shift and spread), all fp32, seeded by the
shape.

reference(X, f, power_iters, power_tol): the definition of include/gmagg.h in d-space, numpy fp64:
the weighted mean, the centred rows, B = sqrt(p) o U and M = B B^T applied as B (B^T w), the same
start vector and stopping rule, no eigh.  Once the planted rows are gone the honest spectrum is
flat, the power iteration stops at its cap unconverged, and an exact eigenvector differs from its
iterate: a reference built on eigh gives weights 0.1 away.

kspace_emulated(X, f, ..., D=None): the K-space route of the definition's identities on the
squared distances D; D None: emulated_dist(X), the distances as the exact path forms them (fp32
differences, fp32 fused multiply-adds per 32-column stage, fp64 across stages).  With fp64
distances it must match reference to rounding, which is what pins the identities; with the
emulated ones its distance from reference is the error the device is allowed.

Both return {"out" fp32 [d], "weights" c* [K], "rounds", "best_round", "eigenvalue", "weight" S*,
"power_iters" [rounds], "converged" [rounds], "min_gap"}; min_gap is the smallest |S - (K - 2f)|
over every evaluation of the loop's condition.

The GPU bars.  OUT_TOL is the project's parity gate.  W_TOL (absolute, on c*) and LAM_TOL
(relative, on lambda) are 10 x the largest error of kspace_emulated against reference over
GPU_CASES, rounded up to a power of ten; the factor covers the device's different summation
orders.  `python tests/caf_cases.py` prints the table they were taken from:

  (K, f, d)          rounds  best  min_gap   err c*     err lambda  err out
  (5, 1, 33)              2     1  7.50e-01  2.74e-08   2.20e-08    0.00e+00
  (17, 3, 100)            4     3  1.29e+00  1.05e-07   2.43e-08    7.68e-09
  (64, 13, 517)          13    11  2.56e-02  1.21e-06   6.68e-07    2.49e-08
  (65, 16, 300)          17    13  3.69e+00  1.33e-05   1.03e-06    1.63e-07
  (130, 26, 1031)        15    10  1.39e+00  4.62e-06   1.08e-07    2.75e-08
  (257, 51, 700)         35    33  1.40e+00  6.20e-05   4.21e-06    1.82e-07
  (1025, 200, 64)       201   184  2.65e+00  2.04e-06   3.35e-07    2.98e-09

(err c*: max |c* - c*_ref|; err lambda: relative; err out: relative L2; measured with this file.)

Conditioning.  Late rounds run on a flat spectrum, and an instance can amplify a perturbation of
the distances by many orders: with the planted rows at 1000 x, (130, 26, 1031) drawn from seed
131213 (case(130, 26, 1031, 1000.0, seed=131213)) turns the 1e-16 rounding differences between the two routes on fp64 distances into 2e-8
on c* (1e-13 is typical), and the 2e-6 relative error of the emulated distances into another
round count.  No implementation on those distances can follow the reference there.  Every case
the GPU tests compare against the reference therefore carries a precondition computed from the
two numpy routes alone (tests/test_caf_cpu.py): on fp64 distances they agree to 1e-10 on c*.  The
scaled cases fold the scale into the seed, which gives instances that meet it.
"""
import functools

import numpy as np

F32 = np.float32
OUT_TOL = 1e-5             # relative L2 on out: the project's parity gate
W_TOL = 1e-3               # absolute on c*: 10 x 6.20e-05 (257, 51, 700), up to a power of ten
LAM_TOL = 1e-4             # relative on lambda: 10 x 4.21e-06 (257, 51, 700), up to a power of ten
GAP_MIN = 1e-2             # |S - (K - 2f)| at every test of the loop's condition

# (K, f, d): the smallest shape (2 rounds); below, at and one past a wave (f near K / 4); more
# than one block of the product; one past 1024 rows, about 200 rounds
GPU_CASES = [(5, 1, 33), (17, 3, 100), (64, 13, 517), (65, 16, 300), (130, 26, 1031),
             (257, 51, 700), (1025, 200, 64)]
SCALE_CASES = [(64, 13, 517), (130, 26, 1031)]


def seed_of(K, f, d, scale=1.0):
    return 1000 * K + 7 * f + d + int(scale) - 1


def case(K, f, d, scale=1.0, seed=None):
    rng = np.random.RandomState(seed_of(K, f, d, scale) if seed is None else seed)
    p = 0.05 * rng.randn(d)
    X = p + 0.01 * rng.randn(K, d)
    if f:
        X[K - f:] = p + scale * (0.25 + 0.1 * rng.randn(f, d))
    return np.ascontiguousarray(X.astype(F32))


@functools.lru_cache(maxsize=None)
def gpu_input(K, f, d, scale=1.0):
    X = case(K, f, d, scale)
    X.setflags(write=False)
    return X


def start_row(diag):
    """arg max with NaN first and ties to the lower index."""
    nan = np.isnan(diag)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(diag))


def weighted_mean(X, c, S):
    """float(sum over the rows with c_k > 0, increasing k, of (c_k / S) x_k)."""
    acc = np.zeros(X.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in np.flatnonzero(c > 0):
            acc = acc + (c[k] / S) * X[k].astype(np.float64)
        return acc.astype(F32)


def _filter(X, f, setup, power_iters, power_tol):
    """The rounds of the definition; setup(p, sp) -> (diag of M, column(r) of M, apply(w) ->
    (M w, g)) is the only part the d-space and K-space routes do differently."""
    K = X.shape[0]
    c = np.ones(K)
    best, rec = np.inf, None
    iters, conv = [], []
    min_gap = np.inf
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(K + 1):
            S = c.sum()
            min_gap = min(min_gap, abs(S - (K - 2 * f)))
            if not S > K - 2 * f or t == K:
                break
            p = c / S
            sp = np.sqrt(p)
            diag, column, apply = setup(p, sp)
            m = column(start_row(diag))
            nrm = np.linalg.norm(m)
            it, cv, lam, failed, g = 0, False, 0.0, False, None
            if nrm == 0:
                cv = True
            elif not np.isfinite(nrm):
                failed = True
            else:
                w = m / nrm
                for _ in range(power_iters):
                    v, _g = apply(w)
                    n = np.linalg.norm(v)
                    it += 1
                    if not (n > 0 and np.isfinite(n)):
                        failed = True
                        break
                    w1 = v / n
                    mov = np.linalg.norm(w1 - w)
                    w = w1
                    if mov <= power_tol:
                        cv = True
                        break
                if not failed:
                    v, g = apply(w)
                    lam = float(w @ v)
            if failed or not np.isfinite(lam):
                if rec is None:
                    rec = (c.copy(), S, t, np.nan)
                break
            iters.append(it)
            conv.append(cv)
            if lam < best:
                best, rec = lam, (c.copy(), S, t, lam)
            if g is None:
                break
            tau = g * g
            pos = c > 0
            tmax = tau[pos].max()
            if not (tmax > 0 and np.isfinite(tmax)):
                break
            c = np.where(pos, c * (1.0 - tau / tmax), c)
    if rec is None:
        rec = (np.ones(K), float(K), 0, np.nan)
    cs, Ss, ts, lam = rec
    return {"out": weighted_mean(X, cs, Ss), "weights": cs, "rounds": len(iters), "best_round": ts,
            "eigenvalue": lam, "weight": Ss, "power_iters": iters, "converged": conv,
            "min_gap": float(min_gap)}


def reference(X, f, power_iters=100, power_tol=1e-10):
    x = np.asarray(X, dtype=np.float64)
    if f == 0:                                   # no round: `mean`, summed in row order
        acc = np.zeros(x.shape[1])
        for k in range(x.shape[0]):
            acc += x[k]
        res = _filter(X, 0, None, power_iters, power_tol)
        res["out"] = (acc / x.shape[0]).astype(F32)
        return res

    def setup(p, sp):
        u = x - p @ x
        B = sp[:, None] * u

        def apply(w):
            g = u @ (B.T @ w)
            return sp * g, g
        return (B * B).sum(axis=1), lambda r: B @ B[r], apply
    return _filter(X, f, setup, power_iters, power_tol)


def dist64(X):
    """fp64 squared distances from the differences themselves."""
    x = np.asarray(X, dtype=np.float64)
    D = np.empty((x.shape[0],) * 2)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(x.shape[0]):
            D[i] = ((x - x[i]) ** 2).sum(axis=1)
    return D


def emulated_dist(X):
    """The exact path's distances (coordinate.hip pair_dist): t = x_i - x_j in fp32, acc =
    fmaf(t, t, acc) over the 32 columns of a stage in fp32 (a product of two fp32 values is exact
    in fp64, so the fused step is one fp64 add rounded to fp32), the stages summed in fp64."""
    x = np.asarray(X, dtype=F32)
    K, d = x.shape
    D = np.zeros((K, K))
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, d, 32):
            acc = np.zeros((K, K), dtype=F32)
            for j in range(c0, min(c0 + 32, d)):
                t = (x[:, None, j] - x[None, :, j]).astype(np.float64)
                acc = (acc.astype(np.float64) + t * t).astype(F32)
            D += acc.astype(np.float64)
    return D


def kspace_emulated(X, f, power_iters=100, power_tol=1e-10, D=None):
    if D is None:
        D = emulated_dist(X)

    def setup(p, sp):
        a = D @ p
        q = 0.5 * (p @ a)
        rho = a - q

        def apply(w):
            z = sp * w
            g = 0.5 * (rho * z.sum() + rho @ z - D @ z)
            return sp * g, g
        return p * rho, lambda r: sp * sp[r] * (0.5 * (rho + rho[r] - D[r])), apply
    return _filter(X, f, setup, power_iters, power_tol)


@functools.lru_cache(maxsize=None)
def gpu_reference(K, f, d, scale=1.0):
    """reference() of one GPU case, computed once and shared."""
    return reference(gpu_input(K, f, d, scale), f)


def errors(got, ref):
    """(max |c* - c*_ref|, relative error of lambda, relative L2 of out)."""
    ew = float(np.abs(np.asarray(got["weights"]) - ref["weights"]).max())
    el = abs(got["eigenvalue"] - ref["eigenvalue"]) / abs(ref["eigenvalue"])
    o, r = np.asarray(got["out"], dtype=np.float64), ref["out"].astype(np.float64)
    return ew, float(el), float(np.linalg.norm(o - r) / np.linalg.norm(r))


def byzantine_share(weights, f):
    w = np.asarray(weights)
    return float(w[len(w) - f:].sum() / w.sum())


if __name__ == "__main__":
    print("(K, f, d)          rounds  best  min_gap   err c*     err lambda  err out")
    for K, f, d in GPU_CASES:
        ref = gpu_reference(K, f, d)
        emu = kspace_emulated(gpu_input(K, f, d), f)
        assert (emu["rounds"], emu["best_round"]) == (ref["rounds"], ref["best_round"])
        ew, el, eo = errors(emu, ref)
        print(f"{str((K, f, d)):<20} {ref['rounds']:>4} {ref['best_round']:>5}  "
              f"{ref['min_gap']:.2e}  {ew:.2e}   {el:.2e}    {eo:.2e}")
