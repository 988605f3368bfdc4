"""Cases, inputs and the fp64 model of gm2's correction passes on a bf16 shadow of X
(csrc/stream_pass_kernel.h DELTA, csrc/weiszfeld.hip kspace_gm2_delta), shared by
tests/test_delta_cases_cpu.py and tests/test_gpu_delta.py.  Importing it needs neither a GPU nor
the library.

The loop.  STEP 0 is exact.  From STEP 1 on every exact pass is a base: its coefficients c^b (as
fp32), its output G and its exact distances D^b_k = ||x_k - G||^2 are kept.  After a STEP the
K-space step forms the next coefficients c (rounded to fp32, as the device does) and chooses:
  * no shadow yet: the next exact pass writes it iff the coefficients moved by at most
    ARM_RATIO theta relative to the previous pass's and the movement exceeds ARM_MOVE tol;
  * shadow complete: the next pass is a correction iff |c_k - c^b_k| <= theta c^b_k for all k.
A correction pass computes, on x~ = bf16(x) (round to nearest even),
    g' = G + sum_k (c_k - c^b_k) x~_k,    D_k = D^b_k + C - 2 e_k,
    Delta = g' - G,  e_k = sum_j Delta_j x~_kj,  C = sum_j Delta_j (Delta_j + 2 G_j),
which is ||x~_k - g'||^2 - ||x~_k - G||^2 added to the exact D^b_k.

theta = 2^9 eps_tile / 4 with eps_tile = stream_cases.eps_tile of the fp32 panel tile (59 u at
512 < K <= 1024): the shadow's relative error 2^-9 on sum_k |c_k - c^b_k| |x_kj| <= theta scale_j
is then a quarter of the bar.  The model is held to the exact fp64 loop (stream_cases.engine) at
the full bar eps_tile scale_j, as the GPU results are.

Inputs (bench_input): the flagship benchmark's recipe scaled down: K - K // 5 honest rows
0.05 N(0, 1), K // 5 rows 0.25 + 0.5 N(0, 1), guess 0.01 N(0, 1), from manual_seed(7000 + K).
On it the coefficients settle at once (about 1e-2, 1e-4, 1e-6 relative change per body) at
every width, which test_delta_cases_cpu.py checks for the GPU shapes before the GPU runs them.

Mutations (MUTATIONS): the model computed wrongly on purpose, as a broken pass would:
  stale_g    the correction is added to the base pass's INPUT iterate instead of its output G
  old_db     D^b taken from the pass before the base (distances to the base's input iterate)
  no_cb      the coefficient difference formed without c^b: the pass sums c_k x~_k onto G
  no_dcorr   the distance correction dropped: D_k = D^b_k
  row        one row, the one of largest weight when the shadow is written, missing from it
             (read as zeros)
"""
import numpy as np
import torch

import stream_cases as sc

ARM_RATIO = 64.0
ARM_MOVE = 4096.0
MAX_ITER_BITS = 32
KS = (513, 1000, 1024)
NS = (3, 4, 5)
MUTATIONS = ("stale_g", "old_db", "no_cb", "no_dcorr", "row")


def theta(K):
    return 2.0 ** 9 * sc.eps_tile(K, "panels", "gm2") / 4.0


def small_ds(K):
    """One partial chunk (both kinds of pass walk 32-column chunks), two chunks and a partial
    third, and many chunks plus a tail."""
    assert sc.chunk(K, True, 4) == 32
    return (20, 84, 4100)


def multi_d(K, num_cu):
    """Every block of either kind of pass walks at least 3 chunks (6 of their 32 columns): both
    tiles are capped at two blocks per CU by their launch bounds, so 64 (3 * 2 * num_cu + 1)
    columns + a ragged tail of 20 (98,388 at 256 CUs)."""
    return 64 * (3 * 2 * num_cu + 1) + 20


_INPUTS = {}


def bench_input(K, d):
    """(X [K, d], guess [d]) fp32 CPU tensors; cached, never modified."""
    if (K, d) not in _INPUTS:
        g = torch.Generator().manual_seed(7000 + K)
        nb = K // 5
        X = 0.05 * torch.randn(K, d, generator=g)
        X[K - nb:] = 0.25 + 0.5 * torch.randn(nb, d, generator=g)
        g0 = 0.01 * torch.randn(d, generator=g)
        _INPUTS[(K, d)] = (X, g0)
    return _INPUTS[(K, d)]


WARM = 3
WARM_BELOW = 1000


def guess_of(K, d):
    """The guess of one GPU case.  At d >= WARM_BELOW the recipe's.  Below, the recipe's loop
    after WARM exact bodies, rounded to fp32: at d <= 84 the coefficients move by more than theta
    until the fourth or fifth body from the recipe's random guess (the model shows it: kinds
    'xxxxd' at 1000 x 20), so no run of 3 bodies could take a correction pass; from the warm
    guess, which is what a training loop that passes the previous aggregate starts from, the
    third body does."""
    X, g0 = bench_input(K, d)
    if d >= WARM_BELOW:
        return g0
    return torch.from_numpy(exact(X, g0, WARM)[-1][0]).float()


def conv_tol(d):
    """tol of the run to convergence, from the recipe's own guess: the reference's 1e-5, and 1e-7
    at d < WARM_BELOW, where the movement (which scales with sqrt(d)) is below 1e-5 before the
    coefficients have settled (the model's kinds are 'xxxx' at d = 20 and 84 with 1e-5); 1e-7 is
    still 20 times the fp32 movement floor 2^-23 ||g|| there (||g|| <= 0.1)."""
    return 1e-5 if d >= WARM_BELOW else 1e-7


def gpu_shapes(num_cu):
    """[(K, d)]: the three small widths per K, and the multi-chunk width at K = 1000."""
    return [(K, d) for K in KS for d in small_ds(K) + ((multi_d(K, num_cu),) if K == 1000 else ())]


def _coef(D):
    """gm2's coefficients from squared distances, rounded to fp32 as the K-space step does."""
    w = 1.0 / D.sqrt().float().clamp(min=sc.EPS_CLAMP).double()
    return (w / w.sum()).float().double()


def model(X, g0, n, tol=-1.0, mut=None, force=True):
    """n bodies (fewer if the movement reaches tol) of the loop above in fp64 on the fp32 tensor
    X.  force: GMAGG_DELTA=1, which writes the shadow in STEP 1 whatever the arming rule says (the
    rule, like the size threshold, weighs cost; the guard on theta is never bypassed).
    Returns (iterates [fp64 numpy], kinds: a string of 'x' / 'd' per body)."""
    K, d = X.shape
    th = theta(K)
    Xd = X.double()
    Xs = X.to(torch.bfloat16).double()
    g = g0.double()
    D = ((Xd - g) ** 2).sum(dim=1)
    c = _coef(D)
    shadow, write = False, False
    base = None            # (cb, G, Db, G_in, Db_in)
    out, kinds = [], ""
    for t in range(n):
        corr = base is not None and shadow and t >= 1 and t < MAX_ITER_BITS and \
            bool(((c - base[0]).abs() <= th * base[0]).all())
        if corr:
            cb, G, Db, G_in, Db_in = base
            dc = c if mut == "no_cb" else c - cb
            new = (G_in if mut == "stale_g" else G) + dc @ Xs
            delta = new - G
            e = Xs @ delta
            C = float((delta * (delta + 2.0 * G)).sum())
            Dn = (Db_in if mut == "old_db" else Db) + (0.0 if mut == "no_dcorr" else C - 2.0 * e)
            Dn = Dn.clamp(min=0.0)
        else:
            new = c @ Xd
            Dn = ((Xd - new) ** 2).sum(dim=1)
            if t >= 1:
                base = (c, new, Dn, g, D)
                if write and mut == "row":
                    Xs = Xs.clone()
                    Xs[int(c.argmax())] = 0
                shadow = shadow or write
        write = False
        mv = float((g - new).float().norm())
        kinds += "d" if corr else "x"
        out.append(new.numpy())
        cn = _coef(Dn)
        if not shadow:
            settled = bool(((cn - c).abs() <= ARM_RATIO * th * c).all())
            write = (force or (settled and mv > ARM_MOVE * tol)) and t + 2 < MAX_ITER_BITS
        g, D, c = new, Dn, cn
        if mv <= tol:
            break
    return out, kinds


def exact(X, g0, n):
    """[(iterate, scale)] of the exact fp64 loop (stream_cases.engine)."""
    return sc.engine(X, g0, n, "gm2")


def mask_of(kinds):
    return sum(1 << t for t, k in enumerate(kinds) if k == "d")
