"""Inputs and references shared by the centered-clipping tests (test_cclip_cpu.py,
test_gpu_cclip.py, test_gpu_cclip_sharded.py).  Importable without a GPU.

Inputs: the C3 recipe from torch.Generator().manual_seed(1000 + K): honest rows
0.05 N(0, 1), the last K // 5 rows 0.25 + 0.5 N(0, 1), guess 0.01 N(0, 1); bf16 cases use
X.to(bfloat16) and every reference is computed on the widened values.

Reference: Karimireddy, He & Jaggi (ICML 2021), Algorithm 2, as written in the paper,
    v <- v + mean_k (x_k - v) min(1, tau / ||x_k - v||),
in fp64 numpy (`reference`).  It owes nothing to the library.  `restatement` is the same
iteration in the form the kernels use, v' = sum_k c_k x_k + a v with fp32 c, a and sums: the
CPU test holds it to 1e-6 of the reference, which is what leaves the GPU bar (1e-5, the
project's bar for gm2 against its oracle) its margin.

The three radii, relative to sqrt(d) (an honest row is ~0.05 sqrt(d) from the guess, a
Byzantine row ~0.56 sqrt(d)):  "mid" 0.2 sqrt(d) clips exactly the Byzantine rows, "low"
0.02 sqrt(d) clips every row, "high" 1e6 clips none.
"""
import math

import numpy as np
import torch

TOL = 1e-5                 # GPU bar: relative L2 against the fp64 reference
RESTATEMENT_TOL = 1e-6     # CPU bar of the fp32 restatement against the fp64 reference
SHAPES = [(3, 70), (17, 1000), (50, 7850), (256, 16392), (513, 333), (600, 8200), (1000, 2051),
          (1024, 4096), (1000, 40008)]
BF16_SHAPES = [(17, 1000), (513, 333), (600, 8200), (1000, 2051), (1000, 40008)]
TAUS = ("mid", "low", "high")
ITERS = (1, 3)
MAX_ITERS = max(ITERS)
BLOCK = 4096               # columns per block of the blocked fp64 passes


def tau_of(name, d):
    return {"mid": 0.2 * math.sqrt(d), "low": 0.02 * math.sqrt(d), "high": 1e6}[name]


def initial_clipped(name, K):
    """Clients outside the radius at the guess: the Byzantine rows, every row, none."""
    return {"mid": K // 5, "low": K, "high": 0}[name]


def recipe(K, d):
    g = torch.Generator().manual_seed(1000 + K)
    nb = K // 5
    X = torch.randn(K - nb, d, generator=g) * 0.05
    if nb:
        X = torch.cat([X, torch.randn(nb, d, generator=g) * 0.5 + 0.25])
    g0 = torch.randn(d, generator=g) * 0.01
    return X, g0


_INPUTS = {}


def inputs(K, d, dtype="fp32"):
    """(X, guess) as CPU tensors, X in `dtype` ("fp32" or "bf16"); cached, never modified."""
    if (K, d) not in _INPUTS:
        _INPUTS[(K, d)] = recipe(K, d)
    X, g0 = _INPUTS[(K, d)]
    return (X.to(torch.bfloat16) if dtype == "bf16" else X), g0


def _dists(X32, v):
    """||x_k - v|| in fp64, X32 an fp32 array widened block by block."""
    D = np.zeros(X32.shape[0])
    for j in range(0, X32.shape[1], BLOCK):
        diff = X32[:, j:j + BLOCK].astype(np.float64) - v[j:j + BLOCK]
        D += np.einsum("kj,kj->k", diff, diff)
    return np.sqrt(D)


def reference(X32, v0, tau, iters):
    """The paper's recurrence in fp64.  X32: fp32 numpy [K, d] (widened exactly), v0 any
    float array.  Returns (iterates [v_1 .. v_iters], clipped counts, movements, margins):
    entry l belongs to iteration l (the step from v_l to v_{l+1}); the margin is
    min_k |dist_k / tau - 1| at that step."""
    v = np.asarray(v0, dtype=np.float64).copy()
    vs, clipped, moves, margins = [], [], [], []
    for _ in range(iters):
        dist = _dists(X32, v)
        lam = np.ones_like(dist)
        out = dist > tau
        lam[out] = tau / dist[out]
        new = np.empty_like(v)
        for j in range(0, v.size, BLOCK):
            diff = X32[:, j:j + BLOCK].astype(np.float64) - v[j:j + BLOCK]
            new[j:j + BLOCK] = v[j:j + BLOCK] + (lam[:, None] * diff).mean(axis=0)
        clipped.append(int(out.sum()))
        margins.append(float(np.abs(dist / tau - 1.0).min()))
        moves.append(float(np.linalg.norm(new - v)))
        v = new
        vs.append(v)
    return vs, clipped, moves, margins


def restatement(X32, v0, tau, iters):
    """The same iteration as the kernels state it: squared distances summed in fp64 from fp32
    differences, c_k = fp32(lambda_k / K), a = fp32(1 - sum of the rounded c_k), and
    v' = sum_k c_k x_k + a v in fp32 (the fused pass sums in fp64: this is the looser form)."""
    K = X32.shape[0]
    v = np.asarray(v0, dtype=np.float32).copy()
    vs = []
    for _ in range(iters):
        D = np.zeros(K)
        for j in range(0, v.size, BLOCK):
            diff = X32[:, j:j + BLOCK] - v[j:j + BLOCK]
            D += np.einsum("kj,kj->k", diff, diff, dtype=np.float64)
        dist = np.sqrt(D)
        lam = np.ones_like(dist)
        out = dist > tau
        lam[out] = tau / dist[out]
        c = (lam / K).astype(np.float32)
        a = np.float32(1.0 - c.astype(np.float64).sum())
        v = (c @ X32 + a * v).astype(np.float32)
        vs.append(v)
    return vs


_REFS = {}


def ref_case(K, d, dtype, tau_name):
    """reference() of one input and radius over MAX_ITERS iterations (cached): iteration
    counts 1 and 3 read entries 0 and 2."""
    key = (K, d, dtype, tau_name)
    if key not in _REFS:
        X, g0 = inputs(K, d, dtype)
        _REFS[key] = reference(X.float().numpy(), g0.numpy(), tau_of(tau_name, d), MAX_ITERS)
    return _REFS[key]


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
