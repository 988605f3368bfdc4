"""The fp64 model of gm2's correction passes on a bf16 shadow (tests/delta_cases.py) against the
exact fp64 loop, at the bar the GPU results are held to, and its mutations.  No GPU, no library.

  * On every shape tests/test_gpu_delta.py runs (but the multi-chunk one, checked there against
    the same model), for exactly 3, 4 and 5 bodies and for the run to tol = 1e-5: the model takes
    at least one correction pass, every element is within eps_tile scale_j of the exact loop, and
    the converged run stops at the exact loop's count.
  * On slowly contracting inputs (the recipe at K = 17, d = 2 and 3, 24 bodies: the coefficients
    stay within theta of the base for ten passes and more while still moving by 1e-4) the model
    holds the bar and each mutation misses it by 8x or more.
"""
import numpy as np
import pytest
import torch

import delta_cases as dc
import stream_cases as sc

SHAPES = [(K, d) for K in dc.KS for d in dc.small_ds(K)]
SLOW = [(17, 2), (17, 3)]
SLOW_N = 24


def _eps(K):
    return sc.eps_tile(K, "panels", "gm2")


@pytest.mark.parametrize("K,d", SHAPES)
def test_model_takes_corrections_and_holds_the_bar(K, d):
    X, g0 = dc.bench_input(K, d)[0], dc.guess_of(K, d)
    ref = dc.exact(X, g0, max(dc.NS))
    for n in dc.NS:
        outs, kinds = dc.model(X, g0, n)
        assert len(kinds) == n and "d" in kinds and kinds[:2] == "xx", (n, kinds)
        worst = sc.worst_ratio(outs[-1].astype(np.float32), ref[n - 1][0], ref[n - 1][1], _eps(K))
        print(K, d, n, kinds, f"worst {worst:.3f}")
        assert worst <= 1.0, (n, kinds, worst)


@pytest.mark.parametrize("K,d", SHAPES)
def test_model_converges_at_the_exact_count(K, d):
    X, g0 = dc.bench_input(K, d)
    tol = dc.conv_tol(d)
    outs, kinds = dc.model(X, g0, 100, tol=tol)
    g, n_exact = g0.double(), 0
    for it, (new, _) in enumerate(sc.engine(X, g0, len(kinds) + 2, "gm2")):
        mv = float(np.float32(np.linalg.norm((g.numpy() - new).astype(np.float32))))
        g, n_exact = torch.from_numpy(new), it + 1
        if mv <= tol:
            break
    print(K, d, kinds, n_exact)
    assert "d" in kinds and len(kinds) == n_exact, (kinds, n_exact)


def test_theta_is_a_quarter_of_the_bar():
    for K in dc.KS:
        assert dc.theta(K) == 59 * 2.0 ** -17
        assert 2.0 ** -9 * dc.theta(K) == _eps(K) / 4


@pytest.mark.parametrize("K,d", SLOW)
def test_mutations_miss_the_bar(K, d):
    X, g0 = dc.bench_input(K, d)
    ref = dc.exact(X, g0, SLOW_N)
    eps = _eps(K)

    def worst(mut):
        outs, kinds = dc.model(X, g0, SLOW_N, mut=mut)
        return max(sc.worst_ratio(o, r[0], r[1], eps) for o, r in zip(outs, ref)), kinds

    w0, kinds = worst(None)
    print(K, d, kinds, f"model {w0:.3f}")
    assert kinds.count("d") >= 8 and w0 <= 1.0, (kinds, w0)
    for mut in dc.MUTATIONS:
        w, k = worst(mut)
        print(K, d, mut, k, f"{w:.1f}")
        assert w >= 8.0, (mut, k, w)
