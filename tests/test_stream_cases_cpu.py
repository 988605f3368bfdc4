"""What keeps tests/test_gpu_stream_tiles.py from being vacuous or unpassable, checked without a
GPU: the case table covers pick_cfg, the fp64 engine of tests/stream_cases.py is the oracle's
iteration, correct fp32 arithmetic in another order meets the bar, and every mutation of the
reference misses it by at least 8x."""
import numpy as np
import pytest
import torch

import cclip_cases as cc
import stream_cases as sc
from oracle import aggregators as orc

MARGIN = 8.0


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def test_tile_table_covers_pick_cfg():
    from byzantine_aircomp_amd.panels import panel_width
    edges, nxt = [], 1
    for lo, hi, rows, pan in sc.TILE_CLASSES:
        assert lo == nxt and hi > lo                     # the classes tile 1 .. K_MAX
        nxt = hi + 1
        edges += [lo, hi]
        for t in (rows, pan):
            assert sc.covers(t) >= hi and 64 % t[1] == 0 and 4 * t[1] <= 64 * t[0]
        for K in (lo, hi):
            assert panel_width(K) == 4 * pan[1], K
            assert panel_width(K, torch.bfloat16) == 8 * pan[1], K
            assert sc.tile(K, True) == pan and sc.tile(K, False) == rows
    assert nxt - 1 == sc.K_MAX == 2048
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(ValueError):
            panel_width(sc.K_MAX + 1, dtype)
    assert sorted(set(edges) - {1}) == sc.EDGE_K
    for lo, hi, t in (sc.INIT_LIGHT, sc.ROWS_KERNEL):
        assert (lo, hi) in [(c[0], c[1]) for c in sc.TILE_CLASSES] and sc.covers(t) >= hi
    # one multi-chunk K per class, the probes' and this file's K inside the table
    assert [sc.tile(K, False) for K in sc.MULTI_K] == [c[2] for c in sc.TILE_CLASSES]
    assert all(1 <= K <= sc.K_MAX for K in sc.PROBE_K + sc.CPU_K + sc.ROWS_KERNEL_K)


def test_small_shapes_are_what_the_issue_asks():
    for K in sc.EDGE_K:
        for op, (bf16, panels, V, (mod, res)) in sc.OPERANDS.items():
            J = sc.chunk(K, panels, V)
            d1, d2 = sc.small_ds(K, op)
            assert 0 < d1 < J and 2 * J < d2 < 3 * J, (K, op, d1, d2)
            assert d1 % mod == res and d2 % mod == res
    for K in sc.MULTI_K:
        for num_cu in (256, 304):
            for op in sc.MULTI_OPS:
                bf16, panels, V, _ = sc.OPERANDS[op]
                nw, lpr = sc.tile(K, panels)[:2]
                d = sc.multi_d(K, op, num_cu)
                # its own J = LPR V: 3 chunks for each of the 32 / NW blocks a CU can hold
                assert d // (V * lpr) >= 3 * num_cu * (32 // nw) + 1, (K, op)
                assert d % 4 == 0 and d % 8 != 0 and d % (V * lpr) != 0
        assert sc.multi_d(K, "rows4", 256) == sc.multi_d(K, "panels", 256)
        assert K * sc.multi_d(K, "bf16_panels", 256) * 4 <= 420e6
    for K in sc.EDGE_K:
        for op in sc.OPERANDS:
            for agg in ("gm2", "gm", "gm_noise", "cclip"):
                assert 33 * sc.U <= sc.eps_tile(K, op, agg) <= 2.0 ** -18 < sc.MAX_EPS


@pytest.mark.parametrize("K", sc.CPU_K)
def test_engine_is_the_oracles_iteration(K):
    """B.1: the fp64 engine against oracle.gm2 / oracle.gm run on fp64 tensors and against
    cclip_cases.reference, at the same fixed count."""
    from oracle.philox import gm_draws
    for d in sc.small_ds(K, "rows4") + sc.small_ds(K, "panels_odd"):
        X, g0 = sc.tile_input(K, d)
        n = max(sc.NS)
        opts = {"maxiter": n, "tol": -1.0, "guess": g0.double()}
        want, tr = orc.gm2(X.double(), dict(opts))
        assert tr.iters == n
        assert _rel(sc.reference(K, d, False, "gm2")[n - 1][0], want.numpy()) <= 1e-12
        draw = gm_draws(sc.GM_SEED, d)
        draw.no_noise()
        opts["guess"] = sc.guess_of(K, d, "gm").double()
        want, tr = orc.gm(X.double(), dict(opts, noise_var=None, P_max=1), draw=draw)
        assert tr.iters == n
        assert _rel(sc.reference(K, d, False, "gm")[n - 1][0], want.numpy()) <= 1e-12
        # (the oracle adds the noise draws rounded to fp32, the engine in fp64: 2^-24 of the
        # noise term)
        want, _ = orc.gm(X.double(), dict(opts, noise_var=sc.GM_NOISE_VAR, P_max=1),
                         draw=gm_draws(sc.GM_SEED, d))
        assert _rel(sc.reference(K, d, False, "gm_noise")[n - 1][0], want.numpy()) <= 1e-6
        for bf16 in (False, True):
            Xw, _ = sc.operand_input(K, d, bf16)
            tau = sc.cclip_tau(Xw, g0)
            vs, clipped, _, _ = cc.reference(Xw.numpy(), g0.numpy(), tau, max(sc.CCLIP_ITERS))
            assert 0 < clipped[0] < K                   # some rows clip and some do not
            ref = sc.reference(K, d, bf16, "cclip")
            for it in sc.CCLIP_ITERS:
                assert _rel(ref[it - 1][0], vs[it - 1]) <= 1e-12


@pytest.mark.parametrize("K", sc.CPU_K)
def test_fp32_restatement_meets_the_bar(K):
    """B.2: fp32 arithmetic in another summation order stays within eps_tile."""
    worst = 0.0
    for op in ("rows4", "rows1", "panels_odd"):
        for d in sc.small_ds(K, op):
            X, g0 = sc.tile_input(K, d)
            ref = sc.reference(K, d, False, "gm2")
            got = sc.restate_gm2_f32(X, g0, max(sc.NS))
            for n in sc.NS:
                r = sc.worst_ratio(got[n - 1], *ref[n - 1], sc.eps_tile(K, op, "gm2"))
                worst = max(worst, r)
                assert r <= 1.0, (K, op, d, n, r)
    print(f"K={K}: fp32 restatement worst ratio {worst:.3f}")


PROBE_D = 4100


@pytest.mark.parametrize("K", sc.PROBE_K)
def test_probes_restatement_meets_the_bar_and_sees_one_row(K):
    """The row probes: the fp32 restatement meets PROBE_EPS, and mutation (c) on the probed
    row misses it by MARGIN."""
    X, _ = sc.tile_input(K, PROBE_D)
    for r in sc.probe_rows(K, "rows4"):
        g0 = sc.probe_guess(X, r)
        eps = sc.PROBE_EPS(K, "rows4", "gm2")
        ref, scale = sc.reference(K, PROBE_D, False, "gm2", guess=g0)[0]
        got = sc.restate_gm2_f32(X, g0, 1)[0]
        ratio = sc.worst_ratio(got, ref, scale, eps)
        bad, _ = sc.reference(K, PROBE_D, False, "gm2", guess=g0, mut=sc.Mut("c", r))[0]
        moved = sc.worst_ratio(bad, ref, scale, eps)
        print(f"K={K} r={r}: restatement {ratio:.3f}, mutation c {moved:.1f}")
        assert ratio <= 1.0, (K, r, ratio)
        assert moved >= MARGIN, (K, r, moved)


def _mutation_cases(K):
    """(operand, d, bf16, aggregators) of the small-d cases."""
    aggs = ("gm2", "gm", "gm_noise", "cclip")
    seen = set()
    for op, (bf16, panels, V, _) in sc.OPERANDS.items():
        for d in sc.small_ds(K, op):
            if (d, bf16) not in seen:
                seen.add((d, bf16))
                yield op, d, bf16, aggs


@pytest.mark.parametrize("K", sc.EDGE_K)
def test_every_mutation_misses_the_bar(K):
    """B.3: each mutation moves some element by at least MARGIN x the bar (n = 2 for the stale
    distances, n = 1 for the others); (e) where the operand has a ragged last group."""
    least = {}
    for op, d, bf16, aggs in _mutation_cases(K):
        ragged = d % (8 if bf16 else 4) != 0
        for agg in aggs:
            eps = 2.0 ** -18                    # the widest eps_tile: the margin holds for all
            ref = sc.reference(K, d, bf16, agg)
            for m in sc.MUTATIONS:
                if m == "e" and not ragged:
                    continue
                n = 2 if m == "d" else 1
                row = 0
                if m == "c":
                    row = sc.distance_rows(K, d, bf16, agg)[0]
                bad = sc.reference(K, d, bf16, agg, mut=sc.Mut(m, row))
                moved = sc.worst_ratio(bad[n - 1][0], *ref[n - 1], eps)
                least[m] = min(least.get(m, np.inf), moved)
                assert moved >= MARGIN, (K, op, d, agg, m, moved)
    print(f"K={K}: least margins " + ", ".join(f"{m} {v:.0f}x" for m, v in sorted(least.items())))
