"""What keeps tests/test_gpu_resident_tiles.py from being vacuous or unpassable, checked without
a GPU: the plan tables of tests/resident_cases.py agree with the sources, its fp64 engine is the
oracle's iteration on the new inputs, an fp32 restatement of each kernel's arithmetic in other
summation orders meets the bar, and the mutations of the reference miss it by at least 8x
(the least margins are printed; every mutation reaches 8x for gm2, noiseless gm and gm with
noise, h in body 3 itself)."""
import os
import re

import numpy as np
import pytest
import torch

import resident_cases as rc
import stream_cases as sc
from oracle import aggregators as orc

MARGIN = 8.0
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "byzantine_aircomp_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


# ------------------------------------------------------------------------------ plan tables

def test_plan_tables_match_the_sources():
    from byzantine_aircomp_amd import batched
    from byzantine_aircomp_amd.panels import panel_width
    res, rb, ctx = _src("resident.hip"), _src("resident_batched.hip"), _src("host_ctx.h")
    tiles = {tuple(int(x) for x in m) for m in
             re.findall(r"GMK_RES\(V_, (\d+), (\d+), (\d+)\)", res)}
    assert tiles == set(rc.RES_TILES)
    assert int(re.search(r"kResTargetBlocks = (\d+);", res).group(1)) == rc.RES_TARGET_BLOCKS
    assert int(re.search(r"#define GMK_RES_TILE_REGS (\d+)", res).group(1)) == rc.RES_TILE_REGS
    assert re.search(r"for \(int c = 1; c <= 8; c \*= 2\)", res)
    assert re.search(r"nb0 >= 90 &&\s+\(nch \+ cpb / 2 - 1\) / \(cpb / 2\) <= 192", res)
    assert re.search(r"cfg->NW == 16 && cfg->R == 4\) \{\s+nw = 8;\s+r = 8;", ctx)
    assert int(re.search(r"constexpr int kRbCols = (\d+);", rb).group(1)) == rc.RB_COLS
    got = {int(a): (int(b), c == "true") for a, b, c in
           re.findall(r"GMK_RB\((\d+), (\d+), (true|false)\)", rb.split("#define GMK_RB(")[1])}
    assert {k: v[0] for k, v in got.items()} == rc.RB_TILES
    assert max(k for k, v in got.items() if v[1]) == rc.RB_GM_KMAX
    assert batched.SEED_STRIDE == rc.SEED_STRIDE
    # every K class: a resident tile that covers it, or the declining class
    for lo, hi, rows, _ in sc.TILE_CLASSES:
        for K in (lo, hi):
            t = rc.resident_tile(K)
            assert (t is None) == (K in (513, 1024)), K
            if t:
                assert t[0] * (64 // t[1]) * t[2] >= K
                assert t == ((8, 64, 8) if 32 < K <= 64 else rows[:3])
    assert all(rc.resident_tile(K) is None for K in rc.DECLINE_K)
    # panels: the single kernel reads them with V = 2, which divides the panel width
    for K in rc.EDGE_K:
        if K <= rc.PANEL_K_MAX:
            assert panel_width(K) % 2 == 0 and rc.resident_tile(K)[1] == 64
    for K in rc.RB_K:
        kr = rc.rb_rows_for(K)
        assert kr >= K and kr in rc.RB_TILES and (K == 1 or rc.rb_rows_for(K - 1) <= kr)
    assert rc.rb_rows_for(53) == 0 and rc.rb_plan(51, 100, "gm") is None
    assert rc.rb_plan(50, 2 * rc.RB_COLS + 20, "gm") == (50, 32, 3)


def test_shapes_land_on_every_cpb_and_exchange():
    """The d of every case gives the plan it is named for (num_cu 256 and 304)."""
    seen = set()
    for num_cu in (256, 304):
        for K in rc.EDGE_K:
            for op, (panels, V, (mod, res)) in rc.OPERANDS.items():
                if panels and K > rc.PANEL_K_MAX:
                    continue
                t = rc.resident_tile(K)
                J = t[1] * V
                ds = rc.single_ds(K, op, num_cu)
                assert all(d % mod == res and d > 0 for d in ds.values()), (K, op, ds)
                assert 0 < ds["part"] < J and rc.resident_plan(K, V, ds["part"]) == (1, 1)
                assert rc.resident_plan(K, V, ds["x32"]) == (1, 32)
                for c in rc.cpbs_of(K, V)[1:]:
                    cpb, nb = rc.resident_plan(K, V, ds[f"cpb{c}"])
                    assert (cpb, nb) == (c, 17) and ds[f"cpb{c}"] % (J * c) != 0, (K, op, c)
                    seen.add((t, V, c))
                if not panels:
                    cpb, nb = rc.resident_plan(K, V, ds["beyond"])
                    assert cpb == rc.cpbs_of(K, V)[-1] and nb == num_cu // 8 + 2
                    assert rc.res_xcd_stride(nb, num_cu) == 1
                    assert rc.exchange_of(K, nb, num_cu) == (
                        "xcd_split" if t == rc.HIER_TILE else "agent")
                    assert K * ds["beyond"] <= 1 << 22
                for d in ds.values():
                    if "beyond" not in ds or d != ds["beyond"]:
                        nb = rc.resident_plan(K, V, d)[1]
                        assert rc.exchange_of(K, nb, num_cu) == "xcd_local"
    # CPB 4 and 8, V = 1 and 2, and the four wide-K tiles are all reached
    assert {c for _, _, c in seen} == {2, 4, 8}
    for t in ((16, 64, 8), (16, 32, 8), (16, 16, 8), (16, 4, 8)):
        assert (t, 1, 2) in seen
    for nb in rc.HIER_NB:
        d = rc.hier_d(nb)
        assert rc.resident_plan(50, 4, d) == ((1 if nb >= 90 else 2), nb), nb
        assert rc.exchange_of(50, nb, 256, hier_mode=2) == "xcd_hier"
    assert sorted(nb % 8 for nb in rc.HIER_NB[:3]) == [0, 1, 7] and rc.HIER_NB[3] >= 90
    assert rc.exchange_of(50, 190, 256) == "xcd_hier" and rc.exchange_of(50, 40, 256) == "xcd_split"
    assert rc.exchange_of(50, 40, 256, split_mode=0) == "agent"
    for num_cu in (256, 304):
        nb, P = rc.rb_group_shape(num_cu)
        for occ in (1, 2):
            ng = occ * num_cu // nb
            assert 1 <= ng and P > 2 * ng
    for K in rc.RB_K:
        for agg in rc.AGGS:
            if rc.rb_plan(K, 1, agg) is None:
                continue
            e = rc.eps_batched(K, agg)
            assert 33 * rc.U <= e <= 114 * rc.U < rc.MAX_EPS
    for K in rc.EDGE_K:
        for agg in rc.AGGS:
            assert 33 * rc.U <= rc.eps_single(K, agg) <= 82 * rc.U


# ----------------------------------------------------------------------------------- engine

CPU_SINGLE = [(16, "rows4", "cpb4"), (17, "rows1", "cpb8"), (50, "rows4", "beyond"),
              (129, "rows1", "cpb2"), (2048, "rows4", "beyond")]


@pytest.mark.parametrize("K,op,which", CPU_SINGLE)
def test_engine_is_the_oracles_iteration(K, op, which):
    from oracle.philox import gm_draws
    d = rc.single_ds(K, op)[which]
    X, g0, JB, _ = rc.single_case(K, op, d)
    assert d > JB and not torch.equal(X, sc.tile_input(K, d)[0])      # block-graded
    n = max(rc.NS)
    opts = {"maxiter": n, "tol": -1.0, "guess": g0.double()}
    want, tr = orc.gm2(X.double(), dict(opts))
    assert tr.iters == n
    assert _rel(rc.engine(X, g0, n, "gm2", JB)[-1][0], want.numpy()) <= 1e-12
    draw = gm_draws(rc.GM_SEED, d)
    draw.no_noise()
    want, tr = orc.gm(X.double(), dict(opts, noise_var=None, P_max=1), draw=draw)
    assert tr.iters == n
    assert _rel(rc.engine(X, g0, n, "gm", JB)[-1][0], want.numpy()) <= 1e-12
    # (the oracle adds the noise draws rounded to fp32, the engine in fp64)
    seed = rc.gm_seed_for(X, g0, "gm_noise", JB)
    want, _ = orc.gm(X.double(), dict(opts, noise_var=rc.GM_NOISE_VAR, P_max=1),
                     draw=gm_draws(seed, d))
    assert _rel(rc.engine(X, g0, n, "gm_noise", JB, seed=seed)[-1][0], want.numpy()) <= 1e-6
    # and it is stream_cases.engine's arithmetic
    ref = sc.engine(X, g0, n, "gm2")
    assert _rel(rc.engine(X, g0, n, "gm2", JB)[-1][0], ref[-1][0]) <= 1e-12


# ------------------------------------------------------------------------ fp32 restatement

@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K,op,which", CPU_SINGLE + [(50, "rows4", "part"), (129, "rows2", "part")])
def test_fp32_restatement_of_the_single_kernel_meets_the_bar(K, op, which, agg):
    d = rc.single_ds(K, op)[which]
    X, g0, JB, _ = rc.single_case(K, op, d)
    g0 = rc.guess_for(K, d, agg, g0)
    seed = rc.gm_seed_for(X, g0, agg, JB)
    ref = rc.engine(X, g0, max(rc.NS), agg, JB, seed=seed)
    got = rc.restate_f32(X, g0, max(rc.NS), agg, JB, K <= 64, seed=seed)
    worst = max(sc.worst_ratio(got[n - 1], *ref[n - 1], rc.eps_single(K, agg)) for n in rc.NS)
    print(f"single K={K} {op} {which} d={d} {agg}: fp32 restatement worst ratio {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K", [16, 50, 52])
def test_fp32_restatement_of_the_batched_kernel_meets_the_bar(K, agg):
    if rc.rb_plan(K, 1, agg) is None:
        return                                  # (gm at K > 50 streams: no kernel to restate)
    worst = 0.0
    for d in rc.RB_DS:
        probs = [rc.block_input(K, d, rc.RB_COLS, q) for q in range(2)]
        key = rc.gm_seed_for(*zip(*probs), agg, rc.RB_COLS)
        for q, (X, g0) in enumerate(probs):
            seed = rc.batched_seed(q, key)
            ref = rc.engine(X, g0, max(rc.NS), agg, rc.RB_COLS, seed=seed)
            got = rc.restate_f32(X, g0, max(rc.NS), agg, rc.RB_COLS, True, seed=seed)
            worst = max([worst] + [sc.worst_ratio(got[n - 1], *ref[n - 1], rc.eps_batched(K, agg))
                                   for n in rc.NS])
    print(f"batched K={K} {agg}: fp32 restatement worst ratio {worst:.3f}")
    assert worst <= 1.0


# -------------------------------------------------------------------------------- mutations

def _margins(X, g0, agg, JB, eps, muts, seed=rc.GM_SEED):
    """{mutation: (margin in its body, best margin over bodies 1..4)}."""
    n = max(rc.NS)
    ref = rc.engine(X, g0, n, agg, JB, seed=seed)
    out = {}
    for name, mut in muts.items():
        bad = rc.engine(X, g0, n, agg, JB, mut, seed=seed)
        per = [sc.worst_ratio(bad[i][0], *ref[i], eps) for i in range(n)]
        out[name] = (per[rc.BODY_OF[name] - 1], max(per))
    return out


def _check(least, what, got):
    """Every mutation misses the bar by MARGIN in the body it is aimed at (BODY_OF: h in body
    3, where the other granule buffer is first reused), which the GPU test checks."""
    for m, (at, best) in got.items():
        least[m] = min(least.get(m, np.inf), at)
        assert at >= MARGIN, (what, m, at, best)


def _report(what, least):
    print(f"{what}: least margins " + ", ".join(f"{m} {v:.1f}x" for m, v in sorted(least.items())))


SINGLE_MUT_K = [16, 17, 50, 129, 300, 2048]


@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K", SINGLE_MUT_K)
def test_row_mutations_miss_the_single_bar(K, agg):
    """a - e on the one-block cases of the GPU test (e where d % 4 != 0)."""
    least = {}
    eps = 82 * rc.U                              # the widest single bar: the margin holds for all
    for op in ("rows4", "rows2", "rows1"):
        d = rc.single_ds(K, op)["part"]
        X, g0, JB, _ = rc.single_case(K, op, d)
        g0 = rc.guess_for(K, d, agg, g0)
        muts = {m: rc.Mut(m, rc.distance_row(X, g0, agg, JB) if m == "c" else 0)
                for m in rc.ROW_MUTATIONS if m != "e" or d % 4}
        _check(least, (K, op, d, agg),
               _margins(X, g0, agg, JB, eps, muts, rc.gm_seed_for(X, g0, agg, JB)))
    _report(f"single rows K={K} {agg}", least)


@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K", SINGLE_MUT_K)
def test_block_mutations_miss_the_single_bar(K, agg):
    """f, g, h (and j where CPB > 1) on the multi-block cases of the GPU test, a full block."""
    least = {}
    eps = 82 * rc.U
    for op in ("rows4", "rows1"):
        V = rc.OPERANDS[op][1]
        ds = rc.single_ds(K, op)
        for which in [w for w in ds if w not in ("part",)]:
            d = ds[which]
            X, g0, JB, J = rc.single_case(K, op, d)
            g0 = rc.guess_for(K, d, agg, g0)
            bm = rc.full_block(d, JB)
            assert (bm + 1) * JB <= d
            muts = {m: rc.Mut(m, block=bm) for m in rc.BLOCK_MUTATIONS}
            if JB > J:
                muts["j"] = rc.Mut("j", block=bm, J=J)
            _check(least, (K, op, which, d, agg),
                   _margins(X, g0, agg, JB, eps, muts, rc.gm_seed_for(X, g0, agg, JB)))
    _report(f"single blocks K={K} {agg}", least)


@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K", [16, 32, 50, 52])
def test_mutations_miss_the_batched_bar(K, agg):
    """a - e at d = 1030 (one block, a partial float4 group), f - i and k at 3 blocks."""
    if rc.rb_plan(K, 1, agg) is None:
        return
    least = {}
    eps = 114 * rc.U                             # the widest batched bar
    kr, kv, _ = rc.rb_plan(K, 1, agg)
    JB = rc.RB_COLS
    d = rc.RB_DS[0]
    probs = [rc.block_input(K, d, JB, q) for q in range(2)]
    seed = rc.batched_seed(1, rc.gm_seed_for(*zip(*probs), agg, JB))
    X, g0 = probs[1]
    muts = {m: rc.Mut(m, rc.distance_row(X, g0, agg, JB) if m == "c" else 0)
            for m in rc.ROW_MUTATIONS}
    _check(least, (K, d, agg), _margins(X, g0, agg, JB, eps, muts, seed))
    d = rc.RB_DS[2]
    probs = [rc.block_input(K, d, JB, q) for q in range(2)]
    seed = rc.batched_seed(1, rc.gm_seed_for(*zip(*probs), agg, JB))
    X, g0 = probs[1]
    bm = rc.full_block(d, JB)
    muts = {m: rc.Mut(m, block=bm) for m in rc.BLOCK_MUTATIONS}
    muts["i"] = rc.Mut("i", block=bm, prev=probs[0])
    if K > kv:
        muts["k"] = rc.Mut("k", kv=kv)
    _check(least, (K, d, agg), _margins(X, g0, agg, JB, eps, muts, seed))
    _report(f"batched K={K} {agg}", least)


@pytest.mark.parametrize("K", [17, 50, 2048])
def test_probes_see_one_row(K):
    """The row probes: the fp32 restatement meets the bar and mutation (c) on the probed row
    misses it by MARGIN (single tile, d = 1028 on one block's plan)."""
    d = 1028
    JB = d
    X, _ = rc.block_input(K, d, JB)
    eps = rc.eps_single(K, "gm2")
    for r in rc.probe_rows(K):
        g0 = sc.probe_guess(X, r)
        ref, scale = rc.engine(X, g0, 1, "gm2", JB)[0]
        got = rc.restate_f32(X, g0, 1, "gm2", 256, False)[0]
        bad = rc.engine(X, g0, 1, "gm2", JB, rc.Mut("c", r))[0][0]
        ratio, moved = sc.worst_ratio(got, ref, scale, eps), sc.worst_ratio(bad, ref, scale, eps)
        print(f"K={K} r={r}: restatement {ratio:.3f}, mutation c {moved:.1f}")
        assert ratio <= 1.0 and moved >= MARGIN, (K, r, ratio, moved)
