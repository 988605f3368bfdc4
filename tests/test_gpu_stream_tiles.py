"""Every tile, vector width and mode of the fused streaming pass against the fp64 references of
tests/stream_cases.py, whose docstring states the inputs, derives the per-element bar
|got_j - ref_j| <= eps_tile * scale_j and lists the mutations the bar is there to catch.

Every call passes algo="stream" and tol = -1 (exactly n bodies) and must report the streaming
path, n iterations and a finite result.  Row-major views sit in NaN-filled buffers and the
panels' padding columns hold a sentinel, so a read past d shows.  Each case prints its worst
|got - ref| / (eps_tile * scale) ("RATIO ..."); DESIGN.md §3.1 records them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stream_cases as sc
import stream_variant_runner as runner
from conftest import rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = 7.0                 # in the panels' padding columns
CHILD_TIMEOUT = 240            # seconds for one forced-variant child (the list takes ~20 s)


def bz():
    import byzantine_aircomp_amd as m
    return m


def make_operand(op, X):
    """The fp32 CPU matrix X (bf16 operands: already rounded) on the GPU as operand `op` of
    stream_cases.OPERANDS, its padding poisoned."""
    bf16, panels, V, _ = sc.OPERANDS[op]
    dt = torch.bfloat16 if bf16 else torch.float32
    K, d = X.shape
    Xt = X.to(dt).cuda()
    if panels:
        P = bz().ClientPanels.from_rows(Xt)
        assert P.W == sc.chunk(K, True, V)
        rem = d - (P.npan - 1) * P.W
        if rem < P.W:
            P.data[-1, :, rem:] = SENTINEL
        return P

    def view(width, off):
        buf = torch.full((K, width), float("nan"), dtype=dt, device="cuda")
        buf[:, off:off + d] = Xt
        return buf[:, off:off + d]

    if op == "misaligned":
        w = view(d + 4, 1)
        assert w.data_ptr() % 16 == 4 and w.stride(0) == d + 4
    elif op == "padded":
        w = view(d + 4, 0)
        assert w.data_ptr() % 16 == 0 and w.stride(0) % 4 == 0
    elif op == "bf16_rows":
        w = view(d + 8, 0)
        assert w.data_ptr() % 16 == 0 and w.stride(0) % 8 == 0 and d % 8 == 0
    else:
        w = Xt
        assert w.is_contiguous() and d % 4 == {"rows4": 0, "rows2": 2}.get(op, d % 4)
    return w


def run(agg, w, g, n, tau=None):
    out, _ = runner.run(agg, w, g, n, tau)
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all()), agg
    return out


def _report(what, worst, failures):
    for key, r in sorted(worst.items()):
        print(f"RATIO {what} {key} worst={r:.3f}")
    assert not failures, failures[:20]


AGGS = ("gm2", "gm", "gm_noise", "cclip")


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("K", sc.EDGE_K)
def test_tiles_meet_the_fp64_bar(K, agg):
    """Both edges of every K class, every operand, a partial chunk and two chunks + a tail."""
    worst, failures, outs = {}, [], {}
    for op, (bf16, _, _, _) in sc.OPERANDS.items():
        eps = sc.eps_tile(K, op, agg)
        for d in sc.small_ds(K, op):
            X = sc.operand_input(K, d, bf16)[0]
            w, g = make_operand(op, X), sc.guess_of(K, d, agg).cuda()
            ref = sc.reference(K, d, bf16, agg)
            tau = sc.tau_of(K, d, bf16) if agg == "cclip" else None
            for n in (sc.CCLIP_ITERS if agg == "cclip" else sc.NS):
                out = run(agg, w, g, n, tau)
                r = sc.worst_ratio(out.cpu().numpy(), *ref[n - 1], eps)
                key = f"K={K} agg={agg} op={op}"
                worst[key] = max(worst.get(key, 0.0), r)
                if r > 1.0:
                    failures.append((K, agg, op, d, n, r))
                if op in sc.BIT_EQUAL:
                    outs[(op, d, n)] = out
    _report("tiles", worst, failures)
    # across layouts: one kernel whatever the row stride; rows and panels where they run one
    # tile (test_gpu_panels.py: not at 32 < K <= 64 or 128 < K <= 256, and not where gm2 or
    # noiseless gm takes the 32-wave rows kernel)
    for (op, d, n), out in outs.items():
        if op == "padded":
            assert torch.equal(out, outs[("rows4", d, n)]), (K, agg, d, n, "padded")
        if (op == "panels" and agg != "cclip" and sc.same_tile(K)
                and not sc.takes_rows_kernel(K, agg)):
            assert torch.equal(out, outs[("rows4", d, n)]), (K, agg, d, n, "panels")


@pytest.mark.parametrize("K", sc.EDGE_K)
def test_fused_pre_oma_equals_oma_then_gm2(K):
    """gm2 with pre_oma_var on the INIT pass (mode 4) at every K class, d % 4 == 0, as
    test_pre_oma_equals_oma_then_gm2: the same noisy X bit for bit, the same aggregate, the
    same count; and that aggregate meets the bar on the noised matrix."""
    worst, failures = {}, []
    for op in ("rows4", "panels"):
        for d in sc.small_ds(K, op):
            X, g0 = sc.tile_input(K, d)
            g = g0.cuda()
            opts = {"maxiter": 2, "tol": -1.0, "guess": g, "algo": "stream"}
            A = make_operand(op, X)
            bz().OMA(A, sc.OMA_VAR, seed=sc.OMA_SEED)
            a = bz().gm2(A, dict(opts))
            ra = bz().aggregators.last_result
            B = make_operand(op, X)
            b = bz().gm2(B, dict(opts, pre_oma_var=sc.OMA_VAR, pre_oma_seed=sc.OMA_SEED))
            rb = bz().aggregators.last_result
            da, db = (A.data, B.data) if op == "panels" else (A, B)
            assert torch.equal(da, db), (K, op, d)
            assert torch.equal(a, b), (K, op, d)
            assert (ra.iters, ra.algo) == (rb.iters, rb.algo) == (2, "stream")
            noised = (B.to_rows() if op == "panels" else B).cpu()
            assert not torch.equal(noised, X)
            ref, scale = sc.engine(noised, g0, 2, "gm2")[1]
            r = sc.worst_ratio(b.cpu().numpy(), ref, scale, sc.eps_tile(K, op, "gm2"))
            key = f"K={K} agg=gm2+pre_oma op={op}"
            worst[key] = max(worst.get(key, 0.0), r)
            if r > 1.0 or not bool(torch.isfinite(b).all()):
                failures.append((K, op, d, r))
    _report("pre_oma", worst, failures)


@pytest.mark.parametrize("group", list(sc.MULTI_GROUPS))
@pytest.mark.parametrize("K", sc.MULTI_K)
def test_multi_chunk_loop_meets_the_bar(K, group):
    """Every block walks at least 3 chunks of the operand's own width J = LPR V (the rolling
    prefetch's prologue, steady state and epilogue): gm2 and cclip, n = 2, the same bar.  fp32
    rows and panels share one d (and their bits, where they share a tile); bf16 panels, twice
    as wide a chunk, have their own."""
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ops = sc.MULTI_GROUPS[group]
    d = sc.multi_d(K, ops[0], num_cu)
    X, g0 = sc.tile_input(K, d)
    bf16 = group == "bf16"
    if bf16:
        X = sc.widen_bf16(X)
    g = g0.cuda()
    tau = sc.cclip_tau(X, g0)
    refs = {agg: sc.engine(X, g0, 2, agg, bf16=bf16, tau=tau)[1] for agg in runner.AGGS}
    worst, failures, outs = {}, [], {}
    for op in ops:
        assert d == sc.multi_d(K, op, num_cu)
        J = sc.chunk(K, sc.OPERANDS[op][1], sc.OPERANDS[op][2])
        assert -(-d // J) >= 3 * num_cu * (32 // sc.tile(K, sc.OPERANDS[op][1])[0]) + 1
        w = make_operand(op, X)
        for agg in runner.AGGS:
            out = run(agg, w, g, 2, tau)
            outs[(op, agg)] = out
            r = sc.worst_ratio(out.cpu().numpy(), *refs[agg], sc.eps_tile(K, op, agg))
            worst[f"K={K} d={d} agg={agg} op={op}"] = r
            if r > 1.0:
                failures.append((K, d, agg, op, r))
        del w
    _report("multi", worst, failures)
    if group == "fp32" and sc.same_tile(K) and not sc.takes_rows_kernel(K, "gm2"):
        assert torch.equal(outs[("rows4", "gm2")], outs[("panels", "gm2")])


PROBE_D = 4100


@pytest.mark.parametrize("K", sc.PROBE_K)
def test_row_probes(K):
    """One row carries most of the weight (guess 1e-2 away from it), n = 1: that row's INIT
    distance decides the output.  Rows 0, NRG - 1, NRG, K - 1 of every tile involved."""
    worst, failures = {}, []
    for op in runner.OPS:
        bf16 = sc.OPERANDS[op][0]
        X, _ = sc.operand_input(K, PROBE_D, bf16)
        w = make_operand(op, X)
        eps = sc.PROBE_EPS(K, op, "gm2")
        for r in sc.probe_rows(K, op):
            g0 = sc.probe_guess(X, r)
            ref, scale = sc.engine(X, g0, 1, "gm2")[0]
            out = run("gm2", w, g0.cuda(), 1)
            ratio = sc.worst_ratio(out.cpu().numpy(), ref, scale, eps)
            worst[f"K={K} op={op} row={r}"] = ratio
            if ratio > 1.0:
                failures.append((K, op, r, ratio))
    _report("probe", worst, failures)


@pytest.mark.parametrize("agg", ["gm2", "gm"])
@pytest.mark.parametrize("K", sc.ROWS_KERNEL_K)
def test_rows_kernel_against_the_generic_tile(K, agg, monkeypatch):
    """gm2 and noiseless AirComp gm on rows with V = 4 at 512 < K <= 1024 take the 32-wave rows
    kernel for their STEP passes; with GMAGG_ROWS_LEAN=0 the generic tile runs: the same count,
    rel L2 <= 1e-6 (test_gpu_rows_pass.py), and the generic tile meets its own bar too.  The
    two kernels sum a column's rows in different orders, so at d = 4100 (as at d >= 4096 in
    test_gpu_rows_pass.py) some bits must differ: the witness that the default run did take the
    rows kernel and the comparison is not of the generic tile with itself."""
    worst, failures, differ = {}, [], {}
    for d in sc.small_ds(K, "rows4") + (PROBE_D,):
        X, g0 = sc.tile_input(K, d)
        w, g = make_operand("rows4", X), g0.cuda()
        ref = sc.reference(K, d, False, agg)
        for n in sc.NS:
            monkeypatch.delenv("GMAGG_ROWS_LEAN", raising=False)
            a = run(agg, w, g, n)
            monkeypatch.setenv("GMAGG_ROWS_LEAN", "0")
            b = run(agg, w, g, n)
            assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= 1e-6, (K, agg, d, n)
            differ[(d, n)] = not torch.equal(a, b)
            nw, lpr, rr, _ = sc.tile(K, False)
            eps = (rr + int(np.log2(64 // lpr)) + nw + sc.COEF_ULPS) * sc.U
            r = sc.worst_ratio(b.cpu().numpy(), *ref[n - 1], eps)
            key = f"K={K} agg={agg} op=rows4(generic)"
            worst[key] = max(worst.get(key, 0.0), r)
            if r > 1.0:
                failures.append((K, agg, d, n, r))
    _report("rows_lean0", worst, failures)
    print(f"rows kernel K={K} agg={agg}: bits differ from the generic tile's at {differ}")
    assert all(differ[(PROBE_D, n)] for n in sc.NS), differ


def test_schedule_variants_give_the_same_bits():
    """GMAGG_PASS_VARIANT = 0 (plain), 2 (rolling prefetch), 3 (two tiles rolled two chunks
    ahead; panels) against the default schedule on the reduced list: identical output bits,
    counts and movements.  One fresh process per variant (the variable is read once), one after
    the other; a child that dies or times out fails the test and no further one is started."""
    assert "GMAGG_PASS_VARIANT" not in os.environ
    base = runner.run_cases()
    assert len(base) == 2 * len(sc.MULTI_K) * len(runner.OPS) * len(runner.AGGS)
    for variant in (0, 2, 3):
        env = dict(os.environ, GMAGG_PASS_VARIANT=str(variant))
        try:
            p = subprocess.run([sys.executable, os.path.abspath(runner.__file__)], env=env,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"GMAGG_PASS_VARIANT={variant}: the runner did not finish in "
                        f"{CHILD_TIMEOUT} s")
        assert p.returncode == 0, (variant, p.returncode, p.stderr[-2000:])
        got = p.stdout.splitlines()
        diff = [(x, y) for x, y in zip(base, got) if x != y]
        assert len(got) == len(base) and not diff, (variant, len(got), diff[:4])
