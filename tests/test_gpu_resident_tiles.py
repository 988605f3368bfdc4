"""Every tile, vector width, CPB and exchange of the single-problem register-resident kernel
(csrc/resident.hip) and every row tile, layout and gather of the batched one
(csrc/resident_batched.hip) against the fp64 references of tests/resident_cases.py, whose
docstring restates the host's plan, states the inputs, derives the per-element bar
|got_j - ref_j| <= eps * scale_j and lists the mutations the bar is there to catch
(tests/test_resident_cases_cpu.py holds each of them to missing it by 8x).

Every call passes algo="resident" and tol = -1 (exactly n bodies, n = 1 .. 4: body 3 is the
first that reads a granule buffer's second occupant, body 4 the other buffer's) and must
report the resident path, n iterations and a finite result; every element of every case is
compared.  Row-major views sit in NaN-filled buffers and the panels' padding columns hold a
sentinel, so a read past d shows.  Each case prints its worst |got - ref| / (eps * scale)
("RATIO ..."); DESIGN.md §3.3 and §3.6 record them."""
import os
import re
import subprocess
import sys

import pytest
import torch

import resident_cases as rc
import resident_plan_runner as plan_runner
import stream_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = 7.0                 # in the panels' padding columns
CHILD_TIMEOUT = 240            # seconds for the plan runner (its list takes ~10 s)


def bz():
    import byzantine_aircomp_amd as m
    return m


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _report(what, worst, failures):
    for key, r in sorted(worst.items()):
        print(f"RATIO {what} {key} worst={r:.3f}")
    assert not failures, failures[:20]


# ---------------------------------------------------------------------------- single problem

def make_operand(op, X):
    """The fp32 CPU matrix X on the GPU as operand `op` of resident_cases.OPERANDS, its padding
    poisoned."""
    K, d = X.shape
    Xt = X.cuda()
    if rc.OPERANDS[op][0]:
        P = bz().ClientPanels.from_rows(Xt)
        rem = d - (P.npan - 1) * P.W
        if rem < P.W:
            P.data[-1, :, rem:] = SENTINEL
        return P

    def view(width, off):
        buf = torch.full((K, width), float("nan"), device="cuda")
        buf[:, off:off + d] = Xt
        return buf[:, off:off + d]

    if op == "misaligned":
        w = view(d + 4, 1)
        assert w.data_ptr() % 16 == 4 and w.stride(0) == d + 4
    elif op == "padded":
        w = view(d + 4, 0)
        assert w.data_ptr() % 16 == 0 and w.stride(0) % 4 == 0
    else:                        # contiguous rows between two NaN rows
        buf = torch.full((K + 2, d), float("nan"), device="cuda")
        buf[1:K + 1] = Xt
        w = buf[1:K + 1]
        assert w.is_contiguous() and d % 4 == {"rows4": 0, "rows2": 2}.get(op, d % 4)
    return w


def run_single(agg, w, g, n, seed=rc.GM_SEED):
    opts = {"maxiter": n, "tol": -1.0, "guess": g, "algo": "resident"}
    if agg != "gm2":
        opts.update(noise_var=rc.GM_NOISE_VAR if agg == "gm_noise" else None, P_max=1, seed=seed)
    out = (bz().gm2 if agg == "gm2" else bz().gm)(w, opts)
    res = bz().aggregators.last_result
    assert res.algo == "resident" and res.iters == n, (agg, res)
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all()), agg
    return out, res


def single_reference(K, op, d, agg):
    """(X, guess, key, reference) of one case; operands of one (V, d) share input and reference."""
    X, g0, JB, _ = rc.single_case(K, op, d)
    g0 = rc.guess_for(K, d, agg, g0)
    seed = rc.gm_seed_for(X, g0, agg, JB)
    ref = rc.reference((K, rc.OPERANDS[op][1], d, agg), X, g0, agg, JB, seed=seed)
    return X, g0, seed, ref


def check_single(K, op, d, agg, worst, failures, key, outs=None, exchange=None):
    X, g0, seed, ref = single_reference(K, op, d, agg)
    w, g = make_operand(op, X), g0.cuda()
    eps = rc.eps_single(K, agg)
    for n in rc.NS:
        out, res = run_single(agg, w, g, n, seed)
        if exchange is not None:
            assert res.exchange == exchange, (K, op, d, agg, n, res)
        r = sc.worst_ratio(out.cpu().numpy(), *ref[n - 1], eps)
        worst[key] = max(worst.get(key, 0.0), r)
        if not r <= 1.0:
            failures.append((K, agg, op, d, n, r))
        if outs is not None:
            outs[(op, d, n)] = out


@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K", rc.EDGE_K)
def test_single_tiles_meet_the_fp64_bar(K, agg):
    """Both edges of every K class with a kernel, every operand, and per operand the shapes
    that land on one partial chunk, 32 one-chunk blocks, every further CPB of the tile and a
    grid beyond one XCD; the multi-block inputs graded block by block (mutations f - j)."""
    worst, failures, outs = {}, [], {}
    for op, (panels, V, _) in rc.OPERANDS.items():
        if panels and K > rc.PANEL_K_MAX:
            continue
        for which, d in rc.single_ds(K, op, num_cu()).items():
            check_single(K, op, d, agg, worst, failures, f"K={K} agg={agg} op={op}", outs)
    _report("single", worst, failures)
    for (op, d, n), out in outs.items():          # one kernel whatever the row stride
        if op == "padded":
            assert torch.equal(out, outs[("rows4", d, n)]), (K, agg, d, n)


@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K", [33, 50, 64])
def test_exchanges_of_the_8_wave_tile(K, agg, monkeypatch):
    """xcd_local (32 blocks on one XCD), xcd_split and, under GMAGG_RES_SPLIT=0, the flat agent
    gather (a grid beyond one XCD; the two bit-identical), and xcd_hier under GMAGG_RES_HIER=2
    at nb = 33, 39, 40 (nb mod 8 = 1, 7, 0) and by default at 190 blocks, where the halving
    rule has applied: each reported as such and within the bar."""
    for v in ("GMAGG_RES_HIER", "GMAGG_RES_SPLIT", "GMAGG_RES_XCD", "GMAGG_RES_CPB"):
        monkeypatch.delenv(v, raising=False)
    worst, failures, a, b = {}, [], {}, {}
    ds = rc.single_ds(K, "rows4", num_cu())
    nb = rc.resident_plan(K, 4, ds["beyond"])[1]
    key = f"K={K} agg={agg}"
    check_single(K, "rows4", ds["x32"], agg, worst, failures, key + " xcd_local",
                 exchange="xcd_local")
    assert rc.exchange_of(K, nb, num_cu()) == "xcd_split"
    check_single(K, "rows4", ds["beyond"], agg, worst, failures, key + " xcd_split", a,
                 exchange="xcd_split")
    monkeypatch.setenv("GMAGG_RES_SPLIT", "0")
    check_single(K, "rows4", ds["beyond"], agg, worst, failures, key + " agent", b,
                 exchange="agent")
    monkeypatch.delenv("GMAGG_RES_SPLIT")
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    for nb in rc.HIER_NB if K == 50 else rc.HIER_NB[:1]:
        d = rc.hier_d(nb)
        assert rc.resident_plan(K, 4, d)[1] == nb
        if nb < 90:
            monkeypatch.setenv("GMAGG_RES_HIER", "2")
        check_single(K, "rows4", d, agg, worst, failures, key + f" xcd_hier nb={nb}",
                     exchange="xcd_hier")
        monkeypatch.delenv("GMAGG_RES_HIER", raising=False)
    _report("exchange", worst, failures)


@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K", [16, 50])
def test_forced_cpb_3(K, agg, monkeypatch):
    """CPB = 3, which the plan never picks, exists behind GMAGG_RES_CPB (read per call): V = 1,
    17 blocks of 3 x 64 columns and a ragged tail, the input graded on those blocks.  (The
    variable only selects among the instantiated kernels; that CPB 3 ran is not asserted.)"""
    assert rc.res_cpb_ok(1, rc.resident_tile(K), 3)
    monkeypatch.setenv("GMAGG_RES_CPB", "3")
    JB = 3 * 64
    d = 16 * JB + 2 * 64 + 37
    X, g0 = rc.block_input(K, d, JB)
    seed = rc.gm_seed_for(X, g0, agg, JB)
    ref = rc.reference(("cpb3", K, d, agg), X, g0, agg, JB, seed=seed)
    w, g = make_operand("rows1", X), g0.cuda()
    worst, failures = {}, []
    for n in rc.NS:
        out, _ = run_single(agg, w, g, n, seed)
        r = sc.worst_ratio(out.cpu().numpy(), *ref[n - 1], rc.eps_single(K, agg))
        worst[f"K={K} agg={agg} CPB=3"] = max(worst.get(f"K={K} agg={agg} CPB=3", 0.0), r)
        if not r <= 1.0:
            failures.append((K, agg, d, n, r))
    _report("cpb3", worst, failures)


PROBE_K = [16, 32, 50, 100, 200, 300, 2048]      # one K per resident tile


@pytest.mark.parametrize("K", PROBE_K)
def test_single_row_probes(K):
    """One row carries most of the weight (guess 1e-2 away from it), n = 1: that row's INIT
    distance decides the output.  Rows 0, NRG - 1, NRG, K - 1; V = 4, V = 1 and panels."""
    worst, failures = {}, []
    for op in ("rows4", "rows1", "panels"):
        panels, V, (mod, res) = rc.OPERANDS[op]
        if panels and K > rc.PANEL_K_MAX:
            continue
        d = rc._fit(1030, mod, res)
        X, _, _, _ = rc.single_case(K, op, d)
        w = make_operand(op, X)
        eps = rc.eps_single(K, "gm2")
        for r in rc.probe_rows(K):
            g0 = sc.probe_guess(X, r)
            ref, scale = rc.engine(X, g0, 1, "gm2", d)[0]
            out, _ = run_single("gm2", w, g0.cuda(), 1)
            ratio = sc.worst_ratio(out.cpu().numpy(), ref, scale, eps)
            worst[f"K={K} op={op} row={r}"] = ratio
            if not ratio <= 1.0:
                failures.append((K, op, r, ratio))
    _report("probe", worst, failures)


@pytest.mark.parametrize("K", rc.DECLINE_K)
def test_the_class_without_a_resident_tile_declines(K):
    """512 < K <= 1024 runs the (8,8,16) streaming tile, which has no resident instantiation:
    AUTO streams a small problem and an explicit algo="resident" raises."""
    X, g0 = sc.tile_input(K, 64)
    Xd, g = X.cuda(), g0.cuda()
    bz().gm2(Xd, {"maxiter": 2, "tol": -1.0, "guess": g})
    assert bz().aggregators.last_result.algo == "stream"
    with pytest.raises(RuntimeError):
        bz().gm2(Xd, {"maxiter": 2, "tol": -1.0, "guess": g, "algo": "resident"})


def test_every_case_runs_the_plan_it_was_written_for():
    """A fresh process under GMAGG_RES_VERBOSE=1 (read once per process) runs every shape of
    the tile test; the nb and stride the library reports per launch equal the restated plan's,
    so each case did run its CPB and its placement."""
    env = dict(os.environ, GMAGG_RES_VERBOSE="1")
    for v in ("GMAGG_RES_HIER", "GMAGG_RES_SPLIT", "GMAGG_RES_XCD", "GMAGG_RES_CPB"):
        env.pop(v, None)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(plan_runner.__file__)], env=env,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the plan runner did not finish in {CHILD_TIMEOUT} s")
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    cases = plan_runner.cases(num_cu())
    assert int(p.stdout.split()[-1]) == len(cases)
    lines = [ln for ln in p.stderr.splitlines()
             if ln.startswith("CASE ") or ln.startswith("gmagg resident")]
    assert len(lines) == 2 * len(cases), (len(lines), len(cases), lines[:6])
    cpbs = set()
    for (K, op, which, d), head, rep in zip(cases, lines[0::2], lines[1::2]):
        assert head == f"CASE {K} {op} {which} {d}", (head, K, op, which, d)
        m = re.match(r"gmagg resident: nb=(\d+) stride=(\d+) .*timed_out=0", rep)
        assert m, (head, rep)
        cpb, nb = rc.resident_plan(K, rc.OPERANDS[op][1], d)
        want = (nb, rc.res_xcd_stride(nb, num_cu()))
        assert (int(m.group(1)), int(m.group(2))) == want, (head, rep)
        cpbs.add(cpb)
    assert cpbs == {1, 2, 4, 8}


# ----------------------------------------------------------------------------------- batched

def rb_operand(layout, Xs):
    """The fp32 CPU problems Xs (a list of [K, d]) on the GPU: 16-byte aligned rows as a
    [P, K, d] view of a NaN-filled [P, K, d rounded up to 4, + 4] buffer, or ProblemPanels with
    the sentinel in their padding columns."""
    from byzantine_aircomp_amd.batched import ProblemPanels
    X = torch.stack(Xs).cuda()
    P, K, d = X.shape
    if layout == "panels":
        pp = ProblemPanels.from_rows(X)
        rem = d - (pp.npan - 1) * pp.W
        if rem < pp.W:
            pp.data[:, -1, :, rem:] = SENTINEL
        return pp
    buf = torch.full((P, K, -(-d // 4) * 4 + 4), float("nan"), device="cuda")
    buf[:, :, :d] = X
    w = buf[:, :, :d]
    assert w.data_ptr() % 16 == 0 and w.stride(1) % 4 == 0 and w.stride(0) % 4 == 0
    return w


def run_batched(agg, w, g, n, seed=rc.GM_SEED, algo="resident", **extra):
    from byzantine_aircomp_amd.batched import gm2_batched, gm_batched
    opts = dict({"maxiter": n, "tol": -1.0, "guess": g, "algo": algo}, **extra)
    if agg != "gm2":
        opts.update(noise_var=rc.GM_NOISE_VAR if agg == "gm_noise" else None, P_max=1, seed=seed)
    out, res = (gm2_batched if agg == "gm2" else gm_batched)(w, opts)
    if algo == "resident":
        assert all(r.algo == "resident" and r.iters == n for r in res), (agg, res[0])
        assert bool(torch.isfinite(out).all()), agg
    return out, res


def rb_problems(K, d, P, agg, n=max(rc.NS)):
    """([X_q], [guess_q], key): P distinct problems and the batch's Philox key (for n bodies)."""
    probs = [rc.block_input(K, d, rc.RB_COLS, q) for q in range(P)]
    Xs = [p[0] for p in probs]
    gs = [rc.guess_for(K, d, agg, p[1]) for p in probs]
    return Xs, gs, rc.gm_seed_for(Xs, gs, agg, rc.RB_COLS, n=n)


def check_batched(K, d, P, agg, layouts, ns, worst, failures, key, bodies=max(rc.NS)):
    Xs, gs, seed = rb_problems(K, d, P, agg, bodies)
    refs = [rc.reference(("rb", K, d, q, agg, bodies), Xs[q], gs[q], agg, rc.RB_COLS,
                         seed=rc.batched_seed(q, seed), n=bodies) for q in range(P)]
    g = torch.stack(gs).cuda()
    eps = rc.eps_batched(K, agg)
    outs = {}
    for layout in layouts:
        w = rb_operand(layout, Xs)
        for n in ns:
            out, _ = run_batched(agg, w, g, n, seed)
            outs[(layout, n)] = out
            for q in range(P):
                r = sc.worst_ratio(out[q].cpu().numpy(), *refs[q][n - 1], eps)
                worst[key] = max(worst.get(key, 0.0), r)
                if not r <= 1.0:
                    failures.append((K, d, agg, layout, n, q, r))
        del w
    return outs


@pytest.mark.parametrize("agg", rc.AGGS)
@pytest.mark.parametrize("K", rc.RB_K)
def test_batched_tiles_meet_the_fp64_bar(K, agg):
    """Both edges of every row tile (16, 32, 32 + 18, 36 + 16 rows), rows and panels, a partial
    float4 group, one block and three blocks (block-graded), P = 3 distinct problems each held to
    the bar; the two layouts bit-identical.  gm at K = 51, 52 has no kernel: AUTO streams."""
    worst, failures = {}, []
    if rc.rb_plan(K, 1, agg) is None:
        Xs, gs, seed = rb_problems(K, rc.RB_DS[0], rc.RB_P, agg)
        _, res = run_batched(agg, rb_operand("rows", Xs), torch.stack(gs).cuda(), 2, seed,
                             algo="auto")
        assert all(r.algo == "stream" for r in res), res[0]
        return
    for d in rc.RB_DS:
        outs = check_batched(K, d, rc.RB_P, agg, ("rows", "panels"), rc.NS, worst, failures,
                             f"K={K} agg={agg}")
        for n in rc.NS:
            assert torch.equal(outs[("rows", n)], outs[("panels", n)]), (K, agg, d, n)
    _report("batched", worst, failures)


@pytest.mark.parametrize("K", [17, 50, 52])
def test_batched_row_probes(K):
    """Rows 0, 15, 16, KV - 1, KV and K - 1 (the last register row and the first LDS row where
    K > KV): one problem per probed row, the same X with the guess 1e-2 away from that row,
    n = 1, three blocks."""
    worst, failures = {}, []
    d = rc.RB_DS[2]
    X, _ = rc.block_input(K, d, rc.RB_COLS)
    rows = rc.rb_probe_rows(K)
    gs = [sc.probe_guess(X, r) for r in rows]
    eps = rc.eps_batched(K, "gm2")
    for layout in ("rows", "panels"):
        out, _ = run_batched("gm2", rb_operand(layout, [X] * len(rows)), torch.stack(gs).cuda(), 1)
        for q, r in enumerate(rows):
            ref, scale = rc.engine(X, gs[q], 1, "gm2", rc.RB_COLS)[0]
            ratio = sc.worst_ratio(out[q].cpu().numpy(), ref, scale, eps)
            worst[f"K={K} {layout} row={r}"] = ratio
            if not ratio <= 1.0:
                failures.append((K, layout, r, ratio))
    _report("batched_probe", worst, failures)


@pytest.mark.parametrize("K", [16, 50, 52])
def test_batched_fused_prenoise(K):
    """gm2 with pre_oma_var: the noised matrix equals oma_batched's bit for bit, in either
    layout, and the aggregate meets the bar on the noised matrix."""
    from byzantine_aircomp_amd.batched import ProblemPanels, oma_batched
    worst, failures = {}, []
    for d in (rc.RB_DS[0], rc.RB_DS[2]):
        Xs, gs, _ = rb_problems(K, d, rc.RB_P, "gm2")
        g = torch.stack(gs).cuda()
        for layout in ("rows", "panels"):
            A, B = rb_operand(layout, Xs), rb_operand(layout, Xs)
            out, _ = run_batched("gm2", A, g, 2, pre_oma_var=rc.OMA_VAR, pre_oma_seed=rc.OMA_SEED)
            oma_batched(B, rc.OMA_VAR, seed=rc.OMA_SEED)
            ra, rb = ((t.to_rows() if isinstance(t, ProblemPanels) else t).cpu() for t in (A, B))
            assert torch.equal(ra, rb), (K, d, layout)
            for q in range(rc.RB_P):
                assert not torch.equal(ra[q], Xs[q])
                ref, scale = rc.engine(ra[q].contiguous(), gs[q], 2, "gm2", rc.RB_COLS)[1]
                r = sc.worst_ratio(out[q].cpu().numpy(), ref, scale, rc.eps_batched(K, "gm2"))
                key = f"K={K} agg=gm2+pre_oma {layout}"
                worst[key] = max(worst.get(key, 0.0), r)
                if not r <= 1.0:
                    failures.append((K, d, layout, q, r))
    _report("batched_pre_oma", worst, failures)


# (K, aggregator, problems, bodies): the small row tile with 7 problems (NG = 1 or 3 groups of
# num_cu / 2 + 1 blocks at one or two blocks per CU: every group runs a second and a third
# problem on one running pass counter, mutation i); K = 50 with 3 problems and 2 bodies (its
# 18 LDS rows x 512 threads x 16 B = 144 KiB leave one block per CU: NG = 1).  gm without its
# noise: problem q's channel draws are keyed seed + q SEED_STRIDE; at this d the receiver's
# noise outweighs s sum_k gain_k / dist_k and no key keeps seven problems' normalisers from
# cancelling (resident_cases.gm_seed_for)
GROUP_CASES = [(16, "gm2", 7, 3), (16, "gm", 7, 3), (50, "gm2", 3, 2)]


def check_groups(K, agg, P, n, worst, failures, what):
    nb, _ = rc.rb_group_shape(num_cu())
    d = nb * rc.RB_COLS - 1000
    assert rc.rb_plan(K, d, agg)[2] == nb and (K == 50 or P > 2 * (2 * num_cu() // nb))
    check_batched(K, d, P, agg, ("panels",), (n,), worst, failures, f"{what} K={K} agg={agg} P={P}",
                  bodies=n)


@pytest.mark.parametrize("K,agg,P,n", GROUP_CASES)
def test_batched_several_problems_per_group(K, agg, P, n):
    worst, failures = {}, []
    check_groups(K, agg, P, n, worst, failures, "flat")
    _report("batched_groups", worst, failures)


@pytest.mark.parametrize("knob", ["GMAGG_RB_HIER=1", "GMAGG_RB_XCD=2"])
def test_batched_short_list_under_the_gather_knobs(knob, monkeypatch):
    """The hierarchical group gather (reported as xcd_hier) and whole groups per XCD: the three
    block shapes at K = 16 and K = 50 (gm2 and gm with noise) and the several-problems-per-group
    case, the same bar."""
    name, value = knob.split("=")
    monkeypatch.setenv(name, value)
    worst, failures = {}, []
    for K in (16, 50):
        for agg in ("gm2", "gm_noise"):
            for d in rc.RB_DS:
                check_batched(K, d, rc.RB_P, agg, ("panels",), (2, 4), worst, failures,
                              f"{knob} K={K} agg={agg}")
    Xs, gs, _ = rb_problems(16, rc.RB_DS[2], rc.RB_P, "gm2")
    _, res = run_batched("gm2", rb_operand("panels", Xs), torch.stack(gs).cuda(), 1)
    assert (res[0].exchange == "xcd_hier") == (name == "GMAGG_RB_HIER"), res[0]
    check_groups(16, "gm2", 7, 3, worst, failures, knob)
    _report("batched_knobs", worst, failures)
