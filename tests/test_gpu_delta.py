"""gm2 on fp32 panels with late STEP passes run as corrections on a bf16 shadow of X
(csrc/stream_pass_kernel.h DELTA, csrc/weiszfeld.hip kspace_gm2_delta).

GMAGG_DELTA is read once per process, so tests/delta_runner.py runs once with GMAGG_DELTA=1 (the
path at any size) and once with 0, each in a fresh process, and the tests compare what they saved:

  * Shapes K = 513, 1000, 1024; d = 20 (one partial chunk), 84 (two chunks and a partial third),
    4100 (a chunk per block and a tail) and, at K = 1000, a width at which every block of either
    kind of pass walks at least three chunks (delta_cases.multi_d).  Inputs: the flagship
    benchmark's recipe (delta_cases.bench_input, guess_of).
  * Exactly 3, 4 and 5 bodies (tol = -1): every element within eps_tile scale_j of the exact fp64
    loop (stream_cases.engine; eps_tile and scale_j as tests/test_gpu_stream_tiles.py has them),
    at least one correction pass, and the kinds of pass the fp64 model of the guard takes.
  * The run to convergence: at least one correction pass, the knob-off run's count, and
    rel L2 <= 1e-5 against oracle.gm2.
  * stream_cases.tile_input from its row-probe guess, where the coefficients move by 0.5 and more
    per body (from tile_input's own guess the third body's move is 2e-4 at d = 4100, inside
    theta): no correction pass, and the output's bits, the count and the movement equal the
    knob-off run's.
  * Two ranks over gloo on one GPU: the same count, kinds of pass and movement on both.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import delta_cases as dc
import stream_cases as sc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RUNNER = os.path.join(HERE, "delta_runner.py")


def _env(knob):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["GMAGG_DELTA"] = knob
    return env


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{knob: the arrays delta_runner.py saved}, one child process per knob value."""
    out = {}
    for knob in ("1", "0"):
        path = str(tmp_path_factory.mktemp("delta") / f"knob{knob}.npz")
        p = subprocess.run([sys.executable, RUNNER, "cases", path], env=_env(knob),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        out[knob] = dict(np.load(path))
    return out


def _meta(run, key):
    it, mv, ncorr, mask, status = run[key + "/meta"]
    return int(it), float(mv), int(ncorr), int(mask), int(status)


def _shapes():
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count \
        if torch.cuda.is_available() else 256
    return dc.gpu_shapes(num_cu)


_REFS = {}


def _ref(K, d):
    """[(iterate, scale)] of the exact fp64 loop for bodies 1 .. 5, computed once per shape."""
    if (K, d) not in _REFS:
        X, g = dc.bench_input(K, d)[0], dc.guess_of(K, d)
        # (with tol = -1 the model's kinds for n bodies are the first n of those for 5)
        _REFS[(K, d)] = (dc.exact(X, g, max(dc.NS)), dc.model(X, g, max(dc.NS))[1])
    return _REFS[(K, d)]


@pytest.mark.parametrize("n", dc.NS)
@pytest.mark.parametrize("K,d", _shapes())
def test_n_bodies_hold_the_bar_with_corrections(runs, K, d, n):
    key = f"n{n}/{K}/{d}"
    it, _, ncorr, mask, status = _meta(runs["1"], key)
    ref, scale = _ref(K, d)[0][n - 1]
    eps = sc.eps_tile(K, "panels", "gm2")
    worst = sc.worst_ratio(runs["1"][key + "/out"], ref, scale, eps)
    worst0 = sc.worst_ratio(runs["0"][key + "/out"], ref, scale, eps)
    kinds = _ref(K, d)[1][:n]
    print(f"K={K} d={d} n={n} mask={mask:#x} model={kinds} worst={worst:.3f} knob-off={worst0:.3f}")
    assert status == 1 and it == n
    assert ncorr >= 1 and ncorr == bin(mask).count("1"), "no correction pass ran"
    assert mask == dc.mask_of(kinds), (mask, kinds)
    assert _meta(runs["0"], key)[2:] == (0, 0, 0)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("K,d", _shapes())
def test_converged_run(runs, K, d):
    from oracle import aggregators as orc
    key = f"conv/{K}/{d}"
    it, mv, ncorr, mask, status = _meta(runs["1"], key)
    it0, mv0, ncorr0, _, _ = _meta(runs["0"], key)
    X, g0 = dc.bench_input(K, d)
    want, _ = orc.gm2(X.clone(), {"maxiter": 100, "tol": dc.conv_tol(d), "guess": g0})
    rel = rel_l2(runs["1"][key + "/out"], want.numpy())
    print(f"K={K} d={d} iters={it} (knob off {it0}) mask={mask:#x} rel_l2={rel:.2e} "
          f"movement={mv:.3e} (knob off {mv0:.3e})")
    assert status == 1 and ncorr >= 1, "no correction pass ran"
    assert ncorr0 == 0 and it == it0
    assert rel <= 1e-5, rel


@pytest.mark.parametrize("K", dc.KS)
def test_guard_refuses_moving_coefficients(runs, K):
    key = f"refuse/{K}/4100"
    on, off = runs["1"], runs["0"]
    it, mv, ncorr, mask, status = _meta(on, key)
    it0, mv0, _, _, _ = _meta(off, key)
    assert status == 1 and ncorr == 0 and mask == 0
    assert (it, mv) == (it0, mv0) and it == 3
    assert on[key + "/out"].tobytes() == off[key + "/out"].tobytes()


def test_two_ranks_take_the_same_passes(tmp_path):
    procs, paths = [], []
    for r in range(2):
        env = _env("1")
        env.update(RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29571")
        paths.append(str(tmp_path / f"rank{r}.json"))
        procs.append(subprocess.Popen([sys.executable, RUNNER, "shard", paths[-1]], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=240) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-2000:] for o in outs]
    a, b = (json.load(open(p)) for p in paths)
    print(a, b)
    assert a["lo"] == 0 and 0 < a["hi"] == b["lo"] < b["hi"] == 4100
    assert a["shadow"] == b["shadow"] == "armed" and a["corrections"] >= 1
    assert all(a[k] == b[k] for k in ("iters", "mask", "corrections", "movement"))
    kinds = dc.model(*dc.bench_input(1000, 4100), 100, tol=dc.conv_tol(4100))[1]
    assert a["iters"] == len(kinds) and a["mask"] == dc.mask_of(kinds), (a, kinds)
