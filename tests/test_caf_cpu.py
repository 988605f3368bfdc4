"""caf without a GPU: the two numpy routes of tests/caf_cases.py against each other (the K-space
identities on fp64 distances; the error of the emulated distances, from which the GPU bars are
derived), the preconditions of every GPU case, what the filter achieves on the planted cases,
the exports and binding, and what is refused before anything touches a device (Python and C ABI).
(The kernels themselves: tests/test_gpu_caf.py.)
"""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import caf_cases as cf
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import caf  # noqa: F401 - the file needs the feature
from byzantine_aircomp_amd import _lib, aggregators as agg


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a GPU context (or to stage a tensor) fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(agg, "context", boom)
    monkeypatch.setattr(agg, "_stage", boom)


@pytest.mark.parametrize("K,f,d,scale", [c + (1.0,) for c in cf.GPU_CASES + [(96, 19, 4099)]] +
                         [c + (1000.0,) for c in cf.SCALE_CASES])
def test_kspace_identities_on_fp64_distances(K, f, d, scale):
    """The identities, and the conditioning precondition of every case the GPU tests compare
    against the reference (caf_cases.py)."""
    X = cf.gpu_input(K, f, d, scale)
    ref = cf.gpu_reference(K, f, d, scale)
    got = cf.kspace_emulated(X, f, D=cf.dist64(X))
    ew, el, eo = cf.errors(got, ref)
    print(f"K={K} f={f} d={d}: c* {ew:.2e}, lambda {el:.2e}, out {eo:.2e}")
    assert (got["rounds"], got["best_round"]) == (ref["rounds"], ref["best_round"])
    assert got["power_iters"] == ref["power_iters"] and got["converged"] == ref["converged"]
    # (out is compared after its rounding to fp32: a sum within 1e-15 of a tie may round the other
    # way, 6e-8 of that element)
    assert ew <= 1e-10 and el <= 1e-9 and eo <= 1e-7


def test_bars_are_powers_of_ten():
    for tol in (cf.W_TOL, cf.LAM_TOL):
        assert abs(np.log10(tol) - round(np.log10(tol))) < 1e-12
    assert cf.OUT_TOL == 1e-5 and cf.GAP_MIN == 1e-2


@pytest.mark.parametrize("K,f,d", cf.GPU_CASES)
def test_gpu_cases_emulation_and_preconditions(K, f, d):
    """The bars leave the device a factor of ten over the emulated distances' own error, and the
    loop's condition is decided by far more than a weight error of W_TOL could move it."""
    X = cf.gpu_input(K, f, d)
    ref = cf.gpu_reference(K, f, d)
    emu = cf.kspace_emulated(X, f)
    ew, el, eo = cf.errors(emu, ref)
    print(f"K={K} f={f} d={d}: rounds {ref['rounds']} best {ref['best_round']} "
          f"min_gap {ref['min_gap']:.2e}; c* {ew:.2e}, lambda {el:.2e}, out {eo:.2e}")
    assert (emu["rounds"], emu["best_round"]) == (ref["rounds"], ref["best_round"])
    assert ew <= cf.W_TOL / 10 and el <= cf.LAM_TOL / 10 and eo <= cf.OUT_TOL / 10
    assert ref["min_gap"] >= cf.GAP_MIN
    assert 1 <= ref["rounds"] <= K and len(ref["power_iters"]) == ref["rounds"]
    # what the filter achieves: the planted rows' share of S*, and the distance to the honest mean
    assert cf.byzantine_share(ref["weights"], f) <= 1e-3
    x = X.astype(np.float64)
    honest = x[:K - f].mean(axis=0)
    e_caf = np.linalg.norm(ref["out"] - honest)
    e_mean = np.linalg.norm(x.mean(axis=0) - honest)
    print(f"  share {cf.byzantine_share(ref['weights'], f):.2e}, mean / caf error {e_mean / e_caf:.0f}")
    assert e_caf * 100 <= e_mean


@pytest.mark.parametrize("K,f,d", cf.SCALE_CASES)
def test_scaled_cases_preconditions(K, f, d):
    ref = cf.gpu_reference(K, f, d, 1000.0)
    assert ref["min_gap"] >= cf.GAP_MIN
    assert cf.byzantine_share(ref["weights"], f) <= 1e-3
    emu = cf.kspace_emulated(cf.gpu_input(K, f, d, 1000.0), f)
    ew, el, eo = cf.errors(emu, ref)
    print(f"scaled K={K}: c* {ew:.2e}, lambda {el:.2e}, out {eo:.2e}")
    assert (emu["rounds"], emu["best_round"]) == (ref["rounds"], ref["best_round"])
    assert eo <= cf.OUT_TOL / 10


def test_no_byzantine_rows_is_the_mean():
    X = cf.case(9, 2, 20)
    for route in (cf.reference, cf.kspace_emulated):
        ref = route(X, 0)
        assert ref["rounds"] == 0 and (ref["weights"] == 1).all() and ref["weight"] == 9
    want = (X.astype(np.float64).sum(axis=0) / 9).astype(np.float32)
    assert np.allclose(cf.reference(X, 0)["out"], want, rtol=0, atol=1e-9)


def test_all_rows_equal():
    # (8 rows: p_k = 1/8 and the d-space route's weighted mean are exact, so its centred rows are
    # exactly zero, as the K-space route's distances are for any K)
    X = np.tile(cf.case(2, 0, 30)[:1], (8, 1))
    for route in (cf.reference, cf.kspace_emulated):
        ref = route(X, 2)
        assert ref["rounds"] == 1 and ref["eigenvalue"] == 0 and ref["power_iters"] == [0]
        assert ref["converged"] == [True]
        assert np.array_equal(ref["out"].view(np.int32), X[0].view(np.int32))


def test_nan_ends_round_zero():
    X = np.array(cf.case(17, 3, 100))
    X[4, 7] = np.nan
    for route in (cf.reference, cf.kspace_emulated):
        ref = route(X, 3)
        assert ref["rounds"] == 0 and (ref["weights"] == 1).all()
        assert np.isnan(ref["out"][7]) and np.isfinite(np.delete(ref["out"], 7)).all()


def test_exported_and_bound():
    assert bz.caf is agg.caf and "caf" in agg.__all__
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert {"gm_caf_f32", "gm_weighted_mean_f32"} <= bound
    assert _lib.ABI_VERSION == 5 and _lib.load().gm_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"gm_caf_f32", "gm_weighted_mean_f32"} <= syms      # C linkage: the plain names


def test_abi_argument_checks():
    """No device needed: every refusal happens before the first HIP call (the context pointer
    is only handed on, never read, before the checks pass)."""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    R, P = _lib.GM_LAYOUT_ROWS, _lib.GM_LAYOUT_PANELS
    ok = dict(ctx=p, X=p, K=8, d=4, ldx=4, layout=R, f=2, pit=100, ptol=1e-10, out=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gm_caf_f32(a["ctx"], a["X"], a["K"], a["d"], a["ldx"], a["layout"], a["f"],
                              a["pit"], a["ptol"], a["out"], None, None, None, None, None, None,
                              None, None)

    def refused(rc_, code):
        assert rc_ == code
        assert b"gm_caf_f32" in lib.gm_last_error()

    for kw in (dict(ctx=None), dict(X=None), dict(out=None), dict(K=1, f=0), dict(d=-1),
               dict(f=-1), dict(f=4), dict(K=7, f=4), dict(layout=7), dict(ldx=3), dict(pit=0),
               dict(ptol=-1.0), dict(ptol=float("nan")),
               dict(layout=P, ldx=8 * lib.gm_panel_width(8) - 1)):
        refused(call(**kw), -1)
    refused(call(K=4097), -3)
    refused(call(K=4096, layout=P, ldx=1 << 30), -3)            # no panel width
    assert lib.gm_weighted_mean_f32(p, p, 4097, 4, 4, R, p, p, None) == -3
    for args in ((None, p, 8, 4, 4, R, p, p), (p, None, 8, 4, 4, R, p, p),
                 (p, p, 8, 4, 4, R, None, p), (p, p, 8, 4, 4, R, p, None), (p, p, 0, 4, 4, R, p, p),
                 (p, p, 8, 4, 3, R, p, p), (p, p, 8, 4, 4, 9, p, p)):
        assert lib.gm_weighted_mean_f32(*args, None) == -1
        assert b"gm_weighted_mean_f32" in lib.gm_last_error()


def test_python_refusals(no_device):
    X = torch.zeros(12, 5)
    opts = {"honestSize": 9}
    for bad in (X.to(torch.bfloat16), X.double()):
        with pytest.raises(TypeError):
            bz.caf(bad, opts)
    with pytest.raises(ValueError):
        bz.caf(torch.zeros(12), opts)
    for o in ({}, None, {"honestSize": None}, {"power_iters": 3}):
        with pytest.raises(ValueError, match="honestSize"):
            bz.caf(X, o)
    for hs in (0, 13):
        with pytest.raises(ValueError, match="honestSize"):
            bz.caf(X, {"honestSize": hs})
    for hs in (6, 5, 1):                                        # 2f >= K
        with pytest.raises(ValueError, match="2f"):
            bz.caf(X, {"honestSize": hs})
    with pytest.raises(ValueError, match="K >= 2"):
        bz.caf(torch.zeros(1, 2), {"honestSize": 1})
    with pytest.raises(ValueError, match="4096"):
        bz.caf(torch.zeros(4097, 2), {"honestSize": 4000})
    with pytest.raises(ValueError, match="power_iters"):
        bz.caf(X, dict(opts, power_iters=0))
    with pytest.raises(ValueError, match="power_tol"):
        bz.caf(X, dict(opts, power_tol=-1e-3))


def test_with_options(no_device, monkeypatch):
    f = bz.caf.with_options(power_iters=7)
    assert f.__name__ == "caf" and f.__qualname__ == "caf"
    with pytest.raises(TypeError, match="honestSize"):
        bz.caf.with_options(honestSize=3)
    with pytest.raises(ValueError, match="power_iters"):
        bz.caf.with_options(power_iters=0)
    seen = {}
    monkeypatch.setattr(agg, "caf", lambda w, o: seen.update(w=w, o=o) or "out")
    X = torch.zeros(12, 5)
    opts = {"honestSize": 9, "power_iters": 50, "maxiter": 3}
    keep = dict(opts)
    assert f(X, opts) == "out" and opts == keep
    assert seen["o"] == {"honestSize": 9, "power_iters": 7, "maxiter": 3}
    assert bz.bucketed(bz.caf, 2).__name__ == "caf_b2"
    assert bz.mixed(bz.caf).__name__ == "caf_nnm"
