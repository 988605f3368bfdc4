"""Centered clipping, the parts that need no GPU: the test inputs' margins (what makes the
GPU bar and the asserted clipped counts well posed), the ABI additions, and the option
checks that run before any GPU is touched."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import cclip_cases as cc
from conftest import ROOT
from byzantine_aircomp_amd import _lib

CASES = [(K, d, "fp32") for K, d in cc.SHAPES] + [(K, d, "bf16") for K, d in cc.SHAPES]


@pytest.mark.parametrize("K,d,dtype", CASES)
def test_restatement_margin_and_clipped_counts(K, d, dtype):
    """On every test input, radius and iteration count: the fp32 restatement in the kernels'
    form stays within 1e-6 of the fp64 reference (the GPU bar of 1e-5 is not set by the
    inputs), the clipped counts at the guess are the asserted ones, and no client sits near
    the radius at any iteration the GPU tests read a count from."""
    X, g0 = cc.inputs(K, d, dtype)
    X32 = X.float().numpy()
    for name in cc.TAUS:
        tau = cc.tau_of(name, d)
        vs, clipped, moves, margins = cc.ref_case(K, d, dtype, name)
        rs = cc.restatement(X32, g0.numpy(), tau, cc.MAX_ITERS)
        for it in cc.ITERS:
            rel = cc.rel_l2(rs[it - 1], vs[it - 1])
            print(f"cclip {K}x{d} {dtype} tau={name} iters={it}: restatement rel_l2={rel:.3e} "
                  f"clipped={clipped[:it]} margin={min(margins[:it]):.3f}")
            assert rel <= cc.RESTATEMENT_TOL
        assert clipped[0] == cc.initial_clipped(name, K)
        assert margins[0] >= 0.7          # every initial dist_k / tau at least 0.7 from 1
        # later iterations: far more than any fp32 / fp64 difference in dist_k could bridge
        assert min(margins) >= 0.5, margins


def test_library_exports_cclip():
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("gm_cclip_f32", "gm_cclip_bf16"):
        assert hasattr(lib, name) and name in syms
        assert getattr(lib, name)(None, None, 0, 0, 0, None, None, None, None, None) == -1
        assert name.encode() in lib.gm_last_error() and b"NULL" in lib.gm_last_error()


def test_cclip_struct_layouts_match_header(tmp_path):
    """ctypes' view of gm_cclip_opts / gm_cclip_result == the C compiler's: field order,
    offsets and sizes."""
    ofields = [f for f, _ in _lib.GmCclipOpts._fields_]
    rfields = [f for f, _ in _lib.GmCclipResult._fields_]
    assert ofields == ["tau", "maxiter", "tol", "layout", "check_every"]
    assert rfields == ["iters", "last_movement", "converged", "clipped"]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "gmagg.h"', "int main(void){",
           'printf("%zu\\n", sizeof(gm_cclip_opts));', 'printf("%zu\\n", sizeof(gm_cclip_result));',
           'printf("%zu\\n", sizeof(gm_opts));', 'printf("%zu\\n", sizeof(gm_result));']
    src += [f'printf("%zu\\n", offsetof(gm_cclip_opts, {f}));' for f in ofields]
    src += [f'printf("%zu\\n", offsetof(gm_cclip_result, {f}));' for f in rfields]
    src += ["return 0;}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"),
                    "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    want = [C.sizeof(_lib.GmCclipOpts), C.sizeof(_lib.GmCclipResult), C.sizeof(_lib.GmOpts),
            C.sizeof(_lib.GmResult)]
    want += [getattr(_lib.GmCclipOpts, f).offset for f in ofields]
    want += [getattr(_lib.GmCclipResult, f).offset for f in rfields]
    assert got == want
    assert got[:2] == [32, 24]


def test_abi_version_unchanged():
    assert _lib.load().gm_abi_version() == 5 == _lib.ABI_VERSION


@pytest.mark.parametrize("opts", [{}, {"tau": None}, {"tau": 0}, {"tau": -1},
                                  {"tau": float("nan")}, {"tau": 0.0, "clip_iters": 0}])
def test_cclip_rejects_bad_tau_without_a_gpu(opts):
    import byzantine_aircomp_amd as bz
    X = torch.zeros(4, 16)
    with pytest.raises(ValueError, match="tau"):
        bz.cclip(X, dict(opts, guess=torch.zeros(16)))
    with pytest.raises(ValueError, match="tau"):
        bz.cclip.with_options(tau=opts.get("tau", 1.0) if opts else float("nan"))


def test_cclip_zero_iterations_and_with_options_need_no_gpu():
    import byzantine_aircomp_amd as bz
    g = torch.ones(16)
    assert bz.cclip(torch.zeros(4, 16), {"tau": 1.0, "clip_iters": 0, "guess": g}) is g
    agg = bz.cclip.with_options(tau=2.0, clip_iters=0)
    assert agg.__name__ == "cclip"
    assert agg(torch.zeros(4, 16), {"maxiter": 1000, "tol": 1e-5, "guess": g}) is g
    with pytest.raises(TypeError):
        bz.cclip.with_options(tau=1.0, maxiter=3)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError):
            bz.cclip(torch.zeros(4, 16, dtype=dt), {"tau": 1.0})
