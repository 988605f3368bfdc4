"""The selection and Krum paths of coordinate.hip that the other f3 tests never reach, against
plain CPU references (tests/coordinate_cases.py: references, tolerance and its derivation).

  A  every default selection kernel on 33 column tiles (the XCD tile permutation active, a
     ragged last tile), float4 and scalar loads
  B  adversarial columns for the trimmed mean, the median and the mean
  C  gm_trimmed_mean_f32's `trim` range and the argument errors, through the C ABI
  D  Krum's exact pair-distance path at 9 - 32 row tiles
  E  the GMAGG_SELECT_* runtime knobs, each in a child process (they are read once per process)
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coordinate_cases as cc

pytestmark = pytest.mark.gpu

GM_ERR_INVALID, GM_ERR_UNSUPPORTED = -1, -3


# ------------------------------------------------------------------------------------- A

@pytest.mark.parametrize("K", [64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024, 1025, 1500, 2048])
def test_full_tiles_both_layouts(K):
    """33 tiles per kernel (d = 517 at 16 columns per tile, 261 at 8): two permuted groups of
    16 tiles and a ragged last one; the aligned view takes the float4 loads, the view one
    element into its buffer the scalar ones.  Every column carries its own marker."""
    import byzantine_aircomp_amd as bz
    X, refs = cc.normal_case(K, cc.full_tile_d(K))
    cc.assert_kappa(X, (0, cc.default_trim(K)))
    assert cc.check_select(bz, torch, X, refs, f"K={K}") is None


@pytest.mark.parametrize("K,d", [(2049, 133), (5000, 132)])
def test_mean_beyond_selection_K(K, d):
    """The mean has no K limit: per-element 1 ulp past K = 2048 (5000 fp64 terms at kappa <=
    1e4: relative 5.6e-9, still far under half an fp32 ulp), special values included; d = 132
    takes the four-columns-per-thread kernel on the aligned layout."""
    import byzantine_aircomp_amd as bz
    X, _ = cc.normal_case(K, d)
    X = np.array(X)
    X[0, 1] = np.inf
    X[1, 2] = -np.inf
    X[2, 3] = np.nan
    X[:2, 4] = (np.inf, -np.inf)
    X[:, 5] = 0.0
    X[::2, 5] = -0.0
    X[: K // 2 + 5, 6] = 3e38
    cc.assert_kappa(X, (0,))
    want = cc.ref_mean(X)
    for lname, V in cc.layouts(torch, X):
        assert cc.mismatch_ulp(bz.mean(V).cpu().numpy(), want, f"K={K} {lname} mean") is None


# ------------------------------------------------------------------------------------- B

@pytest.mark.parametrize("K", [200, 512, 513, 1000, 1024, 1025, 2048])
def test_adversarial_columns(K):
    """Outliers, clusters, > 128 keys sharing 16 leading bits (the select_steps(15, 0) tail),
    subnormals, +-0, ties, infinities and NaNs in and out of the kept middle, and b + 1 / b
    copies of the extreme values (the boundary tie counts) — coordinate_cases.adversarial_case.
    The kappa precondition covers the columns whose kept values are finite; in the 1e30 and
    3e38 columns the kept values either exclude the huge ones (trimmed away) or are dominated
    by them (kappa ~ 1), so the same 1-ulp bound holds there."""
    import byzantine_aircomp_amd as bz
    X, refs = cc.adversarial_case(K)
    cc.assert_kappa(X, (0, cc.default_trim(K)))
    assert np.isfinite(refs["trimmed"][[0, 12, 16, 17]]).all()
    assert np.isnan(refs["trimmed"][[14, 15]]).all() and np.isfinite(refs["trimmed"][13])
    assert cc.check_select(bz, torch, X, refs, f"K={K}") is None


# ------------------------------------------------------------------------------------- C

def _abi():
    import byzantine_aircomp_amd as bz
    ctx = bz.aggregators.context()
    return bz, ctx, torch.cuda.current_stream().cuda_stream


def _trims(K):
    return sorted({0, 1, (K - 1) // 2} | ({K // 2 - 1} if K % 2 == 0 else set()))


@pytest.mark.parametrize("K", [7, 64, 100, 513, 1000, 2048])
def test_trim_range_c_abi(K):
    """trim = 0 (ranks 0 and K-1, next to the padding keys) is the mean; 2 trim = K-1 (the
    lo == hi branch) is the median; 2 trim = K-2 keeps two values; the panel twin returns the
    rows call's bits."""
    bz, ctx, stream = _abi()
    d = 70
    trims = _trims(K)
    X, refs = cc.normal_case(K, d, tuple(trims))
    cc.assert_kappa(X, trims)
    Xc = torch.from_numpy(np.array(X)).cuda()
    P = bz.ClientPanels.from_rows(Xc)
    for trim in trims:
        out = torch.full((d,), float("nan"), device="cuda")
        outp = torch.full((d,), float("nan"), device="cuda")
        rc = ctx.lib.gm_trimmed_mean_f32(ctx.handle, Xc.data_ptr(), K, d, d, trim,
                                         out.data_ptr(), stream)
        assert rc == 0, (trim, rc, ctx.lib.gm_last_error())
        rc = ctx.lib.gm_trimmed_mean_panels_f32(ctx.handle, P.data.data_ptr(), K, d,
                                                P.panel_stride, trim, outp.data_ptr(), stream)
        assert rc == 0, (trim, rc, ctx.lib.gm_last_error())
        got = out.cpu().numpy()
        assert cc.mismatch_ulp(got, refs[("trim", trim)], f"K={K} trim={trim}") is None
        if trim == 0:
            assert cc.mismatch_ulp(got, refs["mean"], f"K={K} trim=0 vs mean") is None
        if 2 * trim == K - 1:
            assert cc.mismatch_exact(got, refs["median"], f"K={K} trim={trim} vs median") is None
        assert np.array_equal(outp.cpu().numpy(), got), (K, trim)


def test_argument_errors_c_abi():
    """Return codes (gm_last_error only words them)."""
    bz, ctx, stream = _abi()
    lib, h = ctx.lib, ctx.handle
    K, d = 100, 16
    X = torch.zeros(4097, d, device="cuda")
    P = bz.ClientPanels.from_rows(X[:K])
    out = torch.zeros(d, device="cuda")
    idx = C.c_int64(-7)
    x, o = X.data_ptr(), out.data_ptr()

    def is_(rc, want):
        assert rc == want, (rc, want, lib.gm_last_error())

    for trim in (K // 2, K // 2 + 1, K, -1):
        is_(lib.gm_trimmed_mean_f32(h, x, K, d, d, trim, o, stream), GM_ERR_INVALID)
        is_(lib.gm_trimmed_mean_panels_f32(h, P.data.data_ptr(), K, d, P.panel_stride, trim, o,
                                           stream), GM_ERR_INVALID)
    is_(lib.gm_trimmed_mean_f32(h, x, 7, d, d, 3, o, stream), 0)          # 2 trim = K - 1: valid
    is_(lib.gm_trimmed_mean_f32(h, x, K, d, d - 1, 10, o, stream), GM_ERR_INVALID)
    is_(lib.gm_median_f32(h, x, K, d, d - 1, o, stream), GM_ERR_INVALID)
    is_(lib.gm_mean_f32(h, x, K, d, d - 1, o, stream), GM_ERR_INVALID)
    is_(lib.gm_krum_f32(h, x, K, d, d - 1, 80, o, C.byref(idx), stream), GM_ERR_INVALID)
    is_(lib.gm_median_f32(h, x, 2049, d, d, o, stream), GM_ERR_UNSUPPORTED)
    is_(lib.gm_trimmed_mean_f32(h, x, 2049, d, d, 204, o, stream), GM_ERR_UNSUPPORTED)
    is_(lib.gm_krum_f32(h, x, 4097, d, d, 3000, o, C.byref(idx), stream), GM_ERR_UNSUPPORTED)
    for honest in (1, K + 2):
        is_(lib.gm_krum_f32(h, x, K, d, d, honest, o, C.byref(idx), stream), GM_ERR_INVALID)
        is_(lib.gm_krum_panels_f32(h, P.data.data_ptr(), K, d, P.panel_stride, honest, o,
                                   C.byref(idx), stream), GM_ERR_INVALID)
    torch.cuda.synchronize()
    assert idx.value == -7 and not out.cpu().any()       # a refused call writes nothing


# ------------------------------------------------------------------------------------- D

def _krum_exact(bz, X, honest):
    out = bz.Krum(X, {"honestSize": honest})
    info = bz.aggregators.Krum.last_info
    assert info["algo"] == "exact", info
    return out.cpu(), bz.aggregators.Krum.last_index


@pytest.mark.parametrize("K,d,honest", cc.KRUM_SHAPES)
def test_krum_exact_many_row_tiles(K, d, honest, monkeypatch):
    """9, 17 and 32 row tiles of 128 (45 - 528 pair tiles through the decode loop), a ragged
    last tile at K = 2049 and 1100, honestSize = K + 1 (every distance summed).  Precondition
    (CPU, fp64): the best score leads by a relative gap >= 1e-3, ~500 x the exact path's fp32
    stage rounding (32 x 2^-24 per distance).  Panels where gm_panel_width(K) != 0: K = 1100
    only; K = 2049 and 4096 have no panel layout."""
    import byzantine_aircomp_amd as bz
    monkeypatch.setenv("GMAGG_KRUM", "0")
    X = cc.krum_case(K, d, honest)
    want, gap = cc.ref_krum(X, honest)
    print(f"K={K} d={d} honestSize={honest}: fp64 index {want}, relative gap {gap:.2e}")
    assert gap >= cc.KRUM_MIN_GAP, gap
    Xc = X.cuda()
    out, index = _krum_exact(bz, Xc, honest)
    assert index == want and torch.equal(out, X[want])
    if bz._lib.load().gm_panel_width(K) != 0:
        out, index = _krum_exact(bz, bz.ClientPanels.from_rows(Xc), honest)
        assert index == want and torch.equal(out, X[want])
    else:
        assert K > 2048


def test_krum_exact_honest_two(monkeypatch):
    """honestSize = 2: every score is the row's distance to itself, exactly 0, so the first
    index wins — 32 row tiles."""
    import byzantine_aircomp_amd as bz
    monkeypatch.setenv("GMAGG_KRUM", "0")
    X = cc.krum_case(4096, 8, 2)
    assert cc.ref_krum_scores(X, 2).max() == 0.0
    out, index = _krum_exact(bz, X.cuda(), 2)
    assert index == 0 and torch.equal(out, X[0])


def test_krum_exact_duplicate_rows(monkeypatch):
    """The fp64-best row copied over rows 3 and 700: three equal scores, the smallest index
    wins (which one, and the gap to the other rows, from the reference)."""
    import byzantine_aircomp_amd as bz
    monkeypatch.setenv("GMAGG_KRUM", "0")
    K, d, honest = cc.KRUM_SHAPES[0]
    X = cc.krum_case(K, d, honest)
    best, _ = cc.ref_krum(X, honest)
    X[3] = X[best]
    X[700] = X[best]
    want, gap = cc.ref_krum(X, honest, tied=[3, 700, best])
    assert want == min(3, best) and gap >= cc.KRUM_MIN_GAP, (want, gap)
    Xc = X.cuda()
    for M in (Xc, bz.ClientPanels.from_rows(Xc)):
        out, index = _krum_exact(bz, M, honest)
        assert index == want and torch.equal(out, X[want])


def test_krum_exact_unaligned_view(monkeypatch):
    """ldx = 43 and a start one element into the buffer: pair_dist's scalar loads over 9 row
    tiles."""
    import byzantine_aircomp_amd as bz
    monkeypatch.setenv("GMAGG_KRUM", "0")
    K, d, honest = cc.KRUM_SHAPES[0]
    X = cc.krum_case(K, d, honest)
    want, gap = cc.ref_krum(X, honest)
    assert gap >= cc.KRUM_MIN_GAP
    base = torch.full((K, d + 3), float("nan"), device="cuda")
    base[:, 1:1 + d] = X.cuda()
    V = base[:, 1:1 + d]
    assert V.stride(0) % 4 != 0
    out, index = _krum_exact(bz, V, honest)
    assert index == want and torch.equal(out, X[want])


# ------------------------------------------------------------------------------------- E

_child_died = False

KNOBS = [
    ({"GMAGG_SELECT_ST": "0"}, []),                                   # the pre-round-5 kernels
    ({"GMAGG_SELECT_ST": "2"}, []),                                   # trimmed mean on col_select_st
    ({"GMAGG_SELECT_ST": "0", "GMAGG_SELECT_1COL": "0"}, []),         # the pair kernel everywhere
    ({"GMAGG_SELECT_ST": "0", "GMAGG_SELECT_1COL": "1"}, []),         # col_select1 for both modes
    ({"GMAGG_SELECT_ST": "0", "GMAGG_SELECT_PERSIST": "1"}, ["--wide"]),   # persistent form
]


@pytest.mark.parametrize("knobs,args", KNOBS, ids=["+".join(f"{k[13:]}={v}" for k, v in kn.items())
                                                   for kn, _ in KNOBS])
def test_runtime_knob_in_child(knobs, args):
    """coordinate_cases.main() (parts A and B at K = 200 .. 2048, median and trimmed mean; the
    persistent form also on more tiles than its grid has blocks) in a fresh process under one
    knob setting.  A child that dies on a signal or runs into the limit fails this case and
    stops the remaining ones: nothing more is started on the card from this file."""
    global _child_died
    if _child_died:
        pytest.skip("an earlier knob child died or hung")
    env = {k: v for k, v in os.environ.items() if not k.startswith("GMAGG_SELECT_")}
    env.update(knobs)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(cc.__file__)] + args, env=env,
                           timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True)
    except subprocess.TimeoutExpired as e:
        _child_died = True
        pytest.fail(f"child under {knobs} ran into its limit:\n{e.stdout}")
    if r.returncode < 0 or r.returncode in (134, 139):
        _child_died = True
    assert r.returncode == 0, f"child under {knobs} exited {r.returncode}:\n{r.stdout[-4000:]}"
