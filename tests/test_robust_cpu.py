"""meamed / multi_krum / bulyan without a GPU: exports and binding, what is refused before
anything touches a device (Python and C ABI), the numpy references against brute-force
restatements of the definitions, and the margin conditions every GPU selection case relies on.
(The kernels themselves: tests/test_gpu_robust.py.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import robust_cases as rc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import bulyan, meamed, multi_krum  # noqa: F401 - the file needs the feature
from byzantine_aircomp_amd import _lib, aggregators as agg


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a GPU context (or to stage a tensor) fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(agg, "context", boom)
    monkeypatch.setattr(agg, "_stage", boom)


def test_exported_and_bound():
    for name in ("multi_krum", "bulyan", "meamed"):
        assert getattr(bz, name) is getattr(agg, name)
        assert name in agg.__all__
    names = {n for n, _, _ in _lib.SIGNATURES}
    assert {"gm_meamed_f32", "gm_multi_krum_f32", "gm_bulyan_f32"} <= names
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 and lib.gm_abi_version() == 5


def test_abi_argument_checks():
    """No device needed: every refusal happens before the first HIP call (the context pointer
    is only handed on, never read, before the checks pass)."""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ctx = p                                     # non-NULL; never dereferenced on these paths
    R, P = _lib.GM_LAYOUT_ROWS, _lib.GM_LAYOUT_PANELS

    def refused(rc_, code, fn):
        assert rc_ == code
        msg = lib.gm_last_error()
        assert msg and fn in msg

    mm, mk, bu = lib.gm_meamed_f32, lib.gm_multi_krum_f32, lib.gm_bulyan_f32
    # gm_meamed_f32(ctx, X, K, d, ldx, layout, rows, n_rows, keep, out, stream)
    refused(mm(None, p, 4, 4, 4, R, None, 4, 2, p, None), -1, b"gm_meamed_f32")
    refused(mm(ctx, None, 4, 4, 4, R, None, 4, 2, p, None), -1, b"gm_meamed_f32")
    refused(mm(ctx, p, 4, 4, 4, R, None, 4, 2, None, None), -1, b"gm_meamed_f32")
    refused(mm(ctx, p, 0, 4, 4, R, None, 0, 0, p, None), -1, b"gm_meamed_f32")
    refused(mm(ctx, p, 4, -1, 4, R, None, 4, 2, p, None), -1, b"gm_meamed_f32")
    refused(mm(ctx, p, 4, 4, 4, 7, None, 4, 2, p, None), -1, b"gm_meamed_f32")     # layout
    refused(mm(ctx, p, 4, 4, 3, R, None, 4, 2, p, None), -1, b"gm_meamed_f32")     # ldx < d
    refused(mm(ctx, p, 4, 4, 4, R, None, 4, 0, p, None), -1, b"gm_meamed_f32")     # keep
    refused(mm(ctx, p, 4, 4, 4, R, None, 4, 5, p, None), -1, b"gm_meamed_f32")
    refused(mm(ctx, p, 4, 4, 4, R, None, 3, 2, p, None), -1, b"gm_meamed_f32")     # n_rows, no rows
    refused(mm(ctx, p, 4, 4, 4, R, p, 5, 2, p, None), -1, b"gm_meamed_f32")        # n_rows > K
    refused(mm(ctx, p, 4, 4, 4, R, p, 3, 4, p, None), -1, b"gm_meamed_f32")        # keep > n_rows
    refused(mm(ctx, p, 4, 4, 4 * lib.gm_panel_width(4) - 1, P, None, 4, 2, p, None), -1,
            b"gm_meamed_f32")                                                      # panel stride
    refused(mm(ctx, p, 1025, 4, 4, R, None, 1025, 2, p, None), -3, b"gm_meamed_f32")
    # gm_multi_krum_f32(ctx, X, K, d, ldx, layout, honest, m, out, selected, stream)
    refused(mk(None, p, 8, 4, 4, R, 6, 3, p, None, None), -1, b"gm_multi_krum_f32")
    refused(mk(ctx, p, 8, 4, 4, 2, 6, 3, p, None, None), -1, b"gm_multi_krum_f32")
    refused(mk(ctx, p, 8, 4, 3, R, 6, 3, p, None, None), -1, b"gm_multi_krum_f32")
    refused(mk(ctx, p, 8, 4, 4, R, 1, 3, p, None, None), -1, b"gm_multi_krum_f32")   # honest
    refused(mk(ctx, p, 8, 4, 4, R, 10, 3, p, None, None), -1, b"gm_multi_krum_f32")
    refused(mk(ctx, p, 8, 4, 4, R, 6, 0, p, None, None), -1, b"gm_multi_krum_f32")   # m
    refused(mk(ctx, p, 8, 4, 4, R, 6, 9, p, None, None), -1, b"gm_multi_krum_f32")
    refused(mk(ctx, p, 4097, 4, 4, R, 4000, 3, p, None, None), -3, b"gm_multi_krum_f32")
    assert lib.gm_panel_width(4096) == 0
    refused(mk(ctx, p, 4096, 4, 1 << 30, P, 4000, 3, p, None, None), -3, b"gm_multi_krum_f32")
    # gm_bulyan_f32(ctx, X, K, d, ldx, layout, honest, out, selected, stream)
    refused(bu(None, p, 8, 4, 4, R, 7, p, None, None), -1, b"gm_bulyan_f32")
    refused(bu(ctx, p, 8, 4, 4, 5, 7, p, None, None), -1, b"gm_bulyan_f32")
    refused(bu(ctx, p, 8, 4, 3, R, 7, p, None, None), -1, b"gm_bulyan_f32")
    refused(bu(ctx, p, 8, 4, 4, R, 6, p, None, None), -1, b"gm_bulyan_f32")     # K = 8 < 4*2 + 3
    refused(bu(ctx, p, 8, 4, 4, R, 9, p, None, None), -1, b"gm_bulyan_f32")     # f < 0
    refused(bu(ctx, p, 1025, 4, 4, R, 1025, p, None, None), -3, b"gm_bulyan_f32")
    # d == 0 is GM_OK, before any device call
    assert mm(ctx, p, 4, 0, 4, R, None, 4, 2, p, None) == 0
    assert mk(ctx, p, 8, 0, 4, R, 6, 3, p, None, None) == 0
    assert bu(ctx, p, 8, 0, 4, R, 7, p, None, None) == 0


def test_python_refusals(no_device):
    X = torch.zeros(12, 5)
    for fn in (bz.multi_krum, bz.bulyan, bz.meamed):
        with pytest.raises(ValueError, match="honestSize"):
            fn(X, {})
        with pytest.raises(ValueError, match="honestSize"):
            fn(X, {"maxiter": 3})
        with pytest.raises(TypeError):
            fn(X.to(torch.bfloat16), {"honestSize": 10})
        with pytest.raises(TypeError):
            fn(X.double(), {"honestSize": 10})
        with pytest.raises(ValueError):
            fn(torch.zeros(12), {"honestSize": 10})
    for m in (0, -1, 13):
        with pytest.raises(ValueError, match="m ="):
            bz.multi_krum(X, {"honestSize": 10, "m": m})
    for h in (1, 14):
        with pytest.raises(ValueError):
            bz.multi_krum(X, {"honestSize": h})
    with pytest.raises(ValueError, match="4f"):
        bz.bulyan(X, {"honestSize": 9})                   # f = 3: needs K >= 15
    with pytest.raises(ValueError):
        bz.bulyan(X, {"honestSize": 13})
    for h in (0, 13):
        with pytest.raises(ValueError):
            bz.meamed(X, {"honestSize": h})
    with pytest.raises(ValueError):
        bz.meamed(torch.zeros(1025, 2), {"honestSize": 3})
    with pytest.raises(ValueError):
        bz.bulyan(torch.zeros(1025, 2), {"honestSize": 1025})


def test_bf16_panels_are_refused(no_device):
    class FakePanels(bz.ClientPanels):
        def __init__(self):                      # no allocation: only the metadata is read
            self.K, self.d, self.W = 12, 5, 8
            self.data = torch.zeros(1, 12, 8, dtype=torch.bfloat16)
    for fn in (bz.multi_krum, bz.bulyan, bz.meamed):
        with pytest.raises(TypeError):
            fn(FakePanels(), {"honestSize": 10})


@pytest.mark.parametrize("n,d,seed", [(1, 3, 0), (2, 4, 1), (5, 6, 2), (8, 7, 3), (9, 5, 4)])
def test_ref_meamed_is_the_definition(n, d, seed):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d).astype(np.float32)
    Q = (np.round(2 * X) / 2).astype(np.float32)            # ties
    Q[0, 0] = -0.0
    for M in (X, Q):
        for keep in range(1, n + 1):
            assert np.array_equal(rc.ref_meamed(M, keep), rc.brute_meamed(M, keep))
    if n >= 5:
        S = Q.copy()
        S[1, 0] = np.inf
        S[2, 1] = -np.inf
        S[3, 1] = np.inf
        S[0, 2] = np.nan
        S[:, 3] = np.inf                                    # inf - inf: NaN deviations
        S[0, 3] = 1.0
        for keep in (1, n - 1, n):
            a, b = rc.ref_meamed(S, keep), rc.brute_meamed(S, keep)
            assert np.array_equal(a, b, equal_nan=True), (keep, a, b)


def test_meamed_ends():
    X = rc.meamed_input(17, 333).numpy()
    assert np.array_equal(rc.ref_meamed(X, 1), np.sort(X, axis=0)[8])
    mean = (X.astype(np.float64).sum(axis=0) / 17).astype(np.float32)
    ref, scale = rc.ref_meamed(X, 17, with_scale=True)
    assert rc.meamed_mismatch(mean, ref, scale).size == 0


@pytest.mark.parametrize("K,f,seed", [(7, 1, 0), (8, 1, 1), (9, 0, 2), (11, 2, 3), (12, 2, 4)])
def test_selection_references_are_the_definitions(K, f, seed):
    rng = np.random.RandomState(100 + seed)
    X = (rng.randn(K, 6) * np.linspace(0.5, 2.0, K)[:, None]).astype(np.float32)
    D = rc.dist64_direct(X)
    assert np.allclose(rc.dist64(X), D, rtol=1e-12, atol=1e-12)
    for m in (1, (K - f) // 2, K - f, K):
        _, sel, _, _ = rc.ref_multi_krum(X, K - f, m, D=D)
        assert sel == rc.brute_multi_krum_select(X, K - f, m)
    sel, _, _ = rc.ref_bulyan_select(D, f)
    assert sel == rc.brute_bulyan_select(X, K - f)
    assert len(sel) == K - 2 * f and len(set(sel)) == len(sel)


def test_tie_matrix_ties_at_the_boundaries():
    X = rc.tie_matrix()
    assert X.shape == (8, 40) and np.abs(X).max() <= 8 and np.array_equal(X, np.round(X))
    D = rc.dist64_direct(X)
    assert np.array_equal(D, rc.dist64(X))
    assert np.array_equal(D.astype(np.float32).astype(np.float64), D)     # exact in fp32 too
    _, sel, gap, tie = rc.ref_multi_krum(X, 7, 3, D=D)
    assert tie and gap == 0.0
    assert sel == rc.brute_multi_krum_select(X, 7, 3)
    bsel, bgap, btie = rc.ref_bulyan_select(D, 1)
    assert btie and bgap == 0.0
    assert bsel == rc.brute_bulyan_select(X, 7)


@pytest.mark.parametrize("K,d,f", rc.MULTI_KRUM_CASES)
def test_multi_krum_cases_are_well_posed(K, d, f):
    for m in rc.ms(K, f):
        _, sel, gap, _ = rc.multi_krum_case(K, d, f, m)
        print(f"multi_krum K={K} d={d} f={f} m={m}: gap {gap:.3e}")
        assert len(sel) == m and gap >= rc.MULTI_KRUM_MIN_GAP


@pytest.mark.parametrize("K,d,f", rc.BULYAN_CASES)
def test_bulyan_cases_are_well_posed(K, d, f):
    _, _, sel, gap, _ = rc.bulyan_case(K, d, f)
    print(f"bulyan K={K} d={d} f={f}: gap {gap:.3e}")
    assert len(sel) == K - 2 * f and gap >= rc.BULYAN_MIN_GAP


@pytest.mark.parametrize("K,d", rc.QUANT_CASES)
def test_quantised_cases_have_threshold_ties(K, d):
    X = rc.quantised_input(K, d).numpy()
    assert rc.threshold_ties(X, K - K // 5).any()
