"""nnm / mixed without a GPU: exports and binding, what is refused before anything touches a
device (Python and C ABI), the wrapper's contract, the numpy references against brute-force
restatements of the definition, and the ambiguity cap of every GPU shape on the reference
alone.  (The kernels themselves: tests/test_gpu_nnm.py.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nnm_cases as nc
import robust_cases as rc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import mixed, nnm  # noqa: F401 - the file needs the feature
from byzantine_aircomp_amd import _lib, aggregators as agg


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a GPU context (or to stage a tensor) fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(agg, "context", boom)
    monkeypatch.setattr(agg, "_stage", boom)


def test_exported_and_bound():
    for name in ("nnm", "mixed"):
        assert getattr(bz, name) is getattr(agg, name)
        assert name in agg.__all__
    assert "gm_nnm_f32" in {n for n, _, _ in _lib.SIGNATURES}
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
    nn = lib.gm_nnm_f32

    def refused(rc_, code):
        assert rc_ == code
        msg = lib.gm_last_error()
        assert msg and b"gm_nnm_f32" in msg

    # gm_nnm_f32(ctx, X, K, d, ldx, layout_in, f, Y, ldy, layout_out, neighbors, stream)
    refused(nn(None, p, 8, 4, 4, R, 2, p, 4, R, None, None), -1)
    refused(nn(ctx, None, 8, 4, 4, R, 2, p, 4, R, None, None), -1)
    refused(nn(ctx, p, 8, 4, 4, R, 2, None, 4, R, None, None), -1)
    refused(nn(ctx, p, 0, 4, 4, R, 0, p, 4, R, None, None), -1)          # K < 1
    refused(nn(ctx, p, 8, -1, 4, R, 2, p, 4, R, None, None), -1)         # d < 0
    refused(nn(ctx, p, 8, 4, 4, R, -1, p, 4, R, None, None), -1)         # f
    refused(nn(ctx, p, 8, 4, 4, R, 8, p, 4, R, None, None), -1)
    refused(nn(ctx, p, 8, 4, 4, 7, 2, p, 4, R, None, None), -1)          # layouts
    refused(nn(ctx, p, 8, 4, 4, R, 2, p, 4, 2, None, None), -1)
    refused(nn(ctx, p, 8, 4, 3, R, 2, p, 4, R, None, None), -1)          # ldx < d
    refused(nn(ctx, p, 8, 4, 4, R, 2, p, 3, R, None, None), -1)          # ldy < d
    W = lib.gm_panel_width(8)
    refused(nn(ctx, p, 8, 4, 8 * W - 1, P, 2, p, 4, R, None, None), -1)  # panel strides
    refused(nn(ctx, p, 8, 4, 4, R, 2, p, 8 * W - 1, P, None, None), -1)
    refused(nn(ctx, p, 4097, 4, 4, R, 2, p, 4, R, None, None), -3)       # K > 4096
    assert lib.gm_panel_width(4096) == 0
    refused(nn(ctx, p, 4096, 4, 1 << 30, P, 2, p, 4, R, None, None), -3)
    refused(nn(ctx, p, 4096, 4, 4, R, 2, p, 1 << 30, P, None, None), -3)
    # d == 0 is GM_OK, before any device call
    assert nn(ctx, p, 8, 0, 4, R, 2, p, 4, R, None, None) == 0
    assert nn(ctx, p, 8, 0, 8 * W, P, 0, p, 8 * W, P, None, None) == 0


def test_python_refusals(no_device):
    X = torch.zeros(12, 5)
    for bad in (X.to(torch.bfloat16), X.double()):
        with pytest.raises(TypeError):
            bz.nnm(bad, 2)
    with pytest.raises(ValueError):
        bz.nnm(torch.zeros(12), 2)
    with pytest.raises(ValueError):
        bz.nnm(torch.zeros(2, 3, 4), 1)
    for f in (-1, 12, 13, 2.0, 1.5, True, None, "2"):
        with pytest.raises(ValueError, match="f"):
            bz.nnm(X, f)
    with pytest.raises(ValueError, match="layout"):
        bz.nnm(X, 2, layout="columns")
    with pytest.raises(ValueError, match="4096"):
        bz.nnm(torch.zeros(4097, 2), 5)
    with pytest.raises(ValueError, match="panel"):
        bz.nnm(torch.zeros(4096, 2), 5, layout="panels")


def test_bf16_panels_are_refused(no_device):
    class FakePanels(bz.ClientPanels):
        def __init__(self):                      # no allocation: only the metadata is read
            self.K, self.d, self.W = 12, 5, 8
            self.data = torch.zeros(1, 12, 8, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        bz.nnm(FakePanels(), 2)


def test_mixed_contract(no_device, monkeypatch):
    assert bz.mixed(bz.gm2).__name__ == "gm2_nnm"
    assert bz.mixed(bz.Krum, 3, layout="rows").__name__ == "Krum_nnm"
    with pytest.raises(ValueError, match="layout"):
        bz.mixed(bz.gm2, layout="columns")
    X = torch.zeros(12, 5)
    for opts in ({}, {"maxiter": 3}, {"honestSize": None}):
        with pytest.raises(ValueError, match="honestSize"):
            bz.mixed(bz.gm2)(X, opts)
    # the inner call gets nnm's result and the caller's options, which are not modified
    seen = {}

    def fake_nnm(wList, f, layout=None, neighbors=False):
        seen["nnm"] = (wList, f, layout)
        return "mixed rows"

    def inner(wList, options):
        seen["inner"] = (wList, options)
        return torch.ones(5)

    monkeypatch.setattr(agg, "nnm", fake_nnm)
    opts = {"honestSize": 9, "maxiter": 7}
    keep = dict(opts)
    out = bz.mixed(inner)(X, opts)
    assert opts == keep and seen["nnm"][0] is X and seen["nnm"][1:] == (3, "panels")
    assert seen["inner"][0] == "mixed rows" and seen["inner"][1] == keep
    assert out.device == X.device
    bz.mixed(inner, f=5, layout=None)(X, opts)
    assert seen["nnm"][0] is X and seen["nnm"][1:] == (5, None) and opts == keep
    bz.mixed(inner, f=2)(torch.zeros(4096, 1), {})           # no panel width: rows
    assert seen["nnm"][1:] == (2, "rows")


def _brute_inputs():
    rng = np.random.RandomState(7)
    out = []
    for K, d in ((1, 3), (2, 4), (5, 6), (8, 7), (9, 5)):
        X = (rng.randn(K, d) * np.linspace(0.5, 2.0, K)[:, None]).astype(np.float32)
        out.append(X)
        if K >= 5:
            Q = X.copy()
            Q[3] = Q[0]                                     # duplicate rows: ties at 0
            Q[4] = Q[1]
            out.append(Q)
            Wd = X.copy()                                   # a wide dynamic range and signed zeros
            Wd[1] *= np.float32(1e6)
            Wd[2] *= np.float32(1e-30)
            Wd[0, 0] = -0.0
            out.append(Wd)
    out.append(rc.tie_matrix())
    return out


@pytest.mark.parametrize("X", _brute_inputs(), ids=lambda X: f"{X.shape[0]}x{X.shape[1]}")
def test_references_are_the_definition(X):
    K = X.shape[0]
    for f in range(K):
        N = nc.ref_neighbors(X, f)
        assert np.array_equal(N, nc.brute_neighbors(X, f))
        ref, scale = nc.ref_mix(X, N, with_scale=True)
        assert ref.dtype == np.float32
        assert np.array_equal(ref, nc.brute_mix(X, N))
        assert np.allclose(scale, np.abs(X.astype(np.float64))[N].mean(axis=1), rtol=1e-12)
        assert nc.mix_mismatch(ref, ref, scale).size == 0
    assert np.array_equal(nc.ref_mix(X, nc.ref_neighbors(X, K - 1)), X)


def test_reference_nonfinite_terms():
    X = np.array([[1, 2, 3, 4], [np.inf, 2, -np.inf, np.nan], [1, np.inf, np.inf, 4],
                  [5, 6, 7, 8]], dtype=np.float32)
    N = np.array([[0, 3], [1, 2], [0, 1], [0, 1]])
    ref, scale = nc.ref_mix(X, N, with_scale=True)
    assert np.isfinite(scale).all() and scale[0].tolist() == [3, 4, 5, 6]
    want = np.array([[3, 4, 5, 6], [np.inf, np.inf, np.nan, np.nan],
                     [np.inf, 2, -np.inf, np.nan], [np.inf, 2, -np.inf, np.nan]], np.float32)
    assert np.array_equal(ref, want, equal_nan=True)
    # an inf row ranks its own entry first (D[i][i] = 0), then ties at inf by index
    Nn = nc.ref_neighbors(X, 2)
    assert Nn[1].tolist() == [0, 1] and Nn[0].tolist() == [0, 3]


def test_check_neighbors_rejects_wrong_lists():
    X, D = nc.case(65, 333, 13)
    N = nc.ref_neighbors(X, 13, D=D)
    assert nc.check_neighbors(N, X, 13, D=D) == 0
    far = np.argmax(D[0])
    bad = N.copy()
    row = [j for j in bad[0] if j != 0][:-1] + [0, int(far)]
    bad[0] = np.sort(row)
    with pytest.raises(AssertionError):
        nc.check_neighbors(bad, X, 13, D=D)
    noself = N.copy()
    others = [j for j in range(65) if j not in set(N[1])]
    noself[1] = np.sort([j for j in N[1] if j != 1] + others[:1])
    with pytest.raises(AssertionError):
        nc.check_neighbors(noself, X, 13, D=D)


@pytest.mark.parametrize("K,d,fo,f", nc.NNM_CASES + nc.BIG_CASES + nc.SMALL_CASES + [nc.LAYOUT_CASE])
def test_gpu_shapes_meet_the_ambiguity_cap(K, d, fo, f):
    """Condition, not measurement: at most 5 % of a shape's rows may have their (m + 1)-th
    distance within the kernel's error band of the m-th (check_neighbors asserts it)."""
    X, D = nc.case(K, d, fo)
    amb = nc.check_neighbors(nc.ref_neighbors(X, f, D=D), X, f, D=D)
    print(f"nnm K={K} d={d} fo={fo} f={f}: {amb} ambiguous rows")


def test_copies_input_has_ten_rows_at_distance_zero():
    X = nc.copies_input()
    D = nc.ref_dist(X)
    assert (D[5] == 0).sum() == 10
    N = nc.ref_neighbors(X, 13, D=D)
    assert set(np.flatnonzero(D[5] == 0)) <= set(N[64])
