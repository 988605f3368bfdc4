"""dnc without a GPU: exports and binding, what is refused before anything touches a device
(Python and C ABI), the column draw, with_options, and the preconditions of every GPU case on
the numpy reference alone.  (The kernels themselves: tests/test_gpu_dnc.py.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dnc_cases as dc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import dnc  # noqa: F401 - the file needs the feature
from byzantine_aircomp_amd import _lib, aggregators as agg


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a GPU context (or to stage a tensor) fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(agg, "context", boom)
    monkeypatch.setattr(agg, "_stage", boom)


def test_exported_and_bound():
    assert bz.dnc is agg.dnc and "dnc" in agg.__all__
    assert "gm_dnc_f32" in {n for n, _, _ in _lib.SIGNATURES}
    assert hasattr(_lib.load(), "gm_dnc_f32")


def _abi_call(lib, ctx, X, K, d, ldx, layout, cols, n, iters, remove, pit, ptol, out, scores,
              good=True, n_good=True, niter=True, conv=True):
    g = (C.c_int32 * max(K, 1))()
    ng = C.c_int64()
    ni, cv = (C.c_int32 * max(iters, 1))(), (C.c_int32 * max(iters, 1))()
    return lib.gm_dnc_f32(ctx, X, K, d, ldx, layout, cols, n, iters, remove, pit, ptol, out, scores,
                          g if good else None, C.byref(ng) if n_good else None,
                          ni if niter else None, cv if conv else None, None)


def test_abi_argument_checks():
    """No device needed: every refusal happens before the first HIP call (the context pointer
    is only handed on, never read, before the checks pass)."""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ctx = p                                     # non-NULL; never dereferenced on these paths
    R, P = _lib.GM_LAYOUT_ROWS, _lib.GM_LAYOUT_PANELS

    def refused(rc_, code):
        assert rc_ == code
        msg = lib.gm_last_error()
        assert msg and b"gm_dnc_f32" in msg

    ok = dict(X=p, K=8, d=4, ldx=4, layout=R, cols=p, n=2, iters=1, remove=2, pit=100, ptol=1e-10,
              out=p, scores=p)

    def call(ctx_=ctx, **kw):
        return _abi_call(lib, ctx_, **{**ok, **kw})

    refused(call(ctx_=None), -1)                                # NULL pointers
    for name in ("X", "cols", "out", "scores"):
        refused(call(**{name: None}), -1)
    for name in ("good", "n_good", "niter", "conv"):
        refused(call(**{name: False}), -1)
    refused(call(K=1, remove=0), -1)                            # K < 2
    refused(call(d=-1), -1)
    refused(call(n=0), -1)                                      # n outside [1, d]
    refused(call(n=5), -1)
    refused(call(iters=0), -1)
    refused(call(remove=-1), -1)
    refused(call(remove=8), -1)                                 # remove * iters >= K
    refused(call(remove=4, iters=2), -1)
    refused(call(remove=3, iters=3), -1)
    refused(call(pit=0), -1)
    refused(call(ptol=-1.0), -1)
    refused(call(ptol=float("nan")), -1)
    refused(call(layout=7), -1)
    refused(call(ldx=3), -1)                                    # rows with ldx < d
    W = lib.gm_panel_width(8)
    refused(call(layout=P, ldx=8 * W - 1), -1)                  # panel stride < K * W
    refused(call(K=4097), -3)                                   # K > 4096
    assert lib.gm_panel_width(4096) == 0
    refused(call(K=4096, layout=P, ldx=1 << 30), -3)            # no panel width
    big = (1 << 27) // 4096 + 1
    refused(call(K=4096, d=big, ldx=big, n=big), -3)            # K * n > 2^27


def test_python_refusals(no_device):
    X = torch.zeros(12, 5)
    opts = {"honestSize": 9}
    for bad in (X.to(torch.bfloat16), X.double()):
        with pytest.raises(TypeError):
            bz.dnc(bad, opts)
    with pytest.raises(ValueError):
        bz.dnc(torch.zeros(12), opts)
    for o in ({}, None, {"honestSize": None}, {"dnc_c": 1.0}):
        with pytest.raises(ValueError, match="honestSize"):
            bz.dnc(X, o)
    for hs in (0, 13):
        with pytest.raises(ValueError, match="honestSize"):
            bz.dnc(X, {"honestSize": hs})
    with pytest.raises(ValueError, match="dnc_c"):
        bz.dnc(X, dict(opts, dnc_c=-0.5))
    with pytest.raises(ValueError, match="dnc_c"):
        bz.dnc(X, dict(opts, dnc_c=float("nan")))
    with pytest.raises(ValueError, match="dnc_iters"):
        bz.dnc(X, dict(opts, dnc_iters=0))
    with pytest.raises(ValueError, match="dnc_dims"):
        bz.dnc(X, dict(opts, dnc_dims=0))
    with pytest.raises(ValueError, match="power_iters"):
        bz.dnc(X, dict(opts, power_iters=0))
    with pytest.raises(ValueError, match="power_tol"):
        bz.dnc(X, dict(opts, power_tol=-1e-3))
    with pytest.raises(ValueError, match=">= K"):               # q * iters >= K
        bz.dnc(X, dict(opts, dnc_iters=4))
    with pytest.raises(ValueError, match=">= K"):
        bz.dnc(X, dict(opts, dnc_c=4.0))
    with pytest.raises(ValueError, match="4096"):
        bz.dnc(torch.zeros(4097, 2), {"honestSize": 4000})
    with pytest.raises(ValueError, match="K"):
        bz.dnc(torch.zeros(1, 2), {"honestSize": 1})
    with pytest.raises(ValueError, match="2\\^27"):
        bz.dnc(torch.zeros(4096, 1).expand(4096, 40000), {"honestSize": 4000, "dnc_dims": 40000})
    # explicit columns: [iters, n], integers, in range, strictly increasing
    for cols in ([[0, 1, 5]], [[-1, 2]], [[2, 2]], [[3, 1]], [[0.0, 1.0]], [[0, 1], [2, 3]],
                 [[]], [[0, 1, 2, 3, 4, 4]], [[True, False]]):
        with pytest.raises(ValueError, match="dnc_columns"):
            bz.dnc(X, dict(opts, dnc_columns=torch.tensor(cols)))
    with pytest.raises(ValueError, match="dnc_columns"):
        bz.dnc(X, dict(opts, dnc_iters=2, dnc_c=0.5, dnc_columns=torch.tensor([0, 1])))


def test_bf16_panels_are_refused(no_device):
    class FakePanels(bz.ClientPanels):
        def __init__(self):                      # no allocation: only the metadata is read
            self.K, self.d, self.W = 12, 5, 8
            self.data = torch.zeros(1, 12, 8, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        bz.dnc(FakePanels(), {"honestSize": 9})


def test_columns_draw():
    g = torch.Generator().manual_seed(5)
    a = bz.dnc.columns(1000, 37, 3, generator=g)
    assert a.shape == (3, 37) and a.dtype == torch.int64
    assert (a[:, 1:] > a[:, :-1]).all() and a.min() >= 0 and a.max() < 1000
    assert not torch.equal(a[0], a[1])
    b = bz.dnc.columns(1000, 37, 3, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b)
    # the documented draw: randperm(d)[:b] sorted, one draw per round
    g2 = torch.Generator().manual_seed(5)
    want = torch.stack([torch.randperm(1000, generator=g2)[:37].sort().values for _ in range(3)])
    assert torch.equal(a, want)
    # b >= d: every column, nothing drawn (neither from the generator given nor the global one)
    g3 = torch.Generator().manual_seed(9)
    s3, s0 = g3.get_state(), torch.get_rng_state()
    for bb in (20, 21, 10000):
        full = bz.dnc.columns(20, bb, 2, generator=g3)
        assert torch.equal(full, torch.arange(20).repeat(2, 1))
    bz.dnc.columns(20, 20, 2)
    assert torch.equal(g3.get_state(), s3) and torch.equal(torch.get_rng_state(), s0)
    for bad in ((0, 1, 1), (5, 0, 1), (5, 1, 0)):
        with pytest.raises(ValueError):
            bz.dnc.columns(*bad)


def test_with_options(no_device, monkeypatch):
    f = bz.dnc.with_options(dnc_c=1.5, dnc_iters=3, dnc_dims=64)
    assert f.__name__ == "dnc" and f.__qualname__ == "dnc"
    with pytest.raises(TypeError, match="tau"):
        bz.dnc.with_options(tau=1.0)
    with pytest.raises(ValueError, match="dnc_c"):
        bz.dnc.with_options(dnc_c=-1)
    with pytest.raises(ValueError, match="dnc_iters"):
        bz.dnc.with_options(dnc_iters=0)
    seen = {}
    monkeypatch.setattr(agg, "dnc", lambda w, o: seen.update(w=w, o=o) or "out")
    X = torch.zeros(12, 5)
    opts = {"honestSize": 9, "dnc_c": 0.5, "maxiter": 3}
    keep = dict(opts)
    assert f(X, opts) == "out" and opts == keep and seen["w"] is X
    assert seen["o"] == {"honestSize": 9, "maxiter": 3, "dnc_c": 1.5, "dnc_iters": 3, "dnc_dims": 64}
    # the fixed options reach the checks: 3 rounds of int(1.5 * 3) = 4 rows are all 12
    monkeypatch.undo()
    monkeypatch.setattr(agg, "context", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=">= K"):
        f(X, opts)


def test_wrappers_name_dnc():
    assert bz.bucketed(bz.dnc, 2).__name__ == "dnc_b2"
    assert bz.mixed(bz.dnc).__name__ == "dnc_nnm"


def test_reference_on_a_hand_case():
    """Two columns, the outlier along (1, 1): the scores are the squared centred projections."""
    X = np.array([[0, 0, 9], [1, 1, 9], [-1, -1, 9], [10, 10, 9]], dtype=np.float32)
    ref = dc.reference(X, np.array([[0, 1]]), 1)
    mu = 2.5
    want = 2 * (np.array([0, 1, -1, 10.0]) - mu) ** 2
    assert np.allclose(ref["scores"][0], want, rtol=1e-12)
    assert ref["good"].tolist() == [0, 1, 2] and ref["out"].tolist() == [0, 0, 9]
    # ties go to the lower index, NaN scores last; one good row is the row itself
    assert dc.score_order(np.array([2.0, np.nan, 1.0, 2.0, np.nan])).tolist() == [2, 0, 3, 1, 4]
    one = dc.reference(X, np.array([[0, 1]]), 3)
    assert one["good"].tolist() == [1] and np.array_equal(one["out"], X[1])
    # q == 0: the column mean of all rows, no scores
    zero = dc.reference(X, np.empty((2, 0)), 0)
    assert zero["good"].tolist() == [0, 1, 2, 3] and not zero["scores"].any()
    assert zero["out"].tolist() == [2.5, 2.5, 9]


@pytest.mark.parametrize("K,f,d,b,c,iters", dc.GPU_CASES)
def test_gpu_cases_meet_the_preconditions(K, f, d, b, c, iters):
    """Conditions on the inputs, not measurements: reference(check=True) asserts sigma_2 /
    sigma_1 <= 0.5 and a score gap across the cut >= 1e-6 of the largest score, every round."""
    X, cols, q, ref = dc.gpu_case(K, f, d, b, c, iters)
    if q is None:                                   # the definition refuses q * iters >= K
        assert int(c * f) * iters >= K
        return
    if q == 0:
        assert ref["good"].size == K
        return
    assert cols.shape == (iters, min(b, d)) and (np.diff(cols, axis=1) > 0).all()
    assert ref["gap"] >= dc.GAP_MIN and ref["sigma_ratio"] <= dc.SIGMA_RATIO_MAX
    assert K - q * iters <= ref["good"].size <= K - q
    print(f"dnc K={K} f={f} d={d} b={b} c={c} iters={iters}: gap {ref['gap']:.2e} "
          f"sigma2/sigma1 {ref['sigma_ratio']:.3f} good {ref['good'].size}")
