"""Nearest-neighbor mixing on the GPU (byzantine_aircomp_amd nnm / mixed, csrc/nnm.hip) against
the references and bars of tests/nnm_cases.py: the neighbour lists inside the distance error
band, every mixed value within one fp32 rounding plus an fp64 reordering of the exact sum of the
kernel's own neighbour list; layouts, ties, the ends of f, Byzantine rows of huge or infinite
size, composition with the aggregators and stream order.
"""
import numpy as np
import pytest
import torch

import nnm_cases as nc
import robust_cases as rc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import mixed, nnm  # noqa: F401 - the file needs the feature
from byzantine_aircomp_amd import _lib, aggregators as agg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu(X):
    return torch.from_numpy(np.array(X)).to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _check_values(Y, X, N, what=""):
    ref, scale = nc.ref_mix(X, N, with_scale=True)
    got = Y.cpu().numpy() if isinstance(Y, torch.Tensor) else Y
    bad = nc.mix_mismatch(got, ref, scale)
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], ref.ravel()[bad[:5]])
    return ref


def _mix_and_check(X, f, D=None, rows=None):
    Y, N = bz.nnm(_gpu(X), f, neighbors=True)
    assert Y.shape == X.shape and Y.dtype == torch.float32
    assert N.dtype == torch.int32 and N.shape == (X.shape[0], X.shape[0] - f) and N.is_cuda
    N = N.cpu().numpy()
    amb = nc.check_neighbors(N, X, f, D=D, rows=rows)
    _check_values(Y, X, N)
    return Y, N, amb


@pytest.mark.parametrize("K,d,fo,f", nc.NNM_CASES + nc.SMALL_CASES)
def test_main_matrix(K, d, fo, f):
    X, D = nc.case(K, d, fo)
    _, _, amb = _mix_and_check(X, f, D=D)
    print(f"nnm K={K} d={d} f={f}: {amb} ambiguous rows")


@pytest.mark.parametrize("K,d,fo,f", nc.BIG_CASES)
def test_beyond_1024(K, d, fo, f):
    X, D = nc.case(K, d, fo)
    _mix_and_check(X, f, D=D)


def _call(Xt, ldx, lin, K, d, f, Yt, ldy, lout, Nt=None):
    agg.context(Xt.device).call("gm_nnm_f32", Xt.data_ptr(), K, d, ldx, lin, f, Yt.data_ptr(), ldy,
                                lout, Nt.data_ptr() if Nt is not None else None,
                                agg._stream_ptr(Xt.device))


def test_layouts_give_the_same_bits():
    K, d, fo, f = nc.LAYOUT_CASE
    X, D = nc.case(K, d, fo)
    m = K - f
    Xa = _gpu(X)                                            # aligned, contiguous
    stride = d + 2 if (d + 2) % 2 else d + 3                # odd row stride, base off by 4 bytes
    buf = torch.full((K, stride), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, 1:1 + d] = Xa
    Xv = buf[:, 1:1 + d]
    assert Xv.data_ptr() % 16 == 4 and Xv.stride(0) % 2 == 1
    P = bz.ClientPanels.from_rows(Xa)
    buf0, P0 = _bits(buf), _bits(P.data)
    Y0, N0 = bz.nnm(Xa, f, neighbors=True)
    nc.check_neighbors(N0.cpu().numpy(), X, f, D=D)
    _check_values(Y0, X, N0.cpu().numpy())
    for name, src in (("aligned", Xa), ("view", Xv), ("panels", P)):
        for layout in ("rows", "panels"):
            Y, N = bz.nnm(src, f, layout=layout, neighbors=True)
            assert torch.equal(N, N0), (name, layout)
            if layout == "panels":
                assert isinstance(Y, bz.ClientPanels) and Y.shape == (K, d)
                pad = Y.data[-1, :, d % Y.W:] if d % Y.W else Y.data[-1, :, :0]
                assert (pad == 0).all()
                Y = Y.to_rows()
            assert np.array_equal(_bits(Y), _bits(Y0)), (name, layout)
    # layout=None keeps the input's
    assert isinstance(bz.nnm(P, f), bz.ClientPanels) and isinstance(bz.nnm(Xa, f), torch.Tensor)
    # Y with a row stride above d, an odd one, one element into a NaN buffer; Y panels whose
    # padding columns hold NaN: nothing outside the K x d values is written
    ybuf = torch.full((K, stride), float("nan"), dtype=torch.float32, device=DEV)
    Nt = torch.empty(K, m, dtype=torch.int32, device=DEV)
    _call(Xv, stride, _lib.GM_LAYOUT_ROWS, K, d, f, ybuf[:, 1:1 + d], stride, _lib.GM_LAYOUT_ROWS, Nt)
    assert np.array_equal(_bits(ybuf[:, 1:1 + d]), _bits(Y0)) and torch.equal(Nt, N0)
    assert torch.isnan(ybuf[:, 0]).all() and torch.isnan(ybuf[:, 1 + d:]).all()
    Q = bz.ClientPanels(K, d, device=DEV)
    Q.data.fill_(float("nan"))
    _call(P.data, P.panel_stride, _lib.GM_LAYOUT_PANELS, K, d, f, Q.data, Q.panel_stride,
          _lib.GM_LAYOUT_PANELS)
    assert d % Q.W and torch.isnan(Q.data[-1, :, d % Q.W:]).all()
    assert np.array_equal(_bits(Q.to_rows()), _bits(Y0))
    # X is never written
    assert np.array_equal(_bits(buf), buf0) and np.array_equal(_bits(P.data), P0)
    assert np.array_equal(_bits(Xa), X.view(np.int32))


@pytest.mark.parametrize("f", [2, 4])
def test_ties_go_to_the_lower_index(f):
    X = rc.tie_matrix()
    Y, N = bz.nnm(_gpu(X), f, neighbors=True)
    Nref = nc.ref_neighbors(X, f)
    assert np.array_equal(N.cpu().numpy(), Nref)
    assert np.array_equal(Y.cpu().numpy(), nc.ref_mix(X, Nref))


def test_copies_of_one_row():
    X = nc.copies_input()
    f = 13
    Y, N = bz.nnm(_gpu(X), f, neighbors=True)
    N = N.cpu().numpy()
    assert (np.diff(N, axis=1) > 0).all() and N.shape == (65, 52)
    _check_values(Y, X, N)
    # whichever copies the kernel took, the value is that of the reference's choice
    ref, scale = nc.ref_mix(X, nc.ref_neighbors(X, f), with_scale=True)
    assert nc.mix_mismatch(Y.cpu().numpy(), ref, scale).size == 0
    copies = [5, 9, 12, 20, 21, 33, 40, 47, 58, 64]
    assert all(np.array_equal(_bits(Y[c]), _bits(Y[5])) for c in copies)


def test_edge_f():
    X, _ = nc.case(65, 333, 13)
    K, d = X.shape
    Xg = _gpu(X)
    # f = 0: every row is the column mean
    Y, N = bz.nnm(Xg, 0, neighbors=True)
    assert np.array_equal(N.cpu().numpy(), np.tile(np.arange(K), (K, 1)))
    _check_values(Y, X, N.cpu().numpy())
    assert all(torch.equal(Y[i], Y[0]) for i in range(K))
    # f = K - 1: Y is X, bit for bit (signed zeros included)
    Z = np.array(X)
    Z[3, :7] = -0.0
    Z[4, :7] = 0.0
    Y, N = bz.nnm(_gpu(Z), K - 1, neighbors=True)
    assert np.array_equal(N.cpu().numpy(), np.arange(K)[:, None])
    assert np.array_equal(_bits(Y), Z.view(np.int32))
    # K = 1
    one = _gpu(X[:1])
    Y, N = bz.nnm(one, 0, neighbors=True)
    assert np.array_equal(_bits(Y), _bits(one)) and N.cpu().tolist() == [[0]]
    P = bz.nnm(bz.ClientPanels.from_rows(one), 0)
    assert np.array_equal(_bits(P.to_rows()), _bits(one))
    # no columns
    Y, N = bz.nnm(torch.empty(5, 0, device=DEV), 2, neighbors=True)
    assert Y.shape == (5, 0) and N.cpu().tolist() == [[0, 1, 2]] * 5


def test_byzantine_scale():
    """The outlier rows a million times larger, then one of them holding inf: the honest rows'
    mixes do not see them (a complement form, column sum minus the excluded rows, would).  The
    neighbour band is checked on the honest rows: from a row at 1e6 every honest row is equally
    far within fp32, so which 800 of them it takes is open; its values are still held to the
    exact sum of the list the kernel returned."""
    X0, _ = nc.case(1000, 520, 100)
    out = np.flatnonzero(X0.mean(axis=1) > 0.5)
    assert out.size == 100
    honest = np.setdiff1d(np.arange(1000), out)
    X = np.array(X0)
    X[out] *= np.float32(1e6)
    Y, N, _ = _mix_and_check(X, 100, rows=honest)
    Yh = Y.cpu().numpy()[honest]
    assert np.isfinite(Yh).all() and np.abs(Yh).max() < 10.0
    assert not np.isin(N[honest], out).any()
    X[out[0], 7] = np.inf
    Y, N, _ = _mix_and_check(X, 100, rows=honest)           # (non-finite entries match exactly)
    Y = Y.cpu().numpy()
    assert np.isfinite(Y[honest]).all() and not np.isin(N[honest], out).any()
    assert out[0] in N[out[0]] and Y[out[0], 7] == np.inf
    assert not np.isin(out[0], np.delete(N, out[0], axis=0))


def test_composition():
    X, _ = nc.case(50, 7850, 10)
    Xg = _gpu(X)
    f = 10
    opts = {"honestSize": 40, "maxiter": 100, "tol": 1e-5}
    keep = dict(opts)
    two = bz.gm2(bz.nnm(Xg, f, layout="panels"), opts)
    one = bz.mixed(bz.gm2)(Xg, opts)
    assert opts == keep and one.is_cuda and np.array_equal(_bits(one), _bits(two))
    assert np.array_equal(_bits(bz.mixed(bz.gm2, f=f)(Xg, {"maxiter": 100, "tol": 1e-5})),
                          _bits(two))
    cc = bz.cclip.with_options(tau=1.0)
    for inner in (bz.median, bz.Krum, cc):
        for layout in ("panels", "rows"):
            got = bz.mixed(inner, layout=layout)(Xg, opts)
            want = inner(bz.nnm(Xg, f, layout=layout), opts)
            assert got.shape == (7850,) and np.array_equal(_bits(got), _bits(want)), inner.__name__
    # a CPU wList gives a CPU result
    Xc = torch.from_numpy(np.array(X))
    got = bz.mixed(bz.gm2)(Xc, opts)
    assert got.device.type == "cpu" and np.array_equal(_bits(got), _bits(two))
    Yc = bz.nnm(Xc, f)
    assert Yc.device.type == "cpu" and np.array_equal(_bits(Yc), _bits(bz.nnm(Xg, f)))


def test_training_run_with_mixed_gm2(tmp_path):
    from byzantine_aircomp_amd import training as T
    from test_gpu_training import synthetic_mnist
    tr = torch.utils.data.TensorDataset(*synthetic_mnist(601, 400))
    va = torch.utils.data.TensorDataset(*synthetic_mnist(602, 100))
    cfg = {"honestSize": 8, "byzantineSize": 2, "rounds": 2, "displayInterval": 1,
           "weight_decay": 0.0, "fixSeed": True, "SEED": 2021, "batchSize": 20, "shuffle": True,
           "gamma": 1e-2, "CACHE_DIR": str(tmp_path) + "/mnist_K10_B2_", "train_dataset": tr,
           "validate_dataset": va, "loss_func": torch.nn.CrossEntropyLoss(), "verbose": False}
    models = []

    def SGD(model, **kw):  # noqa: N802 - the title takes the optimizer's name
        res = T.SGD(model, **kw)
        models.append(res[0])
        return res

    title, rec = T.run(SGD, bz.mixed(bz.gm2), "alie", cfg, recordInFile=False,
                       device=torch.device("cuda"))
    assert title.endswith("_SGD_alie_gm2_nnm")
    (model,) = models
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert np.isfinite(rec["trainLossPath"]).all() and np.isfinite(rec["valLossPath"]).all()


def test_stream_order():
    """Two calls on one context from two streams share its workspace (the distances, the mask):
    the second waits for the first, and both give the bits of the serial runs."""
    Xa = _gpu(nc.case(600, 1030, 100)[0])
    Xb = _gpu(nc.case(256, 2051, 50)[0])
    Ya, Na = bz.nnm(Xa, 100, neighbors=True)
    Yb, Nb = bz.nnm(Xb, 100, neighbors=True)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        Y1, N1 = bz.nnm(Xa, 100, neighbors=True)
    with torch.cuda.stream(s2):
        Y2, N2 = bz.nnm(Xb, 100, neighbors=True)
    with torch.cuda.stream(s1):
        Y3 = bz.nnm(Xb, 100)
    torch.cuda.synchronize()
    assert torch.equal(N1, Na) and torch.equal(N2, Nb)
    assert np.array_equal(_bits(Y1), _bits(Ya)) and np.array_equal(_bits(Y2), _bits(Yb))
    assert np.array_equal(_bits(Y3), _bits(Yb))


def test_sharded_context_is_refused():
    X = _gpu(nc.case(17, 1000, 3)[0])
    Y = torch.full_like(X, 7.0)
    ctx = agg.Context(torch.cuda.current_device())
    try:
        ctx.set_shard(4000, 1000)
        with pytest.raises(_lib.GmError, match="shard"):
            ctx.call("gm_nnm_f32", X.data_ptr(), 17, 1000, 1000, 0, 3, Y.data_ptr(), 1000, 0, None,
                     agg._stream_ptr(X.device))
        torch.cuda.synchronize()
        assert (Y == 7.0).all()
    finally:
        ctx.close()
