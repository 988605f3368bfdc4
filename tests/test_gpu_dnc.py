"""DnC on the GPU (byzantine_aircomp_amd dnc, csrc/dnc.hip) against the numpy fp64 reference of
tests/dnc_cases.py: the good rows equal, the mean bit-equal, the scores within 1e-9 of the largest
reference score, every layout (aligned rows, rows one element into a NaN-padded buffer, panels, a
CPU tensor) giving the same bits; explicit columns on both sides of a panel edge, the ends of the
options, non-finite inputs, the C ABI's refusals and composition with the wrappers.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import coordinate_cases as cc
import dnc_cases as dc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import dnc  # noqa: F401 - the file needs the feature
from byzantine_aircomp_amd import _lib, aggregators as agg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu(X):
    return torch.from_numpy(np.array(X)).to(DEV)


def _bits(t):
    if isinstance(t, np.ndarray):
        return t.view(np.int32)
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _has_width(K):
    return int(_lib.load().gm_panel_width(K)) > 0


def _sources(X):
    """(name, wList) of every layout one case runs on."""
    src = list(cc.layouts(torch, X))
    if _has_width(X.shape[0]):
        src.append(("panels", bz.ClientPanels.from_rows(_gpu(X))))
    src.append(("cpu", torch.from_numpy(np.array(X))))
    return src


def _run(w, opts):
    out = bz.dnc(w, opts)
    return {"out": out, "selected": list(bz.dnc.last_selected),
            "scores": bz.dnc.last_scores.cpu().numpy(), "info": dict(bz.dnc.last_info),
            "columns": bz.dnc.last_columns.numpy()}


def _check(got, ref, what, tol=dc.SCORE_TOL):
    assert got["selected"] == ref["good"].tolist(), what
    assert np.array_equal(_bits(got["out"].cpu()), _bits(ref["out"])), what
    smax = np.nanmax(ref["scores"]) if ref["scores"].size and not np.isnan(ref["scores"]).all() else 0
    err = np.abs(got["scores"] - ref["scores"])
    print(f"{what}: score error {np.nanmax(err) if err.size else 0:.2e} of {smax:.2e}, "
          f"iterations {got['info']['power_iters']}")
    assert np.array_equal(np.isnan(got["scores"]), np.isnan(ref["scores"])), what
    assert not (err > tol * smax).any(), (what, float(np.nanmax(err)), smax)


def _same(a, b, what):
    assert a["selected"] == b["selected"] and a["info"] == b["info"], what
    assert np.array_equal(_bits(a["out"].cpu()), _bits(b["out"].cpu())), what
    assert np.array_equal(a["scores"].view(np.int64), b["scores"].view(np.int64)), what


@pytest.mark.parametrize("K,f,d,b,c,iters", dc.GPU_CASES)
def test_main_matrix(K, f, d, b, c, iters):
    X, cols, q, ref = dc.gpu_case(K, f, d, b, c, iters)
    seed = dc.seed_of(K, f, d, b) + iters
    base = {"honestSize": K - f, "dnc_dims": b, "dnc_c": c, "dnc_iters": iters}
    if q is None:                          # the definition refuses q * iters >= K rows
        with pytest.raises(ValueError, match=">= K"):
            bz.dnc(_gpu(X), base)
        return
    first = None
    for name, w in _sources(X):
        got = _run(w, dict(base, generator=torch.Generator().manual_seed(seed)))
        what = f"K={K} f={f} d={d} b={b} c={c} iters={iters} {name}"
        assert got["out"].device == w.device and got["out"].dtype == torch.float32, what
        assert np.array_equal(got["columns"], cols), what
        assert got["info"]["removed"] == q and len(got["info"]["power_iters"]) == iters
        if q > 0:
            assert all(got["info"]["converged"]), (what, got["info"])
        _check(got, ref, what)
        if first is None:
            first = got
        else:
            _same(got, first, what)


def test_explicit_columns_across_a_panel_edge():
    """Columns {0, W-1, W, d-1} and a few others; some honest rows carry 1e3 spikes in columns
    that are not sampled: a gather that read a wrong column would change the selection."""
    K, f, d = 64, 13, 517
    W = int(_lib.load().gm_panel_width(K))
    assert 1 < W < d - 1
    X = np.array(dc.case(K, f, d, 77))
    pick = sorted({0, W - 1, W, d - 1, 5, W + 3, 2 * W - 1, 2 * W, d - 2})
    rest = np.setdiff1d(np.arange(d), pick)
    rng = np.random.RandomState(3)
    ref0 = dc.reference(X, np.array([pick]), f, check=True)
    honest = ref0["good"][:5]
    for k in honest:
        X[k, rng.choice(rest, 7, replace=False)] = 1e3
    # the spikes sit next to the sampled columns too
    X[honest[0], [1, W - 2, W + 1, d - 3]] = 1e3
    ref = dc.reference(X, np.array([pick]), f, check=True)
    assert ref["good"].tolist() == ref0["good"].tolist()
    first = None
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K - f, "dnc_columns": torch.tensor([pick])})
        assert got["columns"].tolist() == [pick]
        _check(got, ref, f"explicit {name}")
        first = first or got
        _same(got, first, name)
    # the same columns as a numpy array, another integer dtype, and one row for one round
    got = _run(_gpu(X), {"honestSize": K - f, "dnc_columns": np.array(pick, dtype=np.int32)})
    _same(got, first, "int32 columns")


def test_one_column():
    K, f, d, b = dc.GPU_SHAPES[2]
    X = dc.shape_input(K, f, d, b)
    for j in (0, d - 1):
        ref = dc.reference(X, np.array([[j]]), f)
        for name, w in _sources(X):
            got = _run(w, {"honestSize": K - f, "dnc_columns": torch.tensor([[j]])})
            _check(got, ref, f"b=1 column {j} {name}")
            assert got["info"]["converged"] == [True]
    # drawn: dnc_dims = 1
    got = _run(_gpu(X), {"honestSize": K - f, "dnc_dims": 1,
                         "generator": torch.Generator().manual_seed(4)})
    assert got["columns"].shape == (1, 1)
    _check(got, dc.reference(X, got["columns"], f), "b=1 drawn")


def test_no_byzantine_rows_is_the_mean():
    K, f, d, b = dc.GPU_SHAPES[3]
    X = np.array(dc.shape_input(K, f, d, b))
    X[3, :9] = -0.0
    X[:, 11] = -0.0                                          # a column of negative zeros
    state = torch.get_rng_state()
    for name, w in _sources(X):
        for opts in ({"honestSize": K}, {"honestSize": K - f, "dnc_c": 0.0, "dnc_iters": 2},
                     {"honestSize": K - 1, "dnc_c": 0.5}):
            got = _run(w, opts)
            want = bz.mean(w)
            assert np.array_equal(_bits(got["out"].cpu()), _bits(want.cpu())), (name, opts)
            assert got["selected"] == list(range(K)) and got["info"]["removed"] == 0
            assert got["columns"].shape == (opts.get("dnc_iters", 1), 0)
            assert not got["scores"].any()
    assert torch.equal(torch.get_rng_state(), state)         # nothing was drawn


def test_all_rows_equal():
    K, f = 65, 16
    X = np.tile(dc.case(2, 0, 300, 5)[:1], (K, 1))
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K - f, "dnc_dims": 64,
                       "generator": torch.Generator().manual_seed(1)})
        assert got["selected"] == list(range(K - f)), name
        assert not got["scores"].any() and got["info"]["power_iters"] == [0]
        assert np.array_equal(_bits(got["out"].cpu()), _bits(X[0])), name


def test_nan_in_a_sampled_column():
    K, f, d, b = dc.GPU_SHAPES[1]
    X = np.array(dc.shape_input(K, f, d, b))
    cols = [[3, 40, 41, 250, d - 1]]
    X[K - 2, 41] = np.nan
    ref = dc.reference(X, np.array(cols), f)
    assert ref["good"].tolist() == list(range(K - f)) and np.isnan(ref["scores"]).all()
    first = None
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K - f, "dnc_columns": torch.tensor(cols)})
        assert got["selected"] == list(range(K - f)), name
        assert np.isnan(got["scores"]).all() and got["info"]["converged"] == [False]
        assert np.array_equal(_bits(got["out"].cpu()), _bits(ref["out"])), name
        first = first or got
        assert np.array_equal(_bits(got["out"].cpu()), _bits(first["out"].cpu()))


def test_nan_in_an_unsampled_column():
    K, f, d, b = dc.GPU_SHAPES[1]
    X = np.array(dc.shape_input(K, f, d, b))
    cols = np.array([[3, 40, 41, 250, d - 1]])
    clean = dc.reference(X, cols, f)
    bad = int(clean["good"][2])
    X[bad, 42] = np.nan                                      # next to a sampled column
    X[int(np.setdiff1d(np.arange(K), clean["good"])[0]), 0] = np.nan
    ref = dc.reference(X, cols, f)
    assert ref["good"].tolist() == clean["good"].tolist()
    first = None
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K - f, "dnc_columns": torch.from_numpy(cols)})
        assert got["selected"] == clean["good"].tolist(), name
        err = np.abs(got["scores"] - ref["scores"]).max()
        assert err <= dc.SCORE_TOL * ref["scores"].max(), (name, err)
        o = got["out"].cpu().numpy()
        assert np.isnan(o[42]) and np.isnan(ref["out"][42]), name
        assert np.array_equal(_bits(np.delete(o, 42)), _bits(np.delete(ref["out"], 42))), name
        first = first or got
        _same(got, first, name)


def test_one_power_iteration():
    K, f, d, b = dc.GPU_SHAPES[4]
    X = dc.shape_input(K, f, d, b)
    got = _run(_gpu(X), {"honestSize": K - f, "dnc_dims": b, "power_iters": 1,
                         "generator": torch.Generator().manual_seed(2)})
    assert got["info"] == {"removed": f, "power_iters": [1], "converged": [False]}
    assert len(got["selected"]) == K - f
    # a loose stop ends early and says so
    got = _run(_gpu(X), {"honestSize": K - f, "dnc_dims": b, "power_tol": 0.5,
                         "generator": torch.Generator().manual_seed(2)})
    assert got["info"]["converged"] == [True] and got["info"]["power_iters"][0] <= 3


def test_c_abi_return_codes():
    K, d, n = 17, 100, 10
    X = _gpu(dc.case(K, 3, d, 9))
    out = torch.full((d,), 7.0, device=DEV)
    sc = torch.full((2, K), 7.0, dtype=torch.float64, device=DEV)
    cols = torch.arange(2 * n, device=DEV).reshape(2, n)
    ctx = agg.context(X.device)
    good, ng = (C.c_int32 * K)(*([-1] * K)), C.c_int64(-1)
    ni, cv = (C.c_int32 * 2)(-1, -1), (C.c_int32 * 2)(-1, -1)
    ok = dict(X=X.data_ptr(), K=K, d=d, ldx=d, layout=0, cols=cols.data_ptr(), n=n, iters=2, remove=3,
              pit=100, ptol=1e-10, out=out.data_ptr(), scores=sc.data_ptr())

    def call(**kw):
        a = {**ok, **kw}
        with torch.cuda.device(X.device):
            return ctx.lib.gm_dnc_f32(ctx.handle, a["X"], a["K"], a["d"], a["ldx"], a["layout"],
                                      a["cols"], a["n"], a["iters"], a["remove"], a["pit"], a["ptol"],
                                      a["out"], a["scores"], good, C.byref(ng), ni, cv,
                                      agg._stream_ptr(X.device))

    for kw in (dict(X=None), dict(cols=None), dict(out=None), dict(scores=None), dict(K=1),
               dict(n=0), dict(n=d + 1), dict(remove=9), dict(remove=6, iters=3), dict(ldx=d - 1),
               dict(iters=0), dict(remove=-1), dict(pit=0), dict(layout=5)):
        assert call(**kw) == -1, kw
    for kw in (dict(K=4097), dict(K=4096, layout=1, ldx=1 << 30)):
        assert call(**kw) == -3, kw
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (sc == 7.0).all()
    assert list(good) == [-1] * K and ng.value == -1 and list(ni) == [-1, -1] == list(cv)
    assert call() == 0                                       # and the same arguments run
    torch.cuda.synchronize()
    assert ng.value >= K - 6 and list(good[:ng.value]) == sorted(set(good[:ng.value]))
    assert torch.isfinite(out).all() and not (out == 7.0).all()


def test_sharded_context_is_refused():
    K, f, d, b = dc.GPU_SHAPES[1]
    X = _gpu(dc.shape_input(K, f, d, b))
    opts = {"honestSize": K - f, "dnc_dims": b, "generator": torch.Generator().manual_seed(6)}
    want = _run(X, dict(opts))
    ctx = bz.context()
    ctx.set_shard(4 * d, d)
    try:
        with pytest.raises(_lib.GmError, match=r"\(-3\).*shard"):
            bz.dnc(X, dict(opts, generator=torch.Generator().manual_seed(6)))
    finally:
        ctx.set_shard(-1, 0)
    got = _run(X, dict(opts, generator=torch.Generator().manual_seed(6)))   # usable again
    _same(got, want, "after the refusal")


def test_composition():
    K, f, d, b = dc.GPU_SHAPES[2]
    X = dc.shape_input(K, f, d, b)
    Xg = _gpu(X)
    opts = {"honestSize": K - f, "dnc_dims": b}
    keep = dict(opts)
    for wrap in (bz.bucketed(bz.dnc, 2, generator=torch.Generator().manual_seed(1)),
                 bz.mixed(bz.dnc), bz.mixed(bz.dnc, layout="rows"),
                 bz.bucketed(bz.dnc.with_options(dnc_iters=2, dnc_c=0.5), 2)):
        out = wrap(Xg, opts)
        assert out.shape == (d,) and out.is_cuda and torch.isfinite(out).all(), wrap.__name__
        assert opts == keep
    # under bucketing the inner call sees ceil(K / 2) rows and the same f
    bz.bucketed(bz.dnc, 2)(Xg, opts)
    assert bz.dnc.last_info["removed"] == f and bz.dnc.last_scores.shape == (1, K // 2)
    # a CPU wList gives a CPU result with the GPU call's bits
    g = torch.Generator().manual_seed(8)
    a = bz.dnc(torch.from_numpy(np.array(X)), dict(opts, generator=g))
    b_ = bz.dnc(Xg, dict(opts, generator=torch.Generator().manual_seed(8)))
    assert a.device.type == "cpu" and np.array_equal(_bits(a), _bits(b_.cpu()))


def test_training_run_with_dnc(tmp_path):
    from byzantine_aircomp_amd import training as T
    from test_gpu_training import synthetic_mnist
    tr = torch.utils.data.TensorDataset(*synthetic_mnist(601, 400))
    va = torch.utils.data.TensorDataset(*synthetic_mnist(602, 100))
    cfg = {"honestSize": 8, "byzantineSize": 2, "rounds": 3, "displayInterval": 1,
           "weight_decay": 0.0, "fixSeed": True, "SEED": 2021, "batchSize": 20, "shuffle": True,
           "gamma": 1e-2, "CACHE_DIR": str(tmp_path) + "/mnist_K10_B2_", "train_dataset": tr,
           "validate_dataset": va, "loss_func": torch.nn.CrossEntropyLoss(), "verbose": False}
    models = []

    def SGD(model, **kw):  # noqa: N802 - the title takes the optimizer's name
        res = T.SGD(model, **kw)
        models.append(res[0])
        return res

    title, rec = T.run(SGD, bz.dnc, "minmax", cfg, recordInFile=False,
                       device=torch.device("cuda"))
    assert title.endswith("_SGD_minmax_dnc")
    (model,) = models
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert np.isfinite(rec["trainLossPath"]).all() and np.isfinite(rec["valLossPath"]).all()
    assert bz.dnc.last_info["removed"] == 2 and len(bz.dnc.last_selected) == 8
