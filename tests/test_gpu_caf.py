"""caf on the GPU (byzantine_aircomp_amd caf, csrc/caf.hip) against the numpy fp64 d-space
reference of tests/caf_cases.py: the round counts equal, out, c* and lambda within the bars
derived there, every layout (aligned rows, rows one element into a NaN-padded buffer, panels, a
CPU tensor) giving the same bits; the ends of the options, planted rows at 1000 x the scale, rows
of weight zero not read by the result pass, a NaN input, the C ABI's refusals and composition
with the wrappers and the training loops.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import caf_cases as cf
import coordinate_cases as cc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import caf  # noqa: F401 - the file needs the feature
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
    out = bz.caf(w, opts)
    return {"out": out, "weights": bz.caf.last_weights.cpu().numpy(), "info": dict(bz.caf.last_info)}


def _same(a, b, what):
    assert np.array_equal(_bits(a["out"].cpu()), _bits(b["out"].cpu())), what
    assert np.array_equal(a["weights"].view(np.int64), b["weights"].view(np.int64)), what
    ia, ib = dict(a["info"]), dict(b["info"])
    la, lb = ia.pop("eigenvalue"), ib.pop("eigenvalue")
    assert ia == ib and np.array_equal(np.float64(la).view(np.int64), np.float64(lb).view(np.int64)), what


def _check(got, ref, what, w_tol=cf.W_TOL):
    info = got["info"]
    got_ = {"weights": got["weights"], "eigenvalue": info["eigenvalue"],
            "out": got["out"].cpu().numpy()}
    ew, el, eo = cf.errors(got_, ref)
    print(f"{what}: rounds {info['rounds']} best {info['best_round']} applications "
          f"{sum(info['power_iters'])}; c* {ew:.2e}, lambda {el:.2e}, out {eo:.2e}")
    assert (info["rounds"], info["best_round"]) == (ref["rounds"], ref["best_round"]), what
    assert len(info["power_iters"]) == info["rounds"] == len(info["converged"]), what
    assert eo <= cf.OUT_TOL, (what, eo)
    if w_tol is not None:
        assert ew <= w_tol and el <= cf.LAM_TOL, (what, ew, el)
        assert abs(info["weight"] - ref["weight"]) <= w_tol * len(ref["weights"]), what


@pytest.mark.parametrize("K,f,d", cf.GPU_CASES)
def test_main_matrix(K, f, d):
    X = cf.gpu_input(K, f, d)
    ref = cf.gpu_reference(K, f, d)
    first = None
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K - f})
        what = f"K={K} f={f} d={d} {name}"
        assert got["out"].device == w.device and got["out"].dtype == torch.float32, what
        _check(got, ref, what)
        if first is None:
            first = got
        else:
            _same(got, first, what)


def test_no_byzantine_rows_is_the_mean():
    K, f, d = 65, 16, 300
    X = np.array(cf.gpu_input(K, f, d))
    X[3, :9] = -0.0
    X[:, 11] = -0.0                                          # a column of negative zeros
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K})
        want = bz.mean(w)
        assert np.array_equal(_bits(got["out"].cpu()), _bits(want.cpu())), name
        assert (got["weights"] == 1).all() and got["info"]["rounds"] == 0
        assert got["info"]["weight"] == K and got["info"]["power_iters"] == []


def test_all_rows_equal():
    K, f = 65, 16
    X = np.tile(cf.case(2, 0, 300)[:1], (K, 1))
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K - f})
        info = got["info"]
        assert info["rounds"] == 1 and info["eigenvalue"] == 0 and info["best_round"] == 0, name
        assert info["power_iters"] == [0] and info["converged"] == [True], name
        assert (got["weights"] == 1).all(), name
        assert np.array_equal(_bits(got["out"].cpu()), _bits(X[0])), name


def test_ends_of_the_power_iteration():
    K, f, d = 64, 13, 517
    X = _gpu(cf.gpu_input(K, f, d))
    got = _run(X, {"honestSize": K - f, "power_iters": 1})
    info = got["info"]
    assert info["rounds"] >= 1 and info["power_iters"] == [1] * info["rounds"]
    assert info["converged"] == [False] * info["rounds"]
    ref = cf.reference(cf.gpu_input(K, f, d), f, power_iters=1)
    assert ref["min_gap"] >= cf.GAP_MIN                      # (the round count is decided)
    assert info["rounds"] == ref["rounds"] and info["best_round"] == ref["best_round"]
    # a loose stop ends early and says so
    got = _run(X, {"honestSize": K - f, "power_tol": 0.5})
    info = got["info"]
    assert info["converged"][0] and info["power_iters"][0] <= 3


@pytest.mark.parametrize("K,f,d", cf.SCALE_CASES)
def test_planted_rows_at_a_thousand_times_the_scale(K, f, d):
    X = cf.gpu_input(K, f, d, 1000.0)
    ref = cf.gpu_reference(K, f, d, 1000.0)
    first = None
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K - f})
        # (the weights' error reaches 5e-4 at this scale: W_TOL is not asserted)
        _check(got, ref, f"scaled K={K} {name}", w_tol=None)
        assert cf.byzantine_share(got["weights"], f) <= 1e-3, name
        first = first or got
        _same(got, first, name)


def test_rows_of_weight_zero_are_not_read():
    """The result pass through the C ABI (gm_weighted_mean_f32) with the weights of a caf call:
    the same bits as that call's out, and still the same with NaN in every row of weight 0."""
    K, f, d = 65, 16, 300
    X0 = np.array(cf.gpu_input(K, f, d))
    for name, w in _sources(X0)[:3]:
        got = _run(w, {"honestSize": K - f})
        zero = np.flatnonzero(got["weights"] == 0)
        assert zero.size >= 1, name
        weights = bz.caf.last_weights
        Xn = np.array(X0)
        Xn[zero] = np.nan
        for Xs in (X0, Xn):
            src = dict(_sources(Xs))[name]
            T, ldx, layout, _, _ = agg._operand(src)
            out = torch.full((d,), 7.0, device=DEV)
            ctx = agg.context(T.device)
            with torch.cuda.device(T.device):
                ctx.call("gm_weighted_mean_f32", T.data_ptr(), K, d, ldx, layout,
                         weights.data_ptr(), out.data_ptr(), agg._stream_ptr(T.device))
            assert np.array_equal(_bits(out), _bits(got["out"].cpu())), name


def test_nan_in_one_column():
    K, f, d = 17, 3, 100
    X = np.array(cf.gpu_input(K, f, d))
    X[4, 7] = np.nan
    first = None
    for name, w in _sources(X):
        got = _run(w, {"honestSize": K - f})
        info = got["info"]
        assert info["rounds"] == 0 and info["best_round"] == 0 and np.isnan(info["eigenvalue"]), name
        assert (got["weights"] == 1).all() and info["weight"] == K, name
        o = got["out"].cpu().numpy()
        assert np.isnan(o[7]) and np.isfinite(np.delete(o, 7)).all(), name
        plain = np.delete(X, 7, axis=1).astype(np.float64).mean(axis=0)
        assert np.abs(np.delete(o, 7) - plain).max() <= 1e-7, name
        first = first or got
        assert np.array_equal(_bits(got["out"].cpu()), _bits(first["out"].cpu())), name


def test_c_abi_return_codes():
    K, d, f = 17, 100, 3
    X = _gpu(cf.gpu_input(K, f, d))
    out = torch.full((d,), 7.0, device=DEV)
    wt = torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
    ctx = agg.context(X.device)
    lam, S = C.c_double(-1.0), C.c_double(-1.0)
    rounds, best = C.c_int32(-1), C.c_int32(-1)
    ni, cv = (C.c_int32 * K)(*([-1] * K)), (C.c_int32 * K)(*([-1] * K))
    ok = dict(X=X.data_ptr(), K=K, d=d, ldx=d, layout=0, f=f, pit=100, ptol=1e-10,
              out=out.data_ptr())

    def call(**kw):
        a = {**ok, **kw}
        with torch.cuda.device(X.device):
            return ctx.lib.gm_caf_f32(ctx.handle, a["X"], a["K"], a["d"], a["ldx"], a["layout"],
                                      a["f"], a["pit"], a["ptol"], a["out"], wt.data_ptr(),
                                      C.byref(lam), C.byref(S), C.byref(rounds), C.byref(best), ni,
                                      cv, agg._stream_ptr(X.device))

    for kw in (dict(X=None), dict(out=None), dict(K=1, f=0), dict(d=-1), dict(f=-1), dict(f=9),
               dict(K=16, f=8), dict(layout=5), dict(ldx=d - 1), dict(pit=0), dict(ptol=-1.0),
               dict(ptol=float("nan")), dict(layout=1, ldx=K * 4)):
        assert call(**kw) == -1, kw
    for kw in (dict(K=4097), dict(K=4096, layout=1, ldx=1 << 30)):
        assert call(**kw) == -3, kw
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (wt == 7.0).all()
    assert lam.value == -1.0 == S.value and rounds.value == -1 == best.value
    assert list(ni) == [-1] * K == list(cv)
    assert call() == 0                                       # and the same arguments run
    torch.cuda.synchronize()
    ref = cf.gpu_reference(K, f, d)
    assert rounds.value == ref["rounds"] and best.value == ref["best_round"]
    assert list(ni[rounds.value:]) == [-1] * (K - rounds.value)
    assert torch.isfinite(out).all() and not (out == 7.0).any()
    assert np.abs(wt.cpu().numpy() - ref["weights"]).max() <= cf.W_TOL
    assert abs(lam.value - ref["eigenvalue"]) <= cf.LAM_TOL * ref["eigenvalue"]


def test_sharded_context_is_refused():
    K, f, d = 17, 3, 100
    X = _gpu(cf.gpu_input(K, f, d))
    opts = {"honestSize": K - f}
    want = _run(X, opts)
    ctx = bz.context()
    ctx.set_shard(4 * d, d)
    try:
        with pytest.raises(_lib.GmError, match=r"\(-3\).*shard"):
            bz.caf(X, opts)
    finally:
        ctx.set_shard(-1, 0)
    _same(_run(X, opts), want, "after the refusal")          # usable again


def test_composition():
    K, f, d = 64, 13, 517
    X = cf.gpu_input(K, f, d)
    Xg = _gpu(X)
    opts = {"honestSize": K - f}
    keep = dict(opts)
    for wrap in (bz.bucketed(bz.caf, 2, generator=torch.Generator().manual_seed(1)),
                 bz.mixed(bz.caf), bz.mixed(bz.caf, layout="rows"), bz.clipped(bz.caf, f=f),
                 bz.bucketed(bz.caf.with_options(power_iters=20), 2)):
        out = wrap(Xg, opts)
        assert out.shape == (d,) and out.is_cuda and torch.isfinite(out).all(), wrap.__name__
        assert opts == keep
    # under bucketing the inner call sees ceil(K / 2) rows
    bz.bucketed(bz.caf, 2)(Xg, opts)
    assert bz.caf.last_weights.shape == (K // 2,)
    got = _run(Xg, dict(opts, power_iters=20))
    assert max(got["info"]["power_iters"]) <= 20
    fixed = {"out": bz.caf.with_options(power_iters=20)(Xg, opts),
             "weights": bz.caf.last_weights.cpu().numpy(), "info": dict(bz.caf.last_info)}
    _same(fixed, got, "with_options")
    # a CPU wList gives a CPU result with the GPU call's bits
    a = bz.caf(torch.from_numpy(np.array(X)), opts)
    b_ = bz.caf(Xg, opts)
    assert a.device.type == "cpu" and np.array_equal(_bits(a), _bits(b_.cpu()))


@pytest.mark.parametrize("optimizer", ["SGD", "MomentumSGD"])
def test_training_run_with_caf(optimizer, tmp_path):
    from byzantine_aircomp_amd import training as T
    from test_gpu_training import synthetic_mnist
    tr = torch.utils.data.TensorDataset(*synthetic_mnist(601, 400))
    va = torch.utils.data.TensorDataset(*synthetic_mnist(602, 100))
    cfg = {"honestSize": 8, "byzantineSize": 2, "rounds": 3, "displayInterval": 1,
           "weight_decay": 0.0, "fixSeed": True, "SEED": 2021, "batchSize": 20, "shuffle": True,
           "gamma": 1e-2, "CACHE_DIR": str(tmp_path) + "/mnist_K10_B2_", "train_dataset": tr,
           "validate_dataset": va, "loss_func": torch.nn.CrossEntropyLoss(), "verbose": False}
    models = []
    inner = getattr(T, optimizer)

    def opt(model, **kw):
        res = inner(model, **kw)
        models.append(res[0])
        return res
    opt.__name__ = optimizer

    title, rec = T.run(opt, bz.caf, "minmax", cfg, recordInFile=False,
                       device=torch.device("cuda"))
    assert title.endswith("_minmax_caf") and optimizer in title
    (model,) = models
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert np.isfinite(rec["trainLossPath"]).all() and np.isfinite(rec["valLossPath"]).all()
    assert bz.caf.last_weights.shape == (10,) and bz.caf.last_info["rounds"] >= 0
