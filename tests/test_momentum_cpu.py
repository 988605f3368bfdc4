"""training.MomentumSGD, the worker-momentum loop in gradient space (Karimireddy, He & Jaggi,
ICML 2021, Algorithm 1), on the CPU: the per-client torch path against an fp64 recursion
written out here, the momentum state under channel noise, the guess, the RNG consumption,
the refusals, the record and the C ABI's new symbol."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_gpu_training import synthetic_mnist

K, HONEST, BATCH, GAMMA, WD = 6, 4, 20, 5e-2, 1e-3


def mean_agg(X, o):
    return X.mean(0)


def median_agg(X, o):
    return X.median(0).values


@pytest.fixture(scope="module")
def data():
    tr = torch.utils.data.TensorDataset(*synthetic_mnist(611, 600))
    va = torch.utils.data.TensorDataset(*synthetic_mnist(612, 200))
    return tr, va


def _run(T, data, aggregate, beta, monkeypatch, attack="classflip", noise_var=None, byz=K - HONEST,
         optimizer=None):
    """One run (2 rounds x 3 steps) with every step's batch indices recorded."""
    tr, va = data
    drawn = []
    draw = T._ClientChain.draw
    monkeypatch.setattr(T._ClientChain, "draw",
                        staticmethod(lambda s: drawn.append(draw(s)) or drawn[-1]))
    model = T.modelFactory(SEED=2021)
    theta0 = torch.cat([p.detach().flatten() for p in model.parameters()]).double()
    kw = {} if optimizer is T.SGD else {"beta": beta}
    res = (optimizer or T.MomentumSGD)(
        model, gamma=GAMMA, aggregate=aggregate, weight_decay=WD, noise_var=noise_var,
        honestSize=K - byz, byzantineSize=byz,
        attack=attack if callable(attack) else getattr(T, attack), rounds=2, displayInterval=3, SEED=2021, fixSeed=True, loss_func=torch.nn.CrossEntropyLoss(),
        train_dataset=tr, validate_dataset=va, device=torch.device("cpu"), batchSize=BATCH,
        verbose=False, **kw)
    return res, theta0, drawn


def _grad64(theta, x, y):
    """grad of the mean cross entropy of the linear classifier at theta = [W, b], fp64."""
    C = 10
    W = theta[:C * 784].view(C, 784).clone().requires_grad_()
    b = theta[C * 784:].clone().requires_grad_()
    torch.nn.functional.cross_entropy(x @ W.T + b, y).backward()
    return torch.cat([W.grad.flatten(), b.grad])


def _batch64(tr, local, k, honest, attack):
    x, y = tr.tensors
    n = len(x)
    rows = local[k].long() + (k * n) // K
    xb, yb = x[rows].reshape(len(rows), -1).double(), y[rows]
    if k >= honest and attack == "classflip":
        yb = 9 - yb
    return xb, yb


def _loss64(theta, ds):
    x, y = ds.tensors
    W, b = theta[:7840].view(10, 784), theta[7840:]
    return float(torch.nn.functional.cross_entropy(x.reshape(len(x), -1).double() @ W.T + b, y))


def _recursion(data, theta0, drawn, aggregate, beta):
    """m_k <- beta m_k + (1 - beta)(grad + wd theta) at the shared theta; theta -= gamma R."""
    tr, va = data
    theta, M = theta0.clone(), torch.zeros(K, theta0.numel(), dtype=torch.float64)
    tl, vl = [_loss64(theta, tr)], [_loss64(theta, va)]
    for t, local in enumerate(drawn):
        for k in range(K):
            xb, yb = _batch64(tr, local, k, HONEST, "classflip")
            M[k] = beta * M[k] + (1 - beta) * (_grad64(theta, xb, yb) + WD * theta)
        theta = theta - GAMMA * aggregate(M, None)
        if t % 3 == 2:
            tl.append(_loss64(theta, tr))
            vl.append(_loss64(theta, va))
    return theta, tl, vl


@pytest.mark.parametrize("aggregate", [mean_agg, median_agg])
@pytest.mark.parametrize("beta", [0.9, 0.0])
def test_loop_equals_fp64_recursion(data, aggregate, beta, monkeypatch):
    """4 honest + 2 classflip clients, weight decay, 2 rounds x 3 steps.  beta = 0 is plain
    robust D-SGD.  Bars: the project's loop-against-loop bars (test_gpu_training.py)."""
    from byzantine_aircomp_amd import training as T
    res, theta0, drawn = _run(T, data, aggregate, beta, monkeypatch)
    m, tl, _, vl, _, var = res
    assert len(drawn) == 6 and len(var) == 2
    want, tl64, vl64 = _recursion(data, theta0, drawn, aggregate, beta)
    got = torch.cat([p.detach().flatten() for p in m.parameters()]).numpy()
    assert rel_l2(got, want.numpy()) <= 1e-5
    assert rel_l2(got, theta0.numpy()) > 1e-3          # (the model moved)
    np.testing.assert_allclose(tl, tl64, rtol=1e-5)
    np.testing.assert_allclose(vl, vl64, rtol=1e-5)


def test_momentum_state_is_noise_free_and_guess_is_previous_aggregate(data, monkeypatch):
    """noise_var = 1.0 with a non-gm aggregator: the aggregator sees a noisy COPY; M, seen by
    a recording no-op attack at every step, is the recursion at the model of that step.  The
    first call's guess is None, each later one the previous aggregate."""
    from byzantine_aircomp_amd import training as T
    tr, _ = data
    seen, calls = [], []
    holder = {}

    def recorder(M, byzantine):
        assert byzantine == 1
        theta = torch.cat([p.detach().flatten() for p in holder["model"].parameters()])
        seen.append((M.clone(), theta.double()))

    def aggregate(X, options):
        out = X.mean(0)
        calls.append((options["guess"], out, X.clone()))
        return out

    real = T.calculateAccuracy

    def spy(model, *a):                                # (the loop's model, for the recorder)
        holder["model"] = model
        return real(model, *a)
    monkeypatch.setattr(T, "calculateAccuracy", spy)
    _, theta0, drawn = _run(T, data, aggregate, 0.9, monkeypatch, attack=recorder, noise_var=1.0,
                            byz=1)
    assert len(seen) == len(calls) == 6
    M64 = torch.zeros(K, theta0.numel(), dtype=torch.float64)
    for t, (M, theta) in enumerate(seen):
        for k in range(K):
            xb, yb = _batch64(tr, drawn[t], k, K, None)
            M64[k] = 0.9 * M64[k] + 0.1 * (_grad64(theta, xb, yb) + WD * theta)
        for k in range(K):
            assert rel_l2(M[k].numpy(), M64[k].numpy()) <= 1e-5, (t, k)
        # what was aggregated is M plus noise of variance ~ 1 per element, not M
        assert float((calls[t][2] - M).pow(2).mean()) > 0.1
    assert calls[0][0] is None
    for t in range(1, 6):
        assert calls[t][0] is calls[t - 1][1]


def test_rng_consumption_is_sgds(data, monkeypatch):
    from byzantine_aircomp_amd import training as T
    states = []
    for opt in (T.SGD, T.MomentumSGD):
        _run(T, data, mean_agg, 0.9, monkeypatch, optimizer=opt)
        states.append(torch.get_rng_state())
    assert torch.equal(states[0], states[1])


@pytest.mark.parametrize("beta", [-0.1, 1.0, math.nan])
def test_beta_outside_unit_interval_is_refused(data, beta, monkeypatch):
    from byzantine_aircomp_amd import training as T
    with pytest.raises(ValueError, match="beta"):
        _run(T, data, mean_agg, beta, monkeypatch)


def test_run_titles_and_records_the_loop(data):
    from byzantine_aircomp_amd import training as T
    tr, va = data
    cfg = {"honestSize": 4, "byzantineSize": 2, "rounds": 1, "displayInterval": 1,
           "weight_decay": 0.0, "fixSeed": True, "SEED": 2021, "batchSize": BATCH, "gamma": 1e-2,
           "beta": 0.5, "train_dataset": tr, "validate_dataset": va, "verbose": False,
           "loss_func": torch.nn.CrossEntropyLoss()}
    title, rec = T.run(optimizer=T.MomentumSGD, aggregate=mean_agg, attack="classflip", config=cfg,
                       recordInFile=False, device=torch.device("cpu"))
    assert title == "MLP_MomentumSGD_classflip_mean_agg"
    assert rec["beta"] == 0.5 and len(rec["valLossPath"]) == 2
    assert "MomentumSGD" in T.__all__


def test_abi_exports_the_kernel_at_version_5():
    from byzantine_aircomp_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "gm_client_grads_f32")
    assert "gm_client_grads_f32" in {n for n, _, _ in _lib.SIGNATURES}
    assert lib.gm_abi_version() == 5
