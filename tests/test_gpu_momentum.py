"""gm_client_grads_f32 (client_grads.hip: every client's gradient at ONE model, folded into its
momentum, one workgroup per client) against fp64 autograd, its independence and error
contracts, and training.MomentumSGD with the kernel against its per-client torch path."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_gpu_training import synthetic_mnist

pytestmark = pytest.mark.gpu

K, HONEST, WD = 12, 9, 1e-3
BETA = float(np.float32(0.9))        # the fp32 the C ABI is handed, so the reference uses it too
SHAPES = [(10, 784, 50), (62, 784, 50), (10, 783, 50), (3, 33, 7), (10, 784, 64), (10, 784, 1)]


def _problem(C, F, B, K=K, n=3000, seed=0):
    g = torch.Generator().manual_seed(1000 * C + F + B + seed)
    x = 0.3 * torch.randn(n, F, generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    idx = torch.randint(0, n, (K, B), generator=g, dtype=torch.int32)
    W = 0.05 * torch.randn(C, F, generator=g)
    b = torch.full((C,), 0.01)
    M0 = 0.02 * torch.randn(K, C * F + C, generator=g)
    return x, y, idx, W, b, M0


def _grads64(x, y, idx, W, b, honest, attack, wd):
    """g_k = grad meanCE(theta; batch k) + wd theta in float64 autograd, every client at the
    SAME theta (test_gpu_training._chain_reference without the chain)."""
    C = W.shape[0]
    rows = []
    for k in range(idx.shape[0]):
        xb, yb = x[idx[k].long()].double(), y[idx[k].long()].clone()
        if k >= honest and attack == 1:
            yb = (C - 1) - yb
        if k >= honest and attack == 2:
            xb = 1.0 - xb
        Wv, bv = W.double().clone().requires_grad_(), b.double().clone().requires_grad_()
        torch.nn.functional.cross_entropy(xb @ Wv.T + bv, yb).backward()
        rows.append(torch.cat([(Wv.grad + wd * W.double()).flatten(), bv.grad + wd * b.double()]))
    return torch.stack(rows)


@functools.lru_cache(maxsize=None)
def _case(C, F, B, attack):
    """(problem on the CPU, fp64 gradient rows), computed once per case and never modified."""
    p = _problem(C, F, B)
    return p, _grads64(*p[:5], HONEST, attack, WD)


def _launch(dev, buf, ldx, lay, C, F, B, K, honest, attack, beta, wd=WD, ldd=None):
    """dev = (x, y, idx, W, b) on the GPU; returns the status."""
    import byzantine_aircomp_amd as bz
    x, y, idx, W, b = dev
    ctx = bz.context()
    rc = ctx.lib.gm_client_grads_f32(ctx.handle, x.data_ptr(), F if ldd is None else ldd,
                                     y.data_ptr(), F, C, idx.data_ptr(), K, B, honest, attack, beta,
                                     wd, W.data_ptr(), b.data_ptr(), buf.data_ptr(), ldx, lay,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _run_rows(dev, M0, d, *args, pad=3):
    """Rows with ldx = d + pad in a NaN-filled buffer (M0 None: the rows NaN too)."""
    from byzantine_aircomp_amd import _lib
    Kk = dev[2].shape[0]
    buf = torch.full((Kk, d + pad), float("nan"), device="cuda")
    if M0 is not None:
        buf[:, :d] = M0.cuda()
    assert _launch(dev, buf, d + pad, _lib.GM_LAYOUT_ROWS, *args) == 0
    return buf


def _run_panels(dev, M0, d, *args):
    from byzantine_aircomp_amd import _lib
    from byzantine_aircomp_amd.panels import ClientPanels
    Kk = dev[2].shape[0]
    P = ClientPanels(Kk, d)
    if M0 is None:
        P.data.fill_(float("nan"))
    else:
        P.copy_rows_(M0.cuda())
    assert _launch(dev, P.data, P.panel_stride, _lib.GM_LAYOUT_PANELS, *args) == 0
    return P


@pytest.mark.parametrize("layout", ["rows", "panels"])
@pytest.mark.parametrize("attack", [0, 1, 2])
@pytest.mark.parametrize("C,F,B", SHAPES)
def test_client_grads_kernel_vs_fp64(C, F, B, attack, layout):
    """Every row within rel L2 1e-6 of fp64 (the chain kernel's bar; torch's own fp32 autograd
    sits at 1.4-1.5e-7 on these rows): beta = 0 on a NaN-filled M (write-only) and beta = 0.9
    from a random M0.  Nothing at or past column d is written; W and b are not written."""
    (x, y, idx, W, b, M0), G = _case(C, F, B, attack)
    d = C * F + C
    dev = tuple(t.cuda() for t in (x, y, idx, W, b))
    for beta, start, want in ((0.0, None, G), (BETA, M0, BETA * M0.double() + (1.0 - BETA) * G)):
        args = (C, F, B, K, HONEST, attack, beta)
        if layout == "rows":
            buf = _run_rows(dev, start, d, *args)
            got = buf[:, :d]
            assert bool(torch.isnan(buf[:, d:]).all())
        else:
            P = _run_panels(dev, start, d, *args)
            got = P.to_rows()
            if d % P.W:
                pad = P.data[-1, :, d % P.W:]
                assert bool(torch.isnan(pad).all() if start is None else (pad == 0).all())
        assert bool(torch.isfinite(got).all())
        for k in range(K):
            assert rel_l2(got[k].cpu().numpy(), want[k].numpy()) <= 1e-6, (beta, k)
        assert torch.equal(dev[3].cpu(), W) and torch.equal(dev[4].cpu(), b)


def test_recursion_over_three_launches():
    """M carried over three launches with the model changed between them."""
    C, F, B, attack = 10, 784, 50, 1
    (x, y, idx, W, b, _), _ = _case(C, F, B, attack)
    d = C * F + C
    g = torch.Generator().manual_seed(5)
    M = torch.zeros(K, d, device="cuda")
    M64 = torch.zeros(K, d, dtype=torch.float64)
    from byzantine_aircomp_amd import _lib
    for t in range(3):
        Wt = W + 0.02 * t * torch.randn(C, F, generator=g)
        bt = b + 0.01 * t
        it = torch.randint(0, len(x), (K, B), generator=g, dtype=torch.int32)
        dev = tuple(v.cuda() for v in (x, y, it, Wt, bt))
        assert _launch(dev, M, d, _lib.GM_LAYOUT_ROWS, C, F, B, K, HONEST, attack, BETA) == 0
        M64 = BETA * M64 + (1.0 - BETA) * _grads64(x, y, it, Wt, bt, HONEST, attack, WD)
        for k in range(K):
            assert rel_l2(M[k].cpu().numpy(), M64[k].numpy()) <= 1e-6, (t, k)


@pytest.mark.parametrize("C,F,B", [(10, 784, 50), (62, 784, 50), (3, 33, 7)])
def test_rows_are_independent_bit_for_bit(C, F, B):
    """Row k depends only on (W, b, batch k, k >= honest, M_k): the same bits from a K = 1
    launch with that client's indices and flag, from the other layout, and from a second run."""
    attack = 1
    (x, y, idx, W, b, M0), _ = _case(C, F, B, attack)
    d = C * F + C
    dev = tuple(t.cuda() for t in (x, y, idx, W, b))
    args = (C, F, B, K, HONEST, attack, BETA)
    rows = _run_rows(dev, M0, d, *args)[:, :d]
    assert torch.equal(rows, _run_rows(dev, M0, d, *args, pad=0))
    assert torch.equal(rows, _run_panels(dev, M0, d, *args).to_rows())
    for k in (7, 10):                                   # an honest and a Byzantine client
        one = (dev[0], dev[1], idx[k:k + 1].cuda(), dev[3], dev[4])
        honest1 = 1 if k < HONEST else 0
        got = _run_rows(one, M0[k:k + 1], d, C, F, B, 1, honest1, attack, BETA)[:, :d]
        assert torch.equal(got[0], rows[k]), k


def test_more_blocks_than_cus():
    C, F, B, Kb, honest = 4, 64, 8, 300, 250
    x, y, idx, W, b, M0 = _problem(C, F, B, K=Kb, n=5000)
    d = C * F + C
    want = BETA * M0.double() + (1.0 - BETA) * _grads64(x, y, idx, W, b, honest, 2, WD)
    dev = tuple(t.cuda() for t in (x, y, idx, W, b))
    got = _run_rows(dev, M0, d, C, F, B, Kb, honest, 2, BETA)[:, :d].cpu().numpy()
    for k in range(Kb):
        assert rel_l2(got[k], want[k].numpy()) <= 1e-6, k


def test_c_abi_errors_write_nothing():
    from byzantine_aircomp_amd import _lib
    INVALID, UNSUPPORTED = -1, -3
    n = 200
    x = torch.zeros(n, 833, device="cuda")
    y = torch.zeros(n, dtype=torch.int64, device="cuda")
    idx = torch.zeros(K, 65, dtype=torch.int32, device="cuda")
    W = torch.zeros(65, 833, device="cuda")
    b = torch.zeros(65, device="cuda")
    dev = (x, y, idx, W, b)
    d_max = 65 * 833 + 65
    M = torch.randn(K, d_max, device="cuda")
    before = M.clone()
    C, F, B, d = 10, 784, 50, 7850
    rows = _lib.GM_LAYOUT_ROWS

    def call(C=C, F=F, B=B, honest=HONEST, attack=0, beta=0.5, ldx=d_max, lay=rows):
        rc = _launch(dev, M, ldx, lay, C, F, B, K, honest, attack, beta, ldd=833)
        assert torch.equal(M, before)
        return rc
    assert call(F=833) == UNSUPPORTED and b"F=833" in _lib.load().gm_last_error()
    assert call(C=65) == UNSUPPORTED
    assert call(B=65) == UNSUPPORTED
    assert call(beta=1.0) == INVALID
    assert call(beta=float("nan")) == INVALID
    assert call(beta=-0.1) == INVALID
    assert call(honest=K + 1) == INVALID
    assert call(ldx=d - 1) == INVALID
    assert call(attack=3) == INVALID
    assert call(lay=7) == INVALID
    assert call(B=0) == INVALID


def _loop(T, aggregate, attack, layout, client_kernel, data, noise_var=None, beta=0.9):
    tr, va = data
    model = T.modelFactory(SEED=2021).cuda()
    res = T.MomentumSGD(model, gamma=5e-2, aggregate=aggregate, weight_decay=1e-3,
                        noise_var=noise_var, honestSize=45, byzantineSize=5, attack=attack,
                        rounds=2, displayInterval=3, SEED=2021, fixSeed=True,
                        loss_func=torch.nn.CrossEntropyLoss(), train_dataset=tr,
                        validate_dataset=va, device=torch.device("cuda"), batchSize=50,
                        verbose=False, layout=layout, client_kernel=client_kernel, beta=beta)
    m, tl, _, vl, _, var = res
    w = torch.cat([p.detach().flatten() for p in m.parameters()]).cpu().numpy()
    return w, tl, vl, [float(v) for v in var]


@pytest.fixture(scope="module")
def data():
    return (torch.utils.data.TensorDataset(*synthetic_mnist(601, 2000)),
            torch.utils.data.TensorDataset(*synthetic_mnist(602, 500)))


@pytest.mark.parametrize("layout", ["rows", "panels"])
@pytest.mark.parametrize("combo", ["gm2-classflip", "cclip-alie", "mixed_gm2-ipm"])
def test_loop_kernel_equals_torch_loop(combo, layout, data):
    """MomentumSGD with gm_client_grads_f32 vs its per-client torch path on the GPU: 45 + 5
    clients, 2 rounds x 3 steps, to the bars of test_loop_client_kernel_equals_torch_loop."""
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import attacks
    from byzantine_aircomp_amd import training as T
    aggregate, attack = {
        "gm2-classflip": (bz.gm2, T.classflip),
        "cclip-alie": (bz.cclip.with_options(tau=1.0), attacks.alie),
        "mixed_gm2-ipm": (bz.aggregators.mixed(bz.gm2), attacks.ipm)}[combo]
    w0 = torch.cat([p.detach().flatten() for p in T.modelFactory(SEED=2021).parameters()]).numpy()
    (w1, tl1, vl1, v1), (w2, tl2, vl2, v2) = (
        _loop(T, aggregate, attack, layout, ck, data) for ck in (True, False))
    assert rel_l2(w1, w0) > 1e-3                          # (the model moved)
    assert rel_l2(w1, w2) <= 1e-5
    np.testing.assert_allclose(tl1, tl2, rtol=1e-5)
    np.testing.assert_allclose(vl1, vl2, rtol=1e-5)
    np.testing.assert_allclose(v1, v2, rtol=1e-4)


@pytest.mark.parametrize("layout", ["rows", "panels"])
def test_loop_with_aircomp_noise_stays_finite(layout, data):
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import training as T
    w, tl, vl, var = _loop(T, bz.gm, T.classflip, layout, True, data, noise_var=1e-2)
    assert np.isfinite(w).all() and np.isfinite(tl).all() and np.isfinite(vl).all()
    assert np.isfinite(var).all()
