"""The omniscient attacks on the GPU (byzantine_aircomp_amd.attacks, csrc/attack.hip) against
the numpy fp64 references of tests/attack_cases.py, whose docstring derives the tolerances."""
import numpy as np
import pytest
import torch

import attack_cases as ac
import bucket_cases as bc

pytestmark = pytest.mark.gpu

SENTINEL = 7.0                     # written into the panels' padding columns before an attack


def _operands(X, bf16):
    """[(name, wList, storage, before)]: bucket_cases.input_layouts, the tensor that holds all
    of the operand's memory (a view's NaN-filled buffer, the panels' data) and its bits."""
    import byzantine_aircomp_amd as bz
    out = []
    for name, w in bc.input_layouts(torch, bz, X, bf16):
        if isinstance(w, bz.ClientPanels):
            rem = w.d - (w.npan - 1) * w.W
            if rem < w.W:
                w.data[-1, :, rem:] = SENTINEL
            store = w.data
        else:
            store = w._base
        out.append((name, w, store, bc.raw_bits(torch, store).clone()))
    return out


def _check_untouched(name, w, store, before, B):
    """Everything but columns < d of the last B rows keeps its bits; returns the [K, d] result."""
    import byzantine_aircomp_amd as bz
    after = bc.raw_bits(torch, store)
    K, d = w.shape
    if isinstance(w, bz.ClientPanels):
        assert torch.equal(after[:, :K - B, :], before[:, :K - B, :]), name     # honest rows
        rem = d - (w.npan - 1) * w.W
        if rem < w.W:
            assert torch.equal(after[-1, :, rem:], before[-1, :, rem:]), name   # padding columns
        return w.to_rows().float().cpu().numpy()
    off = (w.data_ptr() - store.data_ptr()) // w.element_size()
    assert 0 <= off < store.shape[1]
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[K - B:, off:off + d] = False
    assert torch.equal(after[keep], before[keep]), name
    return w.float().cpu().numpy()


def _attack_all_layouts(attack, X, B, bf16):
    """The malicious row of every layout (asserted identical within and across layouts)."""
    rows = None
    for name, w, store, before in _operands(X, bf16):
        assert attack(w, B) is w
        R = _check_untouched(name, w, store, before, B)
        K = R.shape[0]
        assert np.array_equal(R[:K - B].view(np.uint32), np.asarray(X[:K - B]).view(np.uint32))
        byz = R[K - B:].view(np.uint32)
        assert (byz == byz[0]).all(), f"{name}: the Byzantine rows differ"
        if rows is None:
            rows = byz[0].copy()
        else:
            assert np.array_equal(rows, byz[0]), f"{name} differs from the first layout"
    return rows.view(np.float32)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,B,d", ac.CASES)
def test_alie_and_ipm_match_the_reference(K, B, d, bf16):
    import byzantine_aircomp_amd as bz
    X = bc.normal_matrix(K, d)
    if bf16:
        X = bc.widen_bf16(X)
    mismatch = ac.mismatch_bf16 if bf16 else ac.mismatch_f32
    got = _attack_all_layouts(bz.alie, X, B, bf16)
    z = ac.ref_z_max(K, B)
    assert bz.alie.last_z == z
    ref, slack = ac.ref_affine(X, B, 1.0, -z)
    assert mismatch(got, ref, slack) == 0
    got = _attack_all_layouts(bz.alie.with_options(z=1.5), X, B, bf16)
    assert bz.alie.last_z == 1.5
    ref, slack = ac.ref_affine(X, B, 1.0, -1.5)
    assert mismatch(got, ref, slack) == 0
    got = _attack_all_layouts(bz.ipm, X, B, bf16)
    ref, slack = ac.ref_affine(X, B, -0.1, 0.0)
    assert mismatch(got, ref, slack) == 0
    got = _attack_all_layouts(bz.ipm.with_options(epsilon=2.0), X, B, bf16)
    ref, slack = ac.ref_affine(X, B, -2.0, 0.0)
    assert mismatch(got, ref, slack) == 0


def _special_matrix():
    """K = 50, B = 10, d = 70: columns 0-5 all equal over the honest rows (small integers,
    1e6 + small integers, a value that is no fp32-exact tenth), column 6 small integers that
    vary, 7 a NaN, 8 and 9 a +inf (in the first row, in a later one), 10 a -inf; N(0, 1)
    elsewhere.  The Byzantine rows hold other values."""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((50, 70)).astype(np.float32)
    const = np.array([3.0, -17.0, 1e6 + 3, 1e6 + 12, 0.1, 0.0], dtype=np.float32)
    X[:40, :6] = const
    X[:40, 6] = 1e6 + (np.arange(40) % 3)
    X[5, 7] = np.nan
    X[0, 8] = np.inf
    X[9, 9] = np.inf
    X[3, 10] = -np.inf
    return X, const


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_exact_columns_and_special_values(bf16):
    import byzantine_aircomp_amd as bz
    X, const = _special_matrix()
    if bf16:
        X = bc.widen_bf16(X)
        const = X[0, :6]
    dt = torch.bfloat16 if bf16 else torch.float32
    mismatch = ac.mismatch_bf16 if bf16 else ac.mismatch_f32

    got = _attack_all_layouts(bz.alie.with_options(z=1.0), X, 10, bf16)
    assert np.array_equal(got[:6].view(np.uint32), const.view(np.uint32))    # sigma == 0: a x
    assert np.isnan(got[7:11]).all()                                          # NaN, inf - inf
    ref, slack = ac.ref_affine(X, 10, 1.0, -1.0)
    assert mismatch(got, ref, slack) == 0

    got = _attack_all_layouts(bz.ipm.with_options(epsilon=0.5), X, 10, bf16)
    assert np.array_equal(got[:6], -0.5 * const)                              # exact halves
    assert np.isnan(got[7]) and got[8] == -np.inf and got[9] == -np.inf and got[10] == np.inf
    got = _attack_all_layouts(bz.ipm, X, 10, bf16)
    want = torch.from_numpy(-0.1 * const.astype(np.float64)).to(dt).float().numpy()
    if not bf16:                              # (torch narrows fp64 to bf16 through fp32)
        assert np.array_equal(got[:6], want)                                  # a x rounded once
    ref, slack = ac.ref_affine(X, 10, -0.1, 0.0)
    assert mismatch(got, ref, slack) == 0


def test_alie_is_column_local():
    import byzantine_aircomp_amd as bz
    X = torch.from_numpy(np.array(bc.normal_matrix(50, 1536))).cuda()
    attack = bz.alie.with_options(z=0.7)
    full = attack(X.clone(), 10)[40:, 256:1280]
    part = X.clone()
    attack(part[:, 256:1280], 10)
    assert torch.equal(part[40:, 256:1280].view(torch.int32), full.view(torch.int32))
    assert torch.equal(part[:, :256], X[:, :256]) and torch.equal(part[:, 1280:], X[:, 1280:])
    P = bz.ClientPanels.from_rows(X[:, 256:1280])
    attack(P, 10)
    assert torch.equal(P.to_rows()[40:].view(torch.int32), full.view(torch.int32))


def test_cpu_and_strided_tensors_get_their_byzantine_rows_back():
    import byzantine_aircomp_amd as bz
    X = np.array(bc.normal_matrix(17, 1000))
    ref, slack = ac.ref_affine(X, 4, -0.1, 0.0)
    cpu = torch.from_numpy(X.copy())
    assert bz.ipm(cpu, 4) is cpu and cpu.device.type == "cpu"
    assert ac.mismatch_f32(cpu[16].numpy(), ref, slack) == 0
    assert np.array_equal(cpu[:13].numpy(), X[:13])
    t = torch.from_numpy(X.T.copy()).cuda().t()               # column stride 17
    assert t.stride(1) != 1
    bz.ipm(t, 4)
    assert torch.equal(t.cpu(), cpu)


@pytest.mark.parametrize("K,B,d", ac.MINMAX_CASES)
def test_minmax_and_minsum(K, B, d):
    import byzantine_aircomp_amd as bz
    X = bc.normal_matrix(K, d)
    geo = ac.honest_geometry(K, B, d)
    mu = geo["mu"]
    for rule, base in (("max", bz.minmax), ("sum", bz.minsum)):
        assert ac.amplification(geo, rule) <= 2.0
        bound = ac.bound_of(geo, rule)
        for dev in ac.DEVS:
            attack = base if dev == "std" else base.with_options(dev=dev)
            want, p = ac.ref_gamma(geo, rule, dev)
            row0 = None
            for name, w, store, before in _operands(X, False):
                base.last_gamma = None
                assert attack(w, B) is w
                g = base.last_gamma
                print(f"{rule} {dev} {name}: gamma {g!r} reference {want!r} "
                      f"rel {abs(g - want) / want:.2e}")
                assert abs(g - want) <= ac.GAMMA_RTOL * want, (rule, dev, name, g, want)
                R = _check_untouched(name, w, store, before, B)
                assert np.array_equal(R[:K - B].view(np.uint32), X[:K - B].view(np.uint32))
                byz = R[K - B:].view(np.uint32)
                assert (byz == byz[0]).all(), name
                m = R[K - B]
                slack = ac.EPS40 * (np.abs(mu) + np.abs(g * p)) + abs(g) * ac.EPS40 * np.abs(p)
                assert ac.mismatch_f32(m, mu - g * p, slack) == 0, (rule, dev, name)
                assert ac.constraint_value(geo, rule, m) <= bound * (1 + ac.GAMMA_RTOL)
                if row0 is None:
                    row0 = byz[0].copy()
                else:
                    assert np.array_equal(row0, byz[0]), f"{name} differs from the first layout"


def test_minmax_refusals_leave_the_matrix_alone():
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import _lib
    X = torch.from_numpy(np.array(bc.normal_matrix(7, 37))).cuda()
    keep = X.clone()
    ctx = bz.context(X.device)
    for args in ((7, 37, 36, 0, 2, 0, 0), (7, 37, 37, 2, 2, 0, 0), (7, 37, 37, 0, 0, 0, 0),
                 (7, 37, 37, 0, 6, 0, 0), (7, 37, 37, 0, 2, 2, 0), (7, 37, 37, 0, 2, 0, 3),
                 (7, 37, 7 * bz.panel_width(7) - 1, 1, 2, 0, 0), (5000, 37, 37, 0, 2, 0, 0)):
        with pytest.raises(_lib.GmError):
            ctx.call("gm_attack_minmax_f32", X.data_ptr(), *args, None, None)
    for args in ((7, 37, 36, 0, 2), (7, 37, 37, 5, 2), (7, 37, 37, 0, 0), (7, 37, 37, 0, 6)):
        with pytest.raises(_lib.GmError):
            ctx.call("gm_attack_affine_f32", X.data_ptr(), *args, 1.0, -1.0, None)
    ctx.call("gm_attack_affine_f32", X.data_ptr(), 7, 0, 37, 0, 2, 1.0, -1.0, None)   # d == 0
    torch.cuda.synchronize()
    assert torch.equal(X, keep)
    P = bz.ClientPanels(7, 37, W=2 * bz.panel_width(7))
    with pytest.raises(ValueError):
        bz.alie(P, 2)


@pytest.mark.parametrize("layout", ["rows", "panels"])
def test_training_loop_with_alie(layout):
    """One federated step of training.SGD under alie: the Byzantine clients train honestly, then
    their rows are overwritten from the honest rows' statistics."""
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import training as T
    from test_gpu_training import synthetic_mnist
    seen = []

    def alie(messages, byzantinesize):
        bz.alie(messages, byzantinesize)
        rows = messages.to_rows() if isinstance(messages, bz.ClientPanels) else messages
        seen.append(rows.detach().cpu().numpy().copy())
    tr = torch.utils.data.TensorDataset(*synthetic_mnist(601, 400))
    va = torch.utils.data.TensorDataset(*synthetic_mnist(602, 100))
    model = T.modelFactory(SEED=2021).cuda()
    T.SGD(model, gamma=1e-2, aggregate=bz.mean, weight_decay=0.0, honestSize=8, byzantineSize=2,
          attack=alie, rounds=1, displayInterval=1, SEED=2021, fixSeed=True,
          loss_func=torch.nn.CrossEntropyLoss(), train_dataset=tr, validate_dataset=va,
          device=torch.device("cuda"), batchSize=20, verbose=False, layout=layout)
    (R,) = seen
    assert R.shape == (10, 7850) and bz.alie.last_z == ac.ref_z_max(10, 2)
    ref, slack = ac.ref_affine(R, 2, 1.0, -ac.ref_z_max(10, 2))
    assert np.ptp(R[:8], axis=0).max() > 0                    # the honest rows differ
    for k in (8, 9):
        assert ac.mismatch_f32(R[k], ref, slack) == 0
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_robust_aggregators_on_an_attacked_matrix():
    import byzantine_aircomp_amd as bz
    X = torch.from_numpy(np.array(bc.normal_matrix(50, 70))).cuda()
    bz.alie(X, 10)
    for agg in (bz.bucketed(bz.gm2, 2), bz.cclip.with_options(tau=10.0)):
        out = agg(X, {"maxiter": 100, "tol": 1e-5, "honestSize": 40})
        assert out.shape == (70,) and torch.isfinite(out).all()
