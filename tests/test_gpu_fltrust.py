"""FLTrust on the GPU (fltrust.hip through gm_fltrust_f32 / _bf16 and aggregators.fltrust)
against the np.longdouble reference of fltrust_cases.py: every K regime and its edges, d ragged
against the 4- and 8-column vectors and the panel widths; contiguous rows, a misaligned strided
view, panels with NaN padding; fp32 and bf16; the server as a vector and as a row; with and
without a centre.  Then the skipped rows, the degenerate inputs, determinism, the d-sharded host
path and the plumbing (CPU tensors, bucketed, the training loop)."""
import threading

import numpy as np
import pytest
import torch

import fltrust_cases as fc

pytestmark = pytest.mark.gpu

LAYOUTS = ("rows", "strided", "panels")
DTYPES = ("fp32", "bf16")
COMBOS = (("vector", True), ("row", True), ("vector", False), ("row", False))


def _operand(X, layout):
    """X (a CUDA [K, d] tensor) as the aggregator's input in `layout`."""
    import byzantine_aircomp_amd as bz
    K, d = X.shape
    if layout == "rows":
        return X.contiguous()
    if layout == "strided":
        # one element into a NaN-filled buffer, an odd row stride: no 16-byte alignment anywhere
        ld = d + 1 if d % 2 == 0 else d + 2
        buf = torch.full((K * ld + 1,), float("nan"), dtype=X.dtype, device=X.device)
        view = buf[1:].view(K, ld)[:, :d]
        view.copy_(X)
        assert view.data_ptr() % 16 != 0 and view.stride(0) % 2 == 1
        return view
    P = bz.ClientPanels.from_rows(X)
    if d % P.W:
        P.data[-1, :, d % P.W:] = float("nan")       # the last panel's padding columns
    return P


def _options(s, row, c, dev):
    o = {"guess": None if c is None else c.to(dev)}
    if s is not None:
        o["server_update"] = s.to(dev)
    else:
        o["server_row"] = row
    return o


def _stats():
    import byzantine_aircomp_amd as bz
    info = bz.fltrust.last_info
    return torch.cat([info["cos"], info["norm2"], info["trust"], info["server_norm2"].reshape(1),
                      info["trust_sum"].reshape(1)]).cpu().numpy()


def _call(K, d, dtype, server, centre, layout):
    import byzantine_aircomp_amd as bz
    (X, s, row, c, _), ref = fc.case(K, d, dtype, server, centre)
    dev = torch.device("cuda")
    W = _operand(X.to(dev), layout)
    out = bz.fltrust(W, _options(s, row, c, dev))
    assert out.dtype == torch.float32 and out.shape == (d,) and out.device.type == "cuda"
    return out, ref


def _combo(si, li, di):
    # every shape meets all four (server, centre) combinations over its six (layout, dtype) cases
    return COMBOS[(si + li + 2 * di) % 4]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K,d", fc.SHAPES)
def test_matches_reference(K, d, layout, dtype):
    server, centre = _combo(fc.SHAPES.index((K, d)), LAYOUTS.index(layout), DTYPES.index(dtype))
    what = f"{K}x{d} {layout} {dtype} server={server} centre={centre}"
    out, ref = _call(K, d, dtype, server, centre, layout)
    fc.check_stats(_stats(), ref, K, d, what)        # (with the trusted set, compared exactly)
    fc.check_out(out.cpu().numpy(), ref, d, what)


@pytest.mark.parametrize("layout,dtype", [("rows", "fp32"), ("panels", "fp32"), ("rows", "bf16")])
def test_large_d_wraps_both_grids(layout, dtype):
    """K = 5, d = 4,300,009.  The figures assume the MI355X's 256 CUs (the host sizes pass A's
    grid from the device's CU count).  Pass A's grid is two blocks per CU (512 blocks) over
    ceil(d / 256) = 16,797 chunks (8,399 chunks of 512 columns for bf16): every block walks 16
    to 33 chunks.  Pass B has ceil(d / 4) / 256 = 4,200 blocks of work (2,100 at 8 columns per
    thread for bf16) for a grid capped at 2,048 blocks: its grid stride wraps."""
    K, d = fc.LARGE
    what = f"{K}x{d} {layout} {dtype}"
    out, ref = _call(K, d, dtype, "vector", True, layout)
    fc.check_stats(_stats(), ref, K, d, what)
    fc.check_out(out.cpu().numpy(), ref, d, what)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_skipped_rows_are_not_read_and_X_is_not_written(layout, dtype):
    import byzantine_aircomp_amd as bz
    K, d = 50, 7850
    (X, s, row, c, kinds), ref = fc.case(K, d, dtype, "vector", True)
    dev = torch.device("cuda")
    opts = _options(s, row, c, dev)
    Xg = X.to(dev)
    W = _operand(Xg, layout)
    data = W.data if isinstance(W, bz.ClientPanels) else W
    before = data.clone()
    out = bz.fltrust(W, opts)
    after = data.clone()
    assert torch.equal(before.view(torch.int16 if dtype == "bf16" else torch.int32),
                       after.view(torch.int16 if dtype == "bf16" else torch.int32))
    bad = [k for k, kind in enumerate(kinds) if kind in ("nan", "inf")]
    assert len(bad) >= 2
    Y = Xg.clone()
    junk = torch.tensor([1e30, float("nan"), float("-inf")], device=dev).to(Y.dtype)
    for k in bad:
        keep = ~torch.isfinite(Y[k].float())         # the row's own NaN / inf entry stays
        fill = junk[torch.arange(d, device=dev) % 3]
        Y[k] = torch.where(keep, Y[k], fill)
    out2 = bz.fltrust(_operand(Y, layout), opts)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    fc.check_out(out2.cpu().numpy(), ref, d, f"junk rows {layout} {dtype}")


@pytest.mark.parametrize("layout", ["rows", "panels"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_inputs_return_the_centre(layout, dtype):
    import byzantine_aircomp_amd as bz
    dev = torch.device("cuda")
    K, d = 17, 2051
    (X, s, _, c, _), _ = fc.case(K, d, dtype, "vector", True)
    tdt = X.dtype
    c, s = c.to(dev), s.to(dev)
    # every row sign-flipped: X = c - 3 (s - c)-ish updates, all cosines negative
    U = (X.to(dev).float() - c)
    honest = U[torch.isfinite(U).all(dim=1) & (U.abs().sum(dim=1) > 0)]
    g = s - c
    honest = honest[(honest @ g) > 0]
    assert honest.shape[0] >= 5
    flipped = (c - 3.0 * honest).to(tdt)
    out = bz.fltrust(_operand(flipped, layout), {"server_update": s, "guess": c})
    assert torch.equal(out.view(torch.int32), c.view(torch.int32))
    assert float(bz.fltrust.last_info["trust_sum"]) == 0.0
    out = bz.fltrust(_operand((-3.0 * honest).to(tdt), layout), {"server_update": g})
    assert torch.equal(out.view(torch.int32), torch.zeros_like(out).view(torch.int32))
    # K = 1 with the row as the server
    out = bz.fltrust(_operand(X[:1].to(dev), layout), {"server_row": 0, "guess": c})
    assert torch.equal(out.view(torch.int32), c.view(torch.int32))
    # a zero server update
    out = bz.fltrust(_operand(X.to(dev), layout), {"server_update": c, "guess": c})
    assert torch.equal(out.view(torch.int32), c.view(torch.int32))
    assert float(bz.fltrust.last_info["server_norm2"]) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,d", [(50, 7850), (1000, 2051)])
def test_deterministic_and_layouts_agree(K, d, dtype):
    import byzantine_aircomp_amd as bz
    (X, s, row, c, _), ref = fc.case(K, d, dtype, "vector", True)
    dev = torch.device("cuda")
    opts = _options(s, row, c, dev)
    outs = {}
    for layout in LAYOUTS:
        W = _operand(X.to(dev), layout)
        a = bz.fltrust(W, opts)
        sa = _stats()
        b = bz.fltrust(W, opts)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), layout
        assert np.array_equal(sa.view(np.int64), _stats().view(np.int64)), layout
        outs[layout] = a.cpu().numpy().astype(np.float64)
    bar = fc.out_bar(ref, d)
    for layout in ("strided", "panels"):
        w = float((np.abs(outs[layout] - outs["rows"]) / bar).max())
        print(f"fltrust {K}x{d} {dtype}: {layout} vs rows {w:.3e} of the bar")
        assert w <= 1.0


# ---- d-sharded, through the real host path ------------------------------------------------

def _sharded(X, s, row, c, P, panels):
    """P virtual ranks in P threads on one GPU, each with its own context holding a column
    shard; their all-reduce callback sums the 2K + 1 sums across the threads."""
    from byzantine_aircomp_amd import ClientPanels, _lib
    from byzantine_aircomp_amd.aggregators import Context
    from byzantine_aircomp_amd.sharded import _wrap, shard_range

    K, d = X.shape
    dev = X.device
    barrier = threading.Barrier(P, timeout=60)   # a rank-dependent collective count fails here
    bufs = [None] * P
    out = [None] * P
    counts = [0] * P
    errs = []

    def run(r):
        try:
            lo, hi = shard_range(d, P, r)
            ctx = Context(dev.index)
            ctx.set_shard(d, lo)

            def allreduce(ptr, count, stream):
                torch.cuda.synchronize(dev)
                assert count == 2 * K + 1
                counts[r] += 1
                t = _wrap(ptr, count, dev)
                bufs[r] = t.clone()
                barrier.wait()
                total = torch.stack(bufs).sum(0)
                barrier.wait()
                t.copy_(total)
                torch.cuda.synchronize(dev)
            ctx.set_allreduce(allreduce)
            Xs = X[:, lo:hi].contiguous()
            ptr, ldx, layout = Xs.data_ptr(), hi - lo, _lib.GM_LAYOUT_ROWS
            if panels:
                Xs = ClientPanels.from_rows(Xs)
                ptr, ldx, layout = Xs.data.data_ptr(), Xs.panel_stride, _lib.GM_LAYOUT_PANELS
            cs = c[lo:hi].contiguous()
            ss = s[lo:hi].contiguous() if s is not None else None
            res = torch.empty(hi - lo, device=dev)
            stats = torch.zeros(3 * K + 2, dtype=torch.float64, device=dev)
            _lib.check(ctx.lib.gm_fltrust_f32(
                ctx.handle, ptr, K, hi - lo, ldx, layout, ss.data_ptr() if ss is not None else None,
                -1 if s is not None else row, cs.data_ptr(), res.data_ptr(), stats.data_ptr(),
                None), "sharded fltrust")
            torch.cuda.synchronize(dev)
            out[r] = (lo, hi, res, stats.cpu().numpy())
            ctx.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
            barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    assert counts == [1] * P                     # one all-reduce per call, on every rank
    full = torch.empty(d, device=dev)
    for lo, hi, res, _ in out:
        full[lo:hi] = res
    return full, [o[3] for o in out]


@pytest.mark.parametrize("panels", [False, True])
@pytest.mark.parametrize("K,d,P,server", [(17, 2051, 3, "vector"), (600, 8200, 2, "row")])
def test_sharded_matches_reference_and_unsharded(K, d, P, server, panels):
    import byzantine_aircomp_amd as bz
    (X, s, row, c, _), ref = fc.case(K, d, "fp32", server, True)
    dev = torch.device("cuda")
    Xg = X.to(dev)
    whole = bz.fltrust(bz.ClientPanels.from_rows(Xg) if panels else Xg, _options(s, row, c, dev))
    got, stats = _sharded(Xg, None if s is None else s.to(dev), row, c.to(dev), P, panels)
    for st in stats[1:]:
        assert np.array_equal(st.view(np.int64), stats[0].view(np.int64))   # identical bits
    what = f"sharded {K}x{d} P={P} panels={panels}"
    fc.check_stats(stats[0], ref, K, d, what)
    fc.check_out(got.cpu().numpy(), ref, d, what)
    w = float((np.abs(got.cpu().numpy().astype(np.float64) - whole.cpu().numpy())
               / fc.out_bar(ref, d)).max())
    print(f"{what}: vs the unsharded call {w:.3e} of the bar")
    assert w <= 1.0


def test_sharded_gm_fltrust_world1():
    """ShardedGM.fltrust through torch.distributed (one rank, the torch all-reduce callback)."""
    import socket

    import torch.distributed as dist

    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd.sharded import ShardedGM
    K, d = 600, 8200
    (X, s, row, c, _), ref = fc.case(K, d, "fp32", "vector", True)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        sg = ShardedGM(d, transport="torch")
        try:
            with pytest.raises(ValueError, match="exactly one"):
                sg.fltrust(X.cuda(), {})
            for W in (X.cuda(), bz.ClientPanels.from_rows(X.cuda())):
                got = sg.fltrust(W, {"server_update": s.cuda(), "guess": c.cuda()})
                torch.cuda.synchronize()
                fc.check_out(got.cpu().numpy(), ref, d, "ShardedGM.fltrust")
                assert ([int(k) for k in torch.nonzero(sg.last_info["trust"] > 0).flatten()]
                        == ref["trusted"])
        finally:
            sg.close()
    finally:
        dist.destroy_process_group()


# ---- plumbing -----------------------------------------------------------------------------

def test_cpu_tensor_returns_on_the_cpu():
    import byzantine_aircomp_amd as bz
    K, d = 17, 2051
    (X, s, row, c, _), ref = fc.case(K, d, "fp32", "vector", True)
    out = bz.fltrust(X, {"server_update": s, "guess": c})
    assert out.device.type == "cpu" and out.dtype == torch.float32
    fc.check_out(out.numpy(), ref, d, "cpu tensor")
    assert bz.fltrust.last_info["cos"].device.type == "cuda"


def test_bucketed_fltrust_is_fltrust_on_the_bucket_means():
    import byzantine_aircomp_amd as bz
    K, d = 50, 7850
    (X, s, _, c, _), _ = fc.case(K, d, "fp32", "vector", True)
    Xg, s, c = X.cuda(), s.cuda(), c.cuda()
    Xg = torch.nan_to_num(Xg, nan=0.0, posinf=1.0)
    got = bz.bucketed(bz.fltrust.with_options(server_update=s), 2)(Xg, {"guess": c})
    means = bz.bucketing(Xg, 2, perm=bz.bucketing.last_perm, layout="panels")
    want = bz.fltrust(means, {"server_update": s, "guess": c})
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.isfinite(got).all() and not torch.equal(got, c)


def synthetic_mnist(seed, n):
    # the recipe of tests/golden/make_golden.py (as test_gpu_training.py's)
    proto = np.random.default_rng(600).standard_normal((10, 1, 28, 28)).astype(np.float32)
    r = np.random.default_rng(seed)
    y = r.integers(0, 10, n).astype(np.int64)
    x = (proto[y] + 2.0 * r.standard_normal((n, 1, 28, 28))).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y)


@pytest.mark.parametrize("layout", ["rows", "panels"])
def test_training_loop_with_fltrust(layout):
    """2 rounds x 3 steps of training.SGD, K = 10 with 2 alie rows, client 0's shard as the root
    dataset: finite losses and the by-products of the last step."""
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import training as T
    tr = torch.utils.data.TensorDataset(*synthetic_mnist(601, 400))
    va = torch.utils.data.TensorDataset(*synthetic_mnist(602, 100))
    model = T.modelFactory(SEED=2021).cuda()
    bz.fltrust.last_info = None
    res = T.SGD(model, gamma=1e-2, aggregate=bz.fltrust.with_options(server_row=0),
                weight_decay=0.0, honestSize=8, byzantineSize=2, attack=bz.alie, rounds=2,
                displayInterval=3, SEED=2021, fixSeed=True, loss_func=torch.nn.CrossEntropyLoss(),
                train_dataset=tr, validate_dataset=va, device=torch.device("cuda"), batchSize=20,
                verbose=False, layout=layout)
    _, tl, _, vl, _, _ = res
    assert len(tl) == 3 and np.isfinite(tl).all() and np.isfinite(vl).all()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    info = bz.fltrust.last_info
    assert info is not None and info["cos"].shape == (10,) and info["cos"].dtype == torch.float64
    assert float(info["trust"][0]) == 0.0            # the server row carries no weight itself
    assert abs(float(info["cos"][0]) - 1.0) < 1e-9
    assert float(info["trust_sum"]) >= 0.0 and float(info["server_norm2"]) > 0.0
