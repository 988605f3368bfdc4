"""Norm clipping on the GPU (clip.hip through gm_clip_rows_f32 / _bf16, aggregators.clip / arc /
clipped, ShardedGM.arc) against the np.longdouble reference of clip_cases.py: every K regime
and its edges, d ragged against the 4- and 8-column items and the panel widths; rows, panels
with NaN padding and misaligned strided views; fp32 and bf16; ARC and the static rule; out of
place and in place.  Then ties, the skipped rows, determinism, the d-sharded host path and the
plumbing (CPU tensors, clipped under mixed and bucketed, the training loop)."""
import threading

import numpy as np
import pytest
import torch

import clip_cases as cc

pytestmark = pytest.mark.gpu

LAYOUTS = ("rows", "panels")
DTYPES = ("fp32", "bf16")
RULES = (cc.ARC, cc.STATIC)


def _has_panels(K):
    from byzantine_aircomp_amd import _lib
    return _lib.load().gm_panel_width(K) > 0


def _strided(X, fill=float("nan")):
    """X in a view 4 bytes into a `fill`ed buffer with an odd row stride: no 16-byte alignment
    anywhere.  Returns (buffer, view)."""
    K, d = X.shape
    off = 1 if X.dtype == torch.float32 else 2
    ld = d + 1 if d % 2 == 0 else d + 2
    buf = torch.full((K * ld + off,), fill, dtype=X.dtype, device=X.device)
    view = buf[off:].view(K, ld)[:, :d]
    view.copy_(X)
    assert view.data_ptr() % 16 != 0 and view.stride(0) % 2 == 1
    return buf, view


def _operand(X, layout):
    """X (a CUDA [K, d] tensor) as the input in `layout`."""
    import byzantine_aircomp_amd as bz
    K, d = X.shape
    if layout == "rows":
        return X.contiguous()
    if layout == "strided":
        return _strided(X)[1]
    P = bz.ClientPanels.from_rows(X)
    if d % P.W:
        P.data[-1, :, d % P.W:] = float("nan")       # the last panel's padding columns
    return P


def _run(rule, W, f, tau, c, **kw):
    """(the clipped rows as the call returned them, the call's 2K + 2 stats as numpy)."""
    import byzantine_aircomp_amd as bz
    fn = bz.arc if rule == cc.ARC else bz.clip
    out = fn(W, f if rule == cc.ARC else tau, centre=c, **kw)
    info = fn.last_info
    stats = torch.cat([info["norm2"], info["scale"], info["threshold2"].reshape(1),
                       info["clipped"].reshape(1)]).cpu().numpy()
    return out, stats


def _np(out):
    """The clipped rows as an fp32 [K, d] numpy array."""
    import byzantine_aircomp_amd as bz
    if isinstance(out, bz.ClientPanels):
        out = out.to_rows()
    assert out.dtype == torch.float32
    return out.cpu().numpy()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check(out, stats, X, c, ref, K, d, rule, what):
    cc.check_stats(stats, ref, K, d, rule, what)
    cc.check_out(_np(out), X.to(torch.float32).numpy(), c.numpy(), ref, stats[K:2 * K], what)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K,d", cc.SHAPES)
def test_matches_reference(K, d, layout, dtype, rule):
    import byzantine_aircomp_amd as bz
    (X, c, _), ref, f, tau = cc.case(K, d, dtype, rule)
    dev = torch.device("cuda")
    what = f"{K}x{d} {layout} {dtype} {rule}"
    if layout == "panels" and not _has_panels(K):
        # K = 4096 has no panel width: the panel form of this case is the refusal
        with pytest.raises(ValueError, match="no panel layout"):
            _run(rule, X.to(dev), f, tau, c.to(dev), layout="panels")
        return
    out, stats = _run(rule, _operand(X.to(dev), layout), f, tau, c.to(dev))
    assert isinstance(out, bz.ClientPanels if layout == "panels" else torch.Tensor)
    assert tuple(out.shape) == (K, d) and out.device.type == "cuda"
    _check(out, stats, X, c, ref, K, d, rule, what)


@pytest.mark.parametrize("layout,dtype", [("rows", "fp32"), ("panels", "fp32"), ("rows", "bf16")])
def test_large_d_wraps_both_grids(layout, dtype):
    """K = 5, d = 4,300,009.  The figures assume the MI355X's 256 CUs.  Pass 1's grid is four
    blocks per CU (1,024 blocks; 768 for bf16) over ceil(d / 256) = 16,797 chunks (8,399 of 512
    columns for bf16): every block walks 8 to 17 chunks.  Pass 2 has 5 rows x ceil(d / 4 / 1024)
    = 5,250 tiles (2,625 for bf16; on panels one per panel, 16,797) for a grid capped at 2,048
    blocks: its grid stride wraps."""
    K, d = cc.LARGE
    (X, c, _), ref, f, _ = cc.case(K, d, dtype)
    dev = torch.device("cuda")
    out, stats = _run(cc.ARC, _operand(X.to(dev), layout), f, None, c.to(dev))
    _check(out, stats, X, c, ref, K, d, cc.ARC, f"{K}x{d} {layout} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,d", [(50, 7850), (1000, 2051)])
def test_out_layouts_hold_the_same_bits_and_calls_repeat(K, d, dtype):
    (X, c, _), ref, f, _ = cc.case(K, d, dtype)
    dev = torch.device("cuda")
    cg = c.to(dev)
    outs = {}
    for layout in LAYOUTS:
        W = _operand(X.to(dev), layout)
        a, sa = _run(cc.ARC, W, f, None, cg, layout="rows")
        b, sb = _run(cc.ARC, W, f, None, cg, layout="panels")
        assert np.array_equal(_np(a).view(np.int32), _np(b).view(np.int32)), layout
        assert np.array_equal(sa.view(np.int64), sb.view(np.int64)), layout
        a2, sa2 = _run(cc.ARC, W, f, None, cg, layout="rows")
        assert torch.equal(_bits(a), _bits(a2)) and np.array_equal(sa.view(np.int64),
                                                                   sa2.view(np.int64)), layout
        outs[layout] = _np(a).astype(np.float64)
    w = float((np.abs(outs["panels"] - outs["rows"]) / cc.out_bar(ref)).max())
    print(f"clip {K}x{d} {dtype}: panels in vs rows in {w:.3e} of the bar")
    assert w <= 1.0


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,d", [(17, 2051), (65, 333), (50, 7850)])
def test_unaligned_strided_views(K, d, dtype, rule):
    """A base 4 bytes off, an odd row stride, d no multiple of 4 or 8: the one-element path of
    both passes, out of place and (fp32) in place on the view itself."""
    (X, c, _), ref, f, tau = cc.case(K, d, dtype, rule)
    dev = torch.device("cuda")
    buf, view = _strided(X.to(dev))
    before = buf.clone()
    out, stats = _run(rule, view, f, tau, c.to(dev))
    assert torch.equal(_bits(before), _bits(buf))            # X and the NaN around it
    _check(out, stats, X, c, ref, K, d, rule, f"strided {K}x{d} {dtype} {rule}")
    if dtype == "fp32":
        got, stats2 = _run(rule, view, f, tau, c.to(dev), inplace=True)
        assert got is view
        assert np.array_equal(stats.view(np.int64), stats2.view(np.int64))
        assert torch.equal(_bits(view.contiguous()), _bits(out))
        pad = torch.ones_like(buf, dtype=torch.bool)
        pad[1:].view(K, -1)[:, :d] = False
        assert torch.equal(_bits(buf[pad]), _bits(before[pad]))   # the gaps between the rows


def _guarded(K, d, layout, X):
    """(operand whose storage sits inside a buffer of sentinels, buffer, mask of the operand's
    own elements): rows contiguous, or panels with NaN padding columns."""
    import byzantine_aircomp_amd as bz
    G = 4096
    if layout == "rows":
        buf = torch.full((K * d + 2 * G,), -7.0, device=X.device)
        W = buf[G:G + K * d].view(K, d)
        W.copy_(X)
        data = W
    else:
        P = bz.ClientPanels.from_rows(X)
        if d % P.W:
            P.data[-1, :, d % P.W:] = float("nan")
        buf = torch.full((P.data.numel() + 2 * G,), -7.0, device=X.device)
        data = buf[G:G + P.data.numel()].view(P.data.shape)
        data.copy_(P.data)
        P.data = data
        W = P
    own = torch.zeros_like(buf, dtype=torch.bool)
    own[G:G + data.numel()] = True
    return W, data, buf, own


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K,d", [(50, 7850), (600, 8200), (2048, 520)])
def test_in_place_equals_out_of_place(K, d, layout, rule):
    import byzantine_aircomp_amd as bz
    (X, c, _), ref, f, tau = cc.case(K, d, "fp32", rule)
    dev = torch.device("cuda")
    W, data, buf, own = _guarded(K, d, layout, X.to(dev))
    before = buf.clone()
    out, stats = _run(rule, W, f, tau, c.to(dev))
    assert torch.equal(_bits(before), _bits(buf))            # out of place: X is not written
    if layout == "panels" and d % W.W:
        assert not _np_pad(out).any()                        # the output's padding: not written
    got, stats2 = _run(rule, W, f, tau, c.to(dev), inplace=True)
    assert got is W
    assert np.array_equal(stats.view(np.int64), stats2.view(np.int64))
    assert np.array_equal(_np(got).view(np.int32), _np(out).view(np.int32))
    assert torch.equal(_bits(buf[~own]), _bits(before[~own]))     # the guard band
    if layout == "panels" and d % W.W:
        pad = data[-1, :, d % W.W:]
        assert torch.isnan(pad).all()                        # neither read as data nor written
    s = stats[K:2 * K]
    keep = torch.from_numpy(np.nonzero(s == 1)[0]).to(dev)
    rows = got.to_rows() if isinstance(got, bz.ClientPanels) else got
    assert torch.equal(_bits(rows[keep]), _bits(X.to(dev)[keep]))  # s = 1: the bits they had
    _check(got, stats2, X, c, ref, K, d, rule, f"in place {K}x{d} {layout} {rule}")


def _np_pad(P):
    return P.data[-1, :, P.d % P.W:].cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_mapped_to_the_centre_are_not_read(layout, dtype):
    K, d = 50, 7850
    (X, c, kinds), ref, f, _ = cc.case(K, d, dtype)
    dev = torch.device("cuda")
    Xg = X.to(dev)
    W = _operand(Xg, layout)
    out, stats = _run(cc.ARC, W, f, None, c.to(dev))
    bad = [k for k, kind in enumerate(kinds) if kind in ("nan", "inf")]
    assert len(bad) >= 2 and all(stats[K + k] == 0 for k in bad)
    Y = Xg.clone()
    junk = torch.tensor([1e30, float("nan"), float("-inf")], device=dev).to(Y.dtype)
    for k in bad:
        keep = ~torch.isfinite(Y[k].float())         # the row's own NaN / inf entry stays
        Y[k] = torch.where(keep, Y[k], junk[torch.arange(d, device=dev) % 3])
    out2, _ = _run(cc.ARC, _operand(Y, layout), f, None, c.to(dev))
    assert np.array_equal(_np(out).view(np.int32), _np(out2).view(np.int32))
    for k in bad:
        assert np.array_equal(_np(out2)[k].view(np.int32), c.numpy().view(np.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_tie_at_the_threshold_leaves_both_rows_unclipped(layout):
    """The threshold row copied over a row inside the radius: the (k + 1)-th largest norm is the
    same T, now held by two rows with the same n_k bits, and both are copies of their input.
    (The 2048 x 520 fp32 recipe case has such a tie of its own.)"""
    K, d = 64, 1000
    (X, c, _), ref, f, _ = cc.case(K, d)
    thr = int(np.nonzero(cc.at_threshold(ref))[0][0])
    small = int(np.nanargmin(np.asarray(ref["n"], dtype=np.float64)))
    assert small != thr and ref["s"][small] == 1
    X2 = X.clone()
    X2[small] = X2[thr]
    ref2 = cc.reference(X2.numpy(), c.numpy(), cc.ARC, f=f)
    cc.check_well_posed(ref2)
    assert ref2["T"] == ref["T"] and int(cc.at_threshold(ref2).sum()) == 2
    dev = torch.device("cuda")
    out, stats = _run(cc.ARC, _operand(X2.to(dev), layout), f, None, c.to(dev))
    n, s = stats[:K], stats[K:2 * K]
    assert n[small].view(np.int64) == n[thr].view(np.int64) == stats[2 * K].view(np.int64)
    assert s[small] == 1 and s[thr] == 1
    _check(out, stats, X2, c, ref2, K, d, cc.ARC, f"tie {layout}")


# ---- d-sharded, through the real host path ------------------------------------------------

def _sharded(X, c, f, P, panels):
    """P virtual ranks in P threads on one GPU, each with its own context holding a column
    shard; their all-reduce callback sums the K squared norms across the threads."""
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
                assert count == K
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
            res = torch.empty(K, hi - lo, device=dev)
            ptr, ldx, layout = Xs.data_ptr(), hi - lo, _lib.GM_LAYOUT_ROWS
            yptr, ldy = res.data_ptr(), hi - lo
            if panels:
                Xs = ClientPanels.from_rows(Xs)
                res = ClientPanels(K, hi - lo, device=dev, zero=False)
                ptr, ldx, layout = Xs.data.data_ptr(), Xs.panel_stride, _lib.GM_LAYOUT_PANELS
                yptr, ldy = res.data.data_ptr(), res.panel_stride
            cs = c[lo:hi].contiguous()
            stats = torch.zeros(2 * K + 2, dtype=torch.float64, device=dev)
            _lib.check(ctx.lib.gm_clip_rows_f32(
                ctx.handle, ptr, K, hi - lo, ldx, layout, cs.data_ptr(), _lib.GM_CLIP_ARC, f, 0.0,
                yptr, ldy, layout, stats.data_ptr(), None), "sharded arc")
            torch.cuda.synchronize(dev)
            out[r] = (lo, hi, res.to_rows() if panels else res, stats.cpu().numpy())
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
    full = torch.empty(K, d, device=dev)
    for lo, hi, res, _ in out:
        full[:, lo:hi] = res
    return full, [o[3] for o in out]


@pytest.mark.parametrize("panels", [False, True])
@pytest.mark.parametrize("K,d,P", [(17, 2051, 3), (600, 8200, 2)])
def test_sharded_matches_reference_and_unsharded(K, d, P, panels):
    import byzantine_aircomp_amd as bz
    (X, c, _), ref, f, _ = cc.case(K, d)
    dev = torch.device("cuda")
    Xg = X.to(dev)
    whole, _ = _run(cc.ARC, bz.ClientPanels.from_rows(Xg) if panels else Xg, f, None, c.to(dev))
    got, stats = _sharded(Xg, c.to(dev), f, P, panels)
    for st in stats[1:]:
        assert np.array_equal(st.view(np.int64), stats[0].view(np.int64))   # identical bits
    what = f"sharded {K}x{d} P={P} panels={panels}"
    _check(got, stats[0], X, c, ref, K, d, cc.ARC, what)
    w = float((np.abs(got.cpu().numpy().astype(np.float64) - _np(whole)) / cc.out_bar(ref)).max())
    print(f"{what}: vs the unsharded call {w:.3e} of the bar")
    assert w <= 1.0


def test_sharded_gm_arc_world1():
    """ShardedGM.arc / .clip through torch.distributed (one rank, the torch all-reduce
    callback)."""
    import socket

    import torch.distributed as dist

    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd.sharded import ShardedGM
    K, d = 600, 8200
    (X, c, _), ref, f, _ = cc.case(K, d)
    (_, _, _), sref, _, tau = cc.case(K, d, "fp32", cc.STATIC)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        sg = ShardedGM(d, transport="torch")
        try:
            with pytest.raises(ValueError, match="f "):
                sg.arc(X.cuda(), K)
            with pytest.raises(TypeError):
                sg.arc(X.cuda().to(torch.bfloat16), f)
            for W in (X.cuda(), bz.ClientPanels.from_rows(X.cuda())):
                got = sg.arc(W, f, centre=c.cuda())
                torch.cuda.synchronize()
                assert type(got) is type(W)
                info = sg.last_info
                stats = torch.cat([info["norm2"], info["scale"], info["threshold2"].reshape(1),
                                   info["clipped"].reshape(1)]).cpu().numpy()
                _check(got, stats, X, c, ref, K, d, cc.ARC, "ShardedGM.arc")
            got = sg.clip(X.cuda(), tau, centre=c.cuda())
            torch.cuda.synchronize()
            cc.check_out(_np(got), X.numpy(), c.numpy(), sref,
                         sg.last_info["scale"].cpu().numpy(), "ShardedGM.clip")
        finally:
            sg.close()
    finally:
        dist.destroy_process_group()


# ---- plumbing -----------------------------------------------------------------------------

def test_cpu_tensor_returns_on_the_cpu():
    import byzantine_aircomp_amd as bz
    K, d = 17, 2051
    (X, c, _), ref, f, _ = cc.case(K, d)
    out = bz.arc(X, f, centre=c)
    assert out.device.type == "cpu" and out.dtype == torch.float32 and out.shape == (K, d)
    s = bz.arc.last_info["scale"]
    assert s.device.type == "cuda"
    cc.check_out(out.numpy(), X.numpy(), c.numpy(), ref, s.cpu().numpy(), "cpu tensor")
    Y = X.clone()
    assert bz.arc(Y, f, centre=c, inplace=True) is Y and Y.device.type == "cpu"
    assert torch.equal(Y.view(torch.int32), out.view(torch.int32))
    P = bz.arc(X, f, centre=c, layout="panels")
    assert isinstance(P, bz.ClientPanels) and P.device.type == "cuda"
    assert torch.equal(P.to_rows().cpu().view(torch.int32), out.view(torch.int32))


def test_clipped_is_the_aggregate_of_the_clipped_rows():
    import byzantine_aircomp_amd as bz
    K, d = 50, 7850
    (X, c, _), _, f, tau = cc.case(K, d, "fp32", cc.STATIC)
    Xg, g = torch.nan_to_num(X.cuda(), nan=0.0, posinf=1.0), c.cuda()
    opts = {"guess": g, "honestSize": K - f, "maxiter": 50, "tol": 1e-6}
    keep, before = dict(opts), Xg.clone()

    def same(a, b):
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), b.view(torch.int32))

    got = bz.clipped(bz.gm2)(Xg, opts)
    same(got, bz.gm2(bz.arc(Xg, f, centre=g, layout="panels"), opts))
    assert got.shape == (d,) and not torch.equal(got, bz.gm2(Xg, opts))
    same(bz.clipped(bz.gm2, tau=tau, layout="rows")(Xg, opts),
         bz.gm2(bz.clip(Xg, tau, centre=g), opts))
    same(bz.clipped(bz.gm2)(Xg.to(torch.bfloat16), opts),
         bz.gm2(bz.arc(Xg.to(torch.bfloat16), f, centre=g, layout="panels"), opts))
    # under mixed: NNM first, then ARC on the mixed rows; and the other way round
    same(bz.mixed(bz.clipped(bz.gm2))(Xg, opts),
         bz.gm2(bz.arc(bz.nnm(Xg, f, layout="panels"), f, centre=g), opts))
    same(bz.clipped(bz.mixed(bz.gm2))(Xg, opts),
         bz.gm2(bz.nnm(bz.arc(Xg, f, centre=g, layout="panels"), f), opts))
    # under bucketed: the bucket means are clipped, with the rescaled honestSize
    got = bz.bucketed(bz.clipped(bz.gm2), 2)(Xg, opts)
    means = bz.bucketing(Xg, 2, perm=bz.bucketing.last_perm, layout="panels")
    same(got, bz.gm2(bz.arc(means, f, centre=g), dict(opts, honestSize=K // 2 - f)))
    for inner in (bz.mean, bz.median, bz.multi_krum):
        same(bz.clipped(inner)(Xg, opts), inner(bz.arc(Xg, f, centre=g, layout="panels"), opts))
    assert opts == keep and torch.equal(Xg.view(torch.int32), before.view(torch.int32))
    out = bz.clipped(bz.gm2)(X.nan_to_num(nan=0.0, posinf=1.0), dict(opts, guess=c))
    assert out.device.type == "cpu"


def synthetic_mnist(seed, n):
    # the recipe of tests/golden/make_golden.py (as test_gpu_training.py's)
    proto = np.random.default_rng(600).standard_normal((10, 1, 28, 28)).astype(np.float32)
    r = np.random.default_rng(seed)
    y = r.integers(0, 10, n).astype(np.int64)
    x = (proto[y] + 2.0 * r.standard_normal((n, 1, 28, 28))).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y)


def test_training_loop_with_clipped_gm2():
    """2 rounds x 3 steps of training.SGD, K = 10 with 2 alie rows, ARC about the current model
    ahead of gm2: finite, and the same losses when run again (to rtol 1e-4, the bar
    test_gpu_training.py holds the loop's losses to: the clients' torch steps are not pinned
    bit for bit)."""
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import training as T
    tr = torch.utils.data.TensorDataset(*synthetic_mnist(601, 400))
    va = torch.utils.data.TensorDataset(*synthetic_mnist(602, 100))

    def run():
        model = T.modelFactory(SEED=2021).cuda()
        bz.arc.last_info = None
        res = T.SGD(model, gamma=1e-2, aggregate=bz.clipped(bz.gm2), weight_decay=0.0,
                    honestSize=8, byzantineSize=2, attack=bz.alie, rounds=2, displayInterval=3,
                    SEED=2021, fixSeed=True, loss_func=torch.nn.CrossEntropyLoss(),
                    train_dataset=tr, validate_dataset=va, device=torch.device("cuda"),
                    batchSize=20, verbose=False)
        _, tl, _, vl, _, _ = res
        assert len(tl) == 3 and np.isfinite(tl).all() and np.isfinite(vl).all()
        assert all(torch.isfinite(p).all() for p in model.parameters())
        return tl, vl, torch.cat([p.detach().reshape(-1) for p in model.parameters()])

    tl, vl, w = run()
    info = bz.arc.last_info
    assert info is not None and info["scale"].shape == (10,)
    assert info["scale"].dtype == torch.float64
    # k = (2 * 2 * 8) // 10 = 3: at most 3 rows lie beyond T; fewer only by a tie at T, and the
    # two equal alie rows cannot fill the four largest places
    assert 1.0 <= float(info["clipped"]) <= 3.0
    assert float(info["threshold2"]) > 0.0
    tl2, vl2, w2 = run()
    np.testing.assert_allclose(tl2, tl, rtol=1e-4)
    np.testing.assert_allclose(vl2, vl, rtol=1e-4)
    np.testing.assert_allclose(w2.cpu().numpy(), w.cpu().numpy(), rtol=1e-4, atol=1e-6)
