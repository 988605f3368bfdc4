"""gm2 / gm on client updates stored as bf16 (gm_weiszfeld_bf16, stream_pass_bf16.hip).

A bf16 value widens to fp32 exactly, and everything but X is fp32 / fp64 as in the fp32
path, so the expected result is the project's oracle on the widened matrix,
oracle.gm2(X.float(), ...), at the project's bar: relative L2 <= 1e-5 and the iteration
count by assert_iter_count.  Inputs: the C3 recipe (honest rows N(0, 0.05^2), the last
K // 5 rows 0.25 + N(0, 0.5^2), guess N(0, 0.01^2)) from torch.Generator().manual_seed(1000
+ K), cast to bf16.  The shapes cover every pick_cfg tile, K not a multiple of the row
groups, K = 1024 exactly, d % 8 == 0 and not, and (1000 x 40008) more chunks (626 of 64
columns) than the grid has blocks (512), so some blocks roll into a second chunk and the
last chunk is ragged.  Every case also runs bz.gm2 / bz.gm on the widened fp32 matrix
(algo="stream") as a control on the input: it must meet the same bar.
"""
import pytest
import torch

from conftest import assert_iter_count, golden_case, rel_l2
from oracle import aggregators as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
# (K, d): the oracle's count on the widened matrix (tol 1e-5, maxiter 200), every window
# determined and 0 wide
SHAPES = {(3, 70): 11, (17, 1000): 5, (50, 7850): 4, (256, 16392): 4, (513, 333): 4,
          (600, 8200): 4, (1000, 2051): 4, (1024, 4096): 4, (1000, 40008): 4}
BF16 = torch.bfloat16


def bz():
    import byzantine_aircomp_amd as m
    return m


def recipe(K, d):
    g = torch.Generator().manual_seed(1000 + K)
    nb = K // 5
    X = torch.randn(K - nb, d, generator=g) * 0.05
    if nb:
        X = torch.cat([X, torch.randn(nb, d, generator=g) * 0.5 + 0.25])
    g0 = torch.randn(d, generator=g) * 0.01
    return X, g0


_CASES = {}


def case(K, d):
    """(bf16 X, guess, oracle aggregate, oracle trace, count window) on the CPU, computed
    once per shape and shared by the tests (never modified)."""
    if (K, d) not in _CASES:
        X, g0 = recipe(K, d)
        Xb = X.to(BF16)
        want, tr = orc.gm2(Xb.float(), {"maxiter": 200, "tol": 1e-5, "guess": g0})
        win = orc.gm2_count_window(Xb.float(), g0, 200, 1e-5)
        _CASES[(K, d)] = (Xb, g0, want, tr, win)
    return _CASES[(K, d)]


def bits(t):
    return t.contiguous().view(torch.int16)


def operand(Xb, layout):
    """The bf16 wList of one layout (on the GPU) and whether gm2 must pack it itself."""
    K, d = Xb.shape
    if layout == "panels":
        return bz().ClientPanels.from_rows(Xb.cuda())
    if layout == "rows":                     # the kernel reads the rows (d % 8 == 0) or gm2
        return Xb.cuda()                     # packs bf16 panels (d % 8 != 0)
    if layout == "strided":                  # ldx > d, rows still 16-byte aligned
        return torch.zeros(K, d + 8, dtype=BF16, device="cuda").copy_(
            torch.nn.functional.pad(Xb, (0, 8)).cuda())[:, :d]
    if layout == "misaligned":               # odd row stride and a 2-byte offset: packed
        buf = torch.zeros(K, d + 3, dtype=BF16, device="cuda")
        buf[:, 1:d + 1] = Xb.cuda()
        return buf[:, 1:d + 1]
    raise ValueError(layout)


def check_gm2(K, d, layout):
    Xb, g0, want, tr, win = case(K, d)
    assert win.determined and win.width <= 1, win
    assert tr.iters == SHAPES[(K, d)]
    W = operand(Xb, layout)
    keep = W.data.clone() if layout == "panels" else W.clone()
    opts = {"maxiter": 200, "tol": 1e-5, "guess": g0.cuda()}
    ctx = bz().context()
    ctx.pass_timing(True)
    got = bz().gm2(W, dict(opts))
    res = bz().aggregators.last_result
    _, launches = ctx.pass_timing(False)
    rel = rel_l2(got.cpu().numpy(), want.numpy())
    print(f"bf16 gm2 {K}x{d} {layout}: rel_l2={rel:.3e} iters={res.iters} (oracle {tr.iters}) "
          f"launches={launches}")
    assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == (d,)
    assert rel <= TOL
    assert_iter_count(res.iters, tr.iters, win)
    assert res.algo == "stream"
    assert launches == res.iters
    assert torch.equal(bits(W.data if layout == "panels" else W), bits(keep))   # X unchanged
    # control on the input: the fp32 streaming path on the widened matrix, same bar
    ctl = bz().gm2(Xb.float().cuda(), dict(opts, algo="stream"))
    rc = bz().aggregators.last_result
    assert rel_l2(ctl.cpu().numpy(), want.numpy()) <= TOL
    assert_iter_count(rc.iters, tr.iters, win)


@pytest.mark.parametrize("layout", ["panels", "rows"])
@pytest.mark.parametrize("K,d", list(SHAPES))
def test_gm2_bf16_matches_oracle(K, d, layout):
    check_gm2(K, d, layout)


@pytest.mark.parametrize("K,d,layout", [(600, 8200, "strided"), (50, 7850, "misaligned"),
                                        (1000, 2051, "misaligned")])
def test_gm2_bf16_strided_views(K, d, layout):
    check_gm2(K, d, layout)


def test_gm2_bf16_default_guess_and_cpu_input():
    """No guess: the fp32 column mean of the widened values; a CPU tensor is staged and the
    fp32 aggregate comes back on the CPU."""
    K, d = 50, 7850
    Xb = case(K, d)[0]
    want, tr = orc.gm2(Xb.float(), {"maxiter": 200, "tol": 1e-5})
    got = bz().gm2(Xb, {"maxiter": 200, "tol": 1e-5})
    assert got.device.type == "cpu" and got.dtype == torch.float32
    assert rel_l2(got.numpy(), want.numpy()) <= TOL
    assert abs(bz().aggregators.last_result.iters - tr.iters) <= 1
    P = bz().ClientPanels.from_rows(Xb.cuda())
    assert P.mean(0).dtype == torch.float32
    gp = bz().gm2(P, {"maxiter": 200, "tol": 1e-5})
    assert rel_l2(gp.cpu().numpy(), want.numpy()) <= TOL
    g0 = torch.zeros(d)
    assert bz().gm2(P, {"maxiter": 0, "guess": g0}) is g0


def test_bf16_padding_is_never_read_as_data():
    """The last panel's columns >= d hold bf16 NaN: the aggregate is the clean run's, bit
    for bit (1000 x 2051: 33 panels of 64 columns, 3 real columns in the last)."""
    K, d = 1000, 2051
    Xb, g0 = case(K, d)[:2]
    P = bz().ClientPanels.from_rows(Xb.cuda())
    opts = {"maxiter": 200, "tol": 1e-5, "guess": g0.cuda()}
    clean = bz().gm2(P, dict(opts))
    r0 = bz().aggregators.last_result
    rem = d - (P.npan - 1) * P.W
    assert 0 < rem < P.W
    P.data[-1, :, rem:] = float("nan")
    assert torch.isnan(P.data[-1, :, rem:].float()).all()
    assert torch.equal(bits(P.to_rows().cpu()), bits(Xb))
    dirty = bz().gm2(P, dict(opts))
    r1 = bz().aggregators.last_result
    assert torch.equal(clean, dirty) and torch.isfinite(dirty).all()
    assert (r0.iters, r0.last_movement) == (r1.iters, r1.last_movement)
    da = bz().gm(P, dict(opts, maxiter=3, noise_var=1e-3, seed=7))
    P.data[-1, :, rem:] = 0
    assert torch.equal(da, bz().gm(P, dict(opts, maxiter=3, noise_var=1e-3, seed=7)))


def _fixture_bf16():
    meta, arr = golden_case("gm_var1e-2_it5")
    assert meta.get("guess_supplied")
    return torch.from_numpy(arr["X"].copy()).to(BF16), torch.from_numpy(arr["guess"].copy()), meta


AIRCOMP = [("fixture", 3, 1e-2), ("fixture", 40, 1e-3), ("fixture", 25, None),
           ("recipe", 3, 1e-3), ("recipe", 5, None)]


@pytest.mark.parametrize("src,maxiter,var", AIRCOMP)
def test_gm_bf16_philox_matches_restatement(src, maxiter, var):
    """AirComp gm with Philox draws against oracle.gm fed the same draws
    (oracle.philox.gm_draws), on the widened matrix: equal iteration counts, rel L2 <= 1e-5."""
    from oracle.philox import gm_draws
    if src == "fixture":                      # 50 x 7850
        Xb, g0, _ = _fixture_bf16()
    else:
        Xb, g0 = case(1000, 2051)[:2]
    o = {"maxiter": maxiter, "tol": 1e-5, "noise_var": var, "P_max": 1, "guess": g0}
    draw = gm_draws(4242, Xb.shape[1])
    if var is None:
        draw.no_noise()
    ref, tr = orc.gm(Xb.float(), dict(o), draw=draw)
    assert torch.isfinite(ref).all() and tr.iters == maxiter
    gpu_o = dict(o, seed=4242, guess=g0.cuda())
    for wl in (bz().ClientPanels.from_rows(Xb.cuda()), Xb.cuda()):
        got = bz().gm(wl, dict(gpu_o))
        res = bz().aggregators.last_result
        rel = rel_l2(got.cpu().numpy(), ref.numpy())
        print(f"bf16 gm {src} maxiter={maxiter} var={var} {type(wl).__name__}: rel_l2={rel:.3e} "
              f"iters={res.iters}")
        assert got.dtype == torch.float32 and res.algo == "stream"
        assert res.iters == tr.iters
        assert rel <= TOL
    ctl = bz().gm(Xb.float().cuda(), dict(gpu_o, algo="stream"))
    assert bz().aggregators.last_result.iters == tr.iters
    assert rel_l2(ctl.cpu().numpy(), ref.numpy()) <= TOL


def test_gm_bf16_host_draws():
    """The reference's own torch.normal draws replayed (noise_source="host")."""
    Xb, g0, meta = _fixture_bf16()
    o = dict(meta["options"], guess=g0)
    torch.manual_seed(meta["rng_seed"])
    ref, tr = orc.gm(Xb.float(), dict(o))
    torch.manual_seed(meta["rng_seed"])
    got = bz().gm(bz().ClientPanels.from_rows(Xb.cuda()),
                  dict(o, guess=g0.cuda(), noise_source="host"))
    res = bz().aggregators.last_result
    assert res.iters == tr.iters and res.algo == "stream"
    assert rel_l2(got.cpu().numpy(), ref.numpy()) <= TOL


def _specials(X):
    """X with values the rounding can get wrong: +-inf, +-0, fp32 and bf16 subnormals, exact
    ties (low half 0x8000: to even), the largest finite fp32 (rounds to inf)."""
    sp = torch.tensor([0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                       0x00007FFF, 0x00008000, 0x00018000, 0x007FFFFF, 0x807F8000, 0x3F808000,
                       0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF,
                       0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF], dtype=torch.int64)
    sp = sp.where(sp < 2 ** 31, sp - 2 ** 32).to(torch.int32).view(torch.float32)
    X = X.clone()
    flat = X.view(-1)
    n = sp.numel()
    flat[:n] = sp                              # the first row segment
    flat[-n:] = sp                             # the ragged last panel
    flat[X.shape[1] * (X.shape[0] // 2) + 5:][:n] = sp
    return X


@pytest.mark.parametrize("K,d", [(1000, 2051), (50, 7850)])
def test_pack_bf16_bit_exact(K, d):
    X = _specials(recipe(K, d)[0])
    want = X.to(BF16)
    assert torch.isinf(want.float()).sum() >= 3 * 5          # the fp32 maxima rounded to inf too
    P = bz().ClientPanels.from_rows(X.cuda(), dtype=BF16)    # the converting kernel, 16-byte items
    assert P.dtype == BF16 and P.W == bz().panel_width(K, BF16)
    assert torch.equal(bits(P.to_rows().cpu()), bits(want))
    assert torch.count_nonzero(P.data[-1, :, d - (P.npan - 1) * P.W:]) == 0   # padding not written
    # a view 4 bytes off 16-byte alignment with an odd row stride: the scalar kernel
    Xo = torch.zeros(K, d + 1, device="cuda")
    Xo[:, 1:] = X.cuda()
    Po = bz().ClientPanels.from_rows(Xo[:, 1:], dtype=BF16)
    assert torch.equal(bits(Po.to_rows().cpu()), bits(want))
    # bf16 rows -> bf16 panels: exact, aligned and not
    Q = bz().ClientPanels.from_rows(want.cuda())
    assert Q.dtype == BF16 and torch.equal(bits(Q.to_rows().cpu()), bits(want))
    Wo = torch.zeros(K, d + 1, dtype=BF16, device="cuda")
    Wo[:, 1:] = want.cuda()
    assert torch.equal(bits(bz().ClientPanels.from_rows(Wo[:, 1:]).to_rows().cpu()), bits(want))
    # store / row on the device
    Q.store(3, want[7].cuda())
    assert torch.equal(bits(Q.row(3).cpu()), bits(want[7]))


def test_bf16_refusals():
    """What gm_weiszfeld_bf16 does not run is refused with the library's message."""
    from byzantine_aircomp_amd._lib import GmError
    Xb, g0 = case(17, 1000)[:2]
    X, g = Xb.cuda(), g0.cuda()
    P = bz().ClientPanels.from_rows(X)
    for wl in (X, P):
        for algo in ("gram", "resident", "twopass"):
            with pytest.raises(GmError, match="streaming pass only"):
                bz().gm2(wl, {"guess": g, "algo": algo})
        with pytest.raises(GmError, match="pre_oma is not supported"):
            bz().gm2(wl, {"guess": g, "pre_oma_var": 1e-2, "pre_oma_seed": 1})
        ctx = bz().context()
        ctx.set_shard(4000, 1000)
        try:
            with pytest.raises(GmError, match="sharded"):
                bz().gm2(wl, {"guess": g})
        finally:
            ctx.set_shard(-1, 0)
        bz().gm2(wl, {"guess": g})                       # the context is usable again
        assert bz().aggregators.last_result.algo == "stream"
    with pytest.raises(GmError, match="no streaming tile for K=4096"):
        bz().gm2(torch.zeros(4096, 64, dtype=BF16, device="cuda"), {"guess": torch.zeros(64)})
    assert torch.equal(bits(X.cpu()), bits(Xb))


def test_bf16_c_abi_rows_contract():
    """What the Python layer never sends: a row-major call the kernel cannot read in place is
    GM_ERR_UNSUPPORTED (the caller packs panels), and maxiter == 0 copies the guess."""
    import ctypes as C
    from byzantine_aircomp_amd import _lib
    K, d = 17, 1000
    g = case(K, d)[1].cuda()
    ctx = bz().context()
    o = _lib.GmOpts()
    o.maxiter, o.tol, o.eps = 5, 1e-5, 1e-4
    out = torch.full((d,), 7.0, device="cuda")
    buf = torch.zeros(K * (d + 8) + 8, dtype=BF16, device="cuda")
    call = lambda ptr, ldx: ctx.lib.gm_weiszfeld_bf16(          # noqa: E731
        ctx.handle, ptr, K, d, ldx, g.data_ptr(), out.data_ptr(), C.byref(o), None, None)
    assert call(buf.data_ptr(), d + 3) == -3                    # ldx % 8 != 0
    assert b"multiples of 8" in ctx.lib.gm_last_error()
    assert call(buf.data_ptr() + 2, d + 8) == -3                # 2 bytes off 16-byte alignment
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                   # nothing ran
    o.maxiter = 0
    assert call(buf.data_ptr(), d + 8) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, g)


def test_other_aggregators_still_refuse_bf16():
    Xb = case(17, 1000)[0]
    X = Xb.cuda()
    P = bz().ClientPanels.from_rows(X)
    for wl in (X, P):
        for f in (bz().mean, bz().median, bz().trimmed_mean):
            with pytest.raises(TypeError):
                f(wl)
        with pytest.raises(TypeError):
            bz().Krum(wl, {"honestSize": 14})
        with pytest.raises(TypeError):
            bz().OMA(wl, 1e-2, seed=1)
        with pytest.raises(TypeError):
            bz().aggregators.honest_variance(wl, 14)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError):
            bz().gm2(X.to(dt))
