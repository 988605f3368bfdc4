"""Centered clipping (bz.cclip, gm_cclip_f32 / gm_cclip_bf16) on the fused streaming pass.

Reference and inputs: tests/cclip_cases.py (the paper's recurrence in fp64 numpy on the C3
recipe).  Bar: relative L2 <= 1e-5 against it, the project's bar for gm2 against its oracle;
tests/test_cclip_cpu.py keeps the fp32 restatement of the kernels' arithmetic within 1e-6 of
the same reference on every input used here, and every dist_k / tau at least 0.5 away from
1 at every iteration, so the clipped counts are determined.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cclip_cases as cc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def bz():
    import byzantine_aircomp_amd as m
    return m


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def operand(X, layout):
    """The wList of one layout on the GPU (X: a CPU fp32 or bf16 [K, d] tensor)."""
    K, d = X.shape
    if layout == "panels":
        return bz().ClientPanels.from_rows(X.cuda())
    if layout == "rows":
        return X.cuda()
    if layout == "strided":                  # ldx > d, rows still 16-byte aligned
        buf = torch.zeros(K, d + 8, dtype=X.dtype, device="cuda")
        buf[:, :d] = X.cuda()
        return buf[:, :d]
    if layout == "misaligned":               # odd row stride, one element off 16-byte alignment
        buf = torch.zeros(K, d + 3, dtype=X.dtype, device="cuda")
        buf[:, 1:d + 1] = X.cuda()
        return buf[:, 1:d + 1]
    raise ValueError(layout)


def data_of(W):
    return W.data if isinstance(W, bz().ClientPanels) else W


def run_checked(W, g, opts, want, want_iters, want_clipped, label):
    """One cclip call with every per-case assertion of the parity tests."""
    keep, gkeep = data_of(W).clone(), g.clone()
    ctx = bz().context()
    ctx.pass_timing(True)
    got = bz().cclip(W, dict(opts, guess=g))
    res = bz().aggregators.last_result
    info = dict(bz().cclip.last_info)
    _, launches = ctx.pass_timing(False)
    rel = cc.rel_l2(got.cpu().numpy(), want)
    print(f"cclip {label}: rel_l2={rel:.3e} iters={res.iters} launches={launches} "
          f"clipped={info['clipped']} (reference {want_clipped}) movement={res.last_movement:.4e}")
    assert got.dtype == torch.float32 and got.device == g.device and got.shape == g.shape
    assert rel <= cc.TOL
    assert res.iters == want_iters and res.algo == "stream"
    assert launches == res.iters
    assert info["clipped"] == want_clipped
    assert torch.equal(bits(data_of(W)), bits(keep))        # X bit-unchanged
    assert torch.equal(bits(g), bits(gkeep))                # and the guess
    return got, res


def check_parity(K, d, dtype, layout):
    X, g0 = cc.inputs(K, d, dtype)
    W, g = operand(X, layout), g0.cuda()
    for name in cc.TAUS:
        vs, clipped, moves, _ = cc.ref_case(K, d, dtype, name)
        for it in cc.ITERS:
            opts = {"tau": cc.tau_of(name, d), "clip_iters": it}
            _, res = run_checked(W, g, opts, vs[it - 1], it, clipped[it - 1],
                                 f"{K}x{d} {dtype} {layout} tau={name} iters={it}")
            assert not res.converged
            # both iterates are within the bar of the reference's, so their distance is within
            # twice the bar (of the larger norm) of the reference's movement
            slack = 2 * cc.TOL * max(np.linalg.norm(v) for v in vs[:it]) + 1e-6 * moves[it - 1]
            assert abs(res.last_movement - moves[it - 1]) <= slack


@pytest.mark.parametrize("layout", ["rows", "panels"])
@pytest.mark.parametrize("K,d", cc.SHAPES)
def test_cclip_fp32_matches_reference(K, d, layout):
    check_parity(K, d, "fp32", layout)


@pytest.mark.parametrize("layout", ["rows", "panels"])
@pytest.mark.parametrize("K,d", cc.BF16_SHAPES)
def test_cclip_bf16_matches_reference(K, d, layout):
    """bf16 client updates; (513, 333) and (1000, 2051) have d % 8 != 0, so their rows are
    packed into bf16 panels by the Python layer."""
    check_parity(K, d, "bf16", layout)


@pytest.mark.parametrize("K,d,dtype,layout", [(600, 8200, "fp32", "strided"),
                                              (50, 7850, "fp32", "misaligned"),
                                              (1000, 2051, "fp32", "misaligned"),
                                              (600, 8200, "bf16", "strided"),
                                              (1000, 2051, "bf16", "misaligned")])
def test_cclip_strided_views(K, d, dtype, layout):
    check_parity(K, d, dtype, layout)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_cclip_cpu_input_is_staged(dtype):
    """A CPU tensor is staged to the GPU and the fp32 result comes back on the CPU; with no
    guess the start is the zero vector."""
    K, d = 50, 7850
    X, g0 = cc.inputs(K, d, dtype)
    vs, clipped, _, _ = cc.ref_case(K, d, dtype, "mid")
    run_checked(X, g0, {"tau": cc.tau_of("mid", d), "clip_iters": 3}, vs[2], 3, clipped[2],
                f"{K}x{d} {dtype} cpu")
    tau = cc.tau_of("mid", d)
    zs, zc, _, _ = cc.reference(X.float().numpy(), np.zeros(d), tau, 1)
    got = bz().cclip(X, {"tau": tau})
    assert got.device.type == "cpu" and got.dtype == torch.float32
    assert cc.rel_l2(got.numpy(), zs[0]) <= cc.TOL
    assert bz().cclip.last_info["clipped"] == zc[0]


def test_cclip_two_pass_beyond_2048_clients():
    """fp32 rows at K = 2049: no fused tile, the two-pass kernels."""
    K, d = 2049, 24
    X, g0 = cc.inputs(K, d)
    W, g = X.cuda(), g0.cuda()
    tau = cc.tau_of("mid", d)
    vs, clipped, _, margins = cc.reference(X.numpy(), g0.numpy(), tau, cc.MAX_ITERS)
    assert clipped[0] == K // 5 and min(margins) >= 0.1, (clipped, margins)
    for it in cc.ITERS:
        run_checked(W, g, {"tau": tau, "clip_iters": it}, vs[it - 1], it, clipped[it - 1],
                    f"{K}x{d} two-pass iters={it}")


# The scaled-guess check below amplifies one property of the arithmetic the library is
# specified to use, v' = sum_k c_k x_k + a v with c_k = fp32(1 / K): K fp32(1 / K) = 1 + e_K
# with |e_K| <= 2^-24, a = -e_K, so v' = mean + e_K (mean - v) — a relative error e_K of the
# STEP, which the bar measures against ||mean||.  On the recipe ||v - mean|| / ||mean|| is
# about 200 at scale 1e3, so the check is well posed only where 200 |e_K| is below the bar:
# e_17 = 3.7e-9, e_50 = -2.2e-8, e_1024 = 0, e_1000 = 4.75e-8 (9.5e-6: the tightest case
# kept); K = 3 (e_3 = 3.0e-8 on a guess 350 times the mean: 1.03e-5) is left out for that
# reason alone.
MEAN_SHAPES = [(17, 1000), (50, 7850), (1024, 4096), (1000, 2051)]
GUESS_SCALE = 1e3


@pytest.mark.parametrize("layout", ["rows", "panels"])
@pytest.mark.parametrize("K,d", MEAN_SHAPES)
def test_cclip_huge_radius_is_the_mean_step(K, d, layout):
    """tau = 1e6, one iteration: the column mean, from the recipe's guess and from a guess
    1e3 times larger (the reference itself is first held to 1e-6 of the fp64 mean there)."""
    X, g0 = cc.inputs(K, d)
    X32 = X.numpy()
    mean = X32.astype(np.float64).mean(axis=0)
    W = operand(X, layout)
    for scale in (1.0, GUESS_SCALE):
        v0 = g0 * scale
        ref = cc.reference(X32, v0.numpy(), 1e6, 1)
        assert ref[1] == [0]
        ref_rel = cc.rel_l2(ref[0][0], mean)
        assert ref_rel <= 1e-6, (scale, ref_rel)
        got = bz().cclip(W, {"tau": 1e6, "guess": v0.cuda()})
        rel = cc.rel_l2(got.cpu().numpy(), mean)
        print(f"cclip mean step {K}x{d} {layout} guess scale {scale:g}: rel_l2={rel:.3e} "
              f"(reference {ref_rel:.1e})")
        assert rel <= cc.TOL
        assert bz().cclip.last_info["clipped"] == 0
    got = bz().cclip(W, {"tau": math.inf, "guess": g0.cuda()})     # +inf is allowed
    assert cc.rel_l2(got.cpu().numpy(), mean) <= cc.TOL


def _ulps(a, b):
    """|a - b| in units of b's fp32 ulp, per element."""
    b64 = b.double()
    ulp = torch.ldexp(torch.ones_like(b64), torch.floor(torch.log2(b64.abs())).int() - 23)
    return ((a.double() - b64).abs() / ulp)


@pytest.mark.parametrize("layout", ["rows", "panels"])
@pytest.mark.parametrize("K,d", [(3, 70), (50, 7850), (1000, 2051), (1024, 4096)])
def test_cclip_identical_clients_are_a_fixed_point(K, d, layout):
    """All rows and the guess one vector u: dist_k = 0 is unclipped, sum c + a = 1, and the
    result is u within 1 fp32 ulp per element.

    The clipping STEP pass sums c_k x_k in fp64 for this: an fp32 sum of K terms c_k u is
    3-6 ulp off at K = 50-1024 (measured) whatever the coefficients are."""
    u = cc.inputs(K, d)[1] + 0.125
    W = operand(u.repeat(K, 1), layout)
    worst = {}
    for it in (1, 3):
        got = bz().cclip(W, {"tau": 0.5, "clip_iters": it, "guess": u.cuda()})
        worst[it] = float(_ulps(got.cpu(), u).max())
        print(f"cclip fixed point {K}x{d} {layout} iters={it}: max error {worst[it]:.2f} ulp")
        assert bz().cclip.last_info["clipped"] == 0
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("K,d", [(50, 7850), (1000, 2051)])
def test_cclip_translation_equivariance(K, d):
    X, g0 = cc.inputs(K, d)
    t = torch.full((d,), 0.5)
    opts = {"tau": cc.tau_of("mid", d), "clip_iters": 3}
    base = bz().cclip(X.cuda(), dict(opts, guess=g0.cuda()))
    moved = bz().cclip((X + t).cuda(), dict(opts, guess=(g0 + t).cuda()))
    rel = cc.rel_l2(moved.cpu().numpy(), (base.cpu().double() + t.double()).numpy())
    print(f"cclip translation {K}x{d}: rel_l2={rel:.3e}")
    assert rel <= cc.TOL


@pytest.mark.parametrize("layout", ["rows", "panels"])
@pytest.mark.parametrize("K,d", [(50, 7850), (1000, 2051)])
def test_cclip_step_is_bounded_by_the_radius(K, d, layout):
    """||v_1 - v_0|| <= mean_k min(dist_k, tau) <= tau, however far the Byzantine rows are."""
    X, g0 = cc.inputs(K, d)
    X = X.clone()
    X[K - K // 5:] *= 1e4
    tau = cc.tau_of("mid", d)
    got = bz().cclip(operand(X, layout), {"tau": tau, "guess": g0.cuda()})
    res = bz().aggregators.last_result
    print(f"cclip step bound {K}x{d} {layout}: movement={res.last_movement:.6e} tau={tau:.6e}")
    assert torch.isfinite(got).all()
    assert res.last_movement <= tau * (1 + 1e-5)
    assert float((got.cpu() - g0).double().norm()) <= tau * (1 + 1e-5)
    assert bz().cclip.last_info["clipped"] == K // 5


@pytest.mark.parametrize("K,d,check_every", [(50, 7850, 0), (50, 7850, 1), (1000, 2051, 1)])
def test_cclip_early_stop_and_exact_count(K, d, check_every):
    """clip_tol above the first movement stops after one iteration with `converged`;
    clip_tol=None runs exactly clip_iters.  check_every=1 takes the lagged poll (the default
    once K d >= 2^24, as in the (1000, 40008) parity cases)."""
    X, g0 = cc.inputs(K, d)
    W, g = X.cuda(), g0.cuda()
    tau = cc.tau_of("mid", d)
    vs, _, moves, _ = cc.ref_case(K, d, "fp32", "mid")
    opts = {"tau": tau, "clip_iters": 7, "guess": g, "check_every": check_every}
    ctx = bz().context()
    ctx.pass_timing(True)
    got = bz().cclip(W, dict(opts, clip_tol=2 * moves[0]))
    res = bz().aggregators.last_result
    _, launches = ctx.pass_timing(False)
    assert (res.iters, res.converged, launches) == (1, True, 1), (res, launches)
    assert res.last_movement == pytest.approx(moves[0], rel=1e-4)
    assert cc.rel_l2(got.cpu().numpy(), vs[0]) <= cc.TOL
    full = cc.reference(X.numpy(), g0.numpy(), tau, 7)
    got = bz().cclip(W, dict(opts, clip_tol=None))
    res = bz().aggregators.last_result
    assert (res.iters, res.converged) == (7, False), res
    assert cc.rel_l2(got.cpu().numpy(), full[0][6]) <= cc.TOL
    assert bz().cclip.last_info["clipped"] == full[1][6]


def test_cclip_zero_iterations_returns_the_guess_object():
    X, g0 = cc.inputs(17, 1000)
    g = g0.cuda()
    assert bz().cclip(X.cuda(), {"tau": 1.0, "clip_iters": 0, "guess": g}) is g
    assert bz().aggregators.last_result.iters == 0


def test_cclip_with_options_takes_the_training_loop_dict():
    """The dict training.SGD builds, unchanged: every key but the guess is ignored."""
    K, d = 50, 7850
    X, g0 = cc.inputs(K, d)
    W, g = X.cuda(), g0.cuda()
    tau = cc.tau_of("mid", d)
    direct = bz().cclip(W, {"tau": tau, "clip_iters": 3, "guess": g})
    agg = bz().cclip.with_options(tau=tau, clip_iters=3)
    assert agg.__name__ == "cclip"
    sgd = {"maxiter": 1000, "tol": 1e-5, "eta": 1, "noise_var": 1e-2, "guess": g,
           "honestSize": K - K // 5}
    keep = dict(sgd)
    got = agg(W, sgd)
    assert sgd == keep                                       # the caller's dict is not edited
    assert torch.equal(got, direct)
    assert bz().aggregators.last_result.iters == 3
    assert cc.rel_l2(got.cpu().numpy(), cc.ref_case(K, d, "fp32", "mid")[0][2]) <= cc.TOL


def test_cclip_non_finite_inputs_return():
    """NaN / inf rows may give a non-finite result; the loop still ends after clip_iters."""
    K, d = 50, 7850
    X, g0 = cc.inputs(K, d)
    X = X.clone()
    X[3, 5] = float("nan")
    X[K - 1, 7] = float("inf")
    for W in (X.cuda(), bz().ClientPanels.from_rows(X.cuda())):
        for tol in (None, 1e-3):
            bz().cclip(W, {"tau": cc.tau_of("mid", d), "clip_iters": 3, "clip_tol": tol,
                           "guess": g0.cuda()})
            res = bz().aggregators.last_result
            assert res.iters == 3 and not res.converged      # a NaN movement never passes


def test_cclip_refusals():
    from byzantine_aircomp_amd._lib import GmError
    Xb, g0 = cc.inputs(17, 1000, "bf16")
    X, g = Xb.cuda(), g0.cuda()
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError):
            bz().cclip(X.to(dt), {"tau": 1.0, "guess": g})
    with pytest.raises(GmError, match="no streaming tile for K=4096"):
        bz().cclip(torch.zeros(4096, 64, dtype=BF16, device="cuda"), {"tau": 1.0})
    for wl in (X, bz().ClientPanels.from_rows(X)):
        ctx = bz().context()
        ctx.set_shard(4000, 1000)
        try:
            with pytest.raises(GmError, match="sharded"):
                bz().cclip(wl, {"tau": 1.0, "guess": g})
        finally:
            ctx.set_shard(-1, 0)
        bz().cclip(wl, {"tau": 1.0, "guess": g})             # the context is usable again
        assert bz().aggregators.last_result.iters == 1
    assert torch.equal(bits(X.cpu()), bits(Xb))


def test_cclip_c_abi_contract():
    """What the Python layer never sends: a bad tau is GM_ERR_INVALID with nothing written,
    a bf16 row-major X the kernel cannot read in place is GM_ERR_UNSUPPORTED, maxiter == 0
    copies the guess, and gm_weiszfeld_f32 still refuses the internal clipping mode."""
    from byzantine_aircomp_amd import _lib
    K, d = 17, 1000
    X, g0 = cc.inputs(K, d)
    X, g = X.cuda(), g0.cuda()
    ctx = bz().context()
    out = torch.full((d,), 7.0, device="cuda")
    o = _lib.GmCclipOpts()
    o.maxiter, o.tol = 3, -1.0
    res = _lib.GmCclipResult()
    call = lambda fn, ptr, ldx: getattr(ctx.lib, fn)(          # noqa: E731
        ctx.handle, ptr, K, d, ldx, g.data_ptr(), out.data_ptr(), C.byref(o), C.byref(res), None)
    for tau in (0.0, -1.0, float("nan"), -math.inf):
        o.tau = tau
        for fn in ("gm_cclip_f32", "gm_cclip_bf16"):
            assert call(fn, X.data_ptr(), d) == -1
            assert b"tau" in ctx.lib.gm_last_error()
    o.tau = 1.0
    buf = torch.zeros(K * (d + 8) + 8, dtype=BF16, device="cuda")
    assert call("gm_cclip_bf16", buf.data_ptr(), d + 3) == -3           # ldx % 8 != 0
    assert b"multiples of 8" in ctx.lib.gm_last_error()
    assert call("gm_cclip_bf16", buf.data_ptr() + 2, d + 8) == -3       # off 16-byte alignment
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                           # nothing ran
    o.maxiter = 0
    assert call("gm_cclip_f32", X.data_ptr(), d) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, g) and res.iters == 0 and math.isnan(res.last_movement)
    w = _lib.GmOpts()
    w.maxiter, w.tol, w.eps, w.mode = 3, 1e-5, 1e-4, 2
    for fn in ("gm_weiszfeld_f32", "gm_weiszfeld_bf16"):
        assert getattr(ctx.lib, fn)(ctx.handle, X.data_ptr(), K, d, d, g.data_ptr(),
                                    out.data_ptr(), C.byref(w), None, None) == -1
        assert b"unknown mode" in ctx.lib.gm_last_error()
