"""s-bucketing on the GPU (byzantine_aircomp_amd.bucketing / bucketed, csrc/bucket.hip).

The kernel against the numpy definition (bucket_cases.ref_bucket_means) within 1 fp32 ulp
(the device's fp64 division and final rounding; the fp64 sums are the reference's, term by
term), exactly where every mean is representable, in every input layout (fp32 and bf16: rows
on the 16-byte path, rows on the scalar path inside NaN-filled buffers, panels) and both
output layouts, all of which must agree bit for bit.  Then the composition: bucketed(gm2, s)
against oracle.gm2 of the numpy bucket means at the project's bar (relative L2 <= 1e-5, the
count by assert_iter_count), and the wrapper around the other aggregators.
"""
import numpy as np
import pytest
import torch

import bucket_cases as bc
from conftest import assert_iter_count, rel_l2
from coordinate_cases import mismatch_exact, mismatch_ulp
from oracle import aggregators as orc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def bz():
    import byzantine_aircomp_amd as m
    return m


def run_all_layouts(X, perm, s, bf16, what, compare=mismatch_ulp):
    """bucketing(X) under `perm` in every input x output layout of one dtype: each matches the
    reference, all are bit-identical, the inputs' bits are unchanged.  Returns the bits."""
    K, d = X.shape
    Kb = bc.n_buckets(K, s)
    ref = bc.ref_bucket_means(bc.widen_bf16(X) if bf16 else X, perm, s)
    first = None
    for lname, W in bc.input_layouts(torch, bz(), X, bf16):
        keep = bc.raw_bits(torch, W)
        for lout in ("rows", "panels"):
            out = bz().bucketing(W, s, perm=torch.as_tensor(perm), layout=lout)
            assert isinstance(out, bz().ClientPanels) == (lout == "panels")
            assert out.device.type == "cuda"
            got, gbits = bc.means_rows(torch, out, Kb, d)
            bad = compare(got.ravel(), ref.ravel(), f"{what} {lname}->{lout}")
            assert bad is None, bad
            if first is None:
                first = gbits
            assert torch.equal(gbits, first), f"{what} {lname}->{lout}: bits differ between layouts"
        assert torch.equal(bc.raw_bits(torch, W), keep), f"{what} {lname}: the input was written"
    assert torch.equal(bz().bucketing.last_perm, torch.as_tensor(perm))
    return first


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,s,d", bc.CASES)
def test_bucketing_matches_definition(K, s, d, bf16):
    X = bc.normal_matrix(K, d)
    run_all_layouts(X, bc.seeded_perm(K, s).numpy(), s, bf16, f"{K}x{d} s={s}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,s,d", bc.EXACT_CASES)
def test_bucketing_exact_integers(K, s, d, bf16):
    """Every mean exactly representable: a wrong row, bucket boundary or panel width cannot
    hide in rounding."""
    assert K % s == 0 and s & (s - 1) == 0
    X = bc.exact_matrix(K, d)
    run_all_layouts(X, bc.seeded_perm(K, s).numpy(), s, bf16, f"exact {K}x{d} s={s}",
                    compare=mismatch_exact)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_bucketing_special_values(bf16):
    """NaN, infinities of one and both signs, +-0, subnormals, 3e38 pairs (an fp32 sum would
    overflow) and 1e30 outliers whose order of addition decides the sum: the pattern and the
    values follow the reference."""
    K, s, d = bc.SPECIAL_CASE
    X, perm = bc.special_matrix()
    ref = bc.ref_bucket_means(bc.widen_bf16(X) if bf16 else X, perm, s)
    assert np.isnan(ref).sum() >= 5 and np.isinf(ref).sum() >= 4      # the case is what it says
    assert np.isfinite(ref[4, 11:14]).all() and abs(ref[4, 11]) > 1e38
    if not bf16:
        assert ref[5, 14] == 0.0 and ref[5, 15] == np.float32(1.0 / 3.0)
        assert 0 < ref[3, 8] < 1.2e-38                                 # a subnormal mean
    run_all_layouts(X, perm, s, bf16, "special values")


@pytest.mark.parametrize("K,s,d", bc.GENERATOR_CASES)
def test_default_assignment_is_one_seeded_randperm(K, s, d):
    X = bc.normal_matrix(K, d)
    Xg = torch.from_numpy(np.array(X)).cuda()
    out = bz().bucketing(Xg, s, generator=torch.Generator().manual_seed(31 * K + s))
    want = torch.randperm(K, generator=torch.Generator().manual_seed(31 * K + s))
    assert torch.equal(bz().bucketing.last_perm, want)
    assert isinstance(out, torch.Tensor) and out.shape == (bc.n_buckets(K, s), d)
    bad = mismatch_ulp(out.cpu().numpy().ravel(), bc.ref_bucket_means(X, want.numpy(), s).ravel(),
                       f"{K}x{d} s={s} generator")
    assert bad is None, bad
    # the global CPU generator when none is given: one draw
    torch.manual_seed(77)
    bz().bucketing(Xg, s)
    used = bz().bucketing.last_perm
    after = torch.get_rng_state()
    torch.manual_seed(77)
    assert torch.equal(used, torch.randperm(K))
    assert torch.equal(torch.get_rng_state(), after)
    # layout=None: ClientPanels in, ClientPanels out; a CPU tensor in, a CPU tensor out
    P = bz().ClientPanels.from_rows(Xg)
    outp = bz().bucketing(P, s, perm=want)
    assert isinstance(outp, bz().ClientPanels) and outp.device.type == "cuda"
    assert torch.equal(outp.to_rows(), out)
    outc = bz().bucketing(torch.from_numpy(np.array(X)), s, perm=want)
    assert outc.device.type == "cpu" and torch.equal(outc, out.cpu())


def test_bucketing_is_column_local():
    """bucketing(X[:, a:b]) == bucketing(X)[:, a:b] bit for bit (rows, and ClientPanels built
    from the slice): what lets every rank of a d-sharded matrix bucket its own shard."""
    K, s, d = 1000, 2, 2051
    perm = bc.seeded_perm(K, s)
    Xg = torch.from_numpy(np.array(bc.normal_matrix(K, d))).cuda()
    full = bz().bucketing(Xg, s, perm=perm)
    for dt in (torch.float32, BF16):
        Xd = Xg.to(dt)
        whole = bz().bucketing(Xd, s, perm=perm)[:, 256:1280]
        if dt == torch.float32:
            assert torch.equal(whole, full[:, 256:1280])
        part = bz().bucketing(Xd[:, 256:1280], s, perm=perm)
        assert torch.equal(part.view(torch.int32), whole.contiguous().view(torch.int32))
        P = bz().ClientPanels.from_rows(Xd[:, 256:1280])
        pp = bz().bucketing(P, s, perm=perm)
        assert torch.equal(pp.to_rows().view(torch.int32), whole.contiguous().view(torch.int32))


def test_c_abi_refusals_write_nothing():
    import ctypes as C
    from byzantine_aircomp_amd import _lib
    ctx = bz().context()
    K, d, s = 3000, 64, 3
    X = torch.ones(K, d, device="cuda")
    Y = torch.full((K, d), 7.0, device="cuda")
    R, P = _lib.GM_LAYOUT_ROWS, _lib.GM_LAYOUT_PANELS
    f = lambda *a: ctx.lib.gm_bucket_means_f32(ctx.handle, *a, None)      # noqa: E731
    x, y = X.data_ptr(), Y.data_ptr()
    assert f(x, K, d, d, P, None, s, y, d, R) == -3                 # K = 3000 has no panel width
    assert b"3000" in ctx.lib.gm_last_error()
    assert f(x, K, d, d, R, None, 1, y, d, P) == -3                 # nor have 3000 bucket means
    assert f(x, K, d, d - 1, R, None, s, y, d, R) == -1             # ldx < d
    assert f(x, K, d, d, R, None, s, y, d - 1, R) == -1             # ldy < d
    assert f(x, K, d, d, R, None, s, y, 1000 * 32 - 1, P) == -1     # panel stride < Kb * Wo
    assert f(x, K, d, d, 2, None, s, y, d, R) == -1                 # unknown layouts
    assert f(x, K, d, d, R, None, s, y, d, -1) == -1
    assert f(x, 0, d, d, R, None, s, y, d, R) == -1
    assert f(x, K, -1, d, R, None, s, y, d, R) == -1
    assert f(x, K, d, d, R, None, 0, y, d, R) == -1
    assert f(None, K, d, d, R, None, s, y, d, R) == -1
    assert f(x, K, d, d, R, None, s, None, d, R) == -1
    assert f(x, K, 0, d, R, None, s, y, d, R) == 0                  # d == 0
    torch.cuda.synchronize()
    assert (Y == 7.0).all() and (X == 1.0).all()
    assert f(x, K, d, d, R, None, s, y, d, R) == 0                  # identity perm (NULL)
    torch.cuda.synchronize()
    assert (Y[:1000] == 1.0).all() and (Y[1000:] == 7.0).all()


# ---------------------------------------------------------------------------- composition

# (K, d, s, bf16) -> the oracle's count on the numpy bucket means (tol 1e-5, maxiter 200);
# every window determined and 0 wide
COMPOSED = {(50, 7850, 2, False): 5, (600, 8200, 3, False): 7, (1000, 2051, 2, False): 5,
            (1000, 2051, 2, True): 5}
_COMPOSED = {}


def composed_case(K, d, s, bf16):
    """The C3 recipe's matrix (cast to bf16 or not), its seeded assignment, the numpy bucket
    means and the oracle's gm2 on them; computed once, never modified."""
    key = (K, d, s, bf16)
    if key not in _COMPOSED:
        X, g0 = bc.c3_recipe(K, d)
        if bf16:
            X = X.to(BF16)
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(7 * K + s))
        means = torch.from_numpy(bc.ref_bucket_means(X.float().numpy(), perm.numpy(), s))
        want, tr = orc.gm2(means.clone(), {"maxiter": 200, "tol": 1e-5, "guess": g0})
        win = orc.gm2_count_window(means, g0, 200, 1e-5)
        _COMPOSED[key] = (X, g0, perm, means, want, tr, win)
    return _COMPOSED[key]


@pytest.mark.parametrize("K,d,s,bf16", list(COMPOSED))
def test_bucketed_gm2_matches_oracle(K, d, s, bf16):
    X, g0, perm, means, want, tr, win = composed_case(K, d, s, bf16)
    assert win.determined and win.width == 0, win
    assert tr.iters == COMPOSED[(K, d, s, bf16)]
    Xg = X.cuda()
    opts = {"maxiter": 200, "tol": 1e-5, "guess": g0.cuda(), "honestSize": K - K // 5}
    keep = dict(opts)
    for wl in (Xg, bz().ClientPanels.from_rows(Xg)):
        panels_in = isinstance(wl, bz().ClientPanels)
        for layout in ("panels", "rows"):
            f = bz().bucketed(bz().gm2, s, generator=torch.Generator().manual_seed(7 * K + s),
                              layout=layout)
            assert f.__name__ == f"gm2_b{s}"
            got = f(wl, opts)
            res = bz().aggregators.last_result
            assert torch.equal(bz().bucketing.last_perm, perm)
            rel = rel_l2(got.cpu().numpy(), want.numpy())
            print(f"bucketed gm2 {K}x{d} s={s} bf16={bf16} panels_in={panels_in} -> {layout}: "
                  f"rel_l2={rel:.3e} iters={res.iters} (oracle {tr.iters}) algo={res.algo}")
            assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == (d,)
            assert rel <= 1e-5
            assert_iter_count(res.iters, tr.iters, win)
            if layout == "panels":
                # ceil(K/s) fp32 bucket means in panels: 25 rows fit the resident kernel (the
                # streaming pass if its grid is refused), 200 and 500 stream
                assert res.algo in (("resident", "stream") if K == 50 else ("stream",)), res
        assert opts == keep and opts["guess"] is keep["guess"]


def _fp32_case(K, s, d):
    X = torch.from_numpy(np.array(bc.normal_matrix(K, d))).cuda()
    perm = bc.seeded_perm(K, s)
    gen = lambda: torch.Generator().manual_seed(7 * K + s)        # noqa: E731 - seeded_perm's
    return X, perm, gen


@pytest.mark.parametrize("name", ["median", "trimmed_mean", "mean"])
def test_bucketed_coordinate_aggregators(name):
    K, s, d = 1000, 2, 517
    X, perm, gen = _fp32_case(K, s, d)
    inner = getattr(bz(), name)
    rows = bz().bucketing(X, s, perm=perm)
    want = inner(rows)
    opts = {"honestSize": 800}
    for wl in (X, bz().ClientPanels.from_rows(X)):
        for layout in ("panels", "rows", None):
            got = bz().bucketed(inner, s, generator=gen(), layout=layout)(wl, opts)
            assert torch.equal(bz().bucketing.last_perm, perm)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, layout)
    assert opts == {"honestSize": 800}


def test_bucketed_krum_rescales_honest_size():
    K, s, d = 1000, 2, 40
    X, perm, gen = _fp32_case(K, s, d)
    rows = bz().bucketing(X, s, perm=perm)
    seen = []

    def spy(wList, options):
        seen.append(options["honestSize"])
        return bz().Krum(wList, options)
    spy.__name__ = "Krum"
    opts = {"honestSize": 800}
    for layout in ("panels", "rows"):
        f = bz().bucketed(spy, s, generator=gen(), layout=layout)
        assert f.__name__ == "Krum_b2"
        got = f(X, opts)
        assert seen[-1] == 300                                    # 500 buckets - 200 Byzantine
        assert torch.equal(got, rows[bz().Krum.last_index])
        assert torch.equal(got, bz().Krum(rows, {"honestSize": 300}))
    assert opts == {"honestSize": 800}
    with pytest.raises(ValueError, match="honestSize"):
        bz().bucketed(bz().Krum, 2)(X, {"honestSize": 400})


def test_bucketed_cclip():
    K, s, d = 1000, 2, 2051
    X, perm, gen = _fp32_case(K, s, d)
    g0 = X[:10].mean(0)
    opts = {"guess": g0, "honestSize": 800, "maxiter": 3}
    keep = dict(opts)
    for dt in (torch.float32, BF16):
        Xd = X.to(dt)
        for layout in ("panels", "rows"):
            means = bz().bucketing(Xd, s, perm=perm, layout=layout)
            want = bz().cclip(means, {"guess": g0, "tau": 5.0, "clip_iters": 3})
            clipped = bz().cclip.last_info["clipped"]
            f = bz().bucketed(bz().cclip.with_options(tau=5.0, clip_iters=3), s, generator=gen(),
                              layout=layout)
            assert f.__name__ == "cclip_b2"
            got = f(Xd, opts)
            assert torch.equal(got, want) and torch.isfinite(got).all()
            assert bz().cclip.last_info["clipped"] == clipped
            assert bz().aggregators.last_result.iters == 3
    assert opts == keep


def test_bucketed_cpu_input_returns_cpu():
    K, s, d = 50, 2, 70
    X = torch.from_numpy(np.array(bc.normal_matrix(K, d)))
    got = bz().bucketed(bz().mean, s, generator=torch.Generator().manual_seed(1))(X, {})
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(1))
    assert got.device.type == "cpu"
    want = bc.ref_bucket_means(X.numpy(), perm.numpy(), s).astype(np.float64).mean(axis=0)
    np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-6)
