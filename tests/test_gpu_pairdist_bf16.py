"""Krum, multi_krum, nnm and pair_distances on bf16 client updates on the GPU
(csrc/pairdist_bf16.hip and the bf16 instantiations of pair_dist, copy_row, gather_mean and
nnm_mix) against tests/pairdist_cases.py: the exact tier bit for bit against the fp32 call on the
widened matrix; both tiers exact on integer inputs at every tile, tail and flush shape; the MFMA
tier inside its stated bound and its consumers inside the band that bound implies; the
device-side fallback on non-finite input; mixed(gm2) on bf16 rows.
"""
import numpy as np
import pytest
import torch

import nnm_cases as nc
import pairdist_cases as pc
import robust_cases as rc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import pair_distances  # noqa: F401 - the file needs the feature
from byzantine_aircomp_amd.panels import panel_width

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32).cpu().numpy()


def _operand(Xb, layout):
    """Xb (bf16, CPU) on the GPU as `layout`; None where K has no bf16 panel width."""
    Xc = Xb.to(DEV)
    K, d = Xc.shape
    if layout == "rows":
        return Xc
    if layout == "offset":
        buf = torch.zeros(K * d + 1, dtype=BF, device=DEV)
        v = buf[1:].view(K, d)
        v.copy_(Xc)
        assert v.data_ptr() % 16 == 2
        return v
    try:
        panel_width(K, BF)
    except ValueError:
        return None
    return bz.ClientPanels.from_rows(Xc)


def _raw(w):
    return w.data if isinstance(w, bz.ClientPanels) else w


def _expect(w, layout, asked):
    """(tier, reason) gm_dist_last_info must report for finite input."""
    if asked == "exact":
        return "exact", "requested_exact"
    return ("mfma", "ok") if pc.eligible(_raw(w), layout) else ("exact", "not_eligible")


def _int_ref(Xb):
    x = pc.widened(Xb)
    rho = (x * x).sum(axis=1)
    D = rho[:, None] + rho[None, :] - 2.0 * (x @ x.T)      # integers: exact in fp64
    return D


@pytest.mark.parametrize("K", pc.KS)
def test_every_shape_on_integers_is_exact_on_both_tiers(K):
    """Integer entries in [-15, 15]: every product and partial sum is an integer below 2^24, so
    pair_dist and the Gram form are exact whatever the order; both tiers must return the fp64
    distances themselves at one tile, a partial tile, off-diagonal tiles, a partial stage, a
    flush boundary and a tail, on aligned rows, rows one element off and panels."""
    for d in pc.DS + (pc.D_TWO_SLICES,):
        Xb = pc.integers(K, d)
        ref = _int_ref(Xb)
        for layout in pc.LAYOUTS:
            w = _operand(Xb, layout)
            if w is None:
                continue
            before = _bits(_raw(w))
            for asked in ("exact", "mfma"):
                D = bz.pair_distances(w, bf16=True, distances=asked)
                info = bz.pair_distances.last_info
                assert D.dtype == torch.float64 and D.shape == (K, K) and D.is_cuda
                assert np.array_equal(D.cpu().numpy(), ref), (K, d, layout, asked)
                assert (info["tier"], info["reason"]) == _expect(w, layout, asked), (d, layout)
                if info["tier"] == "mfma":
                    assert info["flush"] == pc.C_FLUSH
                    assert 1 <= info["slices"] <= -(-d // pc.C_FLUSH)
                    if K == 300 and d == pc.D_TWO_SLICES:
                        # 6 tile pairs leave room for every flush interval to be a slice
                        assert info["slices"] == -(-d // pc.C_FLUSH) >= 2
            assert np.array_equal(_bits(_raw(w)), before)              # X is never written
    # d = 333 on rows and the offset rows are not eligible; aligned rows with d % 8 == 0 are
    assert not pc.eligible(_operand(pc.integers(K, 333), "rows"), "rows")
    assert not pc.eligible(_operand(pc.integers(K, 264), "offset"), "offset")
    assert pc.eligible(_operand(pc.integers(K, 264), "rows"), "rows")


def _ms(K, honest):
    return sorted({1, min(40, K), honest})


@pytest.mark.parametrize("K,d,f", pc.SPREAD_CASES)
def test_exact_tier_returns_the_fp32_bits(K, d, f):
    Xb = pc.spread_bf16(K, d, f)
    honest = K - f
    X32 = Xb.float().to(DEV)
    o = {"honestSize": honest}
    k_ref = bz.Krum(X32, dict(o))
    k_idx = bz.Krum.last_index
    mk_ref = {}
    for m in _ms(K, honest):
        mk_ref[m] = (bz.multi_krum(X32, dict(o, m=m)), list(bz.multi_krum.last_selected))
    Y_ref, N_ref = bz.nnm(X32, f, layout="rows", neighbors=True)
    D_ref = bz.pair_distances(X32)
    for layout in pc.LAYOUTS:
        w = _operand(Xb, layout)
        if w is None:
            continue
        before = _bits(_raw(w))
        ob = dict(o, bf16=True)
        out = bz.Krum(w, dict(ob))
        assert bz.Krum.last_index == k_idx and bz.Krum.last_info["algo"] == "exact"
        assert np.array_equal(_bits(out), _bits(k_ref)), layout
        for m, (ref, sel) in mk_ref.items():
            out = bz.multi_krum(w, dict(ob, m=m))
            assert bz.multi_krum.last_selected == sel, (layout, m)
            assert np.array_equal(_bits(out), _bits(ref)), (layout, m)
            assert bz.multi_krum.last_info["tier"] == "exact"
        Y, N = bz.nnm(w, f, layout="rows", neighbors=True, bf16=True)
        assert torch.equal(N, N_ref), layout
        assert np.array_equal(_bits(Y), _bits(Y_ref)), layout
        assert bz.nnm.last_info["reason"] == "requested_exact"
        D = bz.pair_distances(w, bf16=True)
        assert torch.equal(D, D_ref), layout
        assert np.array_equal(_bits(_raw(w)), before)
    # m == 1 is the Krum row
    assert np.array_equal(_bits(mk_ref[1][0]), _bits(k_ref)) and mk_ref[1][1] == [k_idx]


@pytest.mark.parametrize("K,d,B", [(17, 264, 0), (129, 4120, 5), (300, 520, 0), (257, 264, 40)])
def test_tiers_agree_bit_for_bit_on_integers(K, d, B):
    """The many colliding integer distances (and B identical rows) are decided by index on
    both tiers alike."""
    Xb = pc.integers(K, d, B)
    f = max(1, K // 5)
    honest = K - f
    for layout in ("rows", "panels"):
        w = _operand(Xb, layout)
        if w is None:
            continue
        res = {}
        for asked in ("exact", "mfma"):
            ob = {"honestSize": honest, "bf16": True, "distances": asked}
            r = [bz.Krum(w, dict(ob)), bz.Krum.last_index]
            assert bz.Krum.last_info["algo"] == asked and bz.Krum.last_info["reason"] in (
                "ok", "requested_exact")
            for m in _ms(K, honest):
                r.append(bz.multi_krum(w, dict(ob, m=m)))
                r.append(list(bz.multi_krum.last_selected))
                assert bz.multi_krum.last_info["tier"] == asked
            Y, N = bz.nnm(w, f, layout="rows", neighbors=True, bf16=True, distances=asked)
            assert bz.nnm.last_info["tier"] == asked
            r += [Y, N]
            res[asked] = r
        for a, b in zip(res["exact"], res["mfma"]):
            if isinstance(a, torch.Tensor):
                assert a.dtype == b.dtype and torch.equal(a, b), (layout,)
            else:
                assert a == b, (layout, a, b)


def _bound_checks(Xb, layout, what):
    w = _operand(Xb, layout)
    Dt = bz.pair_distances(w, bf16=True, distances="mfma")
    info = bz.pair_distances.last_info
    assert (info["tier"], info["reason"]) == ("mfma", "ok"), (what, info)
    beta = info["beta"]
    assert 0 < beta <= pc.BETA_MAX
    Dt = Dt.cpu().numpy()
    D, rho = pc.dist_rho(Xb)
    ratio = pc.bound_ratio(Dt, D, rho)
    print(f"pairdist mfma {what}: max |D~ - D| / (rho_i + rho_j) = {ratio:.3e}, beta = {beta:.3e}")
    assert ratio <= beta, (what, ratio, beta)
    assert np.array_equal(Dt, Dt.T) and (Dt >= 0).all() and (np.diag(Dt) == 0).all()


@pytest.mark.parametrize("K,d,layout", pc.BOUND_CASES)
def test_error_bound_on_graded_inputs(K, d, layout):
    _bound_checks(pc.graded(K, d), layout, f"graded K={K} d={d} {layout}")


@pytest.mark.parametrize("K,d,f", [(129, 264, 26), (300, 520, 60)])
def test_error_bound_on_spread_inputs(K, d, f):
    _bound_checks(pc.spread_bf16(K, d, f), "rows", f"spread K={K} d={d}")


@pytest.mark.parametrize("K,d,f", pc.NEIGHBOR_CASES)
def test_neighbour_sets_on_the_mfma_tier(K, d, f):
    Xb = pc.graded(K, d)
    w = _operand(Xb, "panels" if d % 8 else "rows")
    Y, N = bz.nnm(w, f, layout="rows", neighbors=True, bf16=True, distances="mfma")
    info = bz.nnm.last_info
    assert (info["tier"], info["reason"]) == ("mfma", "ok") and info["beta"] <= pc.BETA_MAX
    D, rho = pc.dist_rho(Xb)
    N = N.cpu().numpy()
    amb = pc.check_neighbors_band(N, D, rho, f, info["beta"])
    print(f"nnm mfma K={K} d={d} f={f}: {amb} ambiguous rows")
    X32 = Xb.float().numpy()
    ref, scale = nc.ref_mix(X32, N, with_scale=True)
    bad = nc.mix_mismatch(Y.cpu().numpy(), ref, scale)
    assert bad.size == 0, bad[:5]


@pytest.mark.parametrize("K,d,honest,ms", pc.SELECT_CASES)
def test_selection_on_the_mfma_tier(K, d, honest, ms):
    Xb = pc.graded(K, d)
    w = _operand(Xb, "panels" if d % 8 else "rows")
    D, rho = pc.dist_rho(Xb)
    for m in ms:
        ob = {"honestSize": honest, "m": m, "bf16": True}
        fast = bz.multi_krum(w, dict(ob, distances="mfma"))
        sel = list(bz.multi_krum.last_selected)
        info = bz.multi_krum.last_info
        assert (info["tier"], info["reason"]) == ("mfma", "ok")
        want, determined = pc.selection_determined(D, rho, honest, m, info["beta"])
        assert determined, (K, d, honest, m)
        assert sel == want.tolist()
        exact = bz.multi_krum(w, dict(ob, distances="exact"))
        assert bz.multi_krum.last_selected == sel
        assert np.array_equal(_bits(fast), _bits(exact))
        if m == 1:
            row = bz.Krum(w, {"honestSize": honest, "bf16": True, "distances": "mfma"})
            assert bz.Krum.last_info["algo"] == "mfma" and bz.Krum.last_index == sel[0]
            assert np.array_equal(_bits(row), _bits(fast))
            assert np.array_equal(_bits(row), _bits(Xb[sel[0]].float()))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 3e38])
def test_non_finite_input_falls_back_on_the_device(bad):
    K, d, f = 129, 264, 26
    X = pc.graded(K, d).clone()
    byz = K - 1                                            # the largest row: far from every other
    X[byz, 5] = bad
    assert bad != bad or float(X[byz, 5].float()) ** 2 > 3.4e38
    w = X.to(DEV)
    honest = K - f
    res = {}
    for asked in ("exact", "mfma"):
        ob = {"honestSize": honest, "bf16": True, "distances": asked}
        r = [bz.multi_krum(w, dict(ob)), list(bz.multi_krum.last_selected)]
        i1 = bz.multi_krum.last_info
        r += [bz.Krum(w, dict(ob)), bz.Krum.last_index]
        i2 = bz.Krum.last_info
        Y, N = bz.nnm(w, f, neighbors=True, bf16=True, distances=asked)
        i3 = bz.nnm.last_info
        r += [Y, N, bz.pair_distances(w, bf16=True, distances=asked)]
        i4 = bz.pair_distances.last_info
        if asked == "mfma":
            assert i2["algo"] == "exact"
            for i in (i1, i2, i3, i4):
                assert i["reason"] == "nonfinite_fallback", i
            assert i1["tier"] == i3["tier"] == i4["tier"] == "exact"
        res[asked] = r
    for a, b in zip(res["exact"], res["mfma"]):
        if isinstance(a, torch.Tensor):
            assert a.dtype == b.dtype
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()      # NaNs included
        else:
            assert a == b
    # the excluded row contributes nothing: it is in no other row's list, and their Y is finite
    Y, N = res["mfma"][4].cpu(), res["mfma"][5].cpu().numpy()
    others = np.arange(K) != byz
    assert not (N[others] == byz).any()
    assert torch.isfinite(Y[torch.from_numpy(others)]).all()


def test_mixed_gm2_on_bf16_rows():
    K, d, f = 129, 264, 26
    Xb = pc.graded(K, d).to(DEV)
    opts = {"honestSize": K - f, "maxiter": 50, "tol": 1e-6, "bf16": True, "distances": "mfma"}
    keep = dict(opts)
    got = bz.mixed(bz.gm2)(Xb, opts)
    assert opts == keep
    assert bz.nnm.last_info["tier"] == "mfma"
    rows = bz.nnm(Xb, f, layout="panels", bf16=True, distances="mfma")
    want = bz.gm2(rows, dict(opts))
    assert got.dtype == torch.float32 and got.shape == (d,)
    assert np.array_equal(_bits(got), _bits(want))
    # and the mixing step moved what gm2 sees: the result differs from gm2 on the raw rows
    assert not torch.equal(got, bz.gm2(Xb, {"maxiter": 50, "tol": 1e-6}))
