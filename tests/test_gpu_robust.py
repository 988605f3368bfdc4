"""meamed / multi_krum / bulyan on the GPU (csrc/robust.hip) against the numpy references of
tests/robust_cases.py: the definitions, the bars and the margin conditions are stated there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import robust_cases as rc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import bulyan, meamed, multi_krum  # noqa: F401 - the file needs the feature
from byzantine_aircomp_amd import _lib, aggregators as agg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layouts(X):
    """The same matrix as contiguous rows, as a misaligned strided view and as panels."""
    Xg = X.to(DEV)
    wide = torch.full((X.shape[0], X.shape[1] + 3), 7.0, device=DEV)
    wide[:, 1:1 + X.shape[1]] = Xg
    view = wide[:, 1:1 + X.shape[1]]
    assert view.data_ptr() % 16 != 0 and view.stride(0) != X.shape[1]
    return {"rows": Xg, "view": view, "panels": bz.ClientPanels.from_rows(Xg)}


def _check_meamed(X, keep, forms=("rows", "view", "panels")):
    ref, scale = rc.ref_meamed(X.numpy(), keep, with_scale=True)
    lay = _layouts(X)
    outs = {}
    for name in forms:
        got = bz.meamed(lay[name], {"honestSize": keep})
        assert got.device.type == "cuda" and got.dtype == torch.float32
        outs[name] = got.cpu().numpy()
        bad = rc.meamed_mismatch(outs[name], ref, scale)
        assert bad.size == 0, (name, keep, bad[:5], outs[name][bad[:5]], ref[bad[:5]])
    first = outs[forms[0]]
    for name in forms[1:]:                       # bit for bit across layouts and alignments
        assert np.array_equal(first.view(np.uint32), outs[name].view(np.uint32)), name
    return first, ref, scale


@pytest.mark.parametrize("K,d", rc.MEAMED_CASES)
def test_meamed(K, d):
    X = rc.meamed_input(K, d)
    for keep in rc.keeps(K):
        got, ref, scale = _check_meamed(X, keep)
        if keep == 1:
            med = bz.median(X.to(DEV)).cpu().numpy()
            assert np.array_equal(got, med)
        if keep == K:
            mean = (X.numpy().astype(np.float64).sum(axis=0) / K).astype(np.float32)
            assert rc.meamed_mismatch(got, mean, scale).size == 0


@pytest.mark.parametrize("K,d", rc.QUANT_CASES)
def test_meamed_quantised_ties(K, d):
    X = rc.quantised_input(K, d)
    keep = K - K // 5
    assert rc.threshold_ties(X.numpy(), keep).any()
    for k in sorted({keep, max(1, K // 2), K - 1} - {0}):
        _check_meamed(X, k)


def test_meamed_special_values():
    X = rc.special_input()
    K = X.shape[0]
    for keep in rc.keeps(K) + [K - 2]:
        got, ref, _ = _check_meamed(X, keep)
        assert np.isnan(ref[5]) and np.isnan(got[5])
        assert got[33] == 0.0 and not np.signbit(got[33])           # -0 read as +0
    assert np.isinf(rc.ref_meamed(X.numpy(), K)[0])
    assert np.isnan(rc.ref_meamed(X.numpy(), K)[15])                # +inf and -inf summed


@pytest.mark.parametrize("K,d,n", rc.ROWS_CASES)
@pytest.mark.parametrize("panels", [False, True])
def test_meamed_row_subset_through_the_c_entry(K, d, n, panels):
    X = rc.meamed_input(K, d)
    g = torch.Generator().manual_seed(K + n)
    rows = torch.sort(torch.randperm(K, generator=g)[:n]).values
    keep = n - n // 5
    ref, scale = rc.ref_meamed(X.numpy()[rows.numpy()], keep, with_scale=True)
    Xg = X.to(DEV)
    rdev = rows.to(device=DEV, dtype=torch.int32)
    out = torch.full((d,), 9.0, dtype=torch.float32, device=DEV)
    if panels:
        P = bz.ClientPanels.from_rows(Xg)
        ptr, ldx, layout = P.data.data_ptr(), P.panel_stride, _lib.GM_LAYOUT_PANELS
    else:
        ptr, ldx, layout = Xg.data_ptr(), d, _lib.GM_LAYOUT_ROWS
    agg.context(Xg.device).call("gm_meamed_f32", ptr, K, d, ldx, layout, rdev.data_ptr(), n, keep,
                                out.data_ptr(), agg._stream_ptr(Xg.device))
    torch.cuda.synchronize()
    bad = rc.meamed_mismatch(out.cpu().numpy(), ref, scale)
    assert bad.size == 0, bad[:5]


@pytest.mark.parametrize("K,d,f", rc.MULTI_KRUM_CASES)
def test_multi_krum(K, d, f, monkeypatch):
    X = rc.spread(K, d, f)
    lay = _layouts(X)
    H = K - f
    for m in rc.ms(K, f):
        ref, sel, gap, _ = rc.multi_krum_case(K, d, f, m)
        assert gap >= rc.MULTI_KRUM_MIN_GAP, gap
        for name in ("rows", "panels") + (("view",) if m == H else ()):
            got = bz.multi_krum(lay[name], {"honestSize": H, "m": m})
            assert bz.multi_krum.last_selected == sel, (name, m)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (name, m)
    monkeypatch.setenv("GMAGG_KRUM", "0")
    one = bz.multi_krum(lay["rows"], {"honestSize": H, "m": 1})
    kr = bz.Krum(lay["rows"], {"honestSize": H})
    assert bz.Krum.last_info["algo"] == "exact"
    assert bz.multi_krum.last_selected == [bz.Krum.last_index]
    assert torch.equal(one.view(torch.int32), kr.view(torch.int32))
    dflt = bz.multi_krum(lay["rows"], {"honestSize": H})          # m defaults to honestSize
    assert len(bz.multi_krum.last_selected) == H
    assert torch.equal(dflt, bz.multi_krum(lay["rows"], {"honestSize": H, "m": H}))


@pytest.mark.parametrize("K,d,f", rc.BULYAN_CASES)
def test_bulyan(K, d, f):
    X = rc.spread(K, d, f)
    ref, scale, sel, gap, _ = rc.bulyan_case(K, d, f)
    assert gap >= rc.BULYAN_MIN_GAP, gap
    lay = _layouts(X)
    outs = []
    for name in ("rows", "panels", "view"):
        got = bz.bulyan(lay[name], {"honestSize": K - f})
        assert bz.bulyan.last_selected == sel, name                 # order included
        outs.append(got.cpu().numpy())
        bad = rc.meamed_mismatch(outs[-1], ref, scale)
        assert bad.size == 0, (name, bad[:5])
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))


@pytest.mark.parametrize("K,d", [(17, 333), (64, 70)])
def test_bulyan_without_byzantine_rows_is_the_mean(K, d):
    X = rc.meamed_input(K, d)
    got = bz.bulyan(X.to(DEV), {"honestSize": K}).cpu().numpy()
    assert sorted(bz.bulyan.last_selected) == list(range(K))
    mean = (X.numpy().astype(np.float64).sum(axis=0) / K).astype(np.float32)
    scale = np.abs(X.numpy().astype(np.float64)).sum(axis=0) / K
    assert rc.meamed_mismatch(got, mean, scale).size == 0


def test_exact_ties_go_to_the_lower_index():
    X = rc.tie_matrix()
    D = rc.dist64_direct(X)
    ref, sel, gap, tie = rc.ref_multi_krum(X, 7, 3, D=D)
    assert tie and gap == 0.0
    bref, bscale, bsel, bgap, btie = rc.ref_bulyan(X, 7, D=D)
    assert btie and bgap == 0.0
    for lay in _layouts(torch.from_numpy(X)).values():
        got = bz.multi_krum(lay, {"honestSize": 7, "m": 3})
        assert bz.multi_krum.last_selected == sel
        assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        got = bz.bulyan(lay, {"honestSize": 7})
        assert bz.bulyan.last_selected == bsel
        assert rc.meamed_mismatch(got.cpu().numpy(), bref, bscale).size == 0


@pytest.mark.parametrize("name", ["multi_krum", "bulyan"])
def test_under_bucketing(name):
    fn = getattr(bz, name)
    K, d, f = 50, 1000, 4
    X = rc.spread(K, d, f).to(DEV)
    opts = {"honestSize": K - f}
    wrapped = bz.bucketed(fn, 2, generator=torch.Generator().manual_seed(5))
    assert wrapped.__name__ == f"{name}_b2"
    got = wrapped(X, opts)
    perm = bz.bucketing.last_perm
    means = bz.bucketing(X, 2, perm=perm, layout="panels")
    want = fn(means, {"honestSize": K // 2 - f})
    assert torch.equal(got, want)
    rows = fn(bz.bucketing(X, 2, perm=perm, layout="rows"), {"honestSize": K // 2 - f})
    assert torch.equal(got, rows)
    assert opts == {"honestSize": K - f}


@pytest.mark.parametrize("name", ["multi_krum", "bulyan", "meamed"])
def test_cpu_tensor_returns_on_the_cpu(name):
    fn = getattr(bz, name)
    X = rc.spread(17, 1000, 3)
    got = fn(X, {"honestSize": 14})
    assert got.device.type == "cpu" and got.dtype == torch.float32 and got.shape == (1000,)
    assert torch.equal(got, fn(X.to(DEV), {"honestSize": 14}).cpu())


def test_c_entry_without_selected_and_d_zero():
    K, d, f = 17, 1000, 3
    X = rc.spread(K, d, f).to(DEV)
    ctx = agg.context(X.device)
    out = torch.empty(d, dtype=torch.float32, device=DEV)
    s = agg._stream_ptr(X.device)
    ctx.call("gm_multi_krum_f32", X.data_ptr(), K, d, d, 0, K - f, 5, out.data_ptr(), None, s)
    assert torch.equal(out, bz.multi_krum(X, {"honestSize": K - f, "m": 5}))
    ctx.call("gm_bulyan_f32", X.data_ptr(), K, d, d, 0, K - f, out.data_ptr(), None, s)
    assert torch.equal(out, bz.bulyan(X, {"honestSize": K - f}))
    sel = (C.c_int32 * 5)(*([-1] * 5))
    ctx.call("gm_multi_krum_f32", X.data_ptr(), K, 0, d, 0, K - f, 5, out.data_ptr(), sel, s)
    assert list(sel) == [-1] * 5                                   # d == 0: nothing written
