"""Norm clipping (clip, arc, clipped) without a GPU: the exports, every refusal of the C ABI and
of the Python layer, ARC's k in integers, the reference against a brute-force statement of the
definition, the recipe's conditions at every GPU shape, the bars' discrimination, and the
contract of the ``clipped`` wrapper on a stub aggregate."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clip_cases as cc

import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import _lib
from byzantine_aircomp_amd import aggregators as agg


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a GPU context (or to stage a tensor) fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(agg, "context", boom)
    monkeypatch.setattr(agg, "_stage", boom)


def test_exported_and_bound():
    for name in ("clip", "arc", "clipped"):
        assert getattr(bz, name) is getattr(agg, name) and name in agg.__all__
    names = {n for n, _, _ in _lib.SIGNATURES}
    assert {"gm_clip_rows_f32", "gm_clip_rows_bf16"} <= names
    lib = _lib.load()
    assert lib.gm_clip_rows_f32 and lib.gm_clip_rows_bf16
    assert (_lib.GM_CLIP_STATIC, _lib.GM_CLIP_ARC) == (0, 1)
    assert _lib.ABI_VERSION == 5 and lib.gm_abi_version() == 5
    from byzantine_aircomp_amd.sharded import ShardedGM
    assert callable(ShardedGM.arc) and callable(ShardedGM.clip)


@pytest.mark.parametrize("fn", ["gm_clip_rows_f32", "gm_clip_rows_bf16"])
def test_abi_argument_checks(fn):
    """No device needed: every refusal happens before the first HIP call (the context pointer
    is only handed on, never read, before the checks pass)."""
    lib = _lib.load()
    bx, by = (C.c_float * 16384)(), (C.c_float * 16384)()
    x, y = C.addressof(bx), C.addressof(by)
    ctx = x                                     # non-NULL; never dereferenced on these paths
    R, P = _lib.GM_LAYOUT_ROWS, _lib.GM_LAYOUT_PANELS
    ST, ARC = _lib.GM_CLIP_STATIC, _lib.GM_CLIP_ARC
    ft = getattr(lib, fn)
    b16 = fn.endswith("bf16")
    width = lib.gm_panel_width_bf16 if b16 else lib.gm_panel_width

    def refused(rc_, code, text=b""):
        assert rc_ == code
        msg = lib.gm_last_error()
        assert msg and fn.encode() in msg and text in msg, msg

    # (ctx, X, K, d, ldx, layout_in, centre, rule, f, tau, Y, ldy, layout_out, stats, stream)
    refused(ft(None, x, 8, 4, 4, R, None, ARC, 1, 0.0, y, 4, R, None, None), -1)
    refused(ft(ctx, None, 8, 4, 4, R, None, ARC, 1, 0.0, y, 4, R, None, None), -1)
    refused(ft(ctx, x, 8, 4, 4, R, None, ARC, 1, 0.0, None, 4, R, None, None), -1)
    refused(ft(ctx, x, 0, 4, 4, R, None, ARC, 0, 0.0, y, 4, R, None, None), -1)      # K < 1
    refused(ft(ctx, x, 8, -1, 4, R, None, ARC, 1, 0.0, y, 4, R, None, None), -1)     # d < 0
    refused(ft(ctx, x, 8, 4, 4, 7, None, ARC, 1, 0.0, y, 4, R, None, None), -1)      # layout_in
    refused(ft(ctx, x, 8, 4, 4, R, None, ARC, 1, 0.0, y, 4, 7, None, None), -1)      # layout_out
    refused(ft(ctx, x, 8, 4, 4, R, None, 2, 1, 1.0, y, 4, R, None, None), -1, b"rule")
    refused(ft(ctx, x, 8, 4, 3, R, None, ARC, 1, 0.0, y, 4, R, None, None), -1, b"ldx")
    refused(ft(ctx, x, 8, 4, 4, R, None, ARC, 1, 0.0, y, 3, R, None, None), -1, b"ldy")
    W, Wo = width(8), lib.gm_panel_width(8)
    refused(ft(ctx, x, 8, 4, 8 * W - 1, P, None, ARC, 1, 0.0, y, 4, R, None, None), -1, b"ldx")
    refused(ft(ctx, x, 8, 4, 4, R, None, ARC, 1, 0.0, y, 8 * Wo - 1, P, None, None), -1, b"ldy")
    for f in (-1, 8, 100):
        refused(ft(ctx, x, 8, 4, 4, R, None, ARC, f, 1.0, y, 4, R, None, None), -1, b"f =")
    for tau in (0.0, -1.0, math.nan, -math.inf):
        refused(ft(ctx, x, 8, 4, 4, R, None, ST, 0, tau, y, 4, R, None, None), -1, b"tau")
    # Y overlapping X other than exactly: a shifted pointer, another stride, another layout
    refused(ft(ctx, x, 8, 4, 4, R, None, ARC, 1, 0.0, x + 4, 4, R, None, None), -1, b"overlaps")
    refused(ft(ctx, x, 8, 4, 4, R, None, ARC, 1, 0.0, x, 5, R, None, None), -1, b"overlaps")
    ld = 8 * max(W, Wo)
    refused(ft(ctx, x, 8, 4, ld, R, None, ARC, 1, 0.0, x, ld, P, None, None), -1, b"overlaps")
    # beyond the cap; every K <= 2048 has a panel width and none above has
    refused(ft(ctx, x, 4097, 4, 4, R, None, ARC, 1, 0.0, y, 4, R, None, None), -3, b"4096")
    assert all(width(k) > 0 for k in (1, 16, 17, 64, 65, 256, 257, 1024, 1025, 2048))
    refused(ft(ctx, x, 4096, 4, 1 << 30, P, None, ARC, 1, 0.0, y, 4, R, None, None), -3,
            b"no panel layout")
    refused(ft(ctx, x, 2049, 4, 4, R, None, ARC, 1, 0.0, y, 1 << 30, P, None, None), -3,
            b"no panel layout")
    if b16:
        refused(ft(ctx, x, 8, 4, 4, R, None, ARC, 1, 0.0, x, 4, R, None, None), -3, b"in place")
    # d == 0 is GM_OK and launches nothing (in place too); tau = +inf is a valid radius
    assert ft(ctx, x, 8, 0, 4, R, None, ARC, 7, 0.0, y, 4, R, None, None) == 0
    assert ft(ctx, x, 8, 0, 8 * W, P, x, ST, 0, math.inf, y, 8 * Wo, P, None, None) == 0
    if not b16:
        assert ft(ctx, x, 8, 0, 4, R, None, ARC, 0, 0.0, x, 4, R, None, None) == 0


def test_python_refusals(no_device):
    X = torch.zeros(12, 5)
    for fn, arg in ((bz.clip, 1.0), (bz.arc, 2)):
        for bad in (X.half(), X.double()):
            with pytest.raises(TypeError):
                fn(bad, arg)
        with pytest.raises(ValueError):
            fn(torch.zeros(12), arg)
        with pytest.raises(ValueError):
            fn(torch.zeros(0, 5), arg)
        with pytest.raises(ValueError, match="4096"):
            fn(torch.zeros(4097, 2), arg)
        with pytest.raises(ValueError, match="layout"):
            fn(X, arg, layout="cols")
        with pytest.raises(ValueError, match="no panel layout"):
            fn(torch.zeros(4096, 2), arg, layout="panels")
        with pytest.raises(ValueError, match="centre"):
            fn(X, arg, centre=torch.zeros(4))
        with pytest.raises(TypeError, match="centre"):
            fn(X, arg, centre=[0.0] * 5)
        with pytest.raises(TypeError, match="centre"):
            fn(X, arg, centre=torch.zeros(5, dtype=torch.float64))
        with pytest.raises(TypeError, match="inplace"):
            fn(X.to(torch.bfloat16), arg, inplace=True)
        with pytest.raises(ValueError, match="inplace"):
            fn(X, arg, layout="panels", inplace=True)
        # a valid call: the first thing it does is stage the tensor (bf16 included)
        for ok in (X, X.to(torch.bfloat16)):
            with pytest.raises(AssertionError, match="device"):
                fn(ok, arg, centre=torch.zeros(5))
    for tau in (0, 0.0, -1.0, math.nan, True, "1", None):
        with pytest.raises(ValueError, match="tau"):
            bz.clip(X, tau)
    for f in (True, 1.5, 2.0, "1", None, -1, 12, 100):
        with pytest.raises(ValueError, match="f "):
            bz.arc(X, f)
    with pytest.raises(AssertionError, match="device"):
        bz.clip(X, math.inf)
    with pytest.raises(AssertionError, match="device"):
        bz.arc(X, 11, inplace=True)


def test_k_is_integer_arithmetic():
    assert cc.arc_k(242, 33) == 57 and cc.arc_k_float(242, 33) == 56
    differ = [(K, f) for K in range(1, 4097) for f in range((K + 1) // 2)
              if cc.arc_k(K, f) != cc.arc_k_float(K, f)]
    assert len(differ) == 80 and differ[0] == (242, 33)
    for K in (1, 2, 3, 5, 50, 1000, 4096):
        assert cc.arc_k(K, 0) == 0
        assert all(0 <= cc.arc_k(K, f) <= K // 2 for f in range(K))
    assert cc.arc_k(4096, 819) == 1310 and cc.arc_k(3, 0) == 0 and cc.arc_k(1000, 200) == 320


def _brute(X, c, rule, f=None, tau=None):
    """The definition, one Python float at a time with exactly rounded sums."""
    K, d = X.shape
    cv = [0.0] * d if c is None else [float(v) for v in c]
    n = []
    for k in range(K):
        u = [float(X[k, j]) - cv[j] for j in range(d)]
        if any(math.isnan(v) for v in u):
            n.append(math.nan)
        elif any(math.isinf(v) for v in u):
            n.append(math.inf)
        else:
            n.append(math.fsum(v * v for v in u))
    if rule == cc.ARC:
        k_ = (2 * f * (K - f)) // K
        before = lambda a, i, b, j: (  # noqa: E731 - score_before
            (i < j if math.isnan(a) == math.isnan(b) else math.isnan(b))
            if math.isnan(a) or math.isnan(b) else (a < b or (a == b and i < j)))
        rank = [sum(before(n[j], j, n[i], i) for j in range(K)) for i in range(K)]
        T = n[rank.index(K - 1 - k_)]
    else:
        T = tau * tau
    s, out = [], []
    for k in range(K):
        if math.isnan(n[k]) or n[k] == math.inf:
            s.append(0.0)
            out.append([np.float32(v) for v in cv])
        elif math.isnan(T) or n[k] <= T:
            s.append(1.0)
            out.append(list(X[k]))
        else:
            s.append(math.sqrt(T / n[k]))
            out.append([np.float32(cv[j] + s[k] * (float(X[k, j]) - cv[j])) for j in range(d)])
    return n, T, s, np.array(out, dtype=np.float32)


@pytest.mark.parametrize("centre", [True, False])
@pytest.mark.parametrize("rule", [cc.ARC, cc.STATIC])
def test_reference_is_the_definition(rule, centre):
    r = np.random.default_rng(9)
    K, d, f = 8, 6, 3                               # k = (2 * 3 * 5) // 8 = 3
    c = r.standard_normal(d).astype(np.float32)
    c[2] = -0.0
    X = (c + 0.1 * r.standard_normal((K, d))).astype(np.float32)
    X[0] = (c + 5.0 * r.standard_normal(d)).astype(np.float32)     # far out: clipped
    X[1] = (c + 2.0 * (X[1].astype(np.float64) - c)).astype(np.float32)
    X[1, 4] = -0.0                                   # stays -0 in a copied row
    X[2] = X[1]                                      # an exact copy: the pair that sets T at f = 4
    X[3, 1] = np.nan
    X[4, 0] = np.inf
    X[5] = c                                         # a zero row
    X[6, 3] = -np.inf
    cen = c if centre else None
    if not centre:
        X[5] = 0.0
        X[5, 2] = -0.0
    tau = 0.7
    ref = cc.reference(X, cen, rule, f=f, tau=tau)
    n, T, s, out = _brute(X, cen, rule, f=f, tau=tau)
    np.testing.assert_allclose(np.asarray(ref["n"], dtype=np.float64), n, rtol=1e-15)
    assert float(ref["T"]) == pytest.approx(T, rel=1e-15)
    np.testing.assert_allclose(np.asarray(ref["s"], dtype=np.float64), s, rtol=1e-15)
    assert [k for k in range(K) if s[k] != 1] == ref["clipped"]
    assert np.array_equal(ref["out32"].view(np.int32), out.view(np.int32))
    for k in (3, 4, 6):                              # non-finite norms: the centre, exactly
        assert ref["s"][k] == 0
        assert np.array_equal(ref["out32"][k].view(np.int32),
                              (c if centre else np.zeros(d, np.float32)).view(np.int32))
    if rule == cc.ARC:
        # descending: NaN, +inf, +inf, then the largest finite norm, row 0: T = n_0, and with
        # one more (f = 4: k = 4) the tied pair rows 1 and 2, which both stay unclipped
        assert ref["T"] == ref["n"][0] and ref["clipped"] == [3, 4, 6]
    if rule == cc.ARC and centre:
        ref4 = cc.reference(X, cen, cc.ARC, f=4)
        assert cc.arc_k(8, 4) == 4 and ref4["T"] == ref4["n"][1] == ref4["n"][2]
        assert ref4["clipped"] == [0, 3, 4, 6] and ref4["s"][1] == 1 and ref4["s"][2] == 1
        assert 0 < ref4["s"][0] < 1
        b4 = _brute(X, cen, cc.ARC, f=4)
        assert np.array_equal(ref4["out32"].view(np.int32), b4[3].view(np.int32))
        assert np.signbit(ref4["out32"][1, 4]) and ref4["out32"][1, 4] == 0    # -0 stays -0
    if rule == cc.STATIC:
        assert 0 in ref["clipped"] and 0 < ref["s"][0] < 1
    if centre:
        assert np.signbit(ref["out32"][3, 2])        # the centre's own -0


def test_more_nans_than_k_clips_nothing():
    X = np.ones((3, 4), dtype=np.float32)
    X[0, 0] = X[1, 1] = np.nan
    X[2] *= 1e30
    ref = cc.reference(X, None, cc.ARC, f=1)         # k = 1: T = the second largest = NaN
    assert np.isnan(ref["T"]) and list(ref["s"]) == [0, 0, 1]
    assert np.array_equal(ref["out32"][2], X[2]) and not ref["out32"][:2].any()
    ref = cc.reference(X, None, cc.STATIC, tau=math.inf)
    assert list(ref["s"]) == [0, 0, 1]


@pytest.mark.parametrize("K,d", cc.SHAPES + [cc.LARGE])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gpu_shapes_meet_the_recipes_conditions(K, d, dtype):
    """Conditions, not measurements: no distinct finite n_k within 1e-8 of T (case() asserts
    it), every kind present when K // 5 >= 7, and what the definition makes of each kind."""
    (X, c, kinds), ref, f, _ = cc.case(K, d, dtype)
    assert X.shape == (K, d) and len(kinds) == K and f == K // 5
    if f >= len(cc.KINDS):
        assert set(cc.KINDS) <= set(kinds)
    k = cc.arc_k(K, f)
    assert (K <= 3) == (k == 0)
    finite = sum(kind not in ("nan", "inf") for kind in kinds)
    n_bad = K - finite
    assert len(ref["clipped"]) <= max(k, n_bad) and (K < 5 or len(ref["clipped"]) >= n_bad)
    ties = int(cc.at_threshold(ref).sum())
    print(f"clip recipe {K}x{d} {dtype}: k = {k}, clipped {len(ref['clipped'])}, rows at the "
          f"threshold {ties}")
    for i, kind in enumerate(kinds):
        if kind in ("nan", "inf"):
            assert ref["s"][i] == 0
        if kind in ("zero", "tiny"):
            assert ref["s"][i] == 1
        if kind == "zero":
            assert ref["n"][i] == 0
        if kind == "scaled" and k > n_bad:
            assert 0 < ref["s"][i] < 0.1
    (_, _, _), sref, _, tau = cc.case(K, d, dtype, cc.STATIC)
    assert tau > 0 or K <= 3
    fixed = ~cc.at_threshold(ref)
    assert np.array_equal((sref["s"] != 1)[fixed], (ref["s"] != 1)[fixed])


@pytest.mark.parametrize("K,d", [(50, 7850), (600, 8200)])
def test_n_bar_separates_fp64_from_fp32_accumulation(K, d):
    (X, c, _), ref, f, _ = cc.case(K, d)
    Xn, cn = X.numpy(), c.numpy()
    good = cc.worst_n(cc.restate(Xn, cn, f, np.float64)[0], ref)
    bad = cc.worst_n(cc.restate(Xn, cn, f, np.float32)[0], ref)
    print(f"clip n bar {K}x{d}: fp64 chunked restatement {good:.3e}, fp32 accumulation "
          f"{bad:.3e}, bar {d * 2.0 ** -52:.3e}")
    assert good <= d * 2.0 ** -52 < bad
    n, s, out = cc.restate(Xn, cn, f, np.float64)
    stats = np.concatenate([n, s, [n[cc.order_of(n)[K - 1 - cc.arc_k(K, f)]]],
                            [float((s != 1).sum())]])
    cc.check_stats(stats, ref, K, d, cc.ARC, "fp64 restatement")
    cc.check_out(out, Xn, cn, ref, s, "fp64 restatement")


def test_float_evaluated_k_fails_the_bars():
    K, f, d = 242, 33, 64
    X, c, _ = cc.inputs(K, d)
    Xn, cn = X.numpy(), c.numpy()
    ref = cc.reference(Xn, cn, cc.ARC, f=f)
    cc.check_well_posed(ref)

    def stats_of(k_of):
        n, s, _ = cc.restate(Xn, cn, f, np.float64, k_of=k_of)
        return np.concatenate([n, s, [n[cc.order_of(n)[K - 1 - k_of(K, f)]]],
                               [float((s != 1).sum())]])
    cc.check_stats(stats_of(cc.arc_k), ref, K, d, cc.ARC, "integer k")
    with pytest.raises(AssertionError):
        cc.check_stats(stats_of(cc.arc_k_float), ref, K, d, cc.ARC, "float k")


def test_multiplying_nonfinite_rows_by_zero_fails_the_match():
    K, d = 50, 7850
    (X, c, kinds), ref, f, _ = cc.case(K, d)
    assert "nan" in kinds and "inf" in kinds
    Xn, cn = X.numpy(), c.numpy()
    n, s, out = cc.restate(Xn, cn, f, np.float64, skip=True)
    cc.check_out(out, Xn, cn, ref, s, "skipped")
    n, s, out = cc.restate(Xn, cn, f, np.float64, skip=False)
    assert np.isnan(out[kinds.index("nan")]).any()    # 0 * NaN at the row's NaN entry
    with pytest.raises(AssertionError):
        cc.worst_out(out, ref)


# ---- the wrapper, on a stub aggregate -------------------------------------------------------

def test_clipped_contract(no_device, monkeypatch):
    seen = {}

    def fake(name):
        def fn(wList, arg, centre=None, layout=None, inplace=False):
            seen.update(rule=name, arg=arg, centre=centre, layout=layout, inplace=inplace,
                        wList=wList)
            return "rows"
        return fn
    monkeypatch.setattr(agg, "arc", fake("arc"))
    monkeypatch.setattr(agg, "clip", fake("clip"))

    def stub(wList, options):
        seen["inner"] = (wList, options)
        return "out"
    assert bz.clipped(stub).__name__ == "stub_arc" == bz.clipped(stub).__qualname__
    assert bz.clipped(stub, f=3).__name__ == "stub_arc"
    assert bz.clipped(stub, tau=2.0).__name__ == "stub_clip"
    assert bz.clipped(bz.gm2).__name__ == "gm2_arc"
    assert bz.mixed(bz.clipped(bz.gm2)).__name__ == "gm2_arc_nnm"
    assert bz.bucketed(bz.clipped(bz.gm2, tau=1), 2).__name__ == "gm2_clip_b2"
    assert bz.clipped(bz.mixed(bz.gm2)).__name__ == "gm2_nnm_arc"
    with pytest.raises(ValueError, match="layout"):
        bz.clipped(stub, layout="cols")
    with pytest.raises(ValueError, match="not both"):
        bz.clipped(stub, tau=1.0, f=2)
    for tau in (0, -1.0, math.nan, True, "1"):
        with pytest.raises(ValueError, match="tau"):
            bz.clipped(stub, tau=tau)

    X = torch.zeros(10, 4)
    g = torch.ones(4)
    opts = {"guess": g, "honestSize": 8, "maxiter": 7, "other": "x"}
    keep = dict(opts)
    assert bz.clipped(stub)(X, opts) == "out"
    assert seen["rule"] == "arc" and seen["arg"] == 2 and seen["centre"] is g
    assert seen["layout"] == "panels" and seen["inplace"] is False and seen["wList"] is X
    assert seen["inner"][0] == "rows" and seen["inner"][1] is opts and opts == keep
    # without honestSize ARC cannot choose f; a fixed f or a radius needs none
    for o in ({}, None, {"guess": g}):
        with pytest.raises(ValueError, match="honestSize"):
            bz.clipped(stub)(X, o)
    bz.clipped(stub, f=4, layout="rows")(X, {"guess": g})
    assert seen["arg"] == 4 and seen["layout"] == "rows"
    bz.clipped(stub, tau=2.5, layout=None)(X, {})
    assert seen["rule"] == "clip" and seen["arg"] == 2.5 and seen["centre"] is None
    assert seen["layout"] is None
    # K without a panel width: the clipped rows are handed over row-major
    bz.clipped(stub, f=1)(torch.zeros(2049, 2), {})
    assert seen["layout"] == "rows"
