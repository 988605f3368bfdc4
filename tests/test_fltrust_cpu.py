"""FLTrust without a GPU: the exports, every refusal of the C ABI and of the Python layer, the
with_options contract, the reference against a brute-force loop, the recipe's conditions at
every GPU shape and the bar's discrimination between fp64 and fp32 accumulation."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fltrust_cases as fc

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
    assert bz.fltrust is agg.fltrust and "fltrust" in agg.__all__
    names = {n for n, _, _ in _lib.SIGNATURES}
    assert {"gm_fltrust_f32", "gm_fltrust_bf16"} <= names
    lib = _lib.load()
    assert lib.gm_fltrust_f32 and lib.gm_fltrust_bf16
    assert _lib.ABI_VERSION == 5 and lib.gm_abi_version() == 5
    from byzantine_aircomp_amd.sharded import ShardedGM
    assert callable(ShardedGM.fltrust)


@pytest.mark.parametrize("fn", ["gm_fltrust_f32", "gm_fltrust_bf16"])
def test_abi_argument_checks(fn):
    """No device needed: every refusal happens before the first HIP call (the context pointer
    is only handed on, never read, before the checks pass)."""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ctx = p                                     # non-NULL; never dereferenced on these paths
    R, P = _lib.GM_LAYOUT_ROWS, _lib.GM_LAYOUT_PANELS
    ft = getattr(lib, fn)
    width = lib.gm_panel_width_bf16 if fn.endswith("bf16") else lib.gm_panel_width

    def refused(rc_, code, text=b""):
        assert rc_ == code
        msg = lib.gm_last_error()
        assert msg and fn.encode() in msg and text in msg, msg

    # (ctx, X, K, d, ldx, layout, server, server_row, centre, out, stats, stream)
    refused(ft(None, p, 8, 4, 4, R, p, -1, None, p, None, None), -1)
    refused(ft(ctx, None, 8, 4, 4, R, p, -1, None, p, None, None), -1)
    refused(ft(ctx, p, 8, 4, 4, R, p, -1, None, None, None, None), -1)
    refused(ft(ctx, p, 0, 4, 4, R, p, -1, None, p, None, None), -1)          # K < 1
    refused(ft(ctx, p, 8, -1, 4, R, p, -1, None, p, None, None), -1)         # d < 0
    refused(ft(ctx, p, 8, 4, 3, R, p, -1, None, p, None, None), -1, b"ldx")  # ldx < d
    refused(ft(ctx, p, 8, 4, 4, 7, p, -1, None, p, None, None), -1)          # layout
    W = width(8)
    refused(ft(ctx, p, 8, 4, 8 * W - 1, P, p, -1, None, p, None, None), -1, b"panel stride")
    refused(ft(ctx, p, 8, 4, 4, R, p, 2, None, p, None, None), -1, b"exactly one")     # both
    refused(ft(ctx, p, 8, 4, 4, R, None, -1, None, p, None, None), -1, b"exactly one")  # neither
    refused(ft(ctx, p, 8, 4, 4, R, None, 8, None, p, None, None), -1, b"server_row")
    refused(ft(ctx, p, 8, 4, 4, R, None, -2, None, p, None, None), -1, b"server_row")
    refused(ft(ctx, p, 2049, 4, 4, R, p, -1, None, p, None, None), -3, b"2048")
    # every K <= 2048 has a panel width, so the "no panel layout" refusal cannot be reached: a
    # panel call beyond the cap meets the K refusal first
    assert all(width(k) > 0 for k in (1, 16, 17, 64, 65, 256, 257, 1024, 1025, 2048))
    refused(ft(ctx, p, 4096, 4, 1 << 30, P, p, -1, None, p, None, None), -3, b"2048")
    # d == 0 is GM_OK and launches nothing
    assert ft(ctx, p, 8, 0, 4, R, p, -1, None, p, None, None) == 0
    assert ft(ctx, p, 8, 0, 8 * W, P, None, 3, p, p, None, None) == 0


def test_python_refusals(no_device):
    X = torch.zeros(12, 5)
    s = torch.zeros(5)
    for bad in (X.half(), X.double()):
        with pytest.raises(TypeError):
            bz.fltrust(bad, {"server_update": s})
    with pytest.raises(ValueError):
        bz.fltrust(torch.zeros(12), {"server_update": s})
    with pytest.raises(ValueError, match="2048"):
        bz.fltrust(torch.zeros(2049, 2), {"server_row": 0})
    with pytest.raises(ValueError, match="exactly one"):
        bz.fltrust(X, {})
    with pytest.raises(ValueError, match="exactly one"):
        bz.fltrust(X, {"server_update": s, "server_row": 0})
    with pytest.raises(ValueError, match="server_update"):
        bz.fltrust(X, {"server_update": torch.zeros(6)})
    with pytest.raises(TypeError, match="server_update"):
        bz.fltrust(X, {"server_update": s.double()})
    with pytest.raises(TypeError, match="server_update"):
        bz.fltrust(X, {"server_update": [0.0] * 5})
    for row in (True, 2.0, 1.5, "1"):
        with pytest.raises(TypeError, match="server_row"):
            bz.fltrust(X, {"server_row": row})
    for row in (-1, 12, 100):
        with pytest.raises(ValueError, match="server_row"):
            bz.fltrust(X, {"server_row": row})
    with pytest.raises(ValueError, match="guess"):
        bz.fltrust(X, {"server_row": 0, "guess": torch.zeros(4)})
    # bf16 inputs are accepted: the first thing a valid call does is stage the tensor
    with pytest.raises(AssertionError, match="device"):
        bz.fltrust(X.to(torch.bfloat16), {"server_row": 0, "guess": torch.zeros(5)})


def test_with_options_contract(no_device, monkeypatch):
    f = bz.fltrust.with_options(server_row=0)
    assert f.__name__ == "fltrust" and f.__qualname__ == "fltrust"
    assert bz.bucketed(f, 2).__name__ == "fltrust_b2"
    with pytest.raises(TypeError, match="server_update, server_row"):
        bz.fltrust.with_options(tau=1.0)
    with pytest.raises(TypeError):
        bz.fltrust.with_options(server_row=1.0)
    with pytest.raises(ValueError):
        bz.fltrust.with_options(server_row=-1)
    with pytest.raises(ValueError):
        bz.fltrust.with_options()
    seen = {}

    def fake(wList, options):
        seen["opts"] = options
        return "out"
    monkeypatch.setattr(agg, "fltrust", fake)
    opts = {"guess": 1, "honestSize": 9, "server_row": 5}
    keep = dict(opts)
    s = torch.zeros(3)
    assert bz.fltrust.with_options(server_row=2)("X", opts) == "out"
    assert seen["opts"] == {"guess": 1, "honestSize": 9, "server_row": 2} and opts == keep
    bz.fltrust.with_options(server_update=s)("X", None)
    assert seen["opts"]["server_update"] is s


def _brute(X, s, row, c):
    """The definition, one Python float at a time with exactly rounded sums."""
    K, d = X.shape
    c = [0.0] * d if c is None else [float(v) for v in c]
    sv = [float(v) for v in (X[row] if s is None else s)]
    g = [sv[j] - c[j] for j in range(d)]
    ng = math.fsum(v * v for v in g)
    ts, nk, cos = [], [], []
    for k in range(K):
        u = [float(X[k, j]) - c[j] for j in range(d)]
        bad = any(not math.isfinite(v) for v in u)
        a = math.nan if bad else math.fsum(u[j] * g[j] for j in range(d))
        n = math.nan if bad else math.fsum(v * v for v in u)
        ok = k != row and ng > 0 and not bad and n > 0
        cs = a / math.sqrt(n * ng) if not bad and n > 0 and ng > 0 else math.nan
        cos.append(cs)
        nk.append(n)
        ts.append(cs if ok and cs > 0 else 0.0)
    T = math.fsum(ts)
    out = []
    for j in range(d):
        if T == 0:
            out.append(c[j])
            continue
        out.append(c[j] + math.fsum(ts[k] * math.sqrt(ng / nk[k]) / T * (float(X[k, j]) - c[j])
                                    for k in range(K) if ts[k] > 0))
    return cos, ts, T, out


@pytest.mark.parametrize("as_row", [False, True])
def test_reference_is_the_definition(as_row):
    r = np.random.default_rng(7)
    d = 12
    c = r.standard_normal(d).astype(np.float32)
    g = r.standard_normal(d)
    X = (c + g + 0.5 * r.standard_normal((6, d))).astype(np.float32)
    X[1] = c                                        # a zero row
    X[2, 5] = np.nan                                # a NaN row
    X[3] = (c - 2.0 * g).astype(np.float32)         # a negative cosine
    X[4] = (c + g).astype(np.float32)               # the server as a row
    s, row = (None, 4) if as_row else ((c + g).astype(np.float32), None)
    ref = fc.reference(X, s, row, c)
    cos, ts, T, out = _brute(X, s, row, c)
    assert ref["trusted"] == [k for k in range(6) if ts[k] > 0]
    assert 1 not in ref["trusted"] and 2 not in ref["trusted"] and 3 not in ref["trusted"]
    assert (4 in ref["trusted"]) == (not as_row)
    assert np.isnan(ref["cos"][1]) and np.isnan(ref["cos"][2]) and ref["cos"][3] < -0.9
    assert abs(float(ref["cos"][4]) - 1.0) < 1e-12
    np.testing.assert_allclose(np.asarray(ref["ts"], dtype=np.float64), ts, rtol=0, atol=1e-15)
    assert abs(float(ref["T"]) - T) <= 1e-15 * 6
    np.testing.assert_allclose(np.asarray(ref["out"], dtype=np.float64), out, rtol=1e-14,
                               atol=1e-15)


def test_no_trusted_row_returns_the_centre():
    r = np.random.default_rng(8)
    c = r.standard_normal(9).astype(np.float32)
    g = r.standard_normal(9)
    X = (c - np.abs(r.standard_normal((4, 1))) * g).astype(np.float32)
    ref = fc.reference(X, (c + g).astype(np.float32), None, c)
    assert ref["T"] == 0 and ref["trusted"] == [] and np.array_equal(ref["out32"], c)
    ref = fc.reference(X - c, g.astype(np.float32), None, None)
    assert ref["T"] == 0 and np.array_equal(ref["out32"], np.zeros(9, dtype=np.float32))
    # K = 1 with the row as the server, and a zero server update
    ref = fc.reference(X[:1], None, 0, c)
    assert ref["T"] == 0 and np.array_equal(ref["out32"], c)
    ref = fc.reference(X, c, None, c)
    assert ref["T"] == 0 and np.array_equal(ref["out32"], c)


@pytest.mark.parametrize("K,d", fc.SHAPES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gpu_shapes_meet_the_recipes_conditions(K, d, dtype):
    """Conditions, not measurements: |cos| >= 1e-4 on every finite cosine (case() asserts it),
    each special kind present when K // 5 >= 6, more than half the rows trusted when K >= 5."""
    for server, centre in (("vector", True), ("row", True), ("vector", False), ("row", False)):
        (X, s, row, c, kinds), ref = fc.case(K, d, dtype, server, centre)
        assert X.shape == (K, d) and len(kinds) == K
        if K // 5 >= 6:
            assert set(fc.KINDS) <= set(kinds)
        if K >= 5:
            assert len(ref["trusted"]) > K / 2
        for k, kind in enumerate(kinds):
            if kind in ("flip", "negcos", "nan", "inf", "server"):
                assert k not in ref["trusted"], (k, kind)
            if kind == "zero":
                assert ref["n"][k] == 0 and k not in ref["trusted"]
            if kind in ("honest", "scaled"):
                assert k in ref["trusted"], (k, kind)


@pytest.mark.parametrize("K,d", [(50, 7850), (600, 8200)])
def test_bar_separates_fp64_from_fp32_accumulation(K, d):
    (X, s, row, c, _), ref = fc.case(K, d)
    Xn, sn, cn = X.numpy(), s.numpy(), c.numpy()
    good = fc.worst_out(fc.restate(Xn, sn, row, cn, np.float64), ref, d)
    bad = fc.worst_out(fc.restate(Xn, sn, row, cn, np.float32), ref, d)
    print(f"fltrust bar {K}x{d}: fp64 chunked restatement {good:.3e} of the bar, fp32 "
          f"accumulation {bad:.3e}")
    assert good <= 1.0 < bad
