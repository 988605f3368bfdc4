"""mean / median / trimmed_mean on bf16 client updates (coordinate_bf16.hip) against the CPU
references of tests/coordinate_cases.py, computed on the widened values: the inputs are rounded
to bf16 first, the reference reads ``.float().numpy()`` of them.  The bars are the fp32 kernels'
own: the median compared with == plus an equal NaN mask, the mean and the trimmed mean within
1 fp32 ulp of the fsum reference with the same NaN / inf pattern, under the kappa <= 1e4
precondition (asserted on the widened values before any GPU call).

  A  every kernel of the dispatch (tiers at K = 64, 128, 256, 512, 1024) on 33 tiles of 32
     columns + a ragged one, as an aligned view, a view one element into its buffer and panels
  B  the mean past the selections' K limit
  C  adversarial columns, among them columns made for 16-bit keys
  D  gm_trimmed_mean_bf16's `trim` range and the refusals, through the C ABI
  E  one wide case: more tiles than one round of co-resident blocks
  F  (inside A, C and E) the median's bits equal the fp32 entry point's on the widened matrix
"""
import functools

import numpy as np
import pytest
import torch

import coordinate_cases as cc

pytestmark = pytest.mark.gpu

GM_ERR_INVALID, GM_ERR_UNSUPPORTED = -1, -3
ROWS, PANELS = 0, 1
BF16 = {"bf16": True}            # the option under which the three functions read bf16
TILE = 32                         # columns per block of col_select_bf16, every K tier
FULL_D = 33 * TILE + 5            # 1061


def _bz():
    import byzantine_aircomp_amd as bz
    return bz


def _round(X):
    """fp32 numpy -> (bf16 CPU tensor, its widened values as fp32 numpy)."""
    Xb = torch.from_numpy(np.array(X, dtype=np.float32)).to(torch.bfloat16)
    return Xb, Xb.float().numpy()


def _from_bits(bits):
    """uint16 bit patterns [K, d] -> (bf16 CPU tensor, widened fp32 numpy)."""
    Xb = torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)
    return Xb, Xb.float().numpy()


def _bits_of(Xw):
    """bf16-representable fp32 numpy -> uint16 bit patterns."""
    return (np.ascontiguousarray(Xw, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _kappa_ok(X, trims):
    try:
        cc.assert_kappa(X, trims)
    except AssertionError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def normal_bf16(K, d, trims=None):
    """cc.normal_case's recipe and seed, rounded to bf16: "condition, then round", repeated
    until the precondition holds on the rounded matrix (at K >= 63 the first round does).
    Returns (bf16 tensor, widened matrix, refs)."""
    rng = np.random.default_rng(1000 * K + d)
    tr = tuple(sorted({0, cc.default_trim(K)} | set(trims or ())))
    Xw = cc._normal(rng, K, d)
    for _ in range(64):
        Xb, Xw = _round(cc.condition(Xw, tr))
        if _kappa_ok(Xw, tr):
            break
        Xw = Xw.copy()
    cc.assert_kappa(Xw, tr)
    Xw.setflags(write=False)
    return Xb, Xw, cc._refs(Xw, tr)


def forms(Xb):
    """Xb on the GPU as the forms the launcher tells apart: "aligned" (16-byte base, ldx % 8 ==
    0), "offset" (one element into its buffer: base 2 bytes off 16, odd ldx) and, where K has a
    bf16 panel width, "panels".  The buffers' other columns are NaN: a read past column d
    shows in the result."""
    bz = _bz()
    K, d = Xb.shape
    nan = float("nan")
    a = torch.full((K, d + ((-d) % 8 or 8)), nan, dtype=torch.bfloat16, device="cuda")
    a[:, :d] = Xb.cuda()
    ld = d + 3 if (d + 3) % 2 else d + 4
    b = torch.full((K, ld), nan, dtype=torch.bfloat16, device="cuda")
    b[:, 1:1 + d] = Xb.cuda()
    va, vb = a[:, :d], b[:, 1:1 + d]
    assert va.data_ptr() % 16 == 0 and va.stride(0) % 8 == 0
    assert vb.data_ptr() % 16 == 2 and vb.stride(0) % 2 == 1
    # the views hold Xb's bits (special NaN payloads included)
    assert torch.equal(va.view(torch.int16).cpu(), Xb.view(torch.int16))
    out = [("aligned", va), ("offset", vb)]
    if int(bz._lib.load().gm_panel_width_bf16(K)) > 0:
        P = bz.ClientPanels.from_rows(Xb.cuda())
        assert P.dtype == torch.bfloat16
        out.append(("panels", P))
    return out


def _i32(t):
    return t.cpu().numpy().view(np.int32)


def check_all(Xb, Xw, refs, what, funcs=("median", "trimmed", "mean"), fp32_median=True):
    """The three functions on every form against `refs`; the forms return identical bits; the
    median's bits equal the fp32 entry point's on the widened matrix."""
    bz = _bz()
    K = Xb.shape[0]
    first = {}
    for lname, V in forms(Xb):
        for f in funcs:
            if f == "median":
                got = bz.median(V, BF16)
                bad = cc.mismatch_exact(got.cpu().numpy(), refs["median"], f"{what} {lname} median")
            elif f == "trimmed":
                got = bz.trimmed_mean(V, BF16)
                bad = cc.mismatch_ulp(got.cpu().numpy(), refs["trimmed"],
                                      f"{what} {lname} trimmed_mean")
            else:
                got = bz.mean(V, BF16)
                bad = cc.mismatch_ulp(got.cpu().numpy(), refs["mean"], f"{what} {lname} mean")
            assert bad is None, bad
            assert got.dtype == torch.float32 and got.shape == (Xb.shape[1],)
            if f in first:
                assert np.array_equal(_i32(got), first[f]), f"{what} {f}: {lname} differs in bits"
            else:
                first[f] = _i32(got)
    if fp32_median and "median" in funcs and K <= 2048:
        wide = bz.median(torch.from_numpy(np.array(Xw)).cuda())
        assert np.array_equal(_i32(wide), first["median"]), f"{what}: bf16 vs fp32 median bits"


def _distinct_tiles(ref, what):
    """No two of the kernel's column tiles carry the same reference values: a permuted or
    duplicated tile cannot go unnoticed (the 0.001 j marker of cc._normal is below bf16
    resolution, so this is asserted rather than assumed)."""
    tiles = [ref[j:j + TILE].tobytes() for j in range(0, len(ref), TILE)]
    assert len(set(tiles)) == len(tiles), what


# ------------------------------------------------------------------------------------- A

@pytest.mark.parametrize("K", [1, 2, 3, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024, 1025,
                               1500, 2048])
def test_full_tiles_three_forms(K):
    Xb, Xw, refs = normal_bf16(K, FULL_D)
    cc.assert_kappa(Xw, (0, cc.default_trim(K)))
    for f in ("median", "trimmed", "mean"):
        _distinct_tiles(refs[f], f"K={K} {f}")
    check_all(Xb, Xw, refs, f"K={K}")


# ------------------------------------------------------------------------------------- B

@pytest.mark.parametrize("K", [2049, 5000])
def test_mean_beyond_selection_K(K):
    """The mean has no K limit on rows (5000 fp64 terms at kappa <= 1e4: relative 5.6e-9, far
    under half an fp32 ulp), special values included."""
    bz = _bz()
    d = 133
    _, Xw, _ = normal_bf16(K, d)
    X = np.array(Xw)
    X[0, 1] = np.inf
    X[1, 2] = -np.inf
    X[2, 3] = np.nan
    X[:2, 4] = (np.inf, -np.inf)
    X[:, 5] = 0.0
    X[::2, 5] = -0.0
    X[: K // 2 + 5, 6] = 3e38
    Xb, Xw = _round(X)
    cc.assert_kappa(Xw, (0,))
    want = cc.ref_mean(Xw)
    assert np.isposinf(want[1]) and np.isneginf(want[2]) and np.isnan(want[[3, 4]]).all()
    assert int(bz._lib.load().gm_panel_width_bf16(K)) == 0
    got = {}
    for lname, V in forms(Xb):
        got[lname] = bz.mean(V, BF16)
        bad = cc.mismatch_ulp(got[lname].cpu().numpy(), want, f"K={K} {lname} mean")
        assert bad is None, bad
    assert np.array_equal(_i32(got["aligned"]), _i32(got["offset"]))
    for fn in (bz.median, bz.trimmed_mean):               # the selections stop at K = 2048
        with pytest.raises(bz._lib.GmError, match="K <= 2048"):
            fn(Xb.cuda(), BF16)


# ------------------------------------------------------------------------------------- C

QNAN, SNAN, NNAN = 0x7FC0, 0x7F81, 0xFFFF      # NaN payloads as bf16 bit patterns
PINF, NINF, MAXF = 0x7F80, 0xFF80, 0x7F7F


@functools.lru_cache(maxsize=None)
def adversarial_bf16(K):
    """cc.adversarial_case(K) rounded to bf16, plus columns made for 16-bit keys, built as bit
    patterns.  Returns (bf16 tensor, widened matrix, refs, names of the added columns)."""
    rng = np.random.default_rng(31 * K + 7)
    b, r = cc.default_trim(K), (K - 1) // 2
    assert b >= 4
    base = _bits_of(_round(cc.adversarial_case(K)[0])[1])
    cols, names = [], []

    def add(name, col, permute=True):
        col = np.asarray(col)
        assert col.shape == (K,)
        cols.append(col[rng.permutation(K)] if permute else col)
        names.append(name)

    def f2b(x):
        w = _round(np.asarray(x, dtype=np.float32))[1]
        return _bits_of(w)

    N = lambda: rng.standard_normal(K).astype(np.float32)      # noqa: E731
    # all K values inside [1, 2): 128 distinct bf16 values, the key's top 9 bits shared
    add("in[1,2)", 0x3F80 + (np.arange(K) % 128))
    add("in[1,2) random", 0x3F80 + rng.integers(0, 128, K))
    add("in[-2,-1)", 0xBF80 + rng.integers(0, 128, K))
    add("all equal", np.full(K, 0x3EC0))                        # 0.375
    add("all equal negative", np.full(K, 0xC010))
    # two values only, the count of the smaller one straddling the median rank and both trim
    # boundaries
    for n_lo in (r, r + 1, b, b + 1, K - b - 1, K - b):
        lo, hi = (0xBFC0, 0x4010) if n_lo <= r + 1 else (0x3FC0, 0x4010)   # -1.5 / 1.5, 2.25
        add(f"two values n_lo={n_lo}", np.where(np.arange(K) < n_lo, lo, hi))
    # bf16 subnormals (and zeros of both signs), mostly positive
    sub = rng.integers(0, 0x80, K)
    add("subnormals", np.where(rng.random(K) < 0.2, 0x8000 | sub, sub))
    # the largest finite bf16 in more than half the rows
    add("max finite", np.where(np.arange(K) < K // 2 + 5, MAXF, f2b(N())))
    add("-max finite", np.where(np.arange(K) < K // 2 + 5, 0x8000 | MAXF, f2b(N())))
    # NaNs of several payloads out of the kept middle (3 < b of them: trimmed away) ...
    col = f2b(N() + 3.0)
    col[:3] = (QNAN, SNAN, NNAN)
    add("three NaNs", col)
    # ... and in it
    col = f2b(N() + 3.0)
    col[:K // 3] = np.resize([QNAN, SNAN, NNAN, 0x7FFF, 0xFFC1], K // 3)
    add("K/3 NaNs", col)
    col = f2b(N() + 3.0)
    col[:b + 1] = NNAN                                          # one NaN reaches rank K-b-1
    add("b+1 negative-payload NaNs", col)
    col = f2b(N() + 3.0)
    col[:b] = SNAN                                              # exactly b: none is kept
    add("b signalling NaNs", col)
    # +-inf on both sides of the kept middle
    col = f2b(N() + 3.0)
    col[:2], col[2:4] = PINF, NINF
    add("2 +inf 2 -inf trimmed", col)
    col = f2b(N() + 3.0)
    col[:b + 2] = PINF
    add("b+2 +inf", col)
    col = f2b(N() + 3.0)
    col[:b + 2] = NINF
    add("b+2 -inf", col)
    col = f2b(N() + 3.0)
    col[:b], col[b:2 * b] = PINF, NINF
    add("b +inf b -inf", col)
    # b and b + 1 copies of the extreme values
    for n in (b, b + 1):
        col = f2b(np.clip(N(), -2.5, 2.5) + 1.0)
        col[:n], col[n:2 * n] = 0xC080, 0x40C0                  # -4, 6
        add(f"{n} copies of the extremes", col)
    bits = np.concatenate([base, np.stack(cols, axis=1).astype(np.uint16)], axis=1)
    Xb, Xw = _from_bits(bits)
    Xw.setflags(write=False)
    tr = (0, b)
    return Xb, Xw, cc._refs(Xw, tr), {n: base.shape[1] + i for i, n in enumerate(names)}


@pytest.mark.parametrize("K", [200, 512, 513, 1000, 1024, 1025, 2048])
def test_adversarial_columns(K):
    Xb, Xw, refs, at = adversarial_bf16(K)
    b = cc.default_trim(K)
    cc.assert_kappa(Xw, (0, b))
    t, m = refs["trimmed"], refs["median"]
    # what the recipe is for, from the reference
    assert len(np.unique(Xw[:, at["in[1,2)"]])) == min(K, 128)
    assert np.isfinite(t[at["three NaNs"]]) and np.isnan(m[at["three NaNs"]])
    assert np.isfinite(t[at["b signalling NaNs"]])
    assert np.isnan(t[[at["K/3 NaNs"], at["b+1 negative-payload NaNs"]]]).all()
    assert np.isfinite(t[at["2 +inf 2 -inf trimmed"]]) and np.isfinite(t[at["b +inf b -inf"]])
    assert np.isposinf(t[at["b+2 +inf"]]) and np.isneginf(t[at["b+2 -inf"]])
    assert np.isfinite(t[at["max finite"]]) and m[at["max finite"]] > 3e38
    assert np.isnan(refs["mean"][at["2 +inf 2 -inf trimmed"]])
    assert np.isfinite(refs["trimmed"][[0, 12, 16, 17]]).all()
    assert np.isnan(refs["trimmed"][[14, 15]]).all() and np.isfinite(refs["trimmed"][13])
    check_all(Xb, Xw, refs, f"adversarial K={K}")


# ------------------------------------------------------------------------------------- D

def _abi():
    bz = _bz()
    ctx = bz.aggregators.context()
    return bz, ctx, torch.cuda.current_stream().cuda_stream


def _trims(K):
    return sorted({0, 1, (K - 1) // 2} | ({K // 2 - 1} if K % 2 == 0 else set()))


@pytest.mark.parametrize("K", [7, 64, 100, 513, 1000, 2048])
def test_trim_range_c_abi(K):
    """trim = 0 (ranks 0 and K-1, next to the padding keys) is the mean; 2 trim = K-1 (the
    lo == hi branch) is the median; the panel call returns the rows call's bits."""
    bz, ctx, stream = _abi()
    d = 70
    trims = _trims(K)
    Xb, Xw, refs = normal_bf16(K, d, tuple(trims))
    cc.assert_kappa(Xw, trims)
    Xc = Xb.cuda()
    P = bz.ClientPanels.from_rows(Xc)
    assert P.dtype == torch.bfloat16
    med = torch.full((d,), float("nan"), device="cuda")
    rc = ctx.lib.gm_median_bf16(ctx.handle, Xc.data_ptr(), K, d, d, ROWS, med.data_ptr(), stream)
    assert rc == 0, (rc, ctx.lib.gm_last_error())
    assert cc.mismatch_exact(med.cpu().numpy(), refs["median"], f"K={K} median") is None
    for trim in trims:
        out = torch.full((d,), float("nan"), device="cuda")
        outp = torch.full((d,), float("nan"), device="cuda")
        rc = ctx.lib.gm_trimmed_mean_bf16(ctx.handle, Xc.data_ptr(), K, d, d, ROWS, trim,
                                          out.data_ptr(), stream)
        assert rc == 0, (trim, rc, ctx.lib.gm_last_error())
        rc = ctx.lib.gm_trimmed_mean_bf16(ctx.handle, P.data.data_ptr(), K, d, P.panel_stride,
                                          PANELS, trim, outp.data_ptr(), stream)
        assert rc == 0, (trim, rc, ctx.lib.gm_last_error())
        got = out.cpu().numpy()
        bad = cc.mismatch_ulp(got, refs[("trim", trim)], f"K={K} trim={trim}")
        assert bad is None, bad
        if trim == 0:
            bad = cc.mismatch_ulp(got, refs["mean"], f"K={K} trim=0 vs mean")
            assert bad is None, bad
        if 2 * trim == K - 1:
            bad = cc.mismatch_exact(got, refs["median"], f"K={K} trim={trim} vs median")
            assert bad is None, bad
            assert np.array_equal(got.view(np.int32), _i32(med))
        assert np.array_equal(_i32(outp), got.view(np.int32)), (K, trim)


def test_argument_errors_c_abi():
    """The return codes of the fp32 twins; a refused call writes nothing."""
    bz, ctx, stream = _abi()
    lib, h = ctx.lib, ctx.handle
    K, d = 100, 16
    X = torch.zeros(4097, d, dtype=torch.bfloat16, device="cuda")
    P = bz.ClientPanels.from_rows(X[:K])
    W = int(lib.gm_panel_width_bf16(K))
    out = torch.zeros(d, device="cuda")
    x, p, o = X.data_ptr(), P.data.data_ptr(), out.data_ptr()

    def is_(rc, want, fn):
        assert rc == want, (rc, want, lib.gm_last_error())
        assert want == 0 or fn.encode() in lib.gm_last_error()

    for trim in (K // 2, K // 2 + 1, K, -1):
        is_(lib.gm_trimmed_mean_bf16(h, x, K, d, d, ROWS, trim, o, stream), GM_ERR_INVALID,
            "gm_trimmed_mean_bf16")
        is_(lib.gm_trimmed_mean_bf16(h, p, K, d, P.panel_stride, PANELS, trim, o, stream),
            GM_ERR_INVALID, "gm_trimmed_mean_bf16")
    mean, median, trimmed = "gm_mean_bf16", "gm_median_bf16", "gm_trimmed_mean_bf16"
    # NULL arguments
    is_(lib.gm_mean_bf16(None, x, K, d, d, ROWS, o, stream), GM_ERR_INVALID, mean)
    is_(lib.gm_median_bf16(h, None, K, d, d, ROWS, o, stream), GM_ERR_INVALID, median)
    is_(lib.gm_trimmed_mean_bf16(h, x, K, d, d, ROWS, 10, None, stream), GM_ERR_INVALID, trimmed)
    # ldx < d on rows, a panel stride < K W, an unknown layout
    is_(lib.gm_trimmed_mean_bf16(h, x, K, d, d - 1, ROWS, 10, o, stream), GM_ERR_INVALID, trimmed)
    is_(lib.gm_median_bf16(h, x, K, d, d - 1, ROWS, o, stream), GM_ERR_INVALID, median)
    is_(lib.gm_mean_bf16(h, x, K, d, d - 1, ROWS, o, stream), GM_ERR_INVALID, mean)
    is_(lib.gm_mean_bf16(h, p, K, d, K * W - 1, PANELS, o, stream), GM_ERR_INVALID, mean)
    is_(lib.gm_mean_bf16(h, x, K, d, d, 2, o, stream), GM_ERR_INVALID, mean)
    is_(lib.gm_median_bf16(h, x, K, d, d, -1, o, stream), GM_ERR_INVALID, median)
    is_(lib.gm_trimmed_mean_bf16(h, x, K, d, d, 7, 10, o, stream), GM_ERR_INVALID, trimmed)
    # K > 2048 in the two selections; panels at a K without a bf16 panel width
    is_(lib.gm_median_bf16(h, x, 2049, d, d, ROWS, o, stream), GM_ERR_UNSUPPORTED, median)
    is_(lib.gm_trimmed_mean_bf16(h, x, 2049, d, d, ROWS, 204, o, stream), GM_ERR_UNSUPPORTED,
        trimmed)
    assert lib.gm_panel_width_bf16(4096) == 0
    is_(lib.gm_mean_bf16(h, x, 4096, d, 1 << 30, PANELS, o, stream), GM_ERR_UNSUPPORTED, mean)
    is_(lib.gm_median_bf16(h, x, 4096, d, 1 << 30, PANELS, o, stream), GM_ERR_UNSUPPORTED, median)
    torch.cuda.synchronize()
    assert not out.cpu().any()                            # a refused call writes nothing
    is_(lib.gm_trimmed_mean_bf16(h, x, 7, d, d, ROWS, 3, o, stream), 0, trimmed)   # 2 trim = K-1
    is_(lib.gm_mean_bf16(h, x, 4097, d, d, ROWS, o, stream), 0, mean)              # no K limit
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- E

def test_wide_case():
    """K = 513 x d = 12309: 385 tiles of 32 columns, more blocks than are co-resident."""
    K, d = cc.WIDE
    Xb, Xw, refs = normal_bf16(K, d)
    cc.assert_kappa(Xw, (0, cc.default_trim(K)))
    check_all(Xb, Xw, refs, f"wide K={K} d={d}")
