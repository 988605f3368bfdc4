"""Krum / multi_krum / nnm / pair_distances on bf16 client updates, the parts that need no GPU:
the entry points are declared, bound and exported; the Python layer refuses before a device is
touched and, with the opt-in, gets as far as the device; and the inputs of the GPU tests meet,
in fp64, the conditions those tests rely on (tests/pairdist_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import byzantine_aircomp_amd as bz
import pairdist_cases as pc
from byzantine_aircomp_amd import _lib
from byzantine_aircomp_amd import aggregators as agg

FUNCS = ("gm_krum_bf16", "gm_multi_krum_bf16", "gm_nnm_bf16", "gm_pair_dist_bf16")


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a GPU context (or to stage a tensor) fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(agg, "context", boom)
    monkeypatch.setattr(agg, "_stage", boom)


def test_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "gmagg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    lib = _lib.load()
    for fn in FUNCS:
        assert re.search(rf"^int {fn}\(gm_ctx\* ctx, const uint16_t\* X,", text, flags=re.M), fn
        assert fn in bound and bound[fn][0] is C.c_int
        assert getattr(lib, fn)
    assert re.search(r"^int gm_dist_last_info\(gm_ctx\* ctx, int64_t\* info, double\* beta\);", text,
                     flags=re.M)
    assert re.search(r"enum gm_dist_mode \{ GM_DIST_EXACT = 0, GM_DIST_MFMA = 1 \};", text)
    assert getattr(lib, "gm_dist_last_info")
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    # the _f32 argument lists with an explicit layout, dist_mode ahead of the outputs
    assert bound["gm_krum_bf16"][1] == [p, p, i64, i64, i64, i32, i64, i32, p, C.POINTER(i64), p]
    assert bound["gm_multi_krum_bf16"][1] == [p, p, i64, i64, i64, i32, i64, i64, i32, p, p, p]
    assert bound["gm_nnm_bf16"][1] == [p, p, i64, i64, i64, i32, i64, i32, p, i64, i32, p, p]
    assert bound["gm_pair_dist_bf16"][1] == [p, p, i64, i64, i64, i32, i32, p, p]
    assert (_lib.GM_DIST_EXACT, _lib.GM_DIST_MFMA) == (0, 1)
    assert lib.gm_abi_version() == _lib.ABI_VERSION
    assert bz.pair_distances is agg.pair_distances


def _call(lib, fn, ctx, x, K, d, ldx, layout, mode, out):
    if fn == "gm_krum_bf16":
        return lib.gm_krum_bf16(ctx, x, K, d, ldx, layout, 3, mode, out, None, None)
    if fn == "gm_multi_krum_bf16":
        return lib.gm_multi_krum_bf16(ctx, x, K, d, ldx, layout, 3, 2, mode, out, None, None)
    if fn == "gm_nnm_bf16":
        return lib.gm_nnm_bf16(ctx, x, K, d, ldx, layout, 1, mode, out, max(d, 1), 0, None, None)
    return lib.gm_pair_dist_bf16(ctx, x, K, d, ldx, layout, mode, out, None)


@pytest.mark.parametrize("fn", FUNCS)
def test_abi_refusals_need_no_device(fn):
    """Every refusal happens before the first HIP call, carries the fp32 entries' code and names
    the function; d == 0 is GM_OK and launches nothing."""
    lib = _lib.load()
    bx = (C.c_uint16 * 4096)()
    bo = (C.c_double * 64)(*([7.0] * 64))
    x, o = C.addressof(bx), C.addressof(bo)
    ctx = x                                     # non-NULL; never dereferenced on these paths
    R, P = _lib.GM_LAYOUT_ROWS, _lib.GM_LAYOUT_PANELS

    def refused(rc, code):
        assert rc == code
        msg = lib.gm_last_error()
        assert msg and fn.encode() in msg, msg
        assert list(bo) == [7.0] * 64

    refused(_call(lib, fn, None, x, 8, 4, 4, R, 0, o), -1)
    refused(_call(lib, fn, ctx, None, 8, 4, 4, R, 0, o), -1)
    refused(_call(lib, fn, ctx, x, 8, 4, 4, R, 0, None), -1)
    refused(_call(lib, fn, ctx, x, 0, 4, 4, R, 0, o), -1)          # K < 1
    refused(_call(lib, fn, ctx, x, 8, -1, 4, R, 0, o), -1)         # d < 0
    refused(_call(lib, fn, ctx, x, 8, 4, 3, R, 0, o), -1)          # ldx < d on rows
    refused(_call(lib, fn, ctx, x, 8, 4, 4, 7, 0, o), -1)          # an unknown layout
    refused(_call(lib, fn, ctx, x, 8, 4, 4, R, 2, o), -1)          # an unknown dist_mode
    W = lib.gm_panel_width_bf16(8)
    refused(_call(lib, fn, ctx, x, 8, 4, 8 * W - 1, P, 1, o), -1)  # panel stride < K W
    refused(_call(lib, fn, ctx, x, 4097, 4, 4, R, 1, o), -3)       # K > 4096
    assert lib.gm_panel_width_bf16(4096) == 0
    refused(_call(lib, fn, ctx, x, 4096, 4, 1 << 30, P, 0, o), -3)  # no bf16 panel width
    assert _call(lib, fn, ctx, x, 8, 0, 4, R, 1, o) == 0
    assert list(bo) == [7.0] * 64


def _calls(X):
    """The four public callables on X, as (name, thunk(opt-in, distances))."""
    def opts(b, dist):
        o = {"honestSize": 9}
        if b is not None:
            o["bf16"] = b
        if dist is not None:
            o["distances"] = dist
        return o

    def kw(b, dist):
        k = {}
        if b is not None:
            k["bf16"] = b
        if dist is not None:
            k["distances"] = dist
        return k
    return [("Krum", lambda b, dist: bz.Krum(X, opts(b, dist))),
            ("multi_krum", lambda b, dist: bz.multi_krum(X, opts(b, dist))),
            ("nnm", lambda b, dist: bz.nnm(X, 3, **kw(b, dist))),
            ("pair_distances", lambda b, dist: bz.pair_distances(X, **kw(b, dist))),
            ("mixed", lambda b, dist: bz.mixed(bz.mean)(X, opts(b, dist)))]


def test_python_refuses_before_a_device_is_touched(no_device):
    X = torch.zeros(12, 8)
    Xb = X.to(torch.bfloat16)
    P = bz.ClientPanels(12, 8, device="cpu", dtype=torch.bfloat16)
    # without the opt-in bf16 is refused as before
    for w in (Xb, P):
        for name, call in _calls(w):
            for b in (None, False):
                with pytest.raises(TypeError):
                    call(b, None)
    # an unknown tier, and the fast tier on fp32 (it reads bf16)
    for w, b in ((X, None), (X, True), (Xb, True)):
        for name, call in _calls(w):
            with pytest.raises(ValueError, match="distances"):
                call(b, "fast")
    for name, call in _calls(X):
        for b in (None, True):
            with pytest.raises(ValueError, match="mfma"):
                call(b, "mfma")
    # the opt-in does not widen what else is read
    for name, call in _calls(X.half()):
        with pytest.raises(TypeError):
            call(True, None)


def test_opt_in_reaches_the_device(no_device):
    Xb = torch.zeros(12, 8, dtype=torch.bfloat16)
    P = bz.ClientPanels(12, 8, device="cpu", dtype=torch.bfloat16)
    for w in (Xb, P):
        for name, call in _calls(w):
            for dist in (None, "exact", "mfma"):
                with pytest.raises(AssertionError, match="device"):
                    call(True, dist)
    # fp32 stays what it was, with or without the option
    for name, call in _calls(torch.zeros(12, 8)):
        for b, dist in ((None, None), (True, None), (None, "exact")):
            with pytest.raises(AssertionError, match="device"):
                call(b, dist)


def test_mixed_hands_the_tier_to_nnm(monkeypatch):
    seen = {}

    def fake_nnm(wList, f, layout=None, neighbors=False, bf16=False, distances="exact"):
        seen["nnm"] = (f, bf16, distances)
        return "mixed rows"

    def inner(wList, options):
        seen["inner"] = dict(options)
        return torch.ones(3)

    monkeypatch.setattr(agg, "nnm", fake_nnm)
    X = torch.zeros(12, 3)
    opts = {"honestSize": 9, "bf16": True, "distances": "mfma"}
    keep = dict(opts)
    bz.mixed(inner)(X, opts)
    assert seen["nnm"] == (3, True, "mfma") and seen["inner"] == keep and opts == keep
    bz.mixed(inner)(X, {"honestSize": 9})
    assert seen["nnm"] == (3, False, "exact")


# ---- the inputs of the GPU tests, in fp64 -----------------------------------------------------

def test_beta_condition_and_shapes():
    assert pc.BETA_MAX == 2.0 ** -13 and pc.BETA_CHECKED >= pc.BETA_MAX
    assert pc.C_FLUSH in pc.DS and pc.C_FLUSH + 8 in pc.DS
    assert -(-pc.D_TWO_SLICES // pc.C_FLUSH) >= 2


@pytest.mark.parametrize("K,d,f", pc.NEIGHBOR_CASES)
def test_graded_inputs_meet_the_ambiguity_cap(K, d, f):
    D, rho = pc.dist_rho(pc.graded(K, d))
    amb = pc.ambiguous_rows(D, rho, f, pc.BETA_CHECKED)
    assert amb <= pc.MAX_AMBIGUOUS * K, (amb, K)
    # a smaller band never makes more rows ambiguous
    assert pc.ambiguous_rows(D, rho, f, pc.BETA_MAX) <= amb


@pytest.mark.parametrize("K,d,honest,ms", pc.SELECT_CASES)
def test_graded_selections_are_determined(K, d, honest, ms):
    D, rho = pc.dist_rho(pc.graded(K, d))
    for m in ms:
        sel, ok = pc.selection_determined(D, rho, honest, m, pc.BETA_CHECKED)
        assert ok, (K, d, honest, m)
        assert sel.size == m


def test_integer_inputs_are_exact_in_fp32():
    for K, d, B in ((17, 264, 0), (129, 4120, 5), (300, 333, 0)):
        x = pc.widened(pc.integers(K, d, B))
        assert np.abs(x).max() <= 15 and (x == np.round(x)).all()
        assert d * 30 * 30 < 2 ** 24                       # every distance and partial sum
        if B:
            assert (x[K - B:] == x[K - B]).all()
        D, _ = pc.dist_rho(pc.integers(K, d, B))
        # colliding distances: the index decides many neighbour choices
        assert np.unique(D).size < D.size // 2


def test_band_helpers_on_a_hand_case():
    # three rows on a line at 0, 1, 1 + tiny: with a band wider than the gap the farther two are
    # undecided for row 0, with a narrow one everything is decided
    x = np.array([[0.0], [1.0], [1.0 + 2.0 ** -10]])
    D = (x - x.T) ** 2
    rho = (x * x).sum(axis=1)
    ins, out = pc.neighbor_sets(D, pc.band(rho, 2.0 ** -20), 2)
    assert ins[0].tolist() == [True, True, False] and out[0].tolist() == [False, False, True]
    ins, out = pc.neighbor_sets(D, pc.band(rho, 2.0 ** -8), 2)
    assert ins[0].tolist() == [True, False, False] and out[0].tolist() == [False, False, False]
