"""mean / median / trimmed_mean on bf16 client updates, the parts that need no GPU: the three
C-ABI entry points are declared, bound and exported, they refuse before the first HIP call, and
the Python layer checks the dtype before anything is staged (bf16 is read under
``options={"bf16": True}``; a call without it stays fp32)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import _lib
from byzantine_aircomp_amd import aggregators as agg

FUNCS = ("gm_mean_bf16", "gm_median_bf16", "gm_trimmed_mean_bf16")


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
    # (ctx, X, K, d, ldx, layout, [trim,] out, stream): the layout follows ldx
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert bound["gm_mean_bf16"][1] == [p, p, i64, i64, i64, i32, p, p]
    assert bound["gm_median_bf16"][1] == [p, p, i64, i64, i64, i32, p, p]
    assert bound["gm_trimmed_mean_bf16"][1] == [p, p, i64, i64, i64, i32, i64, p, p]
    assert _lib.ABI_VERSION == 5 and lib.gm_abi_version() == 5


def _call(lib, fn, ctx, x, K, d, ldx, layout, trim, out):
    if fn == "gm_trimmed_mean_bf16":
        return lib.gm_trimmed_mean_bf16(ctx, x, K, d, ldx, layout, trim, out, None)
    return getattr(lib, fn)(ctx, x, K, d, ldx, layout, out, None)


@pytest.mark.parametrize("fn", FUNCS)
def test_abi_refusals_need_no_device(fn):
    """Every refusal happens before the first HIP call (the context pointer is only handed on,
    never read, before the checks pass), carries the fp32 twins' code, names the function and
    leaves `out` alone."""
    lib = _lib.load()
    bx = (C.c_uint16 * 4096)()
    bo = (C.c_float * 64)(*([7.0] * 64))
    x, o = C.addressof(bx), C.addressof(bo)
    ctx = x                                     # non-NULL; never dereferenced on these paths
    R, P = _lib.GM_LAYOUT_ROWS, _lib.GM_LAYOUT_PANELS
    sel = fn != "gm_mean_bf16"

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
    W = lib.gm_panel_width_bf16(8)
    assert W > 0
    refused(_call(lib, fn, ctx, x, 8, 4, 8 * W - 1, P, 0, o), -1)  # panel stride < K W
    if sel:
        refused(_call(lib, fn, ctx, x, 2049, 4, 1 << 30, P, 0, o), -3)   # K > 2048
    else:
        refused(_call(lib, fn, ctx, x, 4096, 4, 1 << 30, P, 0, o), -3)   # no bf16 panel width
        assert lib.gm_panel_width_bf16(4096) == 0
    if sel:
        refused(_call(lib, fn, ctx, x, 2049, 4, 4, R, 204, o), -3)     # K > 2048
    if fn == "gm_trimmed_mean_bf16":
        for K, trim in ((8, -1), (8, 4), (7, 4), (1, 1)):              # 0 <= 2 trim <= K - 1
            refused(_call(lib, fn, ctx, x, K, 4, 4, R, trim, o), -1)
    # d == 0 is GM_OK and launches nothing
    assert _call(lib, fn, ctx, x, 8, 0, 4, R, 0, o) == 0
    assert _call(lib, fn, ctx, x, 8, 0, 8 * W, P, 3, o) == 0
    assert list(bo) == [7.0] * 64


def test_null_context_is_reported_not_raised():
    lib = _lib.load()
    for fn in FUNCS:
        rc = _call(lib, fn, None, None, 0, 0, 0, 0, 0, None)
        assert rc == -1
        assert fn.encode() in lib.gm_last_error()


@pytest.mark.parametrize("name", ["mean", "median", "trimmed_mean"])
def test_python_checks_the_dtype_before_staging(name, no_device):
    fn = getattr(bz, name)
    X = torch.zeros(12, 5)
    for bad in (X.half(), X.double()):
        with pytest.raises(TypeError):
            fn(bad)
    with pytest.raises(TypeError):
        fn(X.to(torch.int32))
    # bf16 under options={"bf16": True} (and fp32 as before) pass the checks: the next thing is
    # staging the tensor
    Xb = X.to(torch.bfloat16)
    for ok, opts in ((Xb, {"bf16": True}), (X, {}), (X, {"bf16": True})):
        with pytest.raises(AssertionError, match="device"):
            fn(ok, opts)
    # bf16 panels pass too and go straight to the context
    P = bz.ClientPanels(12, 5, device="cpu", dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match="device"):
        fn(P, {"bf16": True})
    # without the option the call stays fp32: bf16 is refused as before, untouched device too
    for opts in ({}, None, {"bf16": False}, {"maxiter": 3}):
        for w in (Xb, P):
            with pytest.raises(TypeError, match="bf16"):
                fn(w, opts)
    with pytest.raises(TypeError):
        fn(Xb)
    # the option does not widen what else is read
    for bad in (X.half(), X.double()):
        with pytest.raises(TypeError):
            fn(bad, {"bf16": True})
