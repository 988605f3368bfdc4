"""What every entry point hands the library for every form a caller may pass: fp32 or bf16, a
[K, d] tensor (contiguous, row-strided, misaligned, transposed, on the CPU) or ClientPanels.  A
recording ``Context.call`` notes each library call (name, scalars, and for every pointer whether
it is the caller's own ``data_ptr()``) and then makes it.  The rules, read from the bindings:

  * a unit-column-stride CUDA tensor with rows >= d apart is passed as it is: the caller's pointer,
    ``ldx == stride(0)``, GM_LAYOUT_ROWS;
  * a non-unit or overlapping stride, or a CPU tensor, goes through a copy with ``ldx == d``;
  * ClientPanels are passed as ``data``, ``panel_stride`` and GM_LAYOUT_PANELS, or to the
    ``*_panels_f32`` twin where the entry point has one;
  * bf16 rows to gm2 / gm / cclip are read in place only with a 16-byte aligned base and d and the
    row stride multiples of 8; otherwise they are packed into bf16 panels first.

The input keeps its bits (the in-place entry points write what the contiguous CUDA call writes),
the result lives on the caller's device, and every entry point but gm2 / gm / cclip (held to
their numeric bars elsewhere) returns the bits of the contiguous CUDA call."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 12
DS = (40, 37)            # d % 8 == 0: aligned bf16 rows are read in place; 37: always packed
LD = 48                  # the row-strided view's leading dimension
B = 3                    # Byzantine rows of the attacks, f of nnm / arc / dnc
FORMS = ("cuda", "strided", "offset", "transposed", "cpu", "panels")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
ROWS, PANELS = 0, 1


def _bz():
    import byzantine_aircomp_amd as bz
    return bz


def _gen():
    return torch.Generator().manual_seed(5)


def _gm2_opts():
    return {"maxiter": 3, "tol": 1e-5}


# name: (call, dtypes it reads, "pure" / "inplace" / "wrapper", bit-identical across forms)
ENTRIES = {
    "gm2": (lambda bz, w: bz.gm2(w, _gm2_opts()), ("fp32", "bf16"), "pure", False),
    "gm": (lambda bz, w: bz.gm(w, dict(_gm2_opts(), seed=11)), ("fp32", "bf16"), "pure", False),
    "cclip": (lambda bz, w: bz.cclip(w, {"tau": 1.0, "clip_iters": 2}), ("fp32", "bf16"), "pure",
              False),
    "mean": (lambda bz, w: bz.mean(w), ("fp32",), "pure", True),
    "median": (lambda bz, w: bz.median(w), ("fp32",), "pure", True),
    "trimmed_mean": (lambda bz, w: bz.trimmed_mean(w), ("fp32",), "pure", True),
    "Krum": (lambda bz, w: bz.Krum(w, {"honestSize": K - B}), ("fp32",), "pure", True),
    "meamed": (lambda bz, w: bz.meamed(w, {"honestSize": K - B}), ("fp32",), "pure", True),
    "multi_krum": (lambda bz, w: bz.multi_krum(w, {"honestSize": K - B}), ("fp32",), "pure", True),
    "bulyan": (lambda bz, w: bz.bulyan(w, {"honestSize": K - 2}), ("fp32",), "pure", True),
    "dnc": (lambda bz, w: bz.dnc(w, {"honestSize": K - B, "dnc_dims": 16, "generator": _gen()}),
            ("fp32",), "pure", True),
    "fltrust": (lambda bz, w: bz.fltrust(w, {"server_row": 0}), ("fp32", "bf16"), "pure", True),
    "bucketing": (lambda bz, w: bz.bucketing(w, 2, generator=_gen()), ("fp32", "bf16"), "pure",
                  True),
    "nnm": (lambda bz, w: bz.nnm(w, B), ("fp32",), "pure", True),
    "clip": (lambda bz, w: bz.clip(w, 1.0), ("fp32", "bf16"), "pure", True),
    "arc": (lambda bz, w: bz.arc(w, B), ("fp32", "bf16"), "pure", True),
    "clip_inplace": (lambda bz, w: bz.clip(w, 1.0, inplace=True), ("fp32",), "inplace", True),
    "arc_inplace": (lambda bz, w: bz.arc(w, B, inplace=True), ("fp32",), "inplace", True),
    "OMA": (lambda bz, w: bz.OMA(w, 0.01, seed=7), ("fp32",), "inplace", True),
    "honest_variance": (lambda bz, w: bz.aggregators.honest_variance(w, K - B), ("fp32",), "pure",
                        True),
    "alie": (lambda bz, w: bz.alie(w, B), ("fp32", "bf16"), "inplace", True),
    "ipm": (lambda bz, w: bz.ipm(w, B), ("fp32", "bf16"), "inplace", True),
    "minmax": (lambda bz, w: bz.minmax(w, B), ("fp32",), "inplace", True),
    "bucketed": (lambda bz, w: bz.bucketed(bz.gm2, 2, generator=_gen())(w, _gm2_opts()),
                 ("fp32", "bf16"), "wrapper", False),
    "mixed": (lambda bz, w: bz.mixed(bz.gm2, f=B)(w, _gm2_opts()), ("fp32",), "wrapper", False),
    "clipped": (lambda bz, w: bz.clipped(bz.gm2, f=B)(w, _gm2_opts()), ("fp32", "bf16"),
                "wrapper", False),
}
STREAM = ("gm2", "gm", "cclip")          # bf16 rows: read in place when aligned, else packed
# (name of the output pointer's argument, after the handle) of the calls that write rows
OUT_AT = {"gm_bucket_means": 7, "gm_nnm": 6, "gm_clip_rows": 9}

CASES = [(e, t, d, f) for e, (_, dts, _, _) in ENTRIES.items() for t in dts for d in DS
         for f in FORMS]


def _values(d, dtype):
    """[K, d] on the CPU: 0.1 N(0, 1) rows, the last B shifted by 0.5."""
    X = 0.1 * torch.randn(K, d, generator=torch.Generator().manual_seed(1000 + d))
    X[-B:] += 0.5
    return X.to(dtype)


def _form(X, form):
    """(the operand, the tensor that backs it) holding X's values in `form`."""
    Kx, d = X.shape
    dev = torch.device("cuda")
    if form == "cuda":
        w = X.to(dev)
        return w, w
    if form == "strided":
        buf = torch.zeros(Kx, LD, dtype=X.dtype, device=dev)
        w = buf[:, :d]
    elif form == "offset":
        buf = torch.zeros(Kx * d + 8, dtype=X.dtype, device=dev)
        w = buf[1:1 + Kx * d].view(Kx, d)
        assert w.data_ptr() % 16 != 0 and w.is_contiguous()
    elif form == "transposed":
        buf = torch.zeros(d, Kx, dtype=X.dtype, device=dev)
        w = buf.t()
        assert w.stride(1) != 1
    elif form == "cpu":
        w = X.clone()
        return w, w
    else:
        P = _bz().ClientPanels.from_rows(X.to(dev))
        return P, P.data
    w.copy_(X)
    return w, buf


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rows(x):
    """A result or an operand as a CPU tensor (ClientPanels as their rows)."""
    if isinstance(x, _bz().ClientPanels):
        x = x.to_rows()
    return x.detach().cpu().clone()


def _own_ptr(w):
    return (w.data if isinstance(w, _bz().ClientPanels) else w).data_ptr()


def _trace(monkeypatch, w, run):
    """(run()'s result, the library calls it made): each call as a dict of the function name,
    the raw arguments after the handle, and their record — scalars as they are, a pointer as
    "own" (the caller's data_ptr()), "other", "null" or "host" (a ctypes object), a struct by
    its type name and layout field."""
    from byzantine_aircomp_amd import _lib
    from byzantine_aircomp_amd.aggregators import Context
    argtypes = {name: args[1:] for name, _, args in _lib.SIGNATURES}
    own = _own_ptr(w)
    calls = []
    real = Context.call

    def call(self, fn, *args):
        rec = []
        for a, t in zip(args, argtypes[fn]):
            if t is C.c_void_p:
                rec.append("null" if a is None else "host" if not isinstance(a, int)
                           else "own" if a == own else "other")
            elif isinstance(a, (int, float)):
                rec.append(a)
            else:
                o = getattr(a, "_obj", a)
                rec.append((type(o).__name__, getattr(o, "layout", None)))
        calls.append({"fn": fn, "raw": args, "rec": rec})
        return real(self, fn, *args)

    with monkeypatch.context() as m:
        m.setattr(Context, "call", call)
        out = run()
    torch.cuda.synchronize()
    return out, calls


def _layout_of(c):
    fn, raw = c["fn"], c["raw"]
    if fn.startswith(("gm_weiszfeld", "gm_cclip")):
        return raw[6]._obj.layout
    if fn in ("gm_mean_f32", "gm_median_f32", "gm_trimmed_mean_f32", "gm_krum_f32",
              "gm_honest_variance_f32", "gm_oma_philox_f32"):
        return ROWS
    if fn.endswith("_panels_f32"):
        return PANELS
    return raw[4]


def _ld_of(c):
    return c["raw"][4 if c["fn"] == "gm_honest_variance_panels_f32" else 3]


def _main(calls):
    return [c for c in calls if not c["fn"].startswith("gm_rows_to_panels")]


def _check_operand(entry, tname, d, form, w, calls):
    """The rule of the module docstring for the first library call that reads the clients."""
    from byzantine_aircomp_amd.panels import panel_width
    main = _main(calls)
    assert main, calls
    c = main[0]
    got = (c["rec"][0], _ld_of(c), _layout_of(c))
    packs = [x["fn"] for x in calls if x["fn"].startswith("gm_rows_to_panels")]
    bf16 = tname == "bf16"
    if len({"gm_weiszfeld", "gm_cclip", "gm_bucket_means", "gm_fltrust", "gm_clip_rows",
            "gm_attack_affine"} & {c["fn"].rsplit("_", 1)[0]}):
        assert c["fn"].endswith("_bf16") == bf16, c["fn"]
    if form == "panels":
        assert got == ("own", w.panel_stride, PANELS), (got, c["fn"])
        assert not packs, packs
        return
    direct = form in ("cuda", "strided", "offset")
    if bf16 and entry in STREAM:
        aligned = d % 8 == 0 and form in ("cuda", "strided", "cpu")
        if not aligned:
            stride = K * panel_width(K, torch.bfloat16)
            assert got == ("other", stride, PANELS), (got, c["fn"])
            assert packs == ["gm_rows_to_panels_bf16"], packs
            return
        direct = form != "cpu"
    assert not packs, packs
    if direct:
        assert got == ("own", w.stride(0), ROWS), (got, c["fn"])
    else:
        assert got == ("other", d, ROWS), (got, c["fn"])


def _check_output(c, w, out, inplace):
    """The rows a pre-step writes: in place the operand itself; else a fresh fp32 matrix, rows
    for a tensor and panels for ClientPanels."""
    at = OUT_AT.get(c["fn"].rsplit("_", 1)[0])
    if at is None:
        return
    raw = c["raw"]
    y, ldy, lout = raw[at], raw[at + 1], raw[at + 2]
    if inplace:
        assert (y, ldy, lout) == (raw[0], raw[3], raw[4]), c["rec"]
        return
    assert c["rec"][at] == "other"
    if isinstance(out, _bz().ClientPanels):
        assert (y, ldy, lout) == (out.data.data_ptr(), out.panel_stride, PANELS), c["rec"]
    else:
        assert (ldy, lout) == (max(out.shape[1], 1), ROWS), c["rec"]
        if out.device.type == "cuda":
            assert y == out.data_ptr()


_REF = {}


def _reference(entry, tname, d):
    """(result, operand afterwards) of the contiguous CUDA call, as CPU rows; computed once."""
    key = (entry, tname, d)
    if key not in _REF:
        w, _ = _form(_values(d, DTYPES[tname]), "cuda")
        out = ENTRIES[entry][0](_bz(), w)
        torch.cuda.synchronize()
        _REF[key] = (_rows(out), _rows(w))
    return _REF[key]


@pytest.mark.parametrize("entry,tname,d,form", CASES,
                         ids=[f"{e}-{t}-d{d}-{f}" for e, t, d, f in CASES])
def test_operand_form(entry, tname, d, form, monkeypatch):
    bz = _bz()
    fn, _, kind, identical = ENTRIES[entry]
    X = _values(d, DTYPES[tname])
    w, backing = _form(X, form)
    if entry == "honest_variance" and form == "cpu":
        with pytest.raises(TypeError):            # it reads device-resident rows only
            fn(bz, w)
        return
    before = backing.clone()
    out, calls = _trace(monkeypatch, w, lambda: fn(bz, w))

    _check_operand(entry, tname, d, form, w, calls)
    main = _main(calls)
    if kind == "wrapper":
        first, last = main
        # the aggregator reads the pre-step's fp32 rows, handed over as panels
        at = OUT_AT[first["fn"].rsplit("_", 1)[0]]
        assert first["rec"][at] == "other" and first["raw"][at + 2] == PANELS, first["rec"]
        assert last["fn"] == "gm_weiszfeld_f32"
        assert (last["raw"][0], _ld_of(last), _layout_of(last)) == (
            first["raw"][at], first["raw"][at + 1], PANELS), last["rec"]
    else:
        _check_output(main[0], w, out, kind == "inplace")

    want_out, want_w = _reference(entry, tname, d)
    if kind == "inplace":
        assert out is w
        assert _same_bits(_rows(w), want_w), "the in-place result differs from the contiguous run"
    else:
        assert _same_bits(backing, before), "the input was written"
    assert kind == "inplace" or (out.device == w.device and out.dtype == torch.float32)
    assert tuple(out.shape) == tuple(want_out.shape)
    if identical:
        assert _same_bits(_rows(out), want_out), "differs from the contiguous CUDA call"


def test_clipped_without_a_panel_width(monkeypatch):
    """K = 2049 has no panel width: ``clipped(gm2)`` hands the clipped rows over row-major."""
    bz = _bz()
    from byzantine_aircomp_amd import _lib
    Kb, d = 2049, 8
    assert _lib.load().gm_panel_width(Kb) <= 0
    w = (0.1 * torch.randn(Kb, d, generator=torch.Generator().manual_seed(3))).cuda()
    before = w.clone()
    out, calls = _trace(monkeypatch, w, lambda: bz.clipped(bz.gm2, f=400)(w, _gm2_opts()))
    first, last = calls
    assert first["fn"] == "gm_clip_rows_f32" and last["fn"] == "gm_weiszfeld_f32"
    assert (first["rec"][0], _ld_of(first), _layout_of(first)) == ("own", d, ROWS)
    assert first["raw"][10:12] == (d, ROWS) and first["rec"][9] == "other"
    assert (last["raw"][0], _ld_of(last), _layout_of(last)) == (first["raw"][9], d, ROWS)
    assert _same_bits(w, before) and out.device == w.device and tuple(out.shape) == (d,)
