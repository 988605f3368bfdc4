"""The rules of tests/test_gpu_operand_forms.py for mean / median / trimmed_mean on bf16 input
(``options={"bf16": True}``), over all six forms: a unit-stride CUDA tensor is read in place (the
caller's pointer, ``ldx == stride(0)``, GM_LAYOUT_ROWS) whatever its alignment and d, other
tensors go through a copy with ``ldx == d``, bf16 ClientPanels are passed as ``data`` /
``panel_stride`` / GM_LAYOUT_PANELS, nothing is ever packed into panels, the input keeps its
bits, and the fp32 result lives on the caller's device with the bits of the contiguous CUDA
call."""
import pytest
import torch

import test_gpu_operand_forms as of

pytestmark = pytest.mark.gpu

ENTRIES = ("mean", "median", "trimmed_mean")
BF16 = {"bf16": True}
_REF = {}


def _run(bz, entry, w):
    return getattr(bz, entry)(w, dict(BF16))


def _reference(entry, d):
    """The contiguous CUDA call's result as CPU rows, computed once."""
    if (entry, d) not in _REF:
        w, _ = of._form(of._values(d, torch.bfloat16), "cuda")
        out = _run(of._bz(), entry, w)
        torch.cuda.synchronize()
        _REF[(entry, d)] = of._rows(out)
    return _REF[(entry, d)]


CASES = [(e, d, f) for e in ENTRIES for d in of.DS for f in of.FORMS]


@pytest.mark.parametrize("entry,d,form", CASES, ids=[f"{e}-bf16-d{d}-{f}" for e, d, f in CASES])
def test_operand_form_bf16(entry, d, form, monkeypatch):
    bz = of._bz()
    X = of._values(d, torch.bfloat16)
    w, backing = of._form(X, form)
    assert (w.data if form == "panels" else w).dtype == torch.bfloat16
    before = backing.clone()
    out, calls = of._trace(monkeypatch, w, lambda: _run(bz, entry, w))

    of._check_operand(entry, "bf16", d, form, w, calls)
    assert [c["fn"] for c in calls] == [f"gm_{entry}_bf16"], calls      # one call, no packing
    c = calls[0]
    if form in ("cuda", "strided", "offset"):
        assert (c["raw"][0], c["raw"][3], c["raw"][4]) == (w.data_ptr(), w.stride(0), of.ROWS)
    if form == "offset":
        assert c["raw"][0] % 16 != 0
    assert c["rec"][-2] == "other"                                      # a fresh output

    want_out = _reference(entry, d)
    assert of._same_bits(backing, before), "the input was written"
    assert out.device == w.device and out.dtype == torch.float32
    assert tuple(out.shape) == (d,) == tuple(want_out.shape)
    assert of._same_bits(of._rows(out), want_out), "differs from the contiguous CUDA call"
