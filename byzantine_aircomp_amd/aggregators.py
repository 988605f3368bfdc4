"""Drop-in aggregators backed by libgmagg.so (HIP kernels for gfx950).

The reference resolves its aggregator with ``eval(args.agg)``
(MNIST_Air_weight.py:580) and calls it once per step as
``weight_vector = aggregate(weight_f, options)`` (M:353).  This module provides
functions with the same names, signatures, option keys, defaults and return
semantics, so the reference's training loop can import them in place of its
own:

  ``gm2(wList, options)``  ideal Weiszfeld geometric median      (M:162-184)
  ``gm(wList, options)``   AirComp Weiszfeld, OMA2 every step    (M:131-160, M:396-414)
  ``OMA(message, noise_var)``  in-place per-client pre-noise     (M:385-394)

Semantics kept from the reference:
  * option keys ``maxiter`` (default 200), ``tol`` (1e-5), ``guess`` (default
    the row mean), plus ``noise_var`` (None) and ``P_max`` (1) for ``gm``;
    ``eta`` / ``honestSize`` are ignored, as in the reference;
  * ``maxiter == 0`` returns the ``guess`` object itself;
  * ``wList`` and ``guess`` are not modified (``OMA`` modifies ``message``);
  * the result lives on ``wList.device``: a CPU input is staged to the GPU and
    the aggregate copied back (the reference's hot path runs on CPU tensors);
  * the tol test is on the fp32 movement, returning the NEW iterate.

Extensions (ignored by the reference's loop): options ``noise_source``
(``"device"``: on-device Philox, the default; ``"host"``: the reference's own
``torch.normal`` draws on the CPU generator, in its order, for exact
comparison), ``seed`` (Philox key; drawn from the torch CPU generator when
absent) and ``algo`` (``"auto"``, ``"stream"``, ``"twopass"``, ``"gram"``,
``"gram_f32"``, ``"resident"``).  ``gm2`` / ``gm`` also accept a
``ClientPanels`` (panels.py: the same K x d values in the panel layout the
streaming pass reads as contiguous blocks) in place of the ``[K, d]`` tensor, and client
updates stored as bf16 (a ``torch.bfloat16`` ``[K, d]`` tensor or bf16 ``ClientPanels``):
the fused streaming pass reads them widened to fp32, which is exact, at half the bytes per
pass; guess, iterates and result are fp32.  The other aggregators are fp32 only.  The trace
of the last call (iterations, last movement) is in ``last_result``.

Beyond the reference: ``cclip(wList, options)``, centered clipping (Karimireddy, He & Jaggi,
ICML 2021) with the same contract and inputs as ``gm2`` on the same streaming pass; options
``tau`` (required), ``clip_iters`` (1), ``clip_tol`` (None), ``guess`` (zeros);
``cclip.with_options(tau=...)`` makes an ``aggregate`` for loops that build the dict.
``bucketing(wList, s)`` is s-bucketing (Karimireddy, He & Jaggi, ICLR 2022): the means of
random groups of s clients, one HIP pass over fp32 or bf16 rows or panels, fp32 out in either
layout; ``bucketed(aggregate, s)`` wraps any aggregator above with it (and rescales
``honestSize``).
``multi_krum(wList, options)`` (Blanchard et al. 2017: the mean of the ``m`` best Krum-scored
rows), ``bulyan(wList, options)`` (El Mhamdi, Guerraoui & Rouault 2018: recursive Krum
selection, then a mean around the median) and ``meamed(wList, options)`` (Xie, Koyejo & Gupta
2018: per coordinate the mean of the ``honestSize`` values nearest to the median) take fp32
rows or panels and ``honestSize`` like ``Krum``; they work under ``bucketed`` and as a
training loop's ``aggregate``.
``nnm(wList, f)`` is nearest-neighbor mixing (Allouah et al., AISTATS 2023): every row replaced
by the mean of its K - f nearest rows, fp32 rows or panels in and out; ``mixed(aggregate)``
wraps any aggregator above with it.
``dnc(wList, options)`` is Divide-and-Conquer (Shejwalkar & Houmansadr, NDSS 2021): spectral
filtering on ``dnc_dims`` sampled columns, in fp64: the rows whose centred projections on the
sample's top singular vector are largest are dropped (``int(dnc_c * f)`` per round, ``dnc_iters``
rounds) and the rest averaged; fp32 rows or panels and ``honestSize`` like ``Krum``;
``dnc.with_options(...)`` fixes its options; it works under ``bucketed`` and ``mixed`` and as a
training loop's ``aggregate``.
``caf(wList, options)`` is the covariance filter (Diakonikolas et al., ICML 2017; ByzFL's CAF):
the rows that stand out along the top eigen-direction of the weighted covariance of all d
coordinates are weighted down round by round, in fp64 on the K x K squared distances, and the
weighted mean of the round with the smallest eigenvalue is returned; fp32 rows or panels and
``honestSize`` like ``Krum``; ``caf.with_options(...)`` fixes its options.
``fltrust(wList, options)`` is FLTrust (Cao, Fang, Liu & Gong, NDSS 2021): every row is scored by
the cosine of its update with the server's own (``server_update``, or row ``server_row``), and
the rows of positive score, rescaled to the server update's norm, are averaged with their scores
as weights, in fp64; fp32 or bf16 rows or panels; ``fltrust.with_options(...)`` fixes the server.
``clip(wList, tau)`` and ``arc(wList, f)`` are norm clipping about a centre, static (Sun et al.
2019) and adaptive (ARC, Allouah et al., ICLR 2025): the updates longer than the radius scaled
back to it, in fp64; fp32 or bf16 rows or panels in, fp32 out, or fp32 in place;
``clipped(aggregate)`` wraps any aggregator above with it, the centre being ``options['guess']``.

There is no CPU path: without a GPU or without libgmagg.so these raise.
"""
from __future__ import annotations

import atexit
import ctypes as C
import functools
import math
import operator
import os
from dataclasses import dataclass

import torch

from . import _lib
from .panels import ClientPanels

__all__ = ["gm2", "gm", "cclip", "OMA", "mean", "median", "trimmed_mean", "Krum", "GMResult",
           "last_result", "Context", "context", "honest_variance", "bucketing", "bucketed",
           "multi_krum", "bulyan", "meamed", "nnm", "mixed", "dnc", "caf", "fltrust", "clip", "arc",
           "clipped"]


@dataclass
class GMResult:
    iters: int
    last_movement: float
    converged: bool
    algo: str
    guard: str = "none"      # Gram guard: "none", "accepted", "accepted_floor", "rejected"
    gram_kind: str = ""      # Gram runs: "f16_split", "bf16_split" (f16 range fallback), "f32"
    exchange: str = "none"   # resident runs: "agent" (flat, over XCDs), "xcd_local" (one XCD's
    #                          L2), "xcd_hier" (per-XCD gather, then the 8 XCD sums) or
    #                          "xcd_split" (one hop, own-XCD blocks from L2-kept copies)
    # fp32 gm2 on the streaming loop (gm_delta_last_info): STEP passes run as corrections on the
    # bf16 shadow, bit t of the mask set when STEP t was one, and "off", "armed" or "no_shadow"
    corrections: int = 0
    correction_mask: int = 0
    shadow: str = "off"


last_result: GMResult | None = None
_ALGOS = {"auto": _lib.GM_ALGO_AUTO, "stream": _lib.GM_ALGO_STREAM,
          "twopass": _lib.GM_ALGO_TWOPASS, "gram": _lib.GM_ALGO_GRAM,
          "resident": _lib.GM_ALGO_RESIDENT, "gram_f32": _lib.GM_ALGO_GRAM_F32}
_ALGO_NAMES = {v: k for k, v in _ALGOS.items()}
_GUARD_NAMES = {_lib.GM_GUARD_NONE: "none", _lib.GM_GUARD_ACCEPTED: "accepted",
                _lib.GM_GUARD_REJECTED: "rejected", _lib.GM_GUARD_ACCEPTED_FLOOR: "accepted_floor"}


def _result(res, ctx=None) -> "GMResult":
    """ctx: the context of an fp32 gm_weiszfeld_f32 call, asked what its streaming loop did
    with the bf16 shadow."""
    r = GMResult(res.iters, res.last_movement, bool(res.converged),
                 _ALGO_NAMES.get(res.algo_used, "?"), _GUARD_NAMES.get(res.guard, "?"),
                 {1: "f16_split", 2: "bf16_split", 3: "f32"}.get(res.gram_kind, ""),
                 {1: "agent", 2: "xcd_local", 3: "xcd_hier",
                  4: "xcd_split"}.get(res.exchange, "none"))
    if ctx is not None and res.algo_used == _lib.GM_ALGO_STREAM:
        info = (C.c_int64 * 3)()
        _lib.check(ctx.lib.gm_delta_last_info(ctx.handle, info), "gm_delta_last_info")
        r.corrections, r.correction_mask = int(info[0]), int(info[1])
        r.shadow = {1: "armed", 2: "no_shadow"}.get(int(info[2]), "off")
    return r


class Context:
    """One libgmagg context (device workspace, optional d-shard / RCCL comm)."""

    def __init__(self, device: int):
        self.lib = _lib.load()
        self.device = device
        h = C.c_void_p()
        _lib.check(self.lib.gm_ctx_create(device, C.byref(h)), "gm_ctx_create")
        self.handle = h
        self._keep = []   # ctypes callbacks that must outlive the context

    def set_shard(self, d_total: int, d_offset: int):
        _lib.check(self.lib.gm_ctx_set_shard(self.handle, d_total, d_offset), "gm_ctx_set_shard")

    def set_allreduce(self, fn):
        """fn(dev_ptr:int, count:int, stream:int) -> None; sums doubles in place."""
        def tramp(user, buf, count, stream):
            try:
                fn(buf, count, stream)
                return 0
            except Exception:  # noqa: BLE001 - reported through the status code
                return 1
        cb = _lib.ALLREDUCE_CB(tramp)
        self._keep.append(cb)
        _lib.check(self.lib.gm_ctx_set_allreduce(self.handle, cb, None), "gm_ctx_set_allreduce")

    def init_rccl(self, unique_id: bytes, nranks: int, rank: int):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _lib.check(self.lib.gm_ctx_init_rccl(self.handle, buf, nranks, rank), "gm_ctx_init_rccl")

    def pass_timing(self, enable: bool):
        """Return (total_ms, launches) of the fused pass since the last call."""
        ms, n = C.c_double(), C.c_int64()
        _lib.check(self.lib.gm_ctx_pass_timing(self.handle, int(enable), C.byref(ms),
                                               C.byref(n)), "gm_ctx_pass_timing")
        return ms.value, n.value

    def call(self, fn: str, *args):
        """The library's ``fn(handle, *args)`` with this context's device current; GmError on a
        negative status."""
        with torch.cuda.device(self.device):
            return _lib.check(getattr(self.lib, fn)(self.handle, *args), fn)

    def close(self):
        """Destroy the context now (workspace, RCCL communicator); idempotent.
        Multi-process callers close before torch.distributed.destroy_process_group()
        rather than leaving the communicator to interpreter teardown."""
        h, self.handle = getattr(self, "handle", None), None
        if h:
            self.lib.gm_ctx_destroy(h)
        for k, v in list(_contexts.items()):
            if v is self:
                del _contexts[k]

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.gm_ctx_destroy(self.handle)
        except Exception:  # noqa: BLE001 - interpreter teardown
            pass


_contexts: dict[int, Context] = {}


def close_all():
    """Destroy every per-device context now (workspace, pinned host buffer, events).
    Registered with atexit, so it runs in Py_Finalize — before the C-level exit
    handlers that tear the HIP runtime down — instead of from Context.__del__ during
    interpreter teardown, when the runtime (or a profiler intercepting it) may already
    be finalised."""
    for ctx in list(_contexts.values()):
        ctx.close()


if os.environ.get("GMAGG_ATEXIT_CLOSE", "1") != "0":    # (=0: the round-2 behaviour, A/B)
    atexit.register(close_all)


def context(device: torch.device | int | None = None) -> Context:
    if not torch.cuda.is_available():
        raise RuntimeError("byzantine_aircomp_amd needs a ROCm GPU (torch.cuda.is_available() "
                           "is False); there is no CPU fallback")
    if device is None:
        idx = torch.cuda.current_device()
    elif isinstance(device, int):
        idx = device
    else:
        idx = device.index if device.index is not None else torch.cuda.current_device()
    ctx = _contexts.get(idx)
    if ctx is None:
        ctx = _contexts[idx] = Context(idx)
    return ctx


def _stream_ptr(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _stage(t: torch.Tensor, bf16_ok: bool = False) -> torch.Tensor:
    """The GPU tensor the kernels read (a copy if `t` lives on the CPU)."""
    if t.dtype != torch.float32 and not (bf16_ok and t.dtype == torch.bfloat16):
        raise TypeError(f"aggregation kernels are fp32 (got {t.dtype})")
    if t.device.type == "cuda":
        return t
    return t.to(torch.device("cuda", torch.cuda.current_device()))


def _unit_rows(X: torch.Tensor):
    """(X or a contiguous copy, ldx): unit column stride, rows of the last two dimensions at
    least d apart."""
    d, ld = X.shape[-1], X.stride(-2)
    if X.stride(-1) != 1 or ld < d or X.shape[-2] == 0:
        X = X.contiguous()
        ld = X.stride(-2)
    return X, max(ld, d)


def _shape(wList, who: str, *, bf16: bool = False, max_k: int | None = None):
    """(K, d) of the client matrix, after the checks that touch no device: a [K, d] tensor or
    ClientPanels (ValueError), fp32 or, with `bf16`, bf16 (TypeError), 1 <= K <= max_k
    (ValueError).  The entry points that promise to refuse before a GPU is touched call it
    first."""
    if isinstance(wList, ClientPanels):
        K, d, dtype = wList.K, wList.d, wList.data.dtype
    elif isinstance(wList, torch.Tensor) and wList.dim() == 2:
        (K, d), dtype = wList.shape, wList.dtype
    else:
        got = tuple(wList.shape) if isinstance(wList, torch.Tensor) else type(wList).__name__
        raise ValueError(f"{who}: the client matrix must be a [K, d] tensor or ClientPanels "
                         f"(got {got})")
    if dtype != torch.float32 and not (bf16 and dtype == torch.bfloat16):
        raise TypeError(f"{who} reads fp32 or bf16 client updates (got {dtype})" if bf16 else
                        f"{who} is fp32 only (got {dtype})")
    if K < 1:
        raise ValueError(f"{who}: the client matrix has no rows")
    if max_k is not None and K > max_k:
        raise ValueError(f"{who}: K <= {max_k} (got {K})")
    return K, d


def _operand(wList, *, bf16: bool = False):
    """(tensor, ld, layout, K, d) of the client matrix as the library reads it, the one place
    that pairs a layout with a tensor: ClientPanels as they are; a [K, d] tensor as rows, a CPU
    tensor staged to the GPU and a non-unit or overlapping stride through a contiguous copy.
    The tensor returned keeps such a copy alive, and ``is not wList`` tells that one was made
    (an in-place caller copies back).  fp32 only unless `bf16`."""
    if isinstance(wList, ClientPanels):
        X = wList.data
        if not bf16 and X.dtype != torch.float32:        # (_stage's refusal, for panels)
            raise TypeError(f"aggregation kernels are fp32 (got {X.dtype})")
        return X, wList.panel_stride, _lib.GM_LAYOUT_PANELS, wList.K, wList.d
    X = _stage(wList, bf16)
    if X.dim() != 2:
        raise ValueError(f"wList must be [K, d] (got {tuple(X.shape)})")
    X, ld = _unit_rows(X)
    return (X, ld, _lib.GM_LAYOUT_ROWS, *X.shape)


def _stream_operand(wList):
    """_operand for the streaming pass (gm2, gm, cclip), whose bf16 kernel reads rows only where
    it can load them 16 bytes at a time (unit column stride, 16-byte aligned, d and the row
    stride multiples of 8): other bf16 rows are packed into bf16 panels first.  wList is never
    written."""
    if isinstance(wList, ClientPanels) or wList.dtype != torch.bfloat16:
        return _operand(wList, bf16=True)
    X = _stage(wList, True)
    if X.dim() != 2:
        raise ValueError(f"wList must be [K, d] (got {tuple(X.shape)})")
    K, d = X.shape
    ld = X.stride(0)
    if (K > 0 and X.stride(1) == 1 and ld >= d and ld % 8 == 0 and d % 8 == 0
            and X.data_ptr() % 16 == 0):
        return X, ld, _lib.GM_LAYOUT_ROWS, K, d
    return _operand(ClientPanels.from_rows(X), bf16=True)


def _twin(fn: str, layout: int) -> str:
    """The ``*_panels_f32`` twin of the rows function `fn` (mean, median, trimmed_mean, Krum,
    honest_variance, OMA: same results) where the operand is panels."""
    return fn.replace("_f32", "_panels_f32") if layout == _lib.GM_LAYOUT_PANELS else fn


@functools.lru_cache(maxsize=None)
def _has_panels(K: int) -> bool:
    """Whether K rows have a panel width (a fixed table of the library's: asked once per K)."""
    return int(_lib.load().gm_panel_width(int(K))) > 0


def _panels_out(layout, wList, K, who: str) -> bool:
    """Whether a pre-step's rows go out as panels: `layout` is None (wList's own), "rows" or
    "panels" (ValueError otherwise), and panels need a panel width for K rows (ValueError; K
    None: not asked, as where a wrapper only validates its argument)."""
    if layout not in (None, "rows", "panels"):
        raise ValueError(f"{who}: layout must be None, 'rows' or 'panels' (got {layout!r})")
    panels = layout == "panels" or (layout is None and isinstance(wList, ClientPanels))
    if panels and K is not None and not _has_panels(K):
        raise ValueError(f"{who}: no panel layout for K = {K} rows (take them row-major)")
    return panels


def _new_rows(K: int, d: int, device, panels: bool):
    """(out, Y, ldy, layout) of a fresh fp32 K x d output: `out` is what the caller gets, a
    [K, d] tensor or ClientPanels(K, d), Y the tensor the library writes."""
    if panels:
        out = ClientPanels(K, d, device=device, zero=False)      # every column < d is written
        return out, out.data, out.panel_stride, _lib.GM_LAYOUT_PANELS
    out = torch.empty(K, d, dtype=torch.float32, device=device)
    return out, out, max(d, 1), _lib.GM_LAYOUT_ROWS


def _to_caller(out, wList):
    """`out` on wList's device (a CPU wList was staged: its result goes back).  ClientPanels, a
    pre-step's rows in the panel layout, stay on the GPU."""
    if out.device == wList.device or isinstance(out, ClientPanels):
        return out
    return out.to(wList.device)


def _index(x, who: str, what: str, lo: int, hi: int | None = None, kind=ValueError) -> int:
    """x as an int in [lo, hi] (hi None: unbounded).  A bool, a float or a string is refused
    with `kind`, a value out of range with ValueError."""
    try:
        if isinstance(x, bool):
            raise TypeError
        n = operator.index(x)
    except TypeError:
        n = None
    if n is None or n < lo or (hi is not None and n > hi):
        rng = f">= {lo}" if hi is None else f"in [{lo}, {hi}]"
        if n is None:
            raise kind(f"{who}: {what} must be an integer {rng} (got {x!r})")
        raise ValueError(f"{who}: {what} = {n} not {rng}")
    return n


def _vector(v, d: int, device, what: str):
    """v (a guess, a centre, the server's update) as contiguous fp32 of d elements on `device`;
    None stays None."""
    if v is None:
        return None
    if v.numel() != d:
        raise ValueError(f"{what} has {v.numel()} elements, the rows have {d}")
    return v.detach().to(device=device, dtype=torch.float32).contiguous()


def _with_options(name: str, keys, make, doc: str):
    """The ``with_options(**fixed)`` of the public callable `name`: keys outside `keys` are a
    TypeError, ``make(fixed)`` (which refuses bad values) is the callable, returned under
    `name` so that loops and logs that go by ``__name__`` see the rule's own."""
    def with_options(**fixed):
        unknown = sorted(set(fixed) - set(keys))
        if unknown:
            raise TypeError(f"{name}.with_options takes {', '.join(keys)} (got {unknown})")
        fn = make(fixed)
        fn.__name__ = fn.__qualname__ = name
        # (a fixed tensor, fltrust's server_update, by its shape: its repr would read the device)
        fn.__doc__ = f"{name} with " + ", ".join(
            f"{k}={f'tensor{tuple(v.shape)}' if isinstance(v, torch.Tensor) else repr(v)}"
            for k, v in fixed.items())
        return fn
    with_options.__doc__ = doc
    return with_options


def _fixed_options(name: str, check):
    """make(fixed) for an ``aggregate(wList, options)``: `check(fixed)` now, then the fixed
    options over the caller's at every call.  The aggregator is looked up by name when called."""
    def make(fixed):
        check(fixed)
        return lambda wList, options={}: globals()[name](wList, {**(options or {}), **fixed})
    return make


def _pre_step(aggregate, suffix: str, doc: str, step):
    """An ``aggregate(wList, options)`` that runs ``step(wList, options, its own name)`` -> (rows,
    options), calls `aggregate` on them and returns the result on wList's device (a CPU wList's
    rows stayed on the GPU as panels).  Named ``f"{aggregate.__name__}_{suffix}"``."""
    def agg(wList, options={}):  # noqa: B006 - the aggregator contract (M:353)
        rows, opts = step(wList, options, agg.__name__)
        out = aggregate(rows, opts)
        # (whatever `aggregate` returns is handed on; only a tensor has a device to match)
        return _to_caller(out, wList) if isinstance(out, torch.Tensor) else out
    agg.__name__ = agg.__qualname__ = f"{aggregate.__name__}_{suffix}"
    agg.__doc__ = doc
    return agg


def _handover(layout, K: int):
    """A wrapper's `layout` for K rows: "panels" falls back to "rows" where K has no panel
    width."""
    return "rows" if layout == "panels" and K >= 1 and not _has_panels(K) else layout


def _noise_source(options) -> int:
    src = options.get("noise_source", os.environ.get("BYZ_AIRCOMP_NOISE", "device"))
    if src == "device":
        return _lib.GM_NOISE_PHILOX
    if src == "host":
        return _lib.GM_NOISE_HOST
    raise ValueError(f"noise_source must be 'device' or 'host' (got {src!r})")


def _seed(options) -> int:
    if options.get("seed") is not None:
        return int(options["seed"]) & (2 ** 64 - 1)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _host_draws(K: int, d: int, noise_var):
    """The reference's OMA2 draws, in order, on the global CPU generator (M:401-411)."""
    def cb(user, it, hr, hi, n):
        try:
            a = torch.normal(torch.zeros(K), 1 / math.sqrt(2))
            b = torch.normal(torch.zeros(K), 1 / math.sqrt(2))
            C.memmove(hr, a.data_ptr(), 4 * K)
            C.memmove(hi, b.data_ptr(), 4 * K)
            if noise_var is not None:
                z = torch.normal(torch.zeros(d + 1), math.sqrt(noise_var / 2))
                C.memmove(n, z.data_ptr(), 4 * (d + 1))
            return 0
        except Exception:  # noqa: BLE001
            return 1
    return _lib.NOISE_CB(cb)


def _gm_opts(opts: dict, aircomp: bool, layout: int, pre_var=None, pre_seed=None, shape=None):
    """The library's options from the merged option dict `opts` (maxiter, tol and, for gm,
    noise_var and P_max are present).  pre_var: the variance of a fused pre-noise, keyed
    pre_seed.  shape: (K, d_total), for the host draws' callback.  A Philox key that is needed
    and not given is drawn from the torch CPU generator, one randint each; with
    ``noise_source="host"`` nothing is drawn here (the callback replays the reference's
    torch.normal sequence, which an extra draw would shift)."""
    o = _lib.GmOpts()
    o.maxiter = int(opts["maxiter"])
    o.tol = float(opts["tol"])
    o.eps = 1e-4
    o.mode = _lib.GM_MODE_AIRCOMP if aircomp else _lib.GM_MODE_IDEAL
    o.algo = _ALGOS[opts.get("algo", "auto")]
    o.check_every = int(opts.get("check_every", 0))
    o.layout = layout
    if pre_var is not None:
        o.pre_oma = 1
        o.pre_oma_var = float(pre_var)
        o.pre_oma_seed = _seed({"seed": pre_seed})
    if aircomp:
        var = opts["noise_var"]
        o.has_noise = int(var is not None)
        o.noise_var = float(var) if var is not None else 0.0
        o.P_max = float(opts["P_max"])
        o.noise_source = _noise_source(opts)
        if o.noise_source == _lib.GM_NOISE_HOST:
            o.noise_cb = o.keep_cb = _host_draws(*shape, var)   # (alive as long as o)
        else:
            o.seed = _seed(opts)
    return o


def _weiszfeld(wList: torch.Tensor, options: dict, aircomp: bool):
    global last_result
    opts = {"maxiter": 200, "tol": 1e-5}
    if aircomp:
        opts.update({"noise_var": None, "P_max": 1})
    opts.update(options or {})
    # pre_oma_var: the reference's OMA(weight_f, var) before a non-gm aggregator
    # (M:351-352), in place on wList, fused into the first streaming pass (pre_oma_seed
    # keys the Philox draws as OMA(..., seed=)).  With the default guess (the column mean
    # of the NOISY rows) it runs as the separate OMA first.
    pre_var = None if aircomp else opts.get("pre_oma_var")
    # (the Philox key is drawn only where Philox draws are made: with host draws OMA
    # replays the reference's torch.normal sequence, which an extra randint would shift)
    pre_seed = opts.get("pre_oma_seed")
    if pre_var is not None and (opts.get("guess") is None or wList.device.type != "cuda"
                                or _noise_source(opts) == _lib.GM_NOISE_HOST):
        # (the reference's own draws are host-side: OMA replays them itself)
        OMA(wList, float(pre_var), noise_source=opts.get("noise_source"), seed=pre_seed)
        pre_var = None
    guess = opts.get("guess")
    bf16 = wList.dtype == torch.bfloat16
    if guess is None:
        # (bf16 rows: the fp32 mean of the widened values, no widened copy of the matrix)
        guess = wList.mean(dim=0, dtype=torch.float32) if bf16 and not isinstance(
            wList, ClientPanels) else wList.mean(dim=0)
    maxiter = int(opts["maxiter"])
    if maxiter <= 0:                        # M:145 / M:173 loop body never runs
        if pre_var is not None:
            OMA(wList, float(pre_var), seed=pre_seed)
        last_result = GMResult(0, float("nan"), False, "none")
        return guess
    X, ldx, layout, K, d = _stream_operand(wList)
    g0 = _vector(guess, d, X.device, "guess")
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    if d == 0:
        last_result = GMResult(1, 0.0, True, "none")
        return _to_caller(out, wList)

    o = _gm_opts(opts, aircomp, layout, pre_var, pre_seed, (K, d))
    res = _lib.GmResult()
    ctx = context(X.device)
    ctx.call("gm_weiszfeld_bf16" if bf16 else "gm_weiszfeld_f32", X.data_ptr(), K, d, ldx,
             g0.data_ptr(), out.data_ptr(), C.byref(o), C.byref(res), _stream_ptr(X.device))
    last_result = _result(res, None if bf16 else ctx)
    if pre_var is not None and not isinstance(wList, ClientPanels) and X is not wList:
        # a strided view was packed into a copy: the fused pre-noise landed in the
        # copy, and OMA's contract is in place on wList (M:351-352, as OMA() copies back)
        wList.copy_(X)
    return _to_caller(out, wList)


def gm2(wList, options={}):  # noqa: B006 - the reference's signature (M:162)
    """Ideal Weiszfeld geometric median (MNIST_Air_weight.py:162-184).  fp32 or bf16 client
    updates; the result is fp32 either way."""
    return _weiszfeld(wList, options, aircomp=False)


def gm(wList, options={}):  # noqa: B006 - the reference's signature (M:131)
    """AirComp Weiszfeld geometric median (MNIST_Air_weight.py:131-160).  fp32 or bf16 client
    updates; the result is fp32 either way."""
    return _weiszfeld(wList, options, aircomp=True)


_CCLIP_KEYS = ("tau", "clip_iters", "clip_tol")


def _cclip_params(options):
    """(tau, clip_iters, tol for the library) from the options; ValueError on a missing or
    invalid value, before anything touches a GPU."""
    if options.get("tau") is None:
        raise ValueError("cclip needs options['tau'] (the clipping radius; there is no default)")
    tau = float(options["tau"])
    if not tau > 0:                                   # NaN fails too; +inf is the mean step
        raise ValueError(f"cclip: tau must be > 0 (got {options['tau']!r})")
    iters = int(options.get("clip_iters", 1))
    if iters < 0:
        raise ValueError(f"cclip: clip_iters must be >= 0 (got {iters})")
    ctol = options.get("clip_tol")
    if ctol is not None and not float(ctol) >= 0:
        raise ValueError(f"cclip: clip_tol must be None or >= 0 (got {ctol!r})")
    # None: exactly clip_iters iterations (a negative tol never passes the movement test)
    return tau, iters, -1.0 if ctol is None else float(ctol)


def _run_cclip(ctx, ptr: int, bf16: bool, K: int, d: int, ldx: int, layout: int, g0, params,
               check_every: int = 0):
    """gm_cclip_f32 / _bf16 on ctx from the fp32 guess g0 [d], params = _cclip_params(...):
    (the result [d] on g0's device, the trace, the clients outside the radius at the last
    iteration run)."""
    tau, iters, tol = params
    out = torch.empty(d, dtype=torch.float32, device=g0.device)
    o = _lib.GmCclipOpts()
    o.tau, o.maxiter, o.tol, o.layout, o.check_every = tau, iters, tol, layout, check_every
    res = _lib.GmCclipResult()
    ctx.call("gm_cclip_bf16" if bf16 else "gm_cclip_f32", ptr, K, d, ldx, g0.data_ptr(),
             out.data_ptr(), C.byref(o), C.byref(res), _stream_ptr(g0.device))
    return out, GMResult(res.iters, res.last_movement, bool(res.converged),
                         "stream" if iters else "none"), int(res.clipped)


def cclip(wList, options={}):  # noqa: B006 - the aggregator contract (M:353)
    """Centered clipping (Karimireddy, He & Jaggi, ICML 2021, Algorithm 2), not one of the
    reference's aggregators: from v = options['guess'] (default the zero vector, as in the
    authors' code; pass the previous aggregate or the current model for the paper's use),
    ``clip_iters`` (default 1) times

        v <- v + mean_k (x_k - v) * min(1, tau / ||x_k - v||)

    on the fused streaming pass: one read of wList per iteration plus one for the first
    distances.  ``options['tau']`` is required.  ``clip_tol`` (default None: run exactly
    clip_iters iterations) stops early once the fp32 movement ||v - v'|| <= clip_tol,
    returning v'.  Every other key (maxiter, tol, eta, honestSize, noise_var, ...) is ignored.
    wList: an fp32 or bf16 [K, d] tensor or ClientPanels, staged as for gm2 and never written;
    the result is fp32 on wList.device.  ``clip_iters == 0`` returns the guess object.
    ``last_result`` holds the trace, ``cclip.last_info['clipped']`` the number of clients
    outside the radius at the last iteration run."""
    global last_result
    options = options or {}
    params = _cclip_params(options)
    _, d = _shape(wList, "cclip", bf16=True)
    guess = options.get("guess")
    if guess is None:
        guess = torch.zeros(d, dtype=torch.float32, device=wList.device)
    if params[1] == 0:
        last_result = GMResult(0, float("nan"), False, "none")
        cclip.last_info = {"clipped": 0}
        return guess
    X, ldx, layout, K, d = _stream_operand(wList)
    g0 = _vector(guess, d, X.device, "guess")
    if d == 0:
        last_result = GMResult(1, 0.0, True, "none")
        cclip.last_info = {"clipped": 0}
        return torch.empty(d, dtype=torch.float32, device=wList.device)
    out, last_result, clipped = _run_cclip(
        context(X.device), X.data_ptr(), X.dtype == torch.bfloat16, K, d, ldx, layout, g0, params,
        int(options.get("check_every", 0)))
    cclip.last_info = {"clipped": clipped}
    return _to_caller(out, wList)


cclip.with_options = _with_options(
    "cclip", _CCLIP_KEYS,
    # (bad values fail when the options are fixed; tau may still come from the caller's)
    _fixed_options("cclip", lambda fixed: _cclip_params(fixed if "tau" in fixed
                                                        else dict(fixed, tau=1.0))),
    """An ``aggregate(wList, options)`` callable named "cclip" that applies tau / clip_iters /
    clip_tol over the caller's options, for loops that build the dict themselves
    (training.run(..., aggregate=cclip.with_options(tau=10.0)), the reference's
    eval(args.agg)).""")
cclip.last_info = {"clipped": 0}


def _coordinate(wList, options, fn_name, *extra):
    """mean / median / trimmed_mean: the fp32 function `fn_name` (its panel twin on fp32
    ClientPanels).  With ``options["bf16"]`` true, bf16 input goes to the ``_bf16`` counterpart,
    which takes the layout as an argument and reads unit-stride rows in place at any alignment;
    without it bf16 is refused as every other 16- or 64-bit dtype is (the call is fp32 unless
    the caller says otherwise).  The dtype is checked before anything is staged."""
    dtype = wList.data.dtype if isinstance(wList, ClientPanels) else wList.dtype
    bf16 = dtype == torch.bfloat16
    if bf16 and not (options and options.get("bf16")):
        raise TypeError("aggregation kernels are fp32 (got torch.bfloat16; options={'bf16': "
                        "True} reads bf16 client updates in place)")
    if dtype != torch.float32 and not bf16:
        raise TypeError(f"aggregation kernels read fp32 or bf16 client updates (got {dtype})")
    X, ldx, layout, K, d = _operand(wList, bf16=bf16)
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    if bf16:
        context(X.device).call(fn_name.replace("_f32", "_bf16"), X.data_ptr(), K, d, ldx, layout,
                               *extra, out.data_ptr(), _stream_ptr(X.device))
    else:
        context(X.device).call(_twin(fn_name, layout), X.data_ptr(), K, d, ldx, *extra,
                               out.data_ptr(), _stream_ptr(X.device))
    return _to_caller(out, wList)


_BF16_INPUT = """wList: an fp32 [K, d] tensor (any stride; a CPU tensor is staged to the GPU) or
    fp32 ClientPanels; never written.  With ``options={"bf16": True}`` also a bf16 [K, d] tensor in
    any form (a unit-stride CUDA tensor is read in place at any alignment) or bf16 ClientPanels:
    the values are widened (exact) and the result is the fp32 call's on ``wList.float()``.
    Without the option bf16 raises TypeError, as fp16 / fp64 always do, before a GPU is
    touched.  The result is fp32 [d] on wList's device."""


def mean(wList, options={}):  # noqa: B006 - reference signature (M:186)
    return _coordinate(wList, options, "gm_mean_f32")


mean.__doc__ = f"""Column mean (MNIST_Air_weight.py:186-187): an fp64 sum per column, rounded once.

    {_BF16_INPUT}"""


def median(wList, options={}):  # noqa: B006 - reference signature (M:194)
    return _coordinate(wList, options, "gm_median_f32")


median.__doc__ = f"""Coordinate-wise lower median, torch.median semantics (M:194-195), K <= 2048:
    the element of rank (K - 1) // 2, NaN for a column that holds one (on bf16: 16-bit order keys,
    half the counting steps).

    {_BF16_INPUT}"""


def trimmed_mean(wList, options={}):  # noqa: B006 - reference signature (M:189)
    return _coordinate(wList, options, "gm_trimmed_mean_f32", int(wList.shape[0] * 0.1))


trimmed_mean.__doc__ = f"""Coordinate-wise mean without the int(0.1 K) smallest and largest
    (M:189-192), K <= 2048: the kept values summed in fp64 and rounded once (on bf16 they are
    selected on 16-bit order keys).

    {_BF16_INPUT}"""


_DIST_MODES = {"exact": _lib.GM_DIST_EXACT, "mfma": _lib.GM_DIST_MFMA}
_DIST_REASONS = ("ok", "requested_exact", "not_eligible", "nonfinite_fallback")


def _dist_request(wList, bf16, distances, who: str):
    """(reads bf16, dist_mode) of a distance-family call, from checks that touch no device.
    `distances` must be "exact" or "mfma" (ValueError); the MFMA tier reads bf16, so "mfma" on
    fp32 input is a ValueError.  bf16 input without the opt-in is not decided here: the caller's
    fp32 path refuses it (TypeError) as before."""
    if distances not in _DIST_MODES:
        raise ValueError(f"{who}: distances must be 'exact' or 'mfma' (got {distances!r})")
    dtype = wList.data.dtype if isinstance(wList, ClientPanels) else getattr(wList, "dtype", None)
    is_bf16 = bool(bf16) and dtype == torch.bfloat16
    if dtype is not None and dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{who} reads fp32 or, when asked to, bf16 client updates (got {dtype})")
    if dtype == torch.bfloat16 and not bf16:
        raise TypeError(f"{who} is fp32 only (got torch.bfloat16) unless bf16 is asked for: "
                        "options={'bf16': True}, nnm / pair_distances: bf16=True")
    if distances == "mfma" and dtype == torch.float32:
        raise ValueError(f"{who}: distances='mfma' reads bf16 client updates (got torch.float32); "
                         "fp32 input has the exact distances only")
    return is_bf16, _DIST_MODES[distances]


def _dist_info(ctx) -> dict:
    """gm_dist_last_info of ctx (waits for the stream of its last bf16 distance call)."""
    info = (C.c_int64 * 4)()
    beta = C.c_double()
    _lib.check(ctx.lib.gm_dist_last_info(ctx.handle, info, C.byref(beta)), "gm_dist_last_info")
    return {"tier": ("exact", "mfma")[info[0]], "reason": _DIST_REASONS[info[1]],
            "slices": info[2], "flush": info[3], "beta": beta.value}


_FP32_DIST_INFO = {"tier": "exact", "reason": "requested_exact", "slices": None, "flush": 32,
                   "beta": None}


def Krum(wList, options):  # noqa: N802 - reference name (M:197)
    """The row with the smallest sum of squared distances to its honestSize-1
    nearest rows, itself included (M:197-204).  With ``options["bf16"]`` true a bf16 [K, d]
    tensor (unit-stride rows are read in place at any alignment) or bf16 ClientPanels is read as
    it is: ``options["distances"]`` "exact" (the default) returns the bits of the fp32 call on
    ``wList.float()``; "mfma" takes the distances from the bf16 matrix cores within
    ``Krum.last_info["beta"] * (rho_i + rho_j)`` (``multi_krum``).  Without the option bf16 is
    refused (TypeError) before a GPU is touched.  ``Krum.last_info["algo"]`` is "exact", "gram"
    or "mfma"."""
    bf16, mode = _dist_request(wList, options.get("bf16"), options.get("distances", "exact"),
                               "Krum")
    if bf16:
        X, ldx, layout, K, d = _operand(wList, bf16=True)
        out = torch.empty(d, dtype=torch.float32, device=X.device)
        idx = C.c_int64()
        ctx = context(X.device)
        ctx.call("gm_krum_bf16", X.data_ptr(), K, d, ldx, layout, int(options["honestSize"]),
                 mode, out.data_ptr(), C.byref(idx), _stream_ptr(X.device))
        info = _dist_info(ctx)
        Krum.last_index = idx.value
        Krum.last_info = {"algo": info["tier"], "candidates": 0, "reason": info["reason"],
                          "beta": info["beta"], "slices": info["slices"]}
        return _to_caller(out, wList)
    X, ldx, layout, K, d = _operand(wList)
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    idx = C.c_int64()
    ctx = context(X.device)
    ctx.call(_twin("gm_krum_f32", layout), X.data_ptr(), K, d, ldx, int(options["honestSize"]),
             out.data_ptr(), C.byref(idx), _stream_ptr(X.device))
    info = (C.c_int64 * 3)()
    _lib.check(ctx.lib.gm_krum_last_info(ctx.handle, info), "gm_krum_last_info")
    Krum.last_index = idx.value
    Krum.last_info = {"algo": ("exact", "gram")[info[0]], "candidates": info[1],
                      "reason": ("ok", "not_chosen", "not_eligible", "gram_nonfinite",
                                 "candidates")[info[2]]}
    return _to_caller(out, wList)


def _honest_size(options, who: str) -> int:
    if not options or options.get("honestSize") is None:
        raise ValueError(f"{who} needs options['honestSize']")
    return int(options["honestSize"])


def meamed(wList, options):
    """Mean-around-median (Xie, Koyejo & Gupta 2018), not one of the reference's aggregators:
    per coordinate, the mean of the ``honestSize`` values nearest to the coordinate's lower
    median (ties at the threshold to the lower row index; fp64 sum, rounded once; a NaN in
    the column gives NaN).  One HIP pass that reads wList once (robust.hip col_meamed).
    wList: an fp32 [K, d] tensor or fp32 ClientPanels, K <= 1024, 1 <= honestSize <= K; the
    result is fp32 on wList.device."""
    K, d = _shape(wList, "meamed", max_k=1024)
    keep = _honest_size(options, "meamed")
    if not 1 <= keep <= K:
        raise ValueError(f"meamed: honestSize {keep} not in [1, {K}]")
    X, ldx, layout, K, d = _operand(wList)
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    context(X.device).call("gm_meamed_f32", X.data_ptr(), K, d, ldx, layout, None, K, keep,
                           out.data_ptr(), _stream_ptr(X.device))
    return _to_caller(out, wList)


def multi_krum(wList, options):
    """Multi-Krum (Blanchard et al., NeurIPS 2017): the mean of the ``options['m']`` (default
    honestSize) rows of smallest Krum score, ties to the lower row index; each coordinate is
    the fp64 sum of the selected rows in increasing row index, divided by m, rounded once.
    The scores are Krum's on the exact distance path (GMAGG_KRUM is ignored); ``m == 1`` is
    that Krum row bit for bit.  wList: an fp32 [K, d] tensor or fp32 ClientPanels, K <= 4096,
    2 <= honestSize <= K + 1, 1 <= m <= K.  ``multi_krum.last_selected`` holds the selected
    rows, increasing.

    ``options["bf16"]`` true also reads a bf16 [K, d] tensor (unit-stride rows in place, at any
    alignment) or bf16 ClientPanels; without it bf16 raises TypeError before a GPU is touched.
    ``options["distances"]``: "exact" (the default) is the fp32 kernels on the widened elements,
    the bits of the fp32 call on ``wList.float()``; "mfma" (bf16 only, ValueError on fp32) forms
    D~ = max(0, G_ii + G_jj - 2 G_ij) from G = X X^T on the bf16 matrix cores, with
    |D~_ij - D_ij| <= beta (||x_i||^2 + ||x_j||^2): the selection can differ from the exact
    tier's only between rows whose scores lie within that bound; the output is the same fp64
    mean of whichever rows are selected.  Rows that are not 16-byte aligned or whose stride is
    not a multiple of 8 take the exact tier (reason "not_eligible"), and so does input with a
    NaN, an infinity or a square beyond fp32 (reason "nonfinite_fallback", decided on the
    device).  ``multi_krum.last_info`` = {"tier", "reason", "slices", "flush", "beta"}."""
    bf16, mode = _dist_request(wList, options and options.get("bf16"),
                               (options or {}).get("distances", "exact"), "multi_krum")
    K, d = _shape(wList, "multi_krum", bf16=bf16, max_k=4096)
    honest = _honest_size(options, "multi_krum")
    if not 2 <= honest <= K + 1:
        raise ValueError(f"multi_krum: honestSize {honest} not in [2, {K + 1}]")
    m = options.get("m")
    m = honest if m is None else int(m)
    if not 1 <= m <= K:
        raise ValueError(f"multi_krum: m = {m} not in [1, {K}]")
    X, ldx, layout, K, d = _operand(wList, bf16=bf16)
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    sel = (C.c_int32 * m)()
    multi_krum.last_info = dict(_FP32_DIST_INFO)
    if d > 0 and bf16:
        ctx = context(X.device)
        ctx.call("gm_multi_krum_bf16", X.data_ptr(), K, d, ldx, layout, honest, m, mode,
                 out.data_ptr(), sel, _stream_ptr(X.device))
        multi_krum.last_info = _dist_info(ctx)
    elif d > 0:
        context(X.device).call("gm_multi_krum_f32", X.data_ptr(), K, d, ldx, layout, honest, m,
                               out.data_ptr(), sel, _stream_ptr(X.device))
    multi_krum.last_selected = list(sel) if d > 0 else []
    return _to_caller(out, wList)


multi_krum.last_selected = multi_krum.last_info = None


def bulyan(wList, options):
    """Bulyan (El Mhamdi, Guerraoui & Rouault, ICML 2018) with f = K - honestSize Byzantine
    rows, K >= 4f + 3: theta = K - 2f rounds of Krum selection on the rows that remain (a
    row's score: the sum of its max(1, |S| - f - 1) smallest squared distances within the
    remaining set S, itself included; the smallest score, ties to the lower index, is selected
    and leaves S; the distances are computed once), then mean-around-median over the selected
    rows keeping theta - 2f values per coordinate (f == 0: the column mean).  wList: an fp32
    [K, d] tensor or fp32 ClientPanels, K <= 1024.  ``bulyan.last_selected`` holds the
    selected rows in selection order."""
    K, d = _shape(wList, "bulyan", max_k=1024)
    honest = _honest_size(options, "bulyan")
    f = K - honest
    if honest < 1 or f < 0:
        raise ValueError(f"bulyan: honestSize {honest} not in [1, {K}]")
    if K < 4 * f + 3:
        raise ValueError(f"bulyan: K = {K} < 4f + 3 = {4 * f + 3} with f = K - honestSize = {f}")
    X, ldx, layout, K, d = _operand(wList)
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    theta = K - 2 * f
    sel = (C.c_int32 * theta)()
    if d > 0:
        context(X.device).call("gm_bulyan_f32", X.data_ptr(), K, d, ldx, layout, honest,
                               out.data_ptr(), sel, _stream_ptr(X.device))
    bulyan.last_selected = list(sel) if d > 0 else []
    return _to_caller(out, wList)


bulyan.last_selected = None


def _assignment(K: int, s: int, generator=None) -> torch.Tensor:
    """The random assignment of K clients to ceil(K/s) buckets: ``torch.randperm(K)``, one
    draw from `generator` (the global CPU generator when None).  Bucket i holds clients
    ``perm[i*s : (i+1)*s]``."""
    _index(s, "bucketing", "s", 1)
    return torch.randperm(int(K), generator=generator)


def _bucket_perm(perm, K: int) -> torch.Tensor:
    """`perm` as a CPU int64 vector, checked to be a permutation of 0..K-1 (the kernel does
    not check: a bad index would read outside the matrix)."""
    p = torch.as_tensor(perm).detach().cpu()
    if p.dim() != 1 or p.numel() != K or p.dtype.is_floating_point or p.dtype == torch.bool:
        raise ValueError(f"bucketing: perm must be {K} integers (got {tuple(p.shape)} {p.dtype})")
    p = p.to(torch.int64)
    if not torch.equal(torch.sort(p).values, torch.arange(K)):
        raise ValueError(f"bucketing: perm is not a permutation of 0..{K - 1}")
    return p


def bucketing(wList, s, perm=None, generator=None, layout=None):
    """s-bucketing (Karimireddy, He & Jaggi, "Byzantine-Robust Learning on Heterogeneous
    Datasets via Bucketing", ICLR 2022), the pre-step that makes gm2 / gm / cclip / Krum / the
    coordinate-wise aggregators work on non-iid clients: permute the K clients at random,
    average each consecutive group of s rows, hand the Kb = ceil(K/s) bucket means to the
    aggregator.  One memory-bound HIP pass (bucket.hip): K*d elements read, Kb*d floats
    written, after which every pass of the aggregator reads 1/s of the bytes.

    wList: an fp32 or bf16 [K, d] tensor (any stride or alignment; a CPU tensor is staged to
    the GPU and the row-major result copied back) or an fp32 or bf16 ClientPanels; never
    written.  Returns the bucket means as fp32: with ``layout=None`` a [Kb, d] tensor for a
    tensor and ``ClientPanels(Kb, d)`` (on the GPU) for ClientPanels; ``"rows"`` / ``"panels"``
    force one.  Each mean is the fp64 sum of its bucket in bucket order, divided by the
    bucket's size (the last bucket is shorter when s does not divide K) and rounded once, so
    the values are bit-identical whatever the input or output layout.

    perm: a length-K integer tensor, validated on the host as a permutation of 0..K-1
    (ValueError) and sent as int32; bucket i is rows ``perm[i*s:(i+1)*s]``.  None:
    ``bucketing.assignment(K, s, generator)`` = ``torch.randperm(K, generator=generator)``, one
    draw, from the global CPU generator when no generator is given.  ``bucketing.last_perm``
    holds the permutation used.  ``s == 1`` returns wList itself: no draw, no launch.

    d-sharded clients (ShardedGM): bucketing is column-local, so each rank buckets its own
    shard with the SAME perm and hands the result to ``ShardedGM.gm2`` / ``.cclip``."""
    s = _index(s, "bucketing", "s", 1)
    K, d = _shape(wList, "bucketing", bf16=True)
    # (the Kb bucket means: a Kb without a panel width is refused where the panels are made)
    panels_out = _panels_out(layout, wList, None, "bucketing")
    if s == 1:
        return wList
    p = _bucket_perm(perm, K) if perm is not None else _assignment(K, s, generator)
    bucketing.last_perm = p
    X, ldx, lin, K, d = _operand(wList, bf16=True)
    out, Y, ldy, lout = _new_rows(-(-K // s), d, X.device, panels_out)
    if d > 0:
        # (pdev goes back to torch's caching allocator, which reuses it in stream order)
        pdev = p.to(device=X.device, dtype=torch.int32)
        context(X.device).call(
            "gm_bucket_means_bf16" if X.dtype == torch.bfloat16 else "gm_bucket_means_f32",
            X.data_ptr(), K, d, ldx, lin, pdev.data_ptr(), s, Y.data_ptr(), ldy, lout,
            _stream_ptr(X.device))
    return _to_caller(out, wList)


bucketing.assignment = _assignment
bucketing.last_perm = None


def bucketed(aggregate, s, generator=None, layout="panels"):
    """An ``aggregate(wList, options)`` callable that s-buckets wList (``bucketing``, a fresh
    random assignment from `generator` per call) and calls `aggregate` on the bucket means,
    handed over in `layout` ("panels", the layout the streaming pass reads fastest, "rows",
    or None for wList's own).  Named ``f"{aggregate.__name__}_b{s}"``; works with gm2, gm,
    ``cclip.with_options(...)``, mean, median, trimmed_mean, Krum, multi_krum, bulyan and meamed,
    and as
    ``training.run(..., aggregate=bucketed(gm2, 2))``.

    Options pass through unchanged except ``honestSize``: with B = K - honestSize Byzantine
    clients at most B buckets are contaminated, so the inner call gets
    ``honestSize' = ceil(K/s) - B`` (ValueError if that is < 2: s is too large for this many
    Byzantine clients).  The caller's dict is not modified.  ``s == 1`` calls `aggregate`
    directly.  The result lives on wList.device, as the aggregators' own."""
    s = _index(s, "bucketed", "s", 1)
    _panels_out(layout, None, None, "bucketed")

    def step(wList, options, name):
        if s == 1:
            return wList, options
        K = int(wList.shape[0])
        Kb = -(-K // s)
        if options and options.get("honestSize") is not None:
            inner = Kb - (K - int(options["honestSize"]))
            if inner < 2:
                raise ValueError(
                    f"{name}: {K - int(options['honestSize'])} Byzantine clients leave "
                    f"honestSize' = {inner} of {Kb} buckets (needs >= 2): use a smaller s")
            options = dict(options, honestSize=inner)
        return bucketing(wList, s, generator=generator, layout=layout), options

    return _pre_step(aggregate, f"b{s}",
                     f"{aggregate.__name__} on the bucket means of s = {s} bucketing", step)


def nnm(wList, f, layout=None, neighbors=False, bf16=False, distances="exact"):
    """Nearest-neighbor mixing (Allouah, Farhadkhani, Guerraoui, Gupta, Pinot & Stephan, "Fixing
    by Mixing: A Recipe for Optimal Byzantine ML under Heterogeneity", AISTATS 2023, Algorithm
    1), the pre-step under which the robust rules reach the optimal heterogeneity bound: every
    client update is replaced by the mean of its K - f nearest updates, itself included.
    Deterministic; all K rows are kept, so ``honestSize`` is unchanged.  Three HIP steps
    (gm_nnm_f32): the exact pair distances multi_krum scores, each row's K - f nearest by
    (distance, index), and the mixing pass (nnm.hip), whose every element is the fp64 sum of its
    K - f terms in increasing row index, divided, rounded once: bit-identical whatever the
    input or output layout.  A row outside a neighbourhood contributes nothing to it, whatever
    it holds (huge, inf, NaN).

    wList: an fp32 [K, d] tensor (any stride or alignment; a CPU tensor is staged to the GPU and
    the row-major result copied back) or fp32 ClientPanels, K <= 4096; never written.  f: an
    integer in [0, K - 1] (``f == 0``: every row becomes the column mean).  Returns the mixed
    rows as fp32: with ``layout=None`` a [K, d] tensor for a tensor and ``ClientPanels(K, d)``
    for ClientPanels; ``"rows"`` / ``"panels"`` force one.  ``neighbors=True`` returns
    ``(Y, N)`` with N the int32 [K, K - f] neighbour lists (increasing within a row) on the GPU.
    d-sharded contexts and K > 4096 are refused.

    ``bf16=True`` also reads a bf16 [K, d] tensor (unit-stride rows in place, at any alignment)
    or bf16 ClientPanels; the mixed rows stay fp32.  Without it bf16 input raises TypeError
    before a GPU is touched.  ``distances``: "exact" (the default) gives the bits of the fp32
    call on ``wList.float()``; "mfma" (bf16 only; ValueError on fp32) takes the distances from
    the bf16 matrix cores within beta (||x_i||^2 + ||x_j||^2), so a neighbour list can differ
    from the exact tier's only in members whose distances lie within that band of the list's
    threshold, and every row of Y is still the fp64 mean of the rows its list names (tiers,
    fallbacks and the reasons: ``multi_krum``).  ``nnm.last_info`` = {"tier", "reason",
    "slices", "flush", "beta"}; a bf16 call waits for its stream to fill it in."""
    bf16, mode = _dist_request(wList, bf16, distances, "nnm")
    K, d = _shape(wList, "nnm", bf16=bf16, max_k=4096)
    f = _index(f, "nnm", "f", 0, K - 1)
    panels_out = _panels_out(layout, wList, K, "nnm")
    X, ldx, lin, K, d = _operand(wList, bf16=bf16)
    m = K - f
    out, Y, ldy, lout = _new_rows(K, d, X.device, panels_out)
    N = torch.empty(K, m, dtype=torch.int32, device=X.device) if neighbors else None
    nnm.last_info = dict(_FP32_DIST_INFO)
    if d > 0 and bf16:
        ctx = context(X.device)
        ctx.call("gm_nnm_bf16", X.data_ptr(), K, d, ldx, lin, f, mode, Y.data_ptr(), ldy, lout,
                 N.data_ptr() if neighbors else None, _stream_ptr(X.device))
        nnm.last_info = _dist_info(ctx)
    elif d > 0:
        context(X.device).call("gm_nnm_f32", X.data_ptr(), K, d, ldx, lin, f, Y.data_ptr(), ldy,
                               lout, N.data_ptr() if neighbors else None, _stream_ptr(X.device))
    elif neighbors:                      # every distance is 0: the m rows of lowest index
        N.copy_(torch.arange(m, dtype=torch.int32, device=X.device).expand(K, m))
    out = _to_caller(out, wList)
    return (out, N) if neighbors else out


nnm.last_info = None


def pair_distances(wList, bf16=False, distances="exact"):
    """The K x K squared distances of the client updates, fp64 [K, K] on the GPU, full and
    symmetric: the matrix Krum, multi_krum, nnm, bulyan and caf work on.  fp32 input (a [K, d]
    tensor or ClientPanels): the exact path.  ``bf16=True`` also reads bf16 rows or bf16
    ClientPanels, ``distances`` "exact" (the fp32 kernels on the widened elements: the bits of
    ``pair_distances(wList.float())``) or "mfma" (the bf16 matrix cores, within
    ``pair_distances.last_info["beta"]`` (||x_i||^2 + ||x_j||^2) of the exact-arithmetic
    distances; bf16 only, ValueError on fp32; see ``multi_krum``).  K <= 4096."""
    is_bf16, mode = _dist_request(wList, bf16, distances, "pair_distances")
    K, d = _shape(wList, "pair_distances", bf16=is_bf16, max_k=4096)
    X, ldx, layout, K, d = _operand(wList, bf16=is_bf16)
    D = torch.zeros(K, K, dtype=torch.float64, device=X.device)
    pair_distances.last_info = dict(_FP32_DIST_INFO)
    if d > 0 and is_bf16:
        ctx = context(X.device)
        ctx.call("gm_pair_dist_bf16", X.data_ptr(), K, d, ldx, layout, mode, D.data_ptr(),
                 _stream_ptr(X.device))
        pair_distances.last_info = _dist_info(ctx)
    elif d > 0:
        context(X.device).call("gm_pair_dist_f32", X.data_ptr(), K, d, ldx, layout, D.data_ptr(),
                               _stream_ptr(X.device))
    return D


pair_distances.last_info = None


def mixed(aggregate, f=None, layout="panels"):
    """An ``aggregate(wList, options)`` callable that mixes wList (``nnm``) and calls `aggregate`
    on the mixed rows, handed over in `layout` ("panels", the layout the streaming pass reads
    fastest — rows where K has no panel width — "rows", or None for wList's own).  Named
    ``f"{aggregate.__name__}_nnm"``; works with every aggregator ``bucketed`` lists, and as
    ``training.run(..., aggregate=mixed(gm2))``.

    f: the number of Byzantine clients to mix against; None takes ``K - options['honestSize']``
    per call (ValueError without it).  Options pass through unchanged (NNM keeps all K rows, so
    ``honestSize`` stands); the caller's dict is not modified.  The mixing step itself reads
    ``options["bf16"]`` and ``options["distances"]`` (``nnm``'s arguments of those names), so
    ``mixed(gm2)(Xbf16, {"bf16": True, "distances": "mfma"})`` mixes bf16 rows on the fast
    distances.  The result lives on wList.device, as the aggregators' own."""
    _panels_out(layout, None, None, "mixed")

    def step(wList, options, name):
        K = int(wList.shape[0])
        f_ = f if f is not None else K - _honest_size(options, name)
        # (only what the call's options name: without them nnm is called as before)
        tier = {k: options[k] for k in ("bf16", "distances") if options and k in options}
        return nnm(wList, f_, layout=_handover(layout, K), **tier), options

    return _pre_step(aggregate, "nnm",
                     f"{aggregate.__name__} on the rows mixed by nearest-neighbor mixing", step)


_DNC_KEYS = ("dnc_iters", "dnc_dims", "dnc_c", "dnc_columns", "generator", "power_iters",
             "power_tol")
_DNC_MAX_ELEMS = 1 << 27          # gm_dnc_f32's cap on K * n


def _dnc_scalars(options):
    """(iters, b, c, power_iters, power_tol) from the options; ValueError on an invalid value."""
    iters = int(options.get("dnc_iters", 1))
    if iters < 1:
        raise ValueError(f"dnc: dnc_iters must be >= 1 (got {options.get('dnc_iters')!r})")
    b = int(options.get("dnc_dims", 10000))
    if b < 1:
        raise ValueError(f"dnc: dnc_dims must be >= 1 (got {options.get('dnc_dims')!r})")
    c = float(options.get("dnc_c", 1.0))
    if not 0 <= c < math.inf:                         # (NaN fails too)
        raise ValueError(f"dnc: dnc_c must be >= 0 (got {options.get('dnc_c')!r})")
    pit = int(options.get("power_iters", 100))
    if pit < 1:
        raise ValueError(f"dnc: power_iters must be >= 1 (got {options.get('power_iters')!r})")
    ptol = float(options.get("power_tol", 1e-10))
    if not ptol >= 0:
        raise ValueError(f"dnc: power_tol must be >= 0 (got {options.get('power_tol')!r})")
    return iters, b, c, pit, ptol


def _dnc_draw(d, b, iters, generator=None) -> torch.Tensor:
    """The columns DnC samples, an int64 [iters, min(b, d)] CPU tensor, each row increasing.
    b < d: per round ``torch.randperm(d, generator=generator)[:b]``, sorted, one draw per round
    (from the global CPU generator when no generator is given).  b >= d: every round is
    ``arange(d)`` and nothing is drawn.  A draw costs O(d) on the host per round, whatever b."""
    d, b, iters = int(d), int(b), int(iters)
    if d < 1 or b < 1 or iters < 1:
        raise ValueError(f"dnc.columns: d, b and iters must be >= 1 (got {d}, {b}, {iters})")
    if b >= d:
        return torch.arange(d).repeat(iters, 1)
    return torch.stack([torch.sort(torch.randperm(d, generator=generator)[:b]).values
                        for _ in range(iters)])


def _dnc_given_columns(cols, iters: int, d: int) -> torch.Tensor:
    """options['dnc_columns'] as a CPU int64 [iters, n] tensor, checked on the host (the kernel
    does not check: a bad index would read outside the matrix)."""
    p = torch.as_tensor(cols).detach().cpu()
    if p.dtype.is_floating_point or p.dtype == torch.bool or p.dtype.is_complex:
        raise ValueError(f"dnc: dnc_columns must hold integers (got {p.dtype})")
    if p.dim() == 1 and iters == 1:
        p = p[None]
    if p.dim() != 2 or p.shape[0] != iters or not 1 <= p.shape[1] <= d:
        raise ValueError(f"dnc: dnc_columns must be [{iters}, n] with 1 <= n <= {d} "
                         f"(got {tuple(p.shape)})")
    p = p.to(torch.int64).contiguous()
    if int(p.min()) < 0 or int(p.max()) >= d:
        raise ValueError(f"dnc: dnc_columns outside [0, {d - 1}]")
    if p.shape[1] > 1 and not bool((p[:, 1:] > p[:, :-1]).all()):
        raise ValueError("dnc: every row of dnc_columns must be strictly increasing")
    return p


def dnc(wList, options):
    """Divide-and-Conquer (Shejwalkar & Houmansadr, "Manipulating the Byzantine", NDSS 2021,
    Algorithm 2), the spectral filter published with the min-max / min-sum attacks: ``dnc_iters``
    (default 1) times, sample ``dnc_dims`` (b, default 10000; b >= d takes every column) columns,
    centre the K x b sub-matrix, find its top right singular vector v by power iteration, score
    every row by (c_k . v)^2 and keep the K - q rows of smallest score, q = int(dnc_c * f),
    ``dnc_c`` default 1.0, f = K - honestSize; the result is the mean of the rows every round
    kept.  All of it in fp64 on the GPU (gm_dnc_f32: the gather, the iteration and the scores in
    dnc.hip, then multi_krum's selection and mean); include/gmagg.h has the definition, tie rules
    and start vector.  Bit-identical for rows, panels and every alignment; q == 0 is ``mean``.

    wList: an fp32 [K, d] tensor (any stride; a CPU tensor is staged and the result copied back)
    or fp32 ClientPanels, 2 <= K <= 4096, K * b <= 2^27; never written.  bf16, fp64 (TypeError),
    a missing ``honestSize``, q * dnc_iters >= K, dnc_c < 0, dnc_iters < 1 (ValueError) are
    refused before a GPU is touched.  Other options: ``power_iters`` (100) and ``power_tol``
    (1e-10), the iteration's cap and its stop on the unit iterate's movement; ``generator`` for
    the column draw (``dnc.columns(d, b, iters, generator)``: ``torch.randperm(d)[:b]`` sorted,
    per round, O(d) host work per round whatever b); ``dnc_columns``, an explicit integer
    [dnc_iters, n] tensor, each row strictly increasing in [0, d), which replaces the draw and
    its cost.  Every other key is ignored.

    After a call ``dnc.last_columns`` holds the columns used (CPU int64 [dnc_iters, n]; n = 0 when
    q == 0: nothing is drawn), ``dnc.last_selected`` the good rows, increasing,
    ``dnc.last_scores`` the fp64 [dnc_iters, K] scores on the GPU and ``dnc.last_info``
    ``{"removed": q, "power_iters": [...], "converged": [...]}`` per round."""
    K, d = _shape(wList, "dnc", max_k=4096)
    honest = _honest_size(options, "dnc")
    iters, b, c, pit, ptol = _dnc_scalars(options)
    f = K - honest
    if honest < 1 or f < 0:
        raise ValueError(f"dnc: honestSize {honest} not in [1, {K}]")
    if K < 2:
        raise ValueError(f"dnc: K >= 2 (got {K})")
    q = int(c * f)
    if q * iters >= K:
        raise ValueError(f"dnc: q * dnc_iters = {q} * {iters} >= K = {K} rows would be removed")
    cols = torch.empty(iters, 0, dtype=torch.int64)
    if q > 0 and d > 0:
        given = options.get("dnc_columns")
        cols = (_dnc_given_columns(given, iters, d) if given is not None
                else _dnc_draw(d, b, iters, options.get("generator")))
        if K * cols.shape[1] > _DNC_MAX_ELEMS:
            raise ValueError(f"dnc: K * n = {K} * {cols.shape[1]} sampled elements exceed 2^27: "
                             "lower dnc_dims")
    X, ldx, layout, K, d = _operand(wList)
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    scores = torch.zeros(iters, K, dtype=torch.float64, device=X.device)
    good, n_good = (C.c_int32 * K)(*range(K)), C.c_int64(K)
    nit, conv = (C.c_int32 * iters)(), (C.c_int32 * iters)(*([1] * iters))
    if d > 0:
        # (cdev goes back to torch's caching allocator, which reuses it in stream order)
        cdev = cols.to(X.device) if q > 0 else None
        context(X.device).call("gm_dnc_f32", X.data_ptr(), K, d, ldx, layout,
                               cdev.data_ptr() if q > 0 else None, cols.shape[1], iters, q, pit,
                               ptol, out.data_ptr(), scores.data_ptr(), good, C.byref(n_good), nit,
                               conv, _stream_ptr(X.device))
    dnc.last_columns = cols
    dnc.last_selected = list(good[:n_good.value])
    dnc.last_scores = scores
    dnc.last_info = {"removed": q, "power_iters": list(nit), "converged": [bool(x) for x in conv]}
    return _to_caller(out, wList)


dnc.columns = _dnc_draw
dnc.with_options = _with_options(
    "dnc", _DNC_KEYS, _fixed_options("dnc", _dnc_scalars),
    """An ``aggregate(wList, options)`` callable named "dnc" that applies the given dnc options
    over the caller's, for loops that build the dict themselves
    (training.run(..., aggregate=dnc.with_options(dnc_c=1.5, dnc_iters=3))).""")
dnc.last_columns = dnc.last_selected = dnc.last_scores = dnc.last_info = None


_CAF_KEYS = ("power_iters", "power_tol")


def _caf_scalars(options):
    """(power_iters, power_tol) of a caf options dict, refused with ValueError where out of
    range."""
    pit = int(options.get("power_iters", 100))
    if pit < 1:
        raise ValueError(f"caf: power_iters must be >= 1 (got {options.get('power_iters')!r})")
    ptol = float(options.get("power_tol", 1e-10))
    if not ptol >= 0:
        raise ValueError(f"caf: power_tol must be >= 0 (got {options.get('power_tol')!r})")
    return pit, ptol


def caf(wList, options):
    """CAF, the covariance filter (the down-weighting filter of Diakonikolas et al., "Being Robust
    (in High Dimensions) Can Be Practical", ICML 2017; ByzFL's Covariance-bound Agnostic Filter):
    while the weights c (all 1 at first) sum to more than K - 2f, f = K - honestSize, find the top
    eigenpair of the weighted covariance of all d coordinates by power iteration, remember the
    weights of the round with the smallest eigenvalue, and scale every weight down by its row's
    squared projection on the eigenvector over the largest one (that row's weight becomes 0).
    The result is the mean weighted by the remembered c*.  All of it in fp64 on the GPU, solved on
    the K x K squared distances without ever forming the covariance (gm_caf_f32, caf.hip);
    include/gmagg.h has the definition, start vector and tie rules.  Bit-identical for rows, panels
    and every alignment; f == 0 is ``mean``.  Where ``dnc`` filters on sampled columns, this sees
    every coordinate.  A non-finite entry ends the filter with all weights 1: compose with
    ``clipped`` / ``arc`` for that.

    wList: an fp32 [K, d] tensor (any stride; a CPU tensor is staged and the result copied back)
    or fp32 ClientPanels, 2 <= K <= 4096; never written.  bf16, fp64 (TypeError), a missing
    ``honestSize``, 2f >= K, K < 2, power_iters < 1 (ValueError) are refused before a GPU is
    touched.  Options: ``honestSize`` (required), ``power_iters`` (100) and ``power_tol`` (1e-10),
    the iteration's cap per round and its stop on the unit iterate's movement.  Every other key is
    ignored.

    After a call ``caf.last_weights`` holds the fp64 [K] c* on the GPU and ``caf.last_info``
    ``{"rounds", "best_round", "eigenvalue", "weight", "power_iters": [...], "converged": [...]}``:
    the rounds run, the round whose weights were kept, its eigenvalue, S* = sum c*, and per round
    the applications run and whether the movement test passed."""
    K, d = _shape(wList, "caf", max_k=4096)
    honest = _honest_size(options, "caf")
    pit, ptol = _caf_scalars(options)
    f = K - honest
    if K < 2:
        raise ValueError(f"caf: K >= 2 (got {K})")
    if honest < 1 or f < 0:
        raise ValueError(f"caf: honestSize {honest} not in [1, {K}]")
    if 2 * f >= K:
        raise ValueError(f"caf: 2f = 2 * {f} >= K = {K}: needs an honest majority")
    X, ldx, layout, K, d = _operand(wList)
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    weights = torch.ones(K, dtype=torch.float64, device=X.device)
    lam, S = C.c_double(math.nan), C.c_double(float(K))
    rounds, best = C.c_int32(0), C.c_int32(0)
    nit, conv = (C.c_int32 * K)(), (C.c_int32 * K)()
    if d > 0:
        context(X.device).call("gm_caf_f32", X.data_ptr(), K, d, ldx, layout, f, pit, ptol,
                               out.data_ptr(), weights.data_ptr(), C.byref(lam), C.byref(S),
                               C.byref(rounds), C.byref(best), nit, conv, _stream_ptr(X.device))
    n = rounds.value
    caf.last_weights = weights
    caf.last_info = {"rounds": n, "best_round": best.value, "eigenvalue": lam.value,
                     "weight": S.value, "power_iters": list(nit[:n]),
                     "converged": [bool(x) for x in conv[:n]]}
    return _to_caller(out, wList)


caf.with_options = _with_options(
    "caf", _CAF_KEYS, _fixed_options("caf", _caf_scalars),
    """An ``aggregate(wList, options)`` callable named "caf" that applies the given caf options
    over the caller's, for loops that build the dict themselves
    (training.run(..., aggregate=caf.with_options(power_iters=50))).""")
caf.last_weights = caf.last_info = None


_FLTRUST_KEYS = ("server_update", "server_row")
_FLTRUST_MAX_K = 2048             # gm_fltrust_f32 / _bf16's cap on K


def _fltrust_server(options, K=None, d=None):
    """(server_update or None, server_row or -1) from the options: exactly one of the two,
    server_row an int (not a bool or a float), in [0, K) when K is known, server_update a tensor
    of d elements when d is known; TypeError / ValueError otherwise."""
    su, sr = options.get("server_update"), options.get("server_row")
    if (su is None) == (sr is None):
        raise ValueError("fltrust needs exactly one of options['server_update'] (a [d] tensor) and "
                         "options['server_row'] (a row of wList)")
    if su is not None:
        if not isinstance(su, torch.Tensor):
            raise TypeError(f"fltrust: server_update must be a tensor (got {type(su).__name__})")
        if su.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"fltrust: server_update must be fp32 or bf16 (got {su.dtype})")
        if d is not None and su.numel() != d:
            raise ValueError(f"server_update has {su.numel()} elements, wList rows have {d}")
        return su, -1
    # (a server_row that is no integer is a TypeError, as a server_update that is no tensor)
    return None, _index(sr, "fltrust", "server_row", 0, None if K is None else K - 1, TypeError)


def _fltrust_args(wList, options, who: str, bf16: bool = True):
    """(K, d, server_update or None, server_row or -1, guess or None) of an fltrust call, checked
    before anything touches a GPU (ShardedGM.fltrust reads fp32 shards only)."""
    options = options or {}
    K, d = _shape(wList, who, bf16=bf16, max_k=_FLTRUST_MAX_K)
    su, row = _fltrust_server(options, K, d)
    guess = options.get("guess")
    if guess is not None and guess.numel() != d:
        raise ValueError(f"guess has {guess.numel()} elements, the rows have {d}")
    return K, d, su, row, guess


def _run_fltrust(ctx, X, K: int, d: int, ldx: int, layout: int, server, row: int, centre):
    """gm_fltrust_f32 / _bf16 on ctx: (out [d] fp32, stats [3K + 2] fp64) on X's device."""
    out = torch.empty(d, dtype=torch.float32, device=X.device)
    stats = torch.zeros(3 * K + 2, dtype=torch.float64, device=X.device)
    ctx.call("gm_fltrust_bf16" if X.dtype == torch.bfloat16 else "gm_fltrust_f32", X.data_ptr(),
             K, d, ldx, layout, server.data_ptr() if server is not None else None, row,
             centre.data_ptr() if centre is not None else None, out.data_ptr(), stats.data_ptr(),
             _stream_ptr(X.device))
    return out, stats


def _fltrust_info(stats, K: int):
    return {"cos": stats[:K], "norm2": stats[K:2 * K], "trust": stats[2 * K:3 * K],
            "server_norm2": stats[3 * K], "trust_sum": stats[3 * K + 1]}


def fltrust(wList, options):
    """FLTrust (Cao, Fang, Liu & Gong, "FLTrust: Byzantine-robust Federated Learning via Trust
    Bootstrapping", NDSS 2021), not one of the reference's aggregators: the server holds an
    update of its own, every client is scored by the cosine of its update with the server's,
    negative scores are cut to zero, and the clients of positive score, each rescaled to the
    server update's norm, are averaged with their scores as weights.  With c = options['guess']
    (default None: zeros, the rows are updates; the training loop passes the current model, so
    the rows are models and c the model they started from), u_k = x_k - c and g = s - c:

        TS_k = max(0, cos(u_k, g)),    out = c + sum_k TS_k ||g|| / ||u_k|| u_k / sum_k TS_k

    in fp64 on the widened values, rounded once (the definition, the skipped rows and the order
    of every sum are in include/gmagg.h).  A row of zero or non-finite norm, a row with a
    non-finite product and the server row itself score 0 and are not read again; when no row is
    trusted the result is c itself (the paper leaves that case undefined).

    The server update s is given by exactly one of
      ``server_update``  a [d] tensor (fp32 or bf16) in the rows' representation: a model when
                         the rows are models, an update when they are updates;
      ``server_row``     an int in [0, K): that row of wList is the server's (the client that
                         trains on the root dataset); it gets no weight itself.  The index is into
                         the rows the CALLER passes: under ``bucketed(...)`` / ``mixed(...)`` the
                         rows are bucket means or mixed rows, and only ``server_update`` is
                         meaningful.
    Every other key (maxiter, tol, honestSize, noise_var, ...) is ignored.

    wList: an fp32 or bf16 [K, d] tensor (any stride; a CPU tensor is staged to the GPU and the
    result copied back) or an fp32 or bf16 ClientPanels, K <= 2048; never written.  fp16 / fp64
    raise TypeError; K > 2048 and wrong lengths ValueError; all before a GPU is touched.  The
    result is fp32 on wList.device.  Two HIP passes (fltrust.hip): one read of wList, one of the
    trusted rows; no host synchronisation.  ``fltrust.last_info`` holds the by-products as views
    of one device buffer: ``cos``, ``norm2`` (||u_k||^2) and ``trust`` (TS_k) as fp64 [K],
    ``server_norm2`` and ``trust_sum`` as 0-dim tensors."""
    K, d, su, row, guess = _fltrust_args(wList, options, "fltrust")
    X, ldx, layout, K, d = _operand(wList, bf16=True)
    server = _vector(su, d, X.device, "server_update")
    centre = _vector(guess, d, X.device, "guess")
    out, stats = _run_fltrust(context(X.device), X, K, d, ldx, layout, server, row, centre)
    fltrust.last_info = _fltrust_info(stats, K)
    return _to_caller(out, wList)


fltrust.with_options = _with_options(
    "fltrust", _FLTRUST_KEYS, _fixed_options("fltrust", _fltrust_server),
    """An ``aggregate(wList, options)`` callable named "fltrust" that applies server_update /
    server_row over the caller's options, for loops that build the dict themselves
    (training.run(..., aggregate=fltrust.with_options(server_row=0)): client 0's shard is the
    root dataset).""")
fltrust.last_info = None


_CLIP_MAX_K = 4096                # gm_clip_rows_f32 / _bf16's cap on K


def _clip_tau(tau, who: str) -> float:
    """tau as a float > 0 (+inf allowed); ValueError otherwise (a bool, a string, 0, NaN)."""
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not tau > 0:
        raise ValueError(f"{who}: tau must be a number > 0 (got {tau!r})")
    return float(tau)


def _clip_centre(centre, d: int, who: str):
    """The centre as given (None, or an fp32 / bf16 tensor of d elements); TypeError /
    ValueError otherwise."""
    if centre is None:
        return None
    if not isinstance(centre, torch.Tensor):
        raise TypeError(f"{who}: centre must be a tensor (got {type(centre).__name__})")
    if centre.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{who}: centre must be fp32 or bf16 (got {centre.dtype})")
    if centre.numel() != d:
        raise ValueError(f"{who}: centre has {centre.numel()} elements, wList rows have {d}")
    return centre


def _clip_args(wList, who: str, rule: int, f, tau, centre, bf16: bool = True):
    """(K, d, f, tau, centre) of a clip / arc call, checked before anything touches a GPU
    (ShardedGM.clip / .arc read fp32 shards only)."""
    K, d = _shape(wList, who, bf16=bf16, max_k=_CLIP_MAX_K)
    if rule == _lib.GM_CLIP_ARC:
        f, tau = _index(f, who, "f", 0, K - 1), 0.0
    else:
        f, tau = 0, _clip_tau(tau, who)
    return K, d, f, tau, _clip_centre(centre, d, who)


def _clip_info(stats, K: int):
    return {"norm2": stats[:K], "scale": stats[K:2 * K], "threshold2": stats[2 * K],
            "clipped": stats[2 * K + 1]}


def _run_clip(ctx, X, K: int, d: int, ldx: int, lin: int, centre, rule: int, f: int, tau: float,
              panels_out: bool, inplace: bool = False):
    """gm_clip_rows_f32 / _bf16 on ctx: (the clipped rows, stats [2K + 2] fp64) on X's device.
    The rows are a [K, d] tensor or ClientPanels(K, d), or None in place (X holds them)."""
    out, Y, ldy, lout = (None, X, ldx, lin) if inplace else _new_rows(K, d, X.device, panels_out)
    stats = torch.zeros(2 * K + 2, dtype=torch.float64, device=X.device)
    if d > 0:
        ctx.call("gm_clip_rows_bf16" if X.dtype == torch.bfloat16 else "gm_clip_rows_f32",
                 X.data_ptr(), K, d, ldx, lin, centre.data_ptr() if centre is not None else None,
                 rule, f, tau, Y.data_ptr(), ldy, lout, stats.data_ptr(), _stream_ptr(X.device))
    else:                                # every n_k is 0: nothing to clip
        stats[K:2 * K] = 1.0
        stats[2 * K] = tau * tau if rule == _lib.GM_CLIP_STATIC else 0.0
    return out, stats


def _clip(fn, wList, rule: int, f, tau, centre, layout, inplace: bool):
    who = fn.__name__
    K, d, f, tau, centre = _clip_args(wList, who, rule, f, tau, centre)
    panels_in = isinstance(wList, ClientPanels)
    # (in place the rows stay where they are: no panel width is asked of K)
    panels_out = _panels_out(layout, wList, None if inplace else K, who)
    if inplace:
        if wList.dtype != torch.float32:
            raise TypeError(f"{who}: inplace=True needs fp32 rows (got {wList.dtype}: the "
                            "clipped rows are fp32)")
        if panels_out != panels_in:
            raise ValueError(f"{who}: inplace=True keeps wList's own layout (got {layout!r})")
    X, ldx, lin, K, d = _operand(wList, bf16=True)
    c = _vector(centre, d, X.device, "centre")
    out, stats = _run_clip(context(X.device), X, K, d, ldx, lin, c, rule, f, tau, panels_out,
                           inplace)
    fn.last_info = _clip_info(stats, K)
    if inplace:
        if not panels_in and X is not wList:
            wList.copy_(X)               # (a CPU or non-unit-stride wList was clipped in a copy)
        return wList
    return _to_caller(out, wList)


def clip(wList, tau, centre=None, layout=None, inplace=False):
    """Static norm clipping (Sun, Kairouz, Suresh & McMahan 2019), the pre-step that bounds what
    one client can move: every row's update about `centre` longer than tau is scaled back to
    length tau.  With c = centre (None: zeros, the rows are updates; a training loop's rows are
    models and c is the model they started from) and u_k = x_k - c:

        y_k = c + min(1, tau / ||u_k||) u_k

    in fp64 on the widened values, rounded once; a row inside the radius is copied bit for bit,
    a row whose norm is not finite becomes c itself (the definition is in include/gmagg.h).
    Two HIP passes (clip.hip): one read of wList for the norms, one that writes the rows; no
    host synchronisation.

    wList: an fp32 or bf16 [K, d] tensor (any stride or alignment; a CPU tensor is staged to the
    GPU and the row-major result copied back) or an fp32 or bf16 ClientPanels, K <= 4096.
    tau: a number > 0 (``math.inf`` clips nothing finite).  Returns the clipped rows as fp32:
    with ``layout=None`` a [K, d] tensor for a tensor and ``ClientPanels(K, d)`` for
    ClientPanels; ``"rows"`` / ``"panels"`` force one.  ``inplace=True`` (fp32 only, wList's own
    layout) overwrites the clipped rows of wList, leaves the others untouched and returns wList
    itself; otherwise wList is never written.  fp16 / fp64 and bf16 in place raise TypeError;
    K > 4096, a bad tau and wrong lengths ValueError; all before a GPU is touched.
    ``clip.last_info`` holds the by-products as views of one device buffer: ``norm2``
    (||u_k||^2) and ``scale`` (s_k) as fp64 [K], ``threshold2`` (tau^2) and ``clipped`` (the
    number of rows with s_k != 1) as 0-dim tensors."""
    return _clip(clip, wList, _lib.GM_CLIP_STATIC, None, tau, centre, layout, inplace)


def arc(wList, f, centre=None, layout=None, inplace=False):
    """Adaptive Robust Clipping, ARC (Allouah, Guerraoui, Gupta, Jellouli, Rizk & Stephan,
    "Adaptive Gradient Clipping for Robust Federated Learning", ICLR 2025): ``clip`` with the
    radius taken from the rows themselves.  With k = (2 f (K - f)) // K, the k updates of largest
    norm about `centre` are scaled back to the norm of the (k + 1)-th largest; ties at the
    threshold stay unclipped, a NaN norm ranks largest and its row becomes the centre.  Meant to
    be composed with ``nnm`` and any aggregator (``clipped``, ``mixed``).

    f: an integer in [0, K - 1], the number of Byzantine clients to clip against (``f == 0``
    clips nothing finite).  Everything else as ``clip``; ``arc.last_info`` likewise, with
    ``threshold2`` the squared radius chosen."""
    return _clip(arc, wList, _lib.GM_CLIP_ARC, f, None, centre, layout, inplace)


clip.last_info = arc.last_info = None


def clipped(aggregate, tau=None, f=None, layout="panels"):
    """An ``aggregate(wList, options)`` callable that clips wList about ``options.get('guess')``
    (the current model in a training loop; None: zeros) and calls `aggregate` on the clipped
    rows, handed over in `layout` ("panels" — rows where K has no panel width — "rows", or None
    for wList's own).  tau None: ARC (``arc``), named ``f"{aggregate.__name__}_arc"``, with f the
    number of Byzantine clients, None taking ``K - options['honestSize']`` per call (ValueError
    without it); tau given: static clipping (``clip``), named ``f"{aggregate.__name__}_clip"``.
    Works with every aggregator ``bucketed`` lists, under ``mixed(...)`` and ``bucketed(...)``,
    and as ``training.run(..., aggregate=clipped(gm2))``.

    Options pass through unchanged (clipping keeps all K rows, so ``honestSize`` stands); the
    caller's dict and wList are not modified.  The result lives on wList.device, as the
    aggregators' own."""
    _panels_out(layout, None, None, "clipped")
    if tau is not None:
        if f is not None:
            raise ValueError("clipped takes tau (static clipping) or f (ARC), not both")
        tau = _clip_tau(tau, "clipped")

    def step(wList, options, name):
        K = int(wList.shape[0])
        centre = options.get("guess") if options else None
        lay = _handover(layout, K)
        if tau is not None:
            return clip(wList, tau, centre=centre, layout=lay), options
        f_ = f if f is not None else K - _honest_size(options, name)
        return arc(wList, f_, centre=centre, layout=lay), options

    return _pre_step(aggregate, "arc" if tau is None else "clip",
                     f"{aggregate.__name__} on the rows clipped about options['guess'] "
                     f"({'ARC' if tau is None else f'radius {tau}'})", step)


def honest_variance(w_local, honestSize: int) -> torch.Tensor:
    """getVarience (M:127-129) on the device: the mean over the first honestSize rows
    of ||x_k - mean||^2, one streaming pass (fp64 sums); a 0-dim fp32 tensor."""
    out = torch.empty((), dtype=torch.float32, device=w_local.device)
    if not isinstance(w_local, ClientPanels) and (
            w_local.device.type != "cuda" or w_local.dtype != torch.float32 or w_local.dim() != 2):
        raise TypeError("honest_variance needs an fp32 CUDA [K, d] matrix or ClientPanels")
    X, ldx, layout, K, d = _operand(w_local)
    if not 1 <= honestSize <= K:
        raise ValueError(f"honestSize {honestSize} not in [1, {K}]")
    # (the rows function takes the honest rows alone, its panel twin K as well)
    rows = (K, int(honestSize)) if layout == _lib.GM_LAYOUT_PANELS else (int(honestSize),)
    context(X.device).call(_twin("gm_honest_variance_f32", layout), X.data_ptr(), *rows, d, ldx,
                           out.data_ptr(), _stream_ptr(X.device))
    return out


def OMA(message, noise_var=0.01, noise_source=None, seed=None):  # noqa: N802 - reference name
    """In-place per-client equalised AWGN (MNIST_Air_weight.py:385-394)."""
    Xc, ldx, layout, K, d = _operand(message)
    src = _noise_source({} if noise_source is None else {"noise_source": noise_source})
    panels = isinstance(message, ClientPanels)
    if panels and src == _lib.GM_NOISE_HOST:   # the reference's [K, d] draws: via rows
        rows = message.to_rows()
        OMA(rows, noise_var, noise_source=noise_source, seed=seed)
        message.copy_rows_(rows)
        return message
    ctx = context(Xc.device)
    stream = _stream_ptr(Xc.device)
    if src == _lib.GM_NOISE_HOST:
        sd = math.sqrt(noise_var)
        hr = torch.normal(torch.zeros(K, 1), 1 / math.sqrt(2))     # M:389-392 order
        hi = torch.normal(torch.zeros(K, 1), 1 / math.sqrt(2))
        nr = torch.normal(torch.zeros(K, d), sd)
        ni = torch.normal(torch.zeros(K, d), sd)
        dev = [t.to(Xc.device) for t in (hr, hi, nr, ni)]
        ctx.call("gm_oma_apply_f32", Xc.data_ptr(), K, d, ldx, *[t.data_ptr() for t in dev],
                 stream)
    else:
        ctx.call(_twin("gm_oma_philox_f32", layout), Xc.data_ptr(), K, d, ldx, float(noise_var),
                 _seed({"seed": seed}), stream)
    if not panels and Xc is not message:
        message.copy_(Xc)                # (a CPU or non-unit-stride message was noised in a copy)
    return message
