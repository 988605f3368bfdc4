"""Omniscient model-poisoning attacks on the client matrix, in place on the GPU.

The reference ships classflip, dataflip and weightflip (MNIST_Air_weight.py:374-383); the
attacks the robust-aggregation papers measure against are not among them.  These four have
the reference's ``attack(messages, byzantinesize)`` signature, so each is a valid ``attack=``
of ``training.SGD`` / ``training.run`` (as a function or by name):

    alie     "A Little Is Enough" (Baruch, Baruch & Goldberg, NeurIPS 2019): mu - z sigma
    ipm      inner-product manipulation (Xie, Koyejo & Gupta, UAI 2019): -epsilon mu
    minmax   min-max  (Shejwalkar & Houmansadr, NDSS 2021): mu - gamma p, the largest gamma with
             max_i ||m - x_i||^2 <= max_ij ||x_i - x_j||^2
    minsum   min-sum  (same paper): sum_i ||m - x_i||^2 <= max_i sum_j ||x_i - x_j||^2

The honest clients are rows 0 .. K-B-1, the Byzantine ones the last B rows (the reference's
``messages[-byzantinesize:]``); mu and sigma are the honest rows' column mean and unbiased
standard deviation in fp64 (include/gmagg.h has the definitions).  Every Byzantine row is
overwritten with the same malicious row; the honest rows keep their bits.  One HIP pass reads
the honest block once and writes the Byzantine block (csrc/attack.hip); min-max and min-sum
add the honest rows' pairwise distances (Krum's exact kernel) and a second read.

``messages``: an fp32 or bf16 [K, d] CUDA tensor (a non-unit column stride or overlapping rows
go through a contiguous copy whose Byzantine rows are copied back, as OMA does), a
ClientPanels of either type, or a CPU tensor (staged to the GPU, the Byzantine rows copied
back).  minmax / minsum are fp32 only.  Returns ``messages``.

alie and ipm are column-local: on a d-sharded matrix every rank attacks its own shard with the
same z or epsilon before ``ShardedGM.gm2`` / ``.cclip``.  minmax and minsum need whole rows.
"""
from __future__ import annotations

import ctypes as C
import operator
from statistics import NormalDist, StatisticsError

import torch

from .aggregators import _index, _operand, _shape, _stream_ptr, _with_options, context
from .panels import ClientPanels, panel_width

__all__ = ["alie", "ipm", "minmax", "minsum", "z_max"]

_DEVS = {"std": 0, "unit": 1, "sign": 2}


def z_max(K: int, B: int) -> float:
    """ALIE's largest undetected shift in standard deviations (Baruch et al., §3):
    ``Phi^-1((K - B - s) / (K - B))`` with ``s = floor(K/2 + 1) - B`` the honest clients the
    Byzantine ones need on their side of the median.  ValueError unless 0 < s."""
    K, B = operator.index(K), operator.index(B)
    s = K // 2 + 1 - B
    H = K - B
    if B < 0 or s <= 0:
        raise ValueError(f"z_max: needs 0 <= B < floor(K/2 + 1) (K = {K}, B = {B})")
    try:
        return NormalDist().inv_cdf((H - s) / H)
    except StatisticsError:
        raise ValueError(f"z_max: no z for K = {K}, B = {B}") from None


def _sizes(messages, byzantinesize, who: str, bf16: bool, max_k=None):
    """(K, d, B) after the checks that need no GPU."""
    K, d = _shape(messages, who, bf16=bf16, max_k=max_k)
    if isinstance(messages, ClientPanels) and messages.W != panel_width(K, messages.dtype):
        raise ValueError(f"{who}: ClientPanels of width {messages.W}, the kernels read "
                         f"W = {panel_width(K, messages.dtype)} for K = {K} {messages.dtype} "
                         "clients")
    # (at least two honest rows: sigma is their unbiased deviation)
    return K, d, _index(byzantinesize, who, "byzantinesize", 1, K - 2)


def _apply(messages, B: int, call):
    """Run ``call(ctx, X, ldx, layout, stream)`` on the device operand of `messages`, then bring
    the Byzantine rows back where the kernel worked on a copy."""
    X, ldx, layout, _, _ = _operand(messages, bf16=True)
    call(context(X.device), X, ldx, layout, _stream_ptr(X.device))
    if not isinstance(messages, ClientPanels) and X is not messages:
        messages[-B:].copy_(X[-B:])
    return messages


def _affine(messages, byzantinesize, who: str, a: float, b: float):
    K, d, B = _sizes(messages, byzantinesize, who, True)
    fn = "gm_attack_affine_bf16" if messages.dtype == torch.bfloat16 else "gm_attack_affine_f32"
    return _apply(messages, B, lambda ctx, X, ldx, layout, stream: ctx.call(
        fn, X.data_ptr(), K, d, ldx, layout, B, float(a), float(b), stream))


def _run_alie(messages, byzantinesize, z=None):
    if z is None:
        K, _, B = _sizes(messages, byzantinesize, "alie", True)
        z = z_max(K, B)
    alie.last_z = float(z)
    return _affine(messages, byzantinesize, "alie", 1.0, -float(z))


def alie(messages, byzantinesize):
    """"A Little Is Enough": the last `byzantinesize` rows become ``mu - z sigma`` of the honest
    rows, per column, with ``z = z_max(K, byzantinesize)`` (ValueError when the Byzantine
    clients are no minority of the median: byzantinesize >= floor(K/2 + 1));
    ``alie.with_options(z=...)`` fixes z and skips that check.  ``alie.last_z`` holds the z
    used.  In place; fp32 or bf16, tensor or ClientPanels."""
    return _run_alie(messages, byzantinesize)


def _alie_fixed(fixed):
    z = None if fixed.get("z") is None else float(fixed["z"])
    return lambda messages, byzantinesize: _run_alie(messages, byzantinesize, z)


alie.with_options = _with_options(
    "alie", ("z",), _alie_fixed,
    """An ``attack(messages, byzantinesize)`` named "alie" with a fixed z.""")
alie.last_z = None


def _run_ipm(messages, byzantinesize, epsilon=0.1):
    return _affine(messages, byzantinesize, "ipm", -float(epsilon), 0.0)


def ipm(messages, byzantinesize):
    """Inner-product manipulation: the last `byzantinesize` rows become ``-epsilon mu`` of the
    honest rows (epsilon = 0.1; ``ipm.with_options(epsilon=...)``).  No sigma is formed, so a
    column holding +inf gives -inf.  In place; fp32 or bf16, tensor or ClientPanels."""
    return _run_ipm(messages, byzantinesize)


def _ipm_fixed(fixed):
    eps = float(fixed.get("epsilon", 0.1))
    return lambda messages, byzantinesize: _run_ipm(messages, byzantinesize, eps)


ipm.with_options = _with_options(
    "ipm", ("epsilon",), _ipm_fixed,
    """An ``attack(messages, byzantinesize)`` named "ipm" with a fixed epsilon.""")


def _dev(who: str, dev) -> int:
    if dev not in _DEVS:
        raise ValueError(f"{who}: dev must be one of {', '.join(_DEVS)} (got {dev!r})")
    return _DEVS[dev]


def _run_minmax(base, rule: int, messages, byzantinesize, dev="std"):
    who = base.__name__
    dev = _dev(who, dev)
    K, d, B = _sizes(messages, byzantinesize, who, False, 4096)
    gamma = C.c_double(0.0)
    out = _apply(messages, B, lambda ctx, X, ldx, layout, stream: ctx.call(
        "gm_attack_minmax_f32", X.data_ptr(), K, d, ldx, layout, B, rule, dev,
        C.byref(gamma), stream))
    base.last_gamma = gamma.value
    return out


def _minmax_fixed(base, rule: int):
    def make(fixed):
        dev = fixed.get("dev", "std")
        _dev(base.__name__, dev)
        return lambda messages, byzantinesize: _run_minmax(base, rule, messages, byzantinesize,
                                                           dev)
    return make


def minmax(messages, byzantinesize):
    """Min-max (Shejwalkar & Houmansadr 2021): the last `byzantinesize` rows become
    ``mu - gamma p`` with the largest gamma whose row is no further from any honest row than
    two honest rows are from each other; p = sigma (``minmax.with_options(dev=...)``: "std",
    "unit" mu / ||mu||, "sign" sign(mu)).  gamma is closed-form, computed on the device;
    ``minmax.last_gamma`` holds it.  fp32 only (TypeError), K <= 4096; in place, tensor or
    ClientPanels."""
    return _run_minmax(minmax, 0, messages, byzantinesize)


def minsum(messages, byzantinesize):
    """Min-sum (Shejwalkar & Houmansadr 2021): as ``minmax`` with the constraint that the row's
    summed squared distance to the honest rows is at most the largest such sum of an honest
    row.  ``minsum.last_gamma`` holds gamma.  fp32 only, K <= 4096."""
    return _run_minmax(minsum, 1, messages, byzantinesize)


for _base, _rule in ((minmax, 0), (minsum, 1)):
    _base.with_options = _with_options(
        _base.__name__, ("dev",), _minmax_fixed(_base, _rule),
        f'An ``attack(messages, byzantinesize)`` named "{_base.__name__}" with a fixed deviation '
        '("std", "unit" or "sign").')
minmax.last_gamma = minsum.last_gamma = None
