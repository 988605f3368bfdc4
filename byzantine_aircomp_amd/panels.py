"""Client updates in the panel layout (GM_LAYOUT_PANELS, include/gmagg.h).

The reference hands its aggregator a fresh ``torch.stack`` of flattened client
vectors, row-major ``[K, d]`` (MNIST_Air_weight.py:206-209, M:353).  The
streaming Weiszfeld pass reads that matrix in chunks of W columns x all K rows
(DESIGN.md §3.1); in row-major order each chunk is K separate W*4-byte
segments, 4*d bytes apart.  ``ClientPanels`` stores the same K x d values as
``[ceil(d/W)][K][W]`` (W = ``gm_panel_width(K)``, 32 at 512 < K <= 1024), so
each chunk is ONE contiguous block of HBM.  It is the device-resident buffer a
training loop writes client rows into (``store``), and ``gm2`` / ``gm`` accept it
wherever they accept a ``[K, d]`` tensor; results are bit-identical to the
row-major call where both layouts run the same tile (same chunks, same reduction
order): every K outside 32 < K <= 64 and 128 < K <= 256 with d % 4 == 0, except
gm2 and noiseless AirComp gm at 512 < K <= 1024, whose row-major STEP pass runs
the 32-wave rows kernel; equal to rounding otherwise.

``ClientPanels(..., dtype=torch.bfloat16)`` stores the values as bf16 in the layout of
``gm_weiszfeld_bf16`` (W = ``gm_panel_width_bf16(K)``): half the bytes per streaming pass.
``gm2`` / ``gm`` / ``cclip`` read them widened to fp32 (exact) and return fp32, and so do
``fltrust``, ``clip`` / ``arc``, the attacks and, under ``options={"bf16": True}``, ``mean`` /
``median`` / ``trimmed_mean`` (coordinate_bf16.hip: the selections on 16-bit order keys; without
the option those three stay fp32 and raise on bf16); ``Krum``, ``meamed``, ``multi_krum``,
``bulyan``, ``nnm``, ``dnc`` and ``caf`` take fp32 panels only.  ``bucketing`` (s-bucketing,
aggregators.py) reads fp32 and bf16 panels alike and writes its fp32 bucket means as
``ClientPanels(ceil(K/s), d)``, whose panel width is that of the smaller K.
"""
from __future__ import annotations

import torch

from . import _lib

__all__ = ["ClientPanels", "panel_width"]

_DTYPES = (torch.float32, torch.bfloat16)


def panel_width(K: int, dtype=torch.float32) -> int:
    """W of the panel layout for K clients (the streaming tile's chunk width)."""
    lib = _lib.load()
    w = int((lib.gm_panel_width_bf16 if dtype == torch.bfloat16 else lib.gm_panel_width)(int(K)))
    if w <= 0:
        raise ValueError(f"no panel layout for K={K}")
    return w


class ClientPanels:
    """K client vectors of length d, stored as ``data[ceil(d/W), K, W]`` fp32 or bf16."""

    def __init__(self, K: int, d: int, device=None, W: int | None = None, dtype=torch.float32,
                 zero: bool = True):
        if dtype not in _DTYPES:
            raise TypeError(f"ClientPanels holds fp32 or bf16 (got {dtype})")
        self.K, self.d = int(K), int(d)
        self.W = int(W) if W is not None else panel_width(K, dtype)
        self.npan = -(-self.d // self.W)
        dev = torch.device(device) if device is not None else torch.device("cuda")
        # zero-filled: the last panel's columns >= d stay 0.  zero=False (a producer that
        # writes every column < d, e.g. bucketing) zeroes that padding only
        if zero:
            self.data = torch.zeros(self.npan, self.K, self.W, dtype=dtype, device=dev)
        else:
            self.data = torch.empty(self.npan, self.K, self.W, dtype=dtype, device=dev)
            if self.npan and self.d % self.W:
                self.data[-1, :, self.d % self.W:] = 0

    # -- shape / metadata, so callers can treat it like the [K, d] matrix --------
    @property
    def shape(self):
        return torch.Size((self.K, self.d))

    @property
    def device(self):
        return self.data.device

    @property
    def dtype(self):
        return self.data.dtype

    @property
    def panel_stride(self) -> int:
        return self.K * self.W

    def _full(self) -> int:
        return self.d // self.W

    # -- writing and reading rows ------------------------------------------------
    def store(self, k: int, vec: torch.Tensor):
        """Write client k's flattened vector (d floats) into its slots."""
        vec = vec.reshape(-1)
        if vec.numel() != self.d:
            raise ValueError(f"vector has {vec.numel()} elements, expected {self.d}")
        nf = self._full()
        with torch.no_grad():
            if nf:
                self.data[:nf, k, :].copy_(vec[:nf * self.W].view(nf, self.W))
            rem = self.d - nf * self.W
            if rem:
                self.data[nf, k, :rem].copy_(vec[nf * self.W:])

    def copy_rows_(self, X: torch.Tensor):
        """Fill from a row-major [K, d] matrix (any device; copied to ours)."""
        if tuple(X.shape) != (self.K, self.d):
            raise ValueError(f"rows must be [{self.K}, {self.d}] (got {tuple(X.shape)})")
        X = X.to(self.device)
        # one HIP kernel (pack.hip) instead of torch's transposed copy; into bf16 panels
        # the fp32 source is rounded to nearest even on the way (the bits of .to(bfloat16))
        pack = {(torch.float32, torch.float32): "gm_rows_to_panels_f32",
                (torch.float32, torch.bfloat16): "gm_rows_to_panels_bf16_from_f32",
                (torch.bfloat16, torch.bfloat16): "gm_rows_to_panels_bf16"}.get(
                    (X.dtype, self.dtype))
        if X.device.type == "cuda" and pack:
            from .aggregators import context, _stream_ptr, _unit_rows
            X, ldx = _unit_rows(X)
            context(X.device).call(pack, X.data_ptr(), self.K, self.d, ldx, self.data.data_ptr(),
                                   self.W, self.panel_stride, _stream_ptr(X.device))
            return self
        nf = self._full()
        with torch.no_grad():
            if nf:
                self.data[:nf].copy_(X[:, :nf * self.W].view(self.K, nf, self.W).transpose(0, 1))
            rem = self.d - nf * self.W
            if rem:
                self.data[nf, :, :rem].copy_(X[:, nf * self.W:])
        return self

    @classmethod
    def from_rows(cls, X: torch.Tensor, device=None, dtype=None) -> "ClientPanels":
        """Panels of a row-major [K, d] matrix.  dtype: X's own if that is bf16, else fp32;
        ``dtype=torch.bfloat16`` on an fp32 matrix rounds to nearest even while packing."""
        K, d = X.shape
        if dtype is None:
            dtype = torch.bfloat16 if X.dtype == torch.bfloat16 else torch.float32
        p = cls(K, d, device=device if device is not None else
                (X.device if X.device.type == "cuda" else None), dtype=dtype)
        return p.copy_rows_(X)

    def row(self, k: int) -> torch.Tensor:
        return self.data[:, k, :].reshape(-1)[: self.d]

    def to_rows(self) -> torch.Tensor:
        """The row-major [K, d] matrix (a copy)."""
        return self.data.transpose(0, 1).reshape(self.K, self.npan * self.W)[:, : self.d].contiguous()

    def mean(self, dim: int = 0) -> torch.Tensor:
        """Column mean (gm2's default guess, M:167); fp32, of the widened values for bf16."""
        if dim != 0:
            raise ValueError("ClientPanels.mean supports dim=0 only")
        return self.data.mean(dim=1, dtype=torch.float32).reshape(-1)[: self.d]
