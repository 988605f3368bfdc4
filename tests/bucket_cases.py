"""Case builders and the numpy reference of s-bucketing (byzantine_aircomp_amd.bucketing,
csrc/bucket.hip), shared by tests/test_bucketing_cpu.py and tests/test_gpu_bucketing.py.
Importing it needs no GPU.

Reference (ref_bucket_means): the definition itself, column-vectorised in numpy.  Bucket i
holds rows perm[i*s : (i+1)*s] (the last one shorter when s does not divide K); per bucket
``acc = acc + X[perm[t]].astype(float64)`` over its rows in that order, ``/ count``,
``.astype(float32)``.  bf16 inputs are widened first (exact).

Tolerance: the kernel adds the same fp64 terms in the same order, so its sum IS the
reference's; what may differ is the fp64 division and the rounding to fp32, hence
coordinate_cases.mismatch_ulp (+-1 fp32 ulp, identical NaN / inf pattern).  Where every mean
is exactly representable (exact_matrix: small integers, s a power of two dividing K) nothing
may differ: mismatch_exact.
"""
import functools

import numpy as np

F32 = np.float32

# (K, s, d): one row group and many, s not dividing K, s == K, s > K (one bucket), every
# panel width of the inputs (K) and outputs (ceil(K/s)), d ragged against 4, 8, the panel
# widths and the 1024-column walk of the row-major output, K = 3000 beyond the panel layout
CASES = [(7, 2, 37), (50, 2, 7850), (50, 3, 70), (17, 17, 1000), (17, 40, 64), (513, 2, 333),
         (600, 3, 8200), (1000, 2, 2051), (1000, 4, 2051), (1024, 2, 4096), (2048, 2, 261),
         (3000, 3, 64)]
NO_INPUT_PANELS = {3000}          # K without a panel width: row-major input only
EXACT_CASES = [(1000, 4, 2051), (50, 2, 70)]
SPECIAL_CASE = (50, 3, 40)
GENERATOR_CASES = [(7, 2, 37), (1000, 4, 2051)]


def n_buckets(K, s):
    return -(-K // s)


def seeded_perm(K, s):
    """The seeded random assignment the tests pass as `perm` (a torch int64 vector)."""
    import torch
    return torch.randperm(K, generator=torch.Generator().manual_seed(7 * K + s))


def c3_recipe(K, d):
    """tests/test_gpu_bf16.py's inputs: honest rows N(0, 0.05^2), the last K // 5 rows
    0.25 + N(0, 0.5^2), guess N(0, 0.01^2), from torch.Generator().manual_seed(1000 + K)."""
    import torch
    g = torch.Generator().manual_seed(1000 + K)
    nb = K // 5
    X = torch.randn(K - nb, d, generator=g) * 0.05
    if nb:
        X = torch.cat([X, torch.randn(nb, d, generator=g) * 0.5 + 0.25])
    g0 = torch.randn(d, generator=g) * 0.01
    return X, g0


def ref_bucket_means(X, perm, s):
    """[ceil(K/s), d] fp32 bucket means of the fp32 matrix X under `perm` (a sequence of K
    row indices)."""
    X = np.asarray(X, dtype=F32)
    perm = np.asarray(perm, dtype=np.int64)
    K, d = X.shape
    out = np.empty((n_buckets(K, s), d), dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(out.shape[0]):
            rows = perm[i * s:min(K, (i + 1) * s)]
            acc = np.zeros(d, dtype=np.float64)
            for r in rows:
                acc = acc + X[r].astype(np.float64)
            out[i] = (acc / len(rows)).astype(F32)
    return out


def widen_bf16(X):
    """The fp32 values of X rounded to bf16 (torch's rounding), as a numpy fp32 matrix."""
    import torch
    return torch.from_numpy(np.array(X)).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=None)
def normal_matrix(K, d):
    """N(0, 1) + 0.001 j per column and 0.01 k per row: a wrong row, column or bucket
    boundary moves the mean by far more than an ulp.  Read-only."""
    rng = np.random.default_rng(100 * K + d)
    X = rng.standard_normal((K, d), dtype=F32)
    X += (0.001 * np.arange(d)).astype(F32)
    X += (0.01 * np.arange(K)).astype(F32)[:, None]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def exact_matrix(K, d):
    """x[k][j] = 64 k + j % 64: sums of up to 4 such integers and their quarters are exact in
    fp32 (and stay so after rounding the inputs to bf16)."""
    X = (64.0 * np.arange(K)[:, None] + (np.arange(d) % 64)[None, :]).astype(F32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def special_matrix():
    """(X, perm) at SPECIAL_CASE: buckets (of the seeded perm) that hold a NaN, +inf, -inf,
    both infinities, +-0, subnormals, and outliers whose fp32 sum would overflow (3e38 pairs)
    or whose order of addition decides the fp64 sum (1e30, 1, -1e30).  Built in bucket order
    (Z[t] is row perm[t]) and scattered to the clients' rows."""
    K, s, d = SPECIAL_CASE
    perm = seeded_perm(K, s).numpy()
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((K, d), dtype=F32)
    b = lambda i: slice(i * s, min(K, (i + 1) * s))            # noqa: E731
    Z[0 * s + 1, 0] = np.nan
    Z[b(0), 1] = np.nan
    Z[1 * s + 0, 2] = np.inf
    Z[1 * s + 2, 3] = -np.inf
    Z[1 * s + 0, 4] = np.inf
    Z[1 * s + 1, 4] = -np.inf                                   # inf - inf = NaN
    Z[1 * s + 0, 5] = np.inf
    Z[1 * s + 2, 5] = np.inf
    Z[b(2), 6] = [0.0, -0.0, 0.0]
    Z[b(2), 7] = -0.0
    Z[b(3), 8] = [1e-40, 2e-40, 0.0]                            # subnormal terms and mean
    Z[b(3), 9] = [1e-40, -1e-40, 1e-45]
    Z[b(3), 10] = [1.2e-38, 1e-40, -1e-39]                      # a subnormal mean of normal terms
    Z[b(4), 11] = [3e38, 3e38, 1.0]                             # the fp32 sum would be inf
    Z[b(4), 12] = 3e38
    Z[b(4), 13] = [-3e38, -3e38, -3e38]
    Z[b(5), 14] = [1e30, 1.0, -1e30]                            # 0 in this order
    Z[b(5), 15] = [1e30, -1e30, 1.0]                            # 1/3 in this one
    Z[b(5), 16] = [3e38, -3e38, 1e30]
    Z[b(6), 17] = [np.inf, 3e38, np.nan]
    last = n_buckets(K, s) - 1                                  # the short bucket: 2 rows
    Z[b(last), 18] = [3e38, 3e38]
    Z[b(last), 19] = [np.inf, 1.0]
    Z[b(last), 20] = [1e-40, 1e-45]
    Z[b(last), 21] = [np.nan, 0.0]
    Z[b(last), 39] = [-np.inf, np.inf]                          # the last column
    X = np.empty_like(Z)
    X[perm] = Z
    X.setflags(write=False)
    return X, perm


# ---------------------------------------------------------------------------- GPU operands

def input_layouts(torch, bz, X, bf16):
    """[(name, wList)] of the fp32 matrix X on the GPU in every input layout of one dtype.
    Row-major views sit in NaN-filled buffers, so a read outside the view shows.
      fp32: "rows" a view of a 16-byte-aligned buffer whose row stride is a multiple of 4
            (vector items), "scalar" a view one element into its buffer, "panels";
      bf16: "rows" 16-byte aligned with a row stride that is a multiple of 8 (vector items;
            d a multiple of 8, of 4, or neither: the ragged last group), "odd" at a 2-byte
            offset with an odd row stride (one column per item), "panels"."""
    K, d = X.shape
    dt = torch.bfloat16 if bf16 else torch.float32
    Xt = torch.from_numpy(np.array(X)).to(dt).cuda()
    g = 8 if bf16 else 4

    def view(width, off):
        buf = torch.full((K, width), float("nan"), dtype=dt, device="cuda")
        buf[:, off:off + d] = Xt
        return buf[:, off:off + d]

    a = view(d + ((-d) % g or g), 0)
    assert a.data_ptr() % 16 == 0 and a.stride(0) % g == 0
    if bf16:
        b = view(d + 3 + d % 2, 1)
        assert b.data_ptr() % 16 == 2 and b.stride(0) % 2 == 1
    else:
        b = view(d + 4, 1)
        assert b.data_ptr() % 16 == 4
    out = [("rows", a), ("odd" if bf16 else "scalar", b)]
    if K not in NO_INPUT_PANELS:
        out.append(("panels", bz.ClientPanels.from_rows(Xt)))
    return out


def raw_bits(torch, w):
    """The stored bits of a wList (tensor, view or ClientPanels) as an integer CPU tensor."""
    t = w.data if hasattr(w, "panel_stride") else w
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def means_rows(torch, out, Kb, d):
    """([Kb, d] fp32 numpy, int32 bits) of a bucketing result in either layout; for
    ClientPanels also asserts the shape and that the padding columns are still zero."""
    if hasattr(out, "panel_stride"):
        assert out.dtype == torch.float32 and tuple(out.shape) == (Kb, d), (out.dtype, out.shape)
        rem = d - (out.npan - 1) * out.W
        if out.npan and rem < out.W:
            assert torch.count_nonzero(out.data[-1, :, rem:].view(torch.int32)) == 0
        rows = out.to_rows()
    else:
        assert out.dtype == torch.float32 and tuple(out.shape) == (Kb, d), (out.dtype, out.shape)
        rows = out
    rows = rows.contiguous().cpu()
    return rows.numpy(), rows.view(torch.int32)
