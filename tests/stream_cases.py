"""Cases, inputs and fp64 references that pin every tile, vector width and mode of the fused
streaming pass (csrc/stream_pass_kernel.h and its instantiations, csrc/rows_pass.hip), shared by
tests/test_stream_cases_cpu.py, tests/test_gpu_stream_tiles.py and
tests/stream_variant_runner.py.  Importing it needs neither a GPU nor the library.

Tiles.  TILE_CLASSES restates host_ctx.h pick_cfg as data: per K class the (NW, LPR, R, OCC)
tile of row-major and of panel operands.  A tile is K_pad x J: lane c of a row segment holds
V columns (J = LPR V; V = 4, 2, 1 on fp32 by alignment, 8 on bf16), a wave holds QW = 64 / LPR
row groups, a block NRG = NW QW, row group rg owns rows rg + NRG i, i < R.  Row-major V = 4 INIT
passes at 128 < K <= 256 run light_cfg's wider tile (INIT_LIGHT), row-major gm2 / noiseless gm
STEP passes at 512 < K <= 1024 with V = 4 the 32-wave rows kernel (ROWS_KERNEL).

Input (tile_input).  From torch.Generator().manual_seed(5000 + K): H = K - K // 5 honest rows
0.05 * 4**(i / (H - 1)) * N(0, 1), drawn as one [H, d] tensor; K // 5 rows 0.25 + 0.5 N(0, 1);
the K rows shuffled by randperm(K); the guess 0.01 N(0, 1) (gm at d <= 7: 4 x that, see
guess_of).  Graded scales give every row a weight of its own, and with an aggregate near 0
nothing hides behind a common offset.  bf16 operands hold tile_input rounded to bf16; every
reference reads the widened values.

References, all in fp64 on the fp32 (or widened bf16) inputs, for a fixed number n of loop
bodies (the GPU calls pass tol = -1, so they run exactly n):
  gm2    dist_k = max(eps, ||x_k - g||), g' = sum_k x_k / dist_k / sum_k 1 / dist_k, eps the
         fp32 value of 1e-4 (M:174-181).
  gm     the restatement of test_gm_philox_matches_restatement (oracle.aggregators.gm, M:131-160)
         on the Philox draws of oracle/philox.py, the channel draws rounded to fp32 as gm_draws
         hands them over:  s = sqrt(mean g^2), p_k = (||x_k||^2 + s^2) / (dist_k^2 (d + 1) |h_k|^2),
         gain_k = sqrt(P_max / max(p_k, 500 s^2)), y_d = s sum_k gain_k / dist_k + n_d,
         g' = sum_k c_k x_k + a n,  c_k = gain_k / dist_k * s / y_d,  a = s / y_d.
  cclip  tests/cclip_cases.py's recurrence, v' = sum_k c_k x_k + a v with c_k = lambda_k / K,
         a = 1 - sum_k c_k; tau is the median distance to the guess, so about half the rows clip.
         (test_stream_cases_cpu.py holds this module's engine to cclip_cases.reference and to
         oracle.gm2 at 1e-12.)
Each body also yields scale_j = sum_k |c_k x_kj|, + |a v_j| for cclip; gm's channel noise adds
nothing to it (its hardware sine and cosine err by a few u of |a| sd, which the bar's share for
the coefficients takes in: the noise term is of the size of scale_j or below on these inputs).
The passes walk the columns in blocks of cclip_cases.BLOCK, so the multi-chunk cases fit in host
memory.

Bar.  Per element, |got_j - ref_j| <= eps_tile * scale_j, with u = 2^-24 and to first order:
  * phase A sums sum_k c_k x_kj in fp32: a product passes through at most R fused
    multiply-adds in its thread, log2(QW) shuffle adds across the wave's row groups and NW
    adds across the waves, so |error| <= (R + log2 QW + NW) u scale_j.  Centered clipping sums
    in fp64 and rounds once: 1 u.  Across chunks and blocks nothing is summed per column.
  * the coefficients.  D_k is summed in fp32 inside a chunk (a rounded difference, squared:
    2 u; V fused multiply-adds, on bf16 V / 2 + 1; log2 LPR adds across the lanes of the row
    segment) and in fp64 across chunks and blocks (2^-53 per add: nothing): at most
    (2 + V + log2 LPR) u <= 14 u on D_k, 7 u on dist_k.  The K-space step is fp64 and rounds c_k
    to fp32 (1 u; gm twice), and c_k is a quotient by a weighted mean of the same dist_k:
    <= 2 * 7 + 1 = 15 u for gm2 and cclip.  gm adds its fp32 s, threshold and |h_k|^2 (4 u) and the
    fast sine / cosine of the channel draw (|h_k|^2 to ~1e-6, 8 u on c_k): <= 29 u.
  * n > 1: the distances are taken to the kernel's own rounded iterate.  Its error e_j is of
    random sign, so it moves dist_k by (x_k - g) . e / dist_k ~ |e_j|, a relative 1 / sqrt(d)
    of what it is itself: no term of its own.
  eps_tile = (A + 32) u with A = R + log2 QW + NW of the STEP tile (1 for cclip) and 32 the
  next power of two above 29: between 33 u = 2.0e-6 and 64 u = 2^-18 = 3.8e-6, under the
  project's 1e-5 (MAX_EPS).  An fp32 numpy restatement that sums the rows in another order and
  the columns in 32-column stages stays within it (test_stream_cases_cpu.py); every mutation
  below misses it by 8x or more.

Row probes.  Guess x_r + 1e-2 u (u a unit vector), rounded to fp32 — the reference reads the
rounded guess — and n = 1: row r then carries most of the weight, so an error in that one row's
INIT distance reaches the output.  x_rj - g_j is exact in fp32 (the operands are within a factor
of two of each other, or the difference is one rounding of a value below 2^-12), and D_r is a
sum of squares: no cancellation, the bound on D_k above holds for D_r, and the probes' bar is
eps_tile again (PROBE_EPS = the same function).

Mutations (MUTATIONS): the reference computed wrongly on purpose, as a broken tile would:
  a  the last row dropped: absent from the distances, the coefficients and the sums (a row
     count one short).  A padding-row mask one row short reads the row as zeros instead, which
     still enters the normaliser at distance ||g|| and moves the result more.
  b  the last row read as its neighbour
  c  row r's distances missing its last 16 columns, d // 2 where d < 32 (r =
     distance_rows(...)[0]: row 0 for gm2, for gm and cclip a row whose coefficient depends on
     its distance)
  d  from the second body on, the distances taken to the previous iterate
  e  the last d % 4 columns (bf16: d % 8) of every row read as 0
"""
import math

import numpy as np
import torch

import cclip_cases as cc

U = 2.0 ** -24
MAX_EPS = 1e-5               # the project's bar; eps_tile stays below it
COEF_ULPS = 32               # the coefficients' share of the bar (derived above)
EPS_CLAMP = float(np.float32(1e-4))
BLOCK = cc.BLOCK
NS = (1, 2, 3)
GM_SEED = 4242
GM_NOISE_VAR = 1e-3
CCLIP_ITERS = (1, 3)
OMA_VAR, OMA_SEED = 1e-2, 77

# (K_lo, K_hi, rows (NW, LPR, R, OCC), panels (NW, LPR, R, OCC)): host_ctx.h pick_cfg
TILE_CLASSES = (
    (1, 16, (16, 64, 1, 1), (16, 64, 1, 1)),
    (17, 32, (16, 64, 2, 1), (16, 64, 2, 1)),
    (33, 64, (16, 64, 4, 1), (8, 32, 4, 1)),
    (65, 128, (16, 64, 8, 1), (16, 64, 8, 1)),
    (129, 256, (16, 32, 8, 1), (16, 16, 4, 1)),
    (257, 512, (16, 16, 8, 1), (16, 16, 8, 1)),
    (513, 1024, (8, 8, 16, 2), (8, 8, 16, 2)),
    (1025, 2048, (16, 4, 8, 1), (16, 4, 8, 1)),
)
INIT_LIGHT = (129, 256, (16, 64, 16, 1))      # light_cfg: row-major V = 4 INIT passes
ROWS_KERNEL = (513, 1024, (16, 8, 8, 2))      # rows_pass.hip: V = 4 gm2 / noiseless gm STEP
K_MAX = TILE_CLASSES[-1][1]

EDGE_K = [16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048]
MULTI_K = [16, 32, 50, 100, 200, 300, 513, 1500]          # one K per class
PROBE_K = [17, 129, 1000, 2048]
ROWS_KERNEL_K = [513, 1024]
CPU_K = [17, 129, 1000, 2048]


def tile(K, panels):
    """The STEP tile (NW, LPR, R, OCC) of K rows."""
    for lo, hi, rows, pan in TILE_CLASSES:
        if lo <= K <= hi:
            return pan if panels else rows
    raise ValueError(f"no streaming tile for K = {K}")


def nrg(t):
    return t[0] * (64 // t[1])


def covers(t):
    """Rows a tile holds."""
    return nrg(t) * t[2]


def chunk(K, panels, V):
    """J, the chunk width in columns."""
    return tile(K, panels)[1] * V


def same_tile(K):
    """Whether rows (V = 4) and panels run one tile (the docstring of test_gpu_panels.py)."""
    return tile(K, False) == tile(K, True) and not INIT_LIGHT[0] <= K <= INIT_LIGHT[1]


def takes_rows_kernel(K, agg):
    return ROWS_KERNEL[0] <= K <= ROWS_KERNEL[1] and agg in ("gm2", "gm")


def tiles_of(K, op, agg):
    """Every tile an operand's passes run on: [STEP, INIT, ...]."""
    out = [tile(K, OPERANDS[op][1])]
    if op in ("rows4", "padded"):
        if INIT_LIGHT[0] <= K <= INIT_LIGHT[1]:
            out.append(INIT_LIGHT[2])
        if takes_rows_kernel(K, agg):
            out.insert(0, ROWS_KERNEL[2])
    return out


def eps_tile(K, op, agg):
    """The per-element bar of one case, in units of scale_j (derived in the docstring)."""
    if agg.startswith("cclip"):
        a = 1
    else:
        nw, lpr, r, _ = tiles_of(K, op, agg)[0]
        a = r + int(math.log2(64 // lpr)) + nw
    e = (a + COEF_ULPS) * U
    assert e <= MAX_EPS
    return e


PROBE_EPS = eps_tile


def probe_rows(K, op, agg="gm2"):
    """Rows 0, NRG - 1, NRG and K - 1 of every tile the operand's passes run on."""
    rows = {0, K - 1}
    for t in tiles_of(K, op, agg):
        rows |= {r for r in (nrg(t) - 1, nrg(t)) if r < K}
    return sorted(rows)


# ------------------------------------------------------------------------------- operands

# name -> (bf16, panels, V, (modulus, residue) of d)
OPERANDS = {
    "rows4": (False, False, 4, (4, 0)),        # contiguous, d % 4 == 0
    "rows2": (False, False, 2, (4, 2)),
    "rows1": (False, False, 1, (2, 1)),
    "misaligned": (False, False, 1, (2, 1)),   # 4 bytes into its buffer, ldx = d + 4
    "padded": (False, False, 4, (4, 0)),       # aligned, ldx = d + 4
    "panels": (False, True, 4, (4, 0)),
    "panels_odd": (False, True, 4, (2, 1)),    # a ragged last float4 group
    "bf16_rows": (True, False, 8, (8, 0)),
    "bf16_panels": (True, True, 8, (8, 0)),
    "bf16_panels_odd": (True, True, 8, (2, 1)),
}
BIT_EQUAL = ("rows4", "padded", "panels")      # one d, one tile where same_tile(K)


def _fit(d, mod, res, below=None):
    """The largest d' <= d (and < below) with d' % mod == res, at least the smallest such."""
    if below is not None:
        d = min(d, below - 1)
    while d % mod != res:
        d -= 1
    return d if d > 0 else (res or mod)


def small_ds(K, op):
    """(one partial chunk, two full chunks and a ragged tail) for an operand: J / 2 + 4 and
    2 J + J / 2 + 4 columns, brought to the operand's residue."""
    bf16, panels, V, (mod, res) = OPERANDS[op]
    J = chunk(K, panels, V)
    return _fit(J // 2 + 4, mod, res, below=J), _fit(2 * J + J // 2 + 4, mod, res, below=3 * J)


MULTI_OPS = ("rows4", "panels", "bf16_panels")
MULTI_GROUPS = {"fp32": ("rows4", "panels"), "bf16": ("bf16_panels",)}   # one d per group


def multi_chunks(K, op, num_cu):
    """Chunks that give every block of operand `op` at least 3: 3 CUs 32 / NW + 1, 32 / NW being
    the hardware limit on resident blocks of NW waves per CU (the grid is at most that)."""
    return 3 * num_cu * (32 // tile(K, OPERANDS[op][1])[0]) + 1


def multi_d(K, op, num_cu):
    """Columns of the multi-chunk case of an operand of MULTI_OPS: J multi_chunks of its own
    J = LPR V (V = 8 on bf16), + a ragged tail of 20 columns.  rows4 and panels, compared bit
    for bit, share the larger of their two."""
    group = next(g for g in MULTI_GROUPS.values() if op in g)
    return max(chunk(K, OPERANDS[o][1], OPERANDS[o][2]) * multi_chunks(K, o, num_cu)
               for o in group) + 20


# --------------------------------------------------------------------------------- inputs

_INPUTS = {}


def tile_input(K, d):
    """(X [K, d], guess [d]) fp32 CPU tensors; cached, never modified."""
    if (K, d) not in _INPUTS:
        g = torch.Generator().manual_seed(5000 + K)
        nb = K // 5
        H = K - nb
        grade = 0.05 * 4.0 ** (torch.arange(H, dtype=torch.float64) / max(H - 1, 1))
        X = torch.randn(H, d, generator=g) * grade.float()[:, None]
        if nb:
            X = torch.cat([X, 0.25 + 0.5 * torch.randn(nb, d, generator=g)])
        X = X[torch.randperm(K, generator=g)].contiguous()
        g0 = 0.01 * torch.randn(d, generator=g)
        if K * d > 1 << 22:
            return X, g0                       # (the large cases are used once)
        _INPUTS[(K, d)] = (X, g0)
    return _INPUTS[(K, d)]


def widen_bf16(X):
    """The fp32 tensor of X's values rounded to bf16 (bucket_cases.widen_bf16's rounding)."""
    return X.to(torch.bfloat16).float()


def operand_input(K, d, bf16):
    X, g0 = tile_input(K, d)
    return (widen_bf16(X) if bf16 else X), g0


GM_SMALL_D, GM_SMALL_D_GUESS = 7, 4.0


def guess_of(K, d, agg):
    """The guess of one case: tile_input's, except for gm at d <= 7, where it is 4 x that.
    gm's c_k depends on dist_k only where client k's power p_k ~ 1 / ((d + 1) |h_k|^2) sits
    below the threshold 500 s^2, s the guess's rms: with s = 0.01 and d + 1 <= 8 entries per
    message hardly any client does, and no output could show a wrong distance.  s = 0.04 puts
    most clients there."""
    g0 = tile_input(K, d)[1]
    return g0 * GM_SMALL_D_GUESS if agg in ("gm", "gm_noise") and d <= GM_SMALL_D else g0


def probe_guess(X, r):
    """x_r + 1e-2 u, rounded to fp32; u a unit vector from manual_seed(9000 + r)."""
    u = torch.randn(X.shape[1], generator=torch.Generator().manual_seed(9000 + r),
                    dtype=torch.float64)
    return (X[r].double() + 1e-2 * u / u.norm()).float()


# ------------------------------------------------------------------------ the fp64 engine

class Mut:
    """How a (broken) tile reads the matrix.  seen(X): the matrix it sees; short: (row,
    columns dropped from that row's distances); stale: distances to the previous iterate."""

    def __init__(self, name=None, row=0):
        self.name, self.row = name, row
        self.stale = name == "d"

    def seen(self, X, bf16):
        if self.name not in ("a", "b", "e"):
            return X
        if self.name == "a":
            return X[:-1]
        X = X.clone()
        if self.name == "b":
            X[-1] = X[-2]
        else:
            tail = X.shape[1] % (8 if bf16 else 4)
            if tail:
                X[:, -tail:] = 0
        return X

    def short(self, d):
        return (self.row, min(16, d // 2)) if self.name == "c" else None


MUTATIONS = ("a", "b", "c", "d", "e")
NONE = Mut()


def _sqdist(X, g, short=None):
    """(||x_k - g||^2, ||x_k||^2) in fp64, X fp32 widened block by block."""
    K, d = X.shape
    D = torch.zeros(K, dtype=torch.float64)
    R = torch.zeros(K, dtype=torch.float64)
    for j in range(0, d, BLOCK):
        Xb = X[:, j:j + BLOCK].double()
        diff = Xb - g[j:j + BLOCK]
        sq = diff * diff
        if short is not None and j + sq.shape[1] > d - short[1]:
            sq[short[0], max(0, d - short[1] - j):] = 0
        D += sq.sum(dim=1)
        R += (Xb * Xb).sum(dim=1)
    return D, R


def _wsum(X, c):
    """(sum_k c_k x_kj, sum_k |c_k x_kj|) in fp64."""
    d = X.shape[1]
    s = torch.empty(d, dtype=torch.float64)
    a = torch.empty(d, dtype=torch.float64)
    ca = c.abs()
    for j in range(0, d, BLOCK):
        Xb = X[:, j:j + BLOCK].double()
        s[j:j + BLOCK] = c @ Xb
        a[j:j + BLOCK] = ca @ Xb.abs()
    return s, a


def _gm_draws(seed, it, K, d):
    """Iteration `it`'s Philox draws (oracle/philox.py gm_draws): |h_k|^2 in fp32 from the channel
    draws rounded to fp32, and the d + 1 standard normals of the noise."""
    from oracle import philox as ph
    h = ph.normal4(seed, ph.STREAM_CHANNEL, np.uint64(it), np.arange(K, dtype=np.uint64))
    hr = (h[:, 0] / math.sqrt(2)).astype(np.float32)
    hi = (h[:, 1] / math.sqrt(2)).astype(np.float32)
    h2 = (hr * hr + hi * hi).astype(np.float64)           # fp32, as the oracle and the kernel
    idx = np.arange(d + 1, dtype=np.uint64)
    z4 = ph.normal4(seed, ph.STREAM_NOISE, np.uint64(it), idx >> np.uint64(2))      # [d + 1, 4]
    e = (idx & np.uint64(3)).astype(np.int64)
    z = np.take_along_axis(z4, e[:, None], axis=1)[:, 0]
    return torch.from_numpy(h2), torch.from_numpy(z)


def engine(X, g0, n, rule, mut=NONE, bf16=False, noise_var=None, tau=None, seed=GM_SEED,
           P_max=1.0, trace=None):
    """n bodies of `rule` ("gm2", "gm", "cclip") in fp64 on the fp32 tensor X [K, d] from the
    fp32 guess g0.  Returns [(iterate, scale)] per body, fp64 numpy arrays.  trace (a dict):
    gets "rows", the rows whose coefficient depends on their distance in the first body."""
    X = mut.seen(X, bf16)
    K, d = X.shape
    g = g0.double()
    prev = g
    out = []
    for it in range(n):
        D, R = _sqdist(X, prev if (mut.stale and it > 0) else g, mut.short(d))
        if rule == "cclip":
            dist = D.sqrt()
            lam = torch.where(dist > tau, tau / dist, torch.ones_like(dist))
            c = lam / K
            if trace is not None and it == 0:
                trace["rows"] = [int(dist.argmax())]
            a = 1.0 - float(c.sum())
            s, sa = _wsum(X, c)
            new, scale = s + a * g, sa + abs(a) * g.abs()
        elif rule == "gm2":
            w = 1.0 / D.sqrt().clamp(min=EPS_CLAMP)
            c = w / w.sum()
            new, scale = _wsum(X, c)
        else:
            dist = D.sqrt().clamp(min=EPS_CLAMP)
            sc = float((g * g).mean().sqrt())
            h2, z = _gm_draws(seed, it, K, d)
            p = (R + sc * sc) / (dist * dist * (d + 1)) / h2
            gain = (P_max / p.clamp(min=500.0 * sc * sc)).sqrt()
            if trace is not None and it == 0:
                # first the rows that stay below the threshold with a distance^2 halved, those
                # whose last columns hold the largest share of their distance leading
                thr, nc = 500.0 * sc * sc, min(16, d // 2)
                tail = X[:, d - nc:].double() - g[d - nc:]
                share = (tail * tail).sum(dim=1) / D
                order = torch.argsort(share - (p >= thr / 2).double(), descending=True)
                trace["rows"] = [int(k) for k in order if p[k] < thr]
            ck = gain / dist
            sd = math.sqrt(noise_var / 2.0) if noise_var is not None else 0.0
            yd = sc * float(ck.sum()) + sd * float(z[d])
            c = ck * (sc / yd)
            new, scale = _wsum(X, c)
            if noise_var is not None:
                new = new + (sc / yd * sd) * z[:d]
        prev, g = g, new
        out.append((new.numpy(), scale.numpy()))
    return out


def distance_rows(K, d, bf16, agg):
    """The rows mutation (c) may take, the first being the one it does: rows whose coefficient
    depends on their distance in the first body.  gm2: every row.  gm: the rows whose power p_k
    sits at the threshold 500 s^2 (above it gain_k is proportional to dist_k and
    c_k = gain_k / dist_k is not), first the one with room below it whose last columns hold
    the largest share of its distance.  cclip: the farthest row (inside the radius c_k = 1 / K, and
    just outside it the clipping hardly bites)."""
    if agg == "gm2":
        return list(range(K))
    X, g0 = operand_input(K, d, bf16)[0], guess_of(K, d, agg)
    tr = {}
    if agg == "cclip":
        engine(X, g0, 1, "cclip", tau=cclip_tau(X, g0), trace=tr)
    else:
        engine(X, g0, 1, "gm", trace=tr)
    return tr["rows"]


def cclip_tau(X, g0):
    """The median fp64 distance to the guess."""
    return float(_sqdist(X, g0.double())[0].sqrt().median())


_TAUS = {}


def tau_of(K, d, bf16):
    """cclip's radius for tile_input(K, d): cclip_tau of the operand's values (cached)."""
    if (K, d, bf16) not in _TAUS:
        _TAUS[(K, d, bf16)] = cclip_tau(*operand_input(K, d, bf16))
    return _TAUS[(K, d, bf16)]


_REFS = {}


def reference(K, d, bf16, agg, guess=None, mut=NONE, key=None):
    """[(iterate, scale)] for bodies 1 .. 3 of aggregator `agg` ("gm2", "gm", "gm_noise",
    "cclip") on tile_input(K, d) (rounded to bf16 and widened where bf16); cached unless a
    guess or a mutation is given."""
    k = key or (K, d, bf16, agg)
    cached = guess is None and mut is NONE and K * d <= 1 << 22
    if cached and k in _REFS:
        return _REFS[k]
    X = operand_input(K, d, bf16)[0]
    g0 = guess_of(K, d, agg) if guess is None else guess
    n = max(NS)
    if agg == "gm2":
        r = engine(X, g0, n, "gm2", mut, bf16)
    elif agg == "gm":
        r = engine(X, g0, n, "gm", mut, bf16)
    elif agg == "gm_noise":
        r = engine(X, g0, n, "gm", mut, bf16, noise_var=GM_NOISE_VAR)
    elif agg == "cclip":
        r = engine(X, g0, max(CCLIP_ITERS), "cclip", mut, bf16, tau=tau_of(K, d, bf16))
    else:
        raise ValueError(agg)
    if cached:
        _REFS[k] = r
    return r


def worst_ratio(got, ref, scale, eps):
    """max_j |got_j - ref_j| / (eps scale_j), got an fp32 array."""
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / (eps * scale)))


def restate_gm2_f32(X, g0, n, seed=1):
    """gm2 in fp32 numpy, summed otherwise than the tile does: the rows in a random order, one
    after the other, and the squared distances in 32-column stages; fp64 only where the
    kernels have it (across stages, the K-space step).  [iterate] per body."""
    X = X.numpy()
    K, d = X.shape
    order = np.random.default_rng(seed).permutation(K)
    g = g0.numpy().astype(np.float32)
    out = []
    for _ in range(n):
        D = np.zeros(K)
        for j in range(0, d, 32):
            diff = X[:, j:j + 32] - g[j:j + 32]
            D += np.add.reduce(diff * diff, axis=1, dtype=np.float32)
        w = 1.0 / np.maximum(np.sqrt(D), EPS_CLAMP).astype(np.float32).astype(np.float64)
        c = (w / w.sum()).astype(np.float32)
        acc = np.zeros(d, dtype=np.float32)
        for k in order:
            acc = (acc + c[k] * X[k]).astype(np.float32)
        g = acc
        out.append(g)
    return out
