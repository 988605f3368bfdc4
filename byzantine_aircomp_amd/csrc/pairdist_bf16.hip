// The squared pair distances of bf16 client updates on the bf16 matrix cores (the "MFMA tier"
// of gm_krum_bf16 / gm_multi_krum_bf16 / gm_nnm_bf16 / gm_pair_dist_bf16), and the host side of
// those entry points on both tiers.  The exact tier is coordinate.hip's pair_dist on widened
// elements; this file adds
//   gram_bf16     the upper tile triangle of G = X X^T, v_mfma_f32_32x32x16_bf16, per column
//                 slice an fp64 partial [S][K][K]
//   gram_diag     rho_i = G_ii (the slices summed in slice order); raises *flag when one is not
//                 finite
//   gram_finish   D~_ij = max(0, rho_i + rho_j - 2 G_ij) for i < j, D~_ii = 0, into the buffer
//                 launch_krum_dist writes (upper triangle, fp64)
// after which krum_score, score_top_m, nnm_neighbors and the closing passes run unchanged.
//
// gram_bf16.  A block of 4 waves owns one 128 x 128 tile pair (bi <= bj, pair_dist's numbering)
// over one column slice; wave (wr, wc) a 64 x 64 quarter as 2 x 2 MFMA tiles.  A bf16 x bf16
// product is exact in fp32, so G needs no centring, scaling or split; and G = X X^T needs no
// transposition: lane l's A fragment is A[row l & 31][k = 8 (l >> 5) + 0..7] and its B fragment
// B[k = 8 (l >> 5) + 0..7][col l & 31], both "8 consecutive columns of one row of X".  So both
// row tiles are staged in LDS as they lie in memory (64 columns per stage, 16-byte loads, the
// next stage's loads in registers during this stage's MFMAs) and a fragment is one
// ds_read_b128.  LDS rows are 144 bytes apart (128 + 16): the 16 rows a quarter-wave reads
// start in 16 different 4-bank groups.  Rows >= K and columns >= d are staged as zeros.
// The fp32 accumulators are added into fp64 and cleared every C = kMfmaFlush = 256 columns.
//
// Same order for every tile: the slices, the stage and flush boundaries (multiples of 64 and of
// C from column 0: a slice is a multiple of C wide) and the order of the MFMAs depend on (K, d)
// only, never on the tile or on a row's position in it.  An entry G_ij is a function of rows i
// and j alone, so bit-identical rows get bit-identical G entries: D~ is exactly 0 between them
// and exactly equal towards third rows, and the consumers' ties-to-lower-index rule decides.
// Partials are summed in slice order by one thread: no atomics, the same bits on every run.
//
// The bound.  Let u = 2^-23 bound the relative error of one fp32 accumulation of the MFMA,
// whether the hardware rounds to nearest or truncates.  One flush interval adds C exact
// products into an fp32 accumulator in C / 16 instructions; counting one rounding per product
// and one per instruction, in any order, the interval's sum is off by at most
// (C + C / 16) u sum_c |x_ic x_jc|.  The fp64 additions across intervals and slices and the
// finish (relative 2^-53 each) are covered by the slack in u.  Over all columns
//   |G~_ij - G_ij| <= (17 / 16) C u sum_c |x_ic x_jc| <= (17 / 32) C u (rho_i + rho_j),
//   |G~_ii - rho_i| <= (17 / 16) C u rho_i,
// hence |D~_ij - D_ij| <= |dG_ii| + |dG_jj| + 2 |dG_ij| <= (17 / 8) C u (rho_i + rho_j); the
// clamp at 0 only moves D~ towards D >= 0.  With C = 256: beta = 544 * 2^-23 = 6.49e-5 <=
// 2^-13 = 1.22e-4 (C = 512 would miss it).  pairdist_mfma_beta() is what the library reports.
//
// Re-reads.  A row tile is read by ceil(K / 128) tile pairs.  Blocks are numbered as nnm_mix
// numbers its sweeps: the tile pairs of one column slice are consecutive on ONE XCD
// (workgroups go round-robin over the 8 XCDs), so a slice's rows come from HBM about once per
// XCD that works on it and otherwise from that XCD's L2.
//
// Non-finite inputs.  A NaN, an infinity or a square that overflows fp32 makes its G_ii
// non-finite, and then G cannot honour the semantics for excluded rows.  gram_diag raises a
// device flag; the exact tier's pair_dist / pair_reduce launches that follow are enqueued
// always and return at once while the flag is down ("later launches are no-ops").  No host
// synchronisation; the result is then the exact tier's, bit for bit.
#include <algorithm>

#include "device_util.h"
#include "host_ctx.h"
#include "select_util.h"

namespace gmk {

namespace {

constexpr int kGT = 128;            // tile edge (rows)
constexpr int kGK = 64;             // columns per LDS stage
constexpr int kGP = kGK + 8;        // LDS row stride in elements (144 bytes)
constexpr int kGThreads = 256;
constexpr int kGLoads = 2 * kGT * (kGK / 8) / kGThreads;   // 16-byte groups per thread and stage
static_assert(kMfmaFlush % kGK == 0, "a flush interval is whole stages");

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(kGThreads)
gram_bf16(const uint16_t* __restrict__ X, int64_t K, int64_t d, int64_t ldx, int ws,
          int64_t chunk, int64_t pairs, int64_t nblk, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint16_t sT[2][kGT][kGP];
  const int64_t per = gridDim.x / 8;                   // (the grid is a multiple of 8)
  const int64_t L = ((int64_t)blockIdx.x % 8) * per + (int64_t)blockIdx.x / 8;
  if (L >= nblk) return;                               // (block-uniform)
  const int64_t slice = L / pairs;
  const int64_t nT = (K + kGT - 1) / kGT;
  int64_t p = L - slice * pairs, bi = 0;
  while (p >= nT - bi) { p -= nT - bi; ++bi; }
  const int64_t bj = bi + p;
  const int64_t cb = slice * chunk, ce = cb + chunk < d ? cb + chunk : d;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;

  f16v acc[2][2];
  double accd[2][2][16];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[a][b][r] = 0.f;
        accd[a][b][r] = 0.0;
      }

  // stage loads: group q of the thread is (tile t, row r, columns 8 cg .. 8 cg + 7)
  u4 pre[kGLoads];
  auto load_stage = [&](int64_t c0) {
#pragma unroll
    for (int q = 0; q < kGLoads; ++q) {
      const int idx = threadIdx.x + kGThreads * q;
      const int t = idx >> 10, r = (idx >> 3) & (kGT - 1), cg = idx & 7;
      const int64_t row = (t ? bj : bi) * kGT + r, col = c0 + 8 * cg;
      u4 v = {0u, 0u, 0u, 0u};
      if (row < K && col < ce) {
        const uint16_t* src = elem(X, ldx, ws, row, col);
        if (col + 8 <= ce) {
          v = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src));
        } else {                                       // the last group of the matrix: d % 8 columns
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const uint32_t h = col + u < ce ? (uint32_t)src[u] : 0u;
            v[u >> 1] |= h << (16 * (u & 1));
          }
        }
      }
      pre[q] = v;
    }
  };
  auto flush = [&]() {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          accd[a][b][r] += (double)acc[a][b][r];
          acc[a][b][r] = 0.f;
        }
  };

  if (cb < ce) load_stage(cb);
  int since = 0;                                       // stages since the last flush
  for (int64_t c0 = cb; c0 < ce; c0 += kGK) {
    __syncthreads();                                   // the previous stage's reads are done
#pragma unroll
    for (int q = 0; q < kGLoads; ++q) {
      const int idx = threadIdx.x + kGThreads * q;
      const int t = idx >> 10, r = (idx >> 3) & (kGT - 1), cg = idx & 7;
      *reinterpret_cast<u4*>(&sT[t][r][8 * cg]) = pre[q];
    }
    __syncthreads();
    if (c0 + kGK < ce) load_stage(c0 + kGK);
#pragma unroll
    for (int ks = 0; ks < kGK / 16; ++ks) {
      const int ko = ks * 16 + 8 * (lane >> 5);
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        fa[a] = *reinterpret_cast<const bf16x8*>(&sT[0][wr * 64 + a * 32 + (lane & 31)][ko]);
        fb[a] = *reinterpret_cast<const bf16x8*>(&sT[1][wc * 64 + a * 32 + (lane & 31)][ko]);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    if (++since == kMfmaFlush / kGK) {
      flush();
      since = 0;
    }
  }
  if (since) flush();

  // C layout of the 32 x 32 tile: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  double* P = part + slice * K * K;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int64_t j = bj * kGT + wc * 64 + b * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t i = bi * kGT + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (i < K && j < K) P[i * K + j] = accd[a][b][r];
      }
    }
}

__global__ void __launch_bounds__(256) gram_diag(const double* __restrict__ part, int64_t S,
                                                 int64_t K, double* __restrict__ rho,
                                                 int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  double g = 0.0;
  for (int64_t t = 0; t < S; ++t) g += part[(t * K + i) * K + i];
  rho[i] = g;
  if (!(fabs(g) <= 1.7976931348623157e308)) *flag = 1;      // NaN or an infinity
}

__global__ void __launch_bounds__(256) gram_finish(const double* __restrict__ part, int64_t S,
                                                   int64_t K, const double* __restrict__ rho,
                                                   double* __restrict__ D) {
  const int64_t n = K * K;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int64_t i = e / K, j = e - i * K;
  if (i > j) return;
  if (i == j) {
    D[e] = 0.0;
    return;
  }
  double g = 0.0;
  for (int64_t t = 0; t < S; ++t) g += part[t * n + e];
  D[e] = fmax(0.0, (rho[i] + rho[j]) - 2.0 * g);
}

__global__ void __launch_bounds__(256) mirror_upper(double* __restrict__ D, int64_t K) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K * K) return;
  const int64_t i = e / K, j = e - i * K;
  if (i > j) D[e] = D[j * K + i];
}

// The slices: enough blocks for two per CU (what the registers and the LDS allow), partials
// <= 512 MiB, a slice a multiple of C wide (so every flush boundary is a multiple of C).
void mfma_slicing(int64_t K, int64_t d, int num_cu, int64_t* S, int64_t* chunk) {
  const int64_t nT = (K + kGT - 1) / kGT, pairs = nT * (nT + 1) / 2;
  int64_t s = std::max<int64_t>(1, 2 * (int64_t)num_cu / pairs);
  s = std::min(s, std::max<int64_t>(1, (int64_t)(512ull << 20) / (8 * K * K)));
  s = std::min(s, std::max<int64_t>(1, (d + kMfmaFlush - 1) / kMfmaFlush));
  *chunk = std::max<int64_t>(1, ((d + s - 1) / s + kMfmaFlush - 1) / kMfmaFlush) * kMfmaFlush;
  *S = std::max<int64_t>(1, (d + *chunk - 1) / *chunk);
}

}  // namespace

double pairdist_mfma_beta() { return 17.0 / 8.0 * kMfmaFlush * 1.1920928955078125e-07; }

int64_t pairdist_mfma_slices(int64_t K, int64_t d, int num_cu) {
  int64_t S, chunk;
  mfma_slicing(K, d, num_cu, &S, &chunk);
  return S;
}

hipError_t launch_pairdist_mfma(const uint16_t* X, int64_t K, int64_t d, int64_t ldx, int ws,
                                int num_cu, double* part, double* rho, double* D, int* flag,
                                hipStream_t s) {
  if (K < 1 || K > 4096 || d < 1) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(X) % 16 != 0 || ldx % 8 != 0 || (ws && ws < 3))
    return hipErrorInvalidValue;
  int64_t S, chunk;
  mfma_slicing(K, d, num_cu, &S, &chunk);
  const int64_t nT = (K + kGT - 1) / kGT, pairs = nT * (nT + 1) / 2, nblk = pairs * S;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gram_bf16, dim3((unsigned)((nblk + 7) / 8 * 8)), dim3(kGThreads), 0, s, X, K,
                     d, ldx, ws, chunk, pairs, nblk, part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gram_diag, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, part, S, K,
                     rho, flag);
  hipLaunchKernelGGL(gram_finish, dim3((unsigned)((K * K + 255) / 256)), dim3(256), 0, s, part, S,
                     K, rho, D);
  return hipGetLastError();
}

hipError_t launch_mirror_upper(double* D, int64_t K, hipStream_t s) {
  hipLaunchKernelGGL(mirror_upper, dim3((unsigned)((K * K + 255) / 256)), dim3(256), 0, s, D, K);
  return hipGetLastError();
}

}  // namespace gmk

// ---- the host side --------------------------------------------------------------------------

using namespace gmh;

namespace {

// The panel shift of a validated bf16 (or, f32 = true, fp32) operand; 0 for rows.
int layout_shift(const char* fn, int64_t K, int64_t d, int64_t ld, int32_t layout, bool f32,
                 int* ws) {
  *ws = 0;
  if (layout == GM_LAYOUT_ROWS) {
    if (ld < d) return fail(GM_ERR_INVALID, "%s: ld = %lld < d = %lld", fn, (long long)ld, (long long)d);
    return GM_OK;
  }
  const int64_t W = f32 ? gm_panel_width(K) : gm_panel_width_bf16(K);
  if (W == 0)
    return fail(GM_ERR_UNSUPPORTED, "%s: no panel layout for K = %lld rows (pass them row-major)",
                fn, (long long)K);
  if (ld < K * W)
    return fail(GM_ERR_INVALID, "%s: panel stride %lld < K * W = %lld", fn, (long long)ld,
                (long long)(K * W));
  *ws = wshift_of(W);
  return GM_OK;
}

bool known(int32_t l) { return l == GM_LAYOUT_ROWS || l == GM_LAYOUT_PANELS; }
bool known_mode(int32_t m) { return m == GM_DIST_EXACT || m == GM_DIST_MFMA; }

// The checks every entry shares after its own argument checks; *done: d == 0, nothing to do.
int common_checks(const char* fn, gm_ctx* c, int64_t K, int64_t d, bool* done) {
  *done = false;
  if (K > 4096) return fail(GM_ERR_UNSUPPORTED, "%s: K <= 4096 (got %lld)", fn, (long long)K);
  if (d == 0) {
    *done = true;
    return GM_OK;
  }
  if (c->d_total > 0 || c->comm || c->ar_fn)
    return fail(GM_ERR_UNSUPPORTED, "%s: a d-sharded or collective context (the distances would "
                "need a K x K all-reduce)", fn);
  return GM_OK;
}

// D (upper triangle) of a bf16 operand into w->G on the tier asked for, Krum's workspace layout:
// the partials of either tier in the float slab (at least min_slab floats), rho in w->alpha, the
// flag in w->st.  Records what gm_dist_last_info reports.
int bf16_distances(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx, int ws,
                   int32_t dist_mode, size_t min_slab, Workspace* w, hipStream_t s) {
  const bool eligible = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 8 == 0;
  const bool mfma = dist_mode == GM_DIST_MFMA && eligible;
  const int64_t Se = krum_slices(K, d);
  const int64_t Sm = mfma ? pairdist_mfma_slices(K, d, c->num_cu) : 0;
  const size_t part_doubles = (size_t)std::max(Se, Sm) * (size_t)(K * K);
  int rc = ensure_ws(c, K, 1, 1, w, std::max(2 * part_doubles, min_slab), (int)K);
  if (rc) return rc;
  double* part = reinterpret_cast<double*>(w->gslab);
  c->dist_pending = false;
  c->dist_info[0] = GM_DIST_EXACT;
  c->dist_info[1] = dist_mode == GM_DIST_MFMA ? GM_DIST_REASON_NOT_ELIGIBLE
                                              : GM_DIST_REASON_REQUESTED_EXACT;
  c->dist_info[2] = Se;
  c->dist_info[3] = 32;
  if (!mfma) {
    HIPCHK(launch_krum_dist(X, K, d, ldx, ws, w->G, part, nullptr, s));
    return GM_OK;
  }
  if (!c->dist_flag) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->dist_flag), sizeof(int), hipHostMallocDefault));
  int* flag = reinterpret_cast<int*>(w->st);
  HIPCHK(launch_pairdist_mfma(X, K, d, ldx, ws, c->num_cu, part, w->alpha, w->G, flag, s));
  HIPCHK(launch_krum_dist(X, K, d, ldx, ws, w->G, part, flag, s));
  HIPCHK(hipMemcpyAsync(c->dist_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  c->dist_pending = true;
  c->dist_stream = s;
  c->dist_info[0] = GM_DIST_MFMA;
  c->dist_info[1] = GM_DIST_REASON_OK;
  c->dist_info[2] = Sm;
  c->dist_info[3] = kMfmaFlush;
  c->dist_exact_slices = Se;
  return GM_OK;
}

}  // namespace

extern "C" {

int gm_dist_last_info(gm_ctx* c, int64_t* info, double* beta) {
  if (!c || !info) return fail(GM_ERR_INVALID, "gm_dist_last_info: bad args");
  if (c->dist_pending) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->dist_stream));
    c->dist_pending = false;
    if (*c->dist_flag) {
      c->dist_info[0] = GM_DIST_EXACT;
      c->dist_info[1] = GM_DIST_REASON_NONFINITE;
      c->dist_info[2] = c->dist_exact_slices;
      c->dist_info[3] = 32;
    }
  }
  for (int i = 0; i < 4; ++i) info[i] = c->dist_info[i];
  if (beta) *beta = pairdist_mfma_beta();
  return GM_OK;
}

int gm_krum_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                 int64_t honest, int32_t dist_mode, float* out, int64_t* index, void* stream) {
  if (!c || !X || !out || K < 1 || d < 0 || !known(layout) || !known_mode(dist_mode) ||
      honest < 2 || honest - 1 > K)
    return fail(GM_ERR_INVALID, "gm_krum_bf16: bad args (a NULL ctx, X or out, K < 1, d < 0, an "
                "unknown layout or dist_mode; needs 2 <= honestSize <= K+1)");
  int ws = 0;
  int rc = layout_shift("gm_krum_bf16", K, d, ldx, layout, false, &ws);
  if (rc) return rc;
  bool done = false;
  rc = common_checks("gm_krum_bf16", c, K, d, &done);
  if (rc) return rc;
  if (done) {
    if (index) *index = 0;
    return GM_OK;
  }
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  Workspace w;
  rc = bf16_distances(c, X, K, d, ldx, ws, dist_mode, 0, &w, s);
  if (rc) return rc;
  HIPCHK(launch_krum_scores(w.G, K, honest - 1, w.alpha, s));
  int64_t* didx = reinterpret_cast<int64_t*>(w.u);
  HIPCHK(launch_krum_argmin_row(w.alpha, K, X, d, ldx, ws, didx, out, s));
  if (index) {
    HIPCHK(hipMemcpyAsync(index, didx, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return GM_OK;
}

int gm_multi_krum_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                       int32_t layout, int64_t honest, int64_t m, int32_t dist_mode, float* out,
                       int32_t* selected, void* stream) {
  if (!c || !X || !out || K < 1 || d < 0 || !known(layout) || !known_mode(dist_mode) ||
      honest < 2 || honest - 1 > K || m < 1 || m > K)
    return fail(GM_ERR_INVALID, "gm_multi_krum_bf16: bad args (a NULL ctx, X or out, K < 1, d < 0, "
                "an unknown layout or dist_mode; needs 2 <= honestSize <= K+1 and 1 <= m <= K)");
  int ws = 0;
  int rc = layout_shift("gm_multi_krum_bf16", K, d, ldx, layout, false, &ws);
  if (rc) return rc;
  bool done = false;
  rc = common_checks("gm_multi_krum_bf16", c, K, d, &done);
  if (rc || done) return rc;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  Workspace w;
  rc = bf16_distances(c, X, K, d, ldx, ws, dist_mode, 0, &w, s);
  if (rc) return rc;
  HIPCHK(launch_krum_scores(w.G, K, honest - 1, w.alpha, s));
  int32_t* flag = reinterpret_cast<int32_t*>(w.u);
  int32_t* list = flag + K;
  HIPCHK(launch_multi_krum_pick(w.alpha, K, m, X, d, ldx, ws, flag, list, out, s));
  if (selected) {
    HIPCHK(hipMemcpyAsync(selected, list, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return GM_OK;
}

int gm_nnm_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                int32_t layout_in, int64_t f, int32_t dist_mode, float* Y, int64_t ldy,
                int32_t layout_out, int32_t* neighbors, void* stream) {
  if (!c || !X || !Y || K < 1 || d < 0 || f < 0 || f > K - 1 || !known(layout_in) ||
      !known(layout_out) || !known_mode(dist_mode))
    return fail(GM_ERR_INVALID, "gm_nnm_bf16: bad args (a NULL ctx, X or Y, K < 1, d < 0, f outside "
                "[0, K - 1], an unknown layout or dist_mode)");
  int ws = 0, wsy = 0;
  int rc = layout_shift("gm_nnm_bf16", K, d, ldx, layout_in, false, &ws);
  if (rc) return rc;
  rc = layout_shift("gm_nnm_bf16", K, d, ldy, layout_out, true, &wsy);
  if (rc) return rc;
  bool done = false;
  rc = common_checks("gm_nnm_bf16", c, K, d, &done);
  if (rc || done) return rc;
  const int64_t m = K - f;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  // (the partials are dead once D is written, and the slab then holds the mask)
  Workspace w;
  rc = bf16_distances(c, X, K, d, ldx, ws, dist_mode, (size_t)nnm_mask_words(K), &w, s);
  if (rc) return rc;
  const int stop = env_int("GMAGG_NNM_STOP", 0);       // (gm_nnm_f32's, for the step timings)
  if (stop == 1) return GM_OK;
  uint32_t* mask = reinterpret_cast<uint32_t*>(w.gslab);
  HIPCHK(launch_nnm_neighbors(w.G, K, m, mask, neighbors, s));
  if (stop == 2) return GM_OK;
  HIPCHK(launch_nnm_mix(X, K, d, ldx, ws, mask, m, Y, ldy, wsy, s));
  return GM_OK;
}

int gm_pair_dist_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                      int32_t layout, int32_t dist_mode, double* D, void* stream) {
  if (!c || !X || !D || K < 1 || d < 0 || !known(layout) || !known_mode(dist_mode))
    return fail(GM_ERR_INVALID, "gm_pair_dist_bf16: bad args (a NULL ctx, X or D, K < 1, d < 0, an "
                "unknown layout or dist_mode)");
  int ws = 0;
  int rc = layout_shift("gm_pair_dist_bf16", K, d, ldx, layout, false, &ws);
  if (rc) return rc;
  bool done = false;
  rc = common_checks("gm_pair_dist_bf16", c, K, d, &done);
  if (rc || done) return rc;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  Workspace w;
  rc = bf16_distances(c, X, K, d, ldx, ws, dist_mode, 0, &w, s);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(D, w.G, sizeof(double) * (size_t)(K * K), hipMemcpyDeviceToDevice, s));
  HIPCHK(launch_mirror_upper(D, K, s));
  return GM_OK;
}

int gm_pair_dist_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                     double* D, void* stream) {
  if (!c || !X || !D || K < 1 || d < 0 || !known(layout))
    return fail(GM_ERR_INVALID, "gm_pair_dist_f32: bad args (a NULL ctx, X or D, K < 1, d < 0 or an "
                "unknown layout)");
  int ws = 0;
  int rc = layout_shift("gm_pair_dist_f32", K, d, ldx, layout, true, &ws);
  if (rc) return rc;
  bool done = false;
  rc = common_checks("gm_pair_dist_f32", c, K, d, &done);
  if (rc || done) return rc;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  Workspace w;
  const size_t part_doubles = (size_t)krum_slices(K, d) * (size_t)(K * K);
  rc = ensure_ws(c, K, 1, 1, &w, 2 * part_doubles, (int)K);
  if (rc) return rc;
  HIPCHK(launch_krum_dist(X, K, d, ldx, ws, w.G, reinterpret_cast<double*>(w.gslab), s));
  HIPCHK(hipMemcpyAsync(D, w.G, sizeof(double) * (size_t)(K * K), hipMemcpyDeviceToDevice, s));
  HIPCHK(launch_mirror_upper(D, K, s));
  return GM_OK;
}

}  // extern "C"
