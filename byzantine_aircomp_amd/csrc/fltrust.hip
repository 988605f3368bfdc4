// FLTrust (Cao, Fang, Liu & Gong, "FLTrust: Byzantine-robust Federated Learning via Trust
// Bootstrapping", NDSS 2021): every client row is scored by the cosine of its update with the
// server's own update, negative scores are cut to zero, and the trusted rows, each rescaled to
// the server update's norm, are averaged with their scores as weights.  The definition (what is
// counted, the order of every sum, the by-products) is in include/gmagg.h; gm_fltrust_f32 /
// gm_fltrust_bf16 at the end of this file are the host side.  Per call:
//   flt_row_stats      pass A, one read of X: a_k = u_k . g and n_k = ||u_k||^2 for every row and
//                      n_g = ||g||^2, fp64, as per-block partials [grid][2K + 1]
//   flt_reduce         the partials summed in block order -> sums [2K + 1]
//                      (a d-sharded context all-reduces sums here, once)
//   flt_kspace         one block: cos, TS, T, the compacted (row, coef) list of the rows with
//                      TS > 0, its length m, and the by-products
//   flt_weighted_rows  pass B, m rows of X: out = c + sum coef_k (x_k - c), fp64, rounded once
// Nothing is read back by the host: pass B takes m and the list from device memory.
//
// Pass A.  A persistent grid walks column chunks of J = LPR * E columns (E = 4 fp32 or 8 bf16
// columns per lane, one 16-byte load; LPR lanes share a row).  A lane keeps c_j and g_j of its
// columns in registers for the chunk; the block's waves walk the rows, 8 loads of 1 KiB in
// flight each.  Rows: LPR = 64, a load instruction reads 1 KiB of one row.  Panels: J = W, the
// chunk is one panel, and a load instruction reads 1 KiB of it, 64 / LPR rows at once.  The 16
// per-lane partials of 8 loads are summed across the LPR lanes of a row by device_util.h's
// transpose_reduce on doubles (a halving transpose: 17 cross-lane moves of a double for
// LPR = 64, against 96 for 16 butterflies), then added to
// the block's 2K LDS accumulators, which collect the block's chunks: the slab is grid x (2K + 1).
// Where the 16-byte path cannot be taken (base or stride not 16-byte aligned) the same kernel
// runs with E = 1; a chunk that reaches past column d guards every element.
#include <algorithm>

#include "device_util.h"
#include "host_ctx.h"

namespace gmk {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// E consecutive elements at p, widened (E > 1: one 16-byte load, p 16-byte aligned)
template <int E>
__device__ __forceinline__ void load_item(const float* p, float (&x)[E]) {
  if constexpr (E == 1) {
    x[0] = __builtin_nontemporal_load(p);
  } else {
    static_assert(E == 4, "fp32 items are 4 columns");
    const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = v[i];
  }
}
template <int E>
__device__ __forceinline__ void load_item(const uint16_t* p, float (&x)[E]) {
  if constexpr (E == 1) {
    x[0] = widen(__builtin_nontemporal_load(p));
  } else {
    static_assert(E == 8, "bf16 items are 8 columns");
    const u4 v = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = __uint_as_float(v[i] << 16);
      x[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
  }
}

struct FltHead {
  double T;        // sum of the trust scores
  int32_t m;       // rows with TS > 0
  int32_t pad;
};

struct FltArgs {
  const void* X;
  int64_t K, d;
  int64_t rs;            // elements between rows: ldx, or the panel width W
  int64_t cstride;       // elements between chunk groups: J (rows), the panel stride (panels)
  int cps;               // log2 of the chunks per panel (0 for rows)
  const float* server;   // [d], or nullptr: row server_row of X
  int64_t server_row;
  const float* centre;   // [d], or nullptr: zeros
  double* slab;          // [gridDim.x][2K + 1]
  int64_t nch;           // chunks
};

constexpr int kFltU = 8;           // loads in flight per lane in pass A
constexpr int kFltTA = 256;        // threads per block of pass A

template <class SRC, int E, int LPR>
__global__ void __launch_bounds__(kFltTA) flt_row_stats(const FltArgs a) {
  extern __shared__ double acc[];                    // [2K]: a_k, n_k over this block's chunks
  constexpr int J = LPR * E, RW = 64 / LPR, N = 2 * kFltU, GR = kFltU * RW;
  const SRC* X = static_cast<const SRC*>(a.X);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const int c = lane % LPR, rl = lane / LPR;
  for (int64_t i = threadIdx.x; i < 2 * a.K; i += blockDim.x) acc[i] = 0.0;
  __syncthreads();
  double ng = 0.0;
  for (int64_t ch = blockIdx.x; ch < a.nch; ch += gridDim.x) {
    const int64_t col = ch * J + (int64_t)c * E;     // this lane's first column
    const SRC* base = X + (ch >> a.cps) * a.cstride +
                      (ch & (((int64_t)1 << a.cps) - 1)) * J + (int64_t)c * E;
    const bool full = ch * J + J <= a.d;             // (block-uniform)
    const int64_t left = a.d - col;
    const int nv = left >= E ? E : (left > 0 ? (int)left : 0);   // this lane's columns < d
    double cc[E], g[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      cc[i] = 0.0;
      g[i] = 0.0;
      if (i < nv) {
        if (a.centre) cc[i] = (double)a.centre[col + i];
        const float s = a.server ? a.server[col + i] : widen(base[a.server_row * a.rs + i]);
        g[i] = (double)s - cc[i];
      }
    }
    if (wave == 0 && rl == 0) {
#pragma unroll
      for (int i = 0; i < E; ++i) ng += g[i] * g[i];
    }
    for (int64_t k0 = (int64_t)wave * GR; k0 < a.K; k0 += (int64_t)nwv * GR) {
      float x[kFltU][E];
      if (full) {
#pragma unroll
        for (int u = 0; u < kFltU; ++u) {
          const int64_t r = k0 + u * RW + rl;
          if (r < a.K) {
            load_item<E>(base + r * a.rs, x[u]);
          } else {
#pragma unroll
            for (int i = 0; i < E; ++i) x[u][i] = 0.f;
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < kFltU; ++u) {
          const int64_t r = k0 + u * RW + rl;
#pragma unroll
          for (int i = 0; i < E; ++i)
            x[u][i] = (r < a.K && i < nv) ? widen(__builtin_nontemporal_load(base + r * a.rs + i))
                                         : 0.f;
        }
      }
      double e[N];
#pragma unroll
      for (int u = 0; u < kFltU; ++u) {
        double sa = 0.0, sn = 0.0;
#pragma unroll
        for (int i = 0; i < E; ++i) {
          // (a column >= d has x = c = g = 0: it adds nothing)
          const double uu = (double)x[u][i] - cc[i];
          sa += uu * g[i];
          sn += uu * uu;
        }
        e[2 * u] = sa;
        e[2 * u + 1] = sn;
      }
      transpose_reduce<LPR, N>(e, c);
      // value v of the 16 is {a, n}[v & 1] of row k0 + (v >> 1) RW + rl; rows belong to one wave
      // of the block, so the LDS adds need no atomics
      constexpr int RPL = N >= LPR ? N / LPR : 1;
      const int v0 = row_of_lane<LPR, N>(c);
      const bool writer = N >= LPR || (c & (LPR / N - 1)) == 0;
#pragma unroll
      for (int m = 0; m < RPL; ++m) {
        const int v = v0 + m;
        const int64_t r = k0 + (v >> 1) * RW + rl;
        if (writer && r < a.K) acc[2 * r + (v & 1)] += e[m];
      }
    }
  }
  __syncthreads();
  double* slab = a.slab + (int64_t)blockIdx.x * (2 * a.K + 1);
  for (int64_t i = threadIdx.x; i < 2 * a.K; i += blockDim.x) slab[i] = acc[i];
  if (wave == 0) {
    ng = wave_sum(ng);
    if (lane == 0) slab[2 * a.K] = ng;
  }
}

// sums[i] = the blocks' partials in block order
__global__ void __launch_bounds__(256) flt_reduce(const double* __restrict__ slab, int nb,
                                                  int64_t S, double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  double s = slab[i];
  for (int b = 1; b < nb; ++b) s += slab[(int64_t)b * S + i];
  sums[i] = s;
}

constexpr int kFltMaxK = 2048;

// One block: the K-space step of the definition.
__global__ void __launch_bounds__(256) flt_kspace(const double* __restrict__ sums, int64_t K,
                                                  int64_t server_row, double* __restrict__ coef,
                                                  int32_t* __restrict__ list,
                                                  FltHead* __restrict__ head,
                                                  double* __restrict__ stats) {
  __shared__ double ts[kFltMaxK];
  __shared__ double s_T;
  const double ng = sums[2 * K];
  const double inf = __builtin_inf();
  const bool ng_ok = ng > 0.0 && ng < inf;
  for (int64_t k = threadIdx.x; k < K; k += blockDim.x) {
    const double ak = sums[2 * k], nk = sums[2 * k + 1];
    const double cs = ak / sqrt(nk * ng);
    const bool counted = k != server_row && ng_ok && nk > 0.0 && nk < inf && ak > -inf && ak < inf;
    const double t = counted && cs > 0.0 ? cs : 0.0;
    ts[k] = t;
    if (stats) {
      stats[k] = cs;
      stats[K + k] = nk;
      stats[2 * K + k] = t;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double T = 0.0;
    for (int64_t k = 0; k < K; ++k) T += ts[k];      // increasing k
    s_T = T;
  }
  __syncthreads();
  const double T = s_T;
  if (threadIdx.x >= 64) return;
  // the first wave: the trusted rows, increasing (flags_to_list's ballot walk)
  const int lane = threadIdx.x;
  int64_t n = 0;
  for (int64_t i0 = 0; i0 < K; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool in = i < K && ts[i < K ? i : 0] > 0.0;
    const uint64_t b = __ballot(in);
    const int64_t pos = n + (int64_t)__builtin_amdgcn_mbcnt_hi(
                                (uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (in) {
      list[pos] = (int32_t)i;
      coef[pos] = ts[i] * sqrt(ng / sums[2 * i + 1]) / T;
    }
    n += __popcll(b);
  }
  if (lane == 0) {
    head->T = T;
    head->m = (int32_t)n;
    head->pad = 0;
    if (stats) {
      stats[3 * K] = ng;
      stats[3 * K + 1] = T;
    }
  }
}

constexpr int kFltUB = 4;          // rows in flight per thread in pass B

// Pass B: a thread owns E columns and walks the m listed rows in order.
template <class SRC, int E>
__global__ void __launch_bounds__(256) flt_weighted_rows(
    const SRC* __restrict__ X, int64_t d, int64_t rs, int64_t pstride, int ws,
    const float* __restrict__ centre, const double* __restrict__ coef,
    const int32_t* __restrict__ list, const FltHead* __restrict__ head, float* __restrict__ out) {
  const int64_t m = head->m;
  const int64_t G = (d + E - 1) / E;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < G;
       gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = gi * E;
    const int nv = d - col >= E ? E : (int)(d - col);
    if (m == 0) {                                    // T == 0: the centre itself
      for (int i = 0; i < nv; ++i) out[col + i] = centre ? centre[col + i] : 0.f;
      continue;
    }
    const SRC* base = ws ? X + (col >> ws) * pstride + (col & (((int64_t)1 << ws) - 1)) : X + col;
    double cc[E], acc[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      cc[i] = centre && i < nv ? (double)centre[col + i] : 0.0;
      acc[i] = 0.0;
    }
    if (nv == E) {
      int64_t t = 0;
      for (; t + kFltUB <= m; t += kFltUB) {
        float x[kFltUB][E];
        double w[kFltUB];
#pragma unroll
        for (int u = 0; u < kFltUB; ++u) {
          load_item<E>(base + (int64_t)list[t + u] * rs, x[u]);
          w[u] = coef[t + u];
        }
#pragma unroll
        for (int u = 0; u < kFltUB; ++u)
#pragma unroll
          for (int i = 0; i < E; ++i) acc[i] += w[u] * ((double)x[u][i] - cc[i]);
      }
      for (; t < m; ++t) {
        float x[E];
        load_item<E>(base + (int64_t)list[t] * rs, x);
        const double w = coef[t];
#pragma unroll
        for (int i = 0; i < E; ++i) acc[i] += w * ((double)x[i] - cc[i]);
      }
#pragma unroll
      for (int i = 0; i < E; ++i) out[col + i] = (float)(cc[i] + acc[i]);
    } else {
      // the ragged last group: its columns < d one at a time, the same sums
      for (int i = 0; i < nv; ++i) {
        double s = 0.0;
        for (int64_t t = 0; t < m; ++t)
          s += coef[t] * ((double)widen(base[(int64_t)list[t] * rs + i]) - cc[i]);
        out[col + i] = (float)(cc[i] + s);
      }
    }
  }
}

template <class SRC, int E>
hipError_t launch_row_stats(int lpr, int grid, size_t lds, const FltArgs& a, hipStream_t s) {
  const dim3 g((unsigned)grid), b(kFltTA);
  switch (lpr) {
    case 64: hipLaunchKernelGGL((flt_row_stats<SRC, E, 64>), g, b, lds, s, a); break;
    case 32: hipLaunchKernelGGL((flt_row_stats<SRC, E, 32>), g, b, lds, s, a); break;
    case 16: hipLaunchKernelGGL((flt_row_stats<SRC, E, 16>), g, b, lds, s, a); break;
    case 8: hipLaunchKernelGGL((flt_row_stats<SRC, E, 8>), g, b, lds, s, a); break;
    case 4: hipLaunchKernelGGL((flt_row_stats<SRC, E, 4>), g, b, lds, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// Blocks of pass A's persistent grid per CU (2K doubles of LDS each) and of pass B's grid in all.
// (pass A's registers allow two 4-wave blocks per CU: with more, the rest would only queue)
constexpr int kFltBlocksPerCU = 2;
constexpr int64_t kFltGridB = 2048;

struct FltWork {
  double* slab;
  double* sums;
  double* coef;
  int32_t* list;
  FltHead* head;
};

template <class SRC>
int fltrust(const char* fn, gm_ctx* c, const SRC* X, int64_t K, int64_t d, int64_t ldx,
            int32_t layout, const float* server, int64_t server_row, const float* centre,
            float* out, double* stats, void* stream) {
  using namespace gmh;
  constexpr bool bf16 = sizeof(SRC) == 2;
  constexpr int EV = bf16 ? 8 : 4;
  if (!c || !X || !out || K < 1 || d < 0 ||
      (layout != GM_LAYOUT_ROWS && layout != GM_LAYOUT_PANELS))
    return fail(GM_ERR_INVALID, "%s: bad args (a NULL ctx, X or out, K < 1, d < 0 or an unknown "
                "layout)", fn);
  if ((server != nullptr) == (server_row != -1))
    return fail(GM_ERR_INVALID, "%s: exactly one of server (a [d] vector) and server_row (a row "
                "of X, else -1) must be given (got %s, server_row = %lld)", fn,
                server ? "a vector" : "NULL", (long long)server_row);
  if (!server && (server_row < 0 || server_row >= K))
    return fail(GM_ERR_INVALID, "%s: server_row = %lld outside [0, %lld)", fn,
                (long long)server_row, (long long)K);
  if (K > kFltMaxK)
    return fail(GM_ERR_UNSUPPORTED, "%s: K <= %d (got %lld)", fn, kFltMaxK, (long long)K);
  int64_t W = 0;
  if (layout == GM_LAYOUT_PANELS) {
    W = bf16 ? gm_panel_width_bf16(K) : gm_panel_width(K);
    if (W == 0)
      return fail(GM_ERR_UNSUPPORTED, "%s: no panel layout for K = %lld rows (pass them "
                  "row-major)", fn, (long long)K);
    if (ldx < K * W)
      return fail(GM_ERR_INVALID, "%s: panel stride %lld < K * W = %lld", fn, (long long)ldx,
                  (long long)(K * W));
  } else if (ldx < d) {
    return fail(GM_ERR_INVALID, "%s: ldx = %lld < d = %lld", fn, (long long)ldx, (long long)d);
  }
  if (d == 0) return GM_OK;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);

  // the 16-byte path: base and strides multiples of E elements (panel widths always are)
  const bool vec = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % EV == 0;
  const int E = vec ? EV : 1;
  // lanes per row segment and chunk width: rows 64 lanes; panels the whole panel, or 64
  // columns of it on the one-column path
  const int64_t J = W ? (vec ? W : std::min<int64_t>(W, 64)) : 64 * E;
  const int lpr = (int)(J / E);
  const int64_t nch = (d + J - 1) / J;
  const int nb = (int)std::min<int64_t>(nch, (int64_t)c->num_cu * kFltBlocksPerCU);
  const size_t S = 2 * (size_t)K + 1;
  FltWork w;
  auto lay = [&](char* base) {
    Carve cv{base};
    w.slab = cv.take<double>(S * (size_t)nb);
    w.sums = cv.take<double>(S);
    w.coef = cv.take<double>(K);
    w.list = cv.take<int32_t>(K);
    w.head = cv.take<FltHead>(1);
    return cv.off;
  };
  int rc = grow_ws(c, lay(nullptr));
  if (rc) return rc;
  lay(c->ws);

  FltArgs a{};
  a.X = X; a.K = K; a.d = d;
  a.rs = W ? W : ldx;
  a.cstride = W ? ldx : J;
  a.cps = W ? wshift_of(W / J) : 0;
  a.server = server; a.server_row = server ? -1 : server_row; a.centre = centre;
  a.slab = w.slab; a.nch = nch;
  const size_t lds = 2 * (size_t)K * sizeof(double);
  HIPCHK((vec ? launch_row_stats<SRC, EV>(lpr, nb, lds, a, s)
              : launch_row_stats<SRC, 1>(lpr, nb, lds, a, s)));
  hipLaunchKernelGGL(flt_reduce, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, w.slab, nb,
                     (int64_t)S, w.sums);
  HIPCHK(hipGetLastError());
  // a d-sharded context: the 2K + 1 sums over every rank's columns (nothing without a
  // communicator or callback)
  rc = allreduce(c, w.sums, (int64_t)S, s);
  if (rc) return rc;
  hipLaunchKernelGGL(flt_kspace, dim3(1), dim3(256), 0, s, w.sums, K, a.server_row, w.coef, w.list,
                     w.head, stats);
  HIPCHK(hipGetLastError());
  const int64_t items = (d + E - 1) / E;
  const dim3 gb((unsigned)std::min<int64_t>((items + 255) / 256, kFltGridB));
  const int ws = W ? wshift_of(W) : 0;
  if (vec)
    hipLaunchKernelGGL((flt_weighted_rows<SRC, EV>), gb, dim3(256), 0, s, X, d, a.rs, ldx, ws,
                       centre, w.coef, w.list, w.head, out);
  else
    hipLaunchKernelGGL((flt_weighted_rows<SRC, 1>), gb, dim3(256), 0, s, X, d, a.rs, ldx, ws,
                       centre, w.coef, w.list, w.head, out);
  HIPCHK(hipGetLastError());
  return GM_OK;
}

}  // namespace

}  // namespace gmk

extern "C" {

int gm_fltrust_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                   const float* server, int64_t server_row, const float* centre, float* out,
                   double* stats, void* stream) {
  return gmk::fltrust("gm_fltrust_f32", c, X, K, d, ldx, layout, server, server_row, centre, out,
                      stats, stream);
}

int gm_fltrust_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                    int32_t layout, const float* server, int64_t server_row, const float* centre,
                    float* out, double* stats, void* stream) {
  return gmk::fltrust("gm_fltrust_bf16", c, X, K, d, ldx, layout, server, server_row, centre, out,
                      stats, stream);
}

}  // extern "C"
