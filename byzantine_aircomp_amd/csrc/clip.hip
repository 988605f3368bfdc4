// Norm clipping ahead of an aggregator: every row's update u_k = x_k - c is scaled back to a
// radius, a given one (static clipping; Sun, Kairouz, Suresh & McMahan 2019) or the norm of the
// (k + 1)-th largest update, k = floor(2 f (K - f) / K) (ARC; Allouah, Guerraoui, Gupta, Jellouli,
// Rizk & Stephan, "Adaptive Gradient Clipping for Robust Federated Learning", ICLR 2025).  The
// definition (the order of the n_k, the threshold, the three kinds of row) is in include/gmagg.h;
// gm_clip_rows_f32 / gm_clip_rows_bf16 at the end of this file are the host side.  Per call:
//   clip_row_norms   pass 1, one read of X: n_k = ||x_k - c||^2 for every row, fp64, as per-block
//                    partials [grid][K]
//   clip_reduce      the partials summed in block order -> sums [K]
//                    (a d-sharded context all-reduces sums here, once)
//   clip_kspace      one block: T, s_k, the list of the rows with s_k != 1, its length, the stats
//   clip_apply       pass 2: Y from X, c and s_k.  Out of place every row is written (s_k = 1: a
//                    copy; s_k = 0: the centre, the row is not read); in place (Y is X) only the
//                    listed rows are touched
// Nothing is read back by the host: pass 2 takes the list and its length from device memory.
//
// Pass 1 is fltrust.hip's pass A with one sum per element instead of two: a persistent grid
// walks column chunks of J = LPR * E columns (E = 4 fp32 or 8 bf16 columns per lane, one 16-byte
// load; LPR lanes share a row), a lane keeps c_j of its columns in registers for the chunk, the
// block's waves walk the rows with 8 loads in flight each, and the 8 per-lane partials are
// summed across the LPR lanes of a row by transpose_reduce on doubles (10 cross-lane moves of a
// double per 8 rows at LPR = 64, against pass A's 17 for its 16 values), then added to the
// block's K LDS accumulators.  Every row takes the same path through these sums, so rows that
// hold the same values have the same n_k bits.  Where the 16-byte path cannot be taken (base or
// stride not 16-byte aligned) the same kernel runs with E = 1; a chunk that reaches past column
// d guards every element.
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

struct ClipHead {
  int32_t m;       // rows with s_k != 1
  int32_t pad;
};

struct ClipArgs {
  const void* X;
  int64_t K, d;
  int64_t rs;            // elements between rows: ldx, or the panel width W
  int64_t cstride;       // elements between chunk groups: J (rows), the panel stride (panels)
  int cps;               // log2 of the chunks per panel (0 for rows)
  const float* centre;   // [d], or nullptr: zeros
  double* slab;          // [gridDim.x][K]
  int64_t nch;           // chunks
};

constexpr int kClipU = 8;          // loads in flight per lane in pass 1
constexpr int kClipT1 = 256;       // threads per block of pass 1

template <class SRC, int E, int LPR>
__global__ void __launch_bounds__(kClipT1) clip_row_norms(const ClipArgs a) {
  extern __shared__ double acc[];                    // [K]: n_k over this block's chunks
  constexpr int J = LPR * E, RW = 64 / LPR, N = kClipU, GR = kClipU * RW;
  const SRC* X = static_cast<const SRC*>(a.X);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const int c = lane % LPR, rl = lane / LPR;
  for (int64_t i = threadIdx.x; i < a.K; i += blockDim.x) acc[i] = 0.0;
  __syncthreads();
  for (int64_t ch = blockIdx.x; ch < a.nch; ch += gridDim.x) {
    const int64_t col = ch * J + (int64_t)c * E;     // this lane's first column
    const SRC* base = X + (ch >> a.cps) * a.cstride +
                      (ch & (((int64_t)1 << a.cps) - 1)) * J + (int64_t)c * E;
    const bool full = ch * J + J <= a.d;             // (block-uniform)
    const int64_t left = a.d - col;
    const int nv = left >= E ? E : (left > 0 ? (int)left : 0);   // this lane's columns < d
    double cc[E];
#pragma unroll
    for (int i = 0; i < E; ++i) cc[i] = a.centre && i < nv ? (double)a.centre[col + i] : 0.0;
    for (int64_t k0 = (int64_t)wave * GR; k0 < a.K; k0 += (int64_t)nwv * GR) {
      float x[kClipU][E];
      if (full) {
#pragma unroll
        for (int u = 0; u < kClipU; ++u) {
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
        for (int u = 0; u < kClipU; ++u) {
          const int64_t r = k0 + u * RW + rl;
#pragma unroll
          for (int i = 0; i < E; ++i)
            x[u][i] = (r < a.K && i < nv) ? widen(__builtin_nontemporal_load(base + r * a.rs + i))
                                         : 0.f;
        }
      }
      double e[N];
#pragma unroll
      for (int u = 0; u < kClipU; ++u) {
        double sn = 0.0;
#pragma unroll
        for (int i = 0; i < E; ++i) {
          // (a column >= d has x = c = 0; a row >= K is not stored)
          const double uu = (double)x[u][i] - cc[i];
          sn += uu * uu;
        }
        e[u] = sn;
      }
      transpose_reduce<LPR, N>(e, c);
      // value v of the 8 is n of row k0 + v RW + rl; rows belong to one wave of the block, so
      // the LDS adds need no atomics
      constexpr int RPL = N >= LPR ? N / LPR : 1;
      const int v0 = row_of_lane<LPR, N>(c);
      const bool writer = N >= LPR || (c & (LPR / N - 1)) == 0;
#pragma unroll
      for (int m = 0; m < RPL; ++m) {
        const int64_t r = k0 + (int64_t)(v0 + m) * RW + rl;
        if (writer && r < a.K) acc[r] += e[m];
      }
    }
  }
  __syncthreads();
  double* slab = a.slab + (int64_t)blockIdx.x * a.K;
  for (int64_t i = threadIdx.x; i < a.K; i += blockDim.x) slab[i] = acc[i];
}

// sums[i] = the blocks' partials in a fixed order: a block of 256 threads owns 32 sums, thread
// (p, i) adds the p-th eighth of the pass-1 blocks in block order, and the eight parts are added
// in order of p.  (One thread per sum walking every block, as flt_reduce does, is a chain of
// dependent loads as long as pass 1's grid.)
constexpr int kClipRedParts = 8;
__global__ void __launch_bounds__(256) clip_reduce(const double* __restrict__ slab, int nb,
                                                   int64_t K, double* __restrict__ sums) {
  __shared__ double part[kClipRedParts][32];
  const int ii = threadIdx.x & 31, p = threadIdx.x >> 5;
  const int64_t i = (int64_t)blockIdx.x * 32 + ii;
  const int per = (nb + kClipRedParts - 1) / kClipRedParts;
  const int b0 = p * per, b1 = min(nb, b0 + per);
  double s = 0.0;
  if (i < K) {
#pragma unroll 4
    for (int b = b0; b < b1; ++b) s += slab[(int64_t)b * K + i];
  }
  part[p][ii] = s;
  __syncthreads();
  if (p == 0 && i < K) {
    for (int q = 1; q < kClipRedParts; ++q) s += part[q][ii];
    sums[i] = s;
  }
}

constexpr int kClipMaxK = 4096;
constexpr int kClipTK = 1024;      // threads of the K-space block

// n_k as an unsigned key in the order of score_before (robust.hip): n >= 0, so the bits are
// ordered as the values; every NaN becomes the one key above +inf, so NaNs tie and the index
// decides (nnm.hip's nnm_key).
__device__ __forceinline__ unsigned long long clip_key(double x) {
  if (x != x) return 0x7FF8000000000000ull;
  return (unsigned long long)__double_as_longlong(x) & 0x7FFFFFFFFFFFFFFFull;
}

// One block: the K-space step of the definition.  rank: the zero-based rank of the threshold row
// in the order of (n_k, k) (ARC); T2: tau^2 (static).  Afterwards buf holds the s_k.
__global__ void __launch_bounds__(kClipTK) clip_kspace(const double* __restrict__ sums, int64_t K,
                                                       int32_t rule, int64_t rank, double T2,
                                                       double* __restrict__ scale,
                                                       int32_t* __restrict__ list,
                                                       ClipHead* __restrict__ head,
                                                       double* __restrict__ stats) {
  __shared__ unsigned long long buf[kClipMaxK];
  __shared__ double s_T;
  if (rule == GM_CLIP_ARC) {
    for (int64_t k = threadIdx.x; k < K; k += blockDim.x) buf[k] = clip_key(sums[k]);
    __syncthreads();
    for (int64_t j = threadIdx.x; j < K; j += blockDim.x) {
      const unsigned long long x = buf[j];
      int64_t r = 0;
      for (int64_t t = 0; t < K; ++t) r += (buf[t] < x) || (buf[t] == x && t < j);
      if (r == rank) s_T = sums[j];                  // (ranks are distinct: exactly one row)
    }
  } else if (threadIdx.x == 0) {
    s_T = T2;
  }
  __syncthreads();
  const double T = s_T;
  const double inf = __builtin_inf();
  for (int64_t k = threadIdx.x; k < K; k += blockDim.x) {
    const double nk = sums[k];
    double s;
    if (nk != nk || nk == inf) s = 0.0;
    else if (T != T || nk <= T) s = 1.0;
    else s = sqrt(T / nk);
    buf[k] = (unsigned long long)__double_as_longlong(s);
    scale[k] = s;
    if (stats) {
      stats[k] = nk;
      stats[K + k] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  // the first wave: the rows with s_k != 1, increasing (flags_to_list's ballot walk)
  const int lane = threadIdx.x;
  const unsigned long long one = (unsigned long long)__double_as_longlong(1.0);
  int64_t n = 0;
  for (int64_t i0 = 0; i0 < K; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool in = i < K && buf[i < K ? i : 0] != one;
    const uint64_t b = __ballot(in);
    const int64_t pos = n + (int64_t)__builtin_amdgcn_mbcnt_hi(
                                (uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (in) list[pos] = (int32_t)i;
    n += __popcll(b);
  }
  if (lane == 0) {
    head->m = (int32_t)n;
    head->pad = 0;
    if (stats) {
      stats[2 * K] = T;
      stats[2 * K + 1] = (double)n;
    }
  }
}

// Pass 2.  A thread owns items of E consecutive columns of one row; a block walks tiles of
// kClipTile items, kClipUB items in flight per thread.  Rows in: a tile is a stretch of one
// listed row and the tiles follow each other along the row, then over the rows, so the grid
// sweeps X and Y front to back.  Panels in: a tile is a stretch of one panel's listed rows,
// W / E items each, so that consecutive lanes read consecutive memory.  An item never crosses a
// panel of X or Y (E divides both widths).  A tile's loads (s_k, then the row's items and, for
// the rows that need them, the c_j) are all issued before its first store: X and Y may be the
// same buffer, so the compiler keeps every load after a store behind it, and a load per item
// between the stores would put the tile's latencies in a chain.  An item is read and written
// by the same thread.
constexpr int kClipUB = 4;
constexpr int kClipT2 = 256;
constexpr int64_t kClipTile = (int64_t)kClipT2 * kClipUB;
constexpr int64_t kClipGrid2 = 2048;

struct ApplyArgs {
  const void* X;
  float* Y;
  int64_t K, d;
  int64_t ldx, ldy;        // row stride, or panel stride
  int wsx, wsy;            // log2 of the panel width, 0 for rows
  int pin;                 // X is in panels
  int vy;                  // 16-byte stores: Y and ldy allow them
  int vc;                  // 16-byte loads of the centre
  const float* centre;     // [d], or nullptr: zeros
  const double* scale;     // [K]
  const int32_t* list;     // the rows to write, or nullptr: all K
  const ClipHead* head;    // list's length
};

__device__ __forceinline__ int64_t elem_off(int64_t ld, int ws, int64_t k, int64_t col) {
  return ws ? (col >> ws) * ld + (k << ws) + (col & (((int64_t)1 << ws) - 1)) : k * ld + col;
}

template <class SRC, int E>
__global__ void __launch_bounds__(kClipT2) clip_apply(const ApplyArgs a) {
  const SRC* X = static_cast<const SRC*>(a.X);
  const int64_t m = a.list ? a.head->m : a.K;
  if (m == 0) return;
  // rows: per listed row G items in ct tiles; panels: per panel m WE items in ct tiles
  const int lwe = a.pin ? a.wsx - ilog2<E>::v : 0;
  const int64_t per = a.pin ? m << lwe : (a.d + E - 1) / E;
  const int64_t ct = (per + kClipTile - 1) / kClipTile;
  const int64_t ntiles = (a.pin ? (a.d + ((int64_t)1 << a.wsx) - 1) >> a.wsx : m) * ct;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    // (block-uniform) tile t is stretch t % ct of listed row (rows) or panel (panels) t / ct
    const int64_t hi = t / ct;
    const int64_t q0 = (t - hi * ct) * kClipTile + threadIdx.x;
    int64_t row[kClipUB], col[kClipUB];
    int nv[kClipUB];
    double s[kClipUB];
    float x[kClipUB][E], cj[kClipUB][E];
#pragma unroll
    for (int u = 0; u < kClipUB; ++u) {
      const int64_t q = q0 + (int64_t)u * kClipT2;
      nv[u] = 0;
      s[u] = 1.0;
      row[u] = col[u] = 0;
      if (q < per) {
        const int64_t li = a.pin ? q >> lwe : hi;
        row[u] = a.list ? (int64_t)a.list[li] : li;
        col[u] = a.pin ? (hi << a.wsx) + ((q & (((int64_t)1 << lwe) - 1)) * E) : q * E;
        const int64_t left = a.d - col[u];
        nv[u] = left >= E ? E : (left > 0 ? (int)left : 0);
        if (nv[u] > 0) s[u] = a.scale[row[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < kClipUB; ++u) {
#pragma unroll
      for (int i = 0; i < E; ++i) x[u][i] = cj[u][i] = 0.f;
      if (nv[u] == 0) continue;
      if (s[u] != 0.0) {                             // (a row with s = 0 is not read)
        const SRC* src = X + elem_off(a.ldx, a.wsx, row[u], col[u]);
        if (nv[u] == E) {
          load_item<E>(src, x[u]);
        } else {
#pragma unroll
          for (int i = 0; i < E; ++i)
            if (i < nv[u]) x[u][i] = widen(src[i]);
        }
      }
      if (s[u] != 1.0 && a.centre) {                 // (a copied row needs no centre)
        const float* cp = a.centre + col[u];
        if (E > 1 && a.vc && nv[u] == E) {
#pragma unroll
          for (int i = 0; i < E; i += 4) {
            const f4 v = *reinterpret_cast<const f4*>(cp + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) cj[u][i + j] = v[j];
          }
        } else {
#pragma unroll
          for (int i = 0; i < E; ++i)
            if (i < nv[u]) cj[u][i] = cp[i];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kClipUB; ++u) {
      if (nv[u] == 0) continue;
      float y[E];
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const double c64 = (double)cj[u][i];
        y[i] = s[u] == 1.0 ? x[u][i]
                           : s[u] == 0.0 ? cj[u][i] : (float)(c64 + s[u] * ((double)x[u][i] - c64));
      }
      float* dst = a.Y + elem_off(a.ldy, a.wsy, row[u], col[u]);
      if (E > 1 && a.vy && nv[u] == E) {
#pragma unroll
        for (int i = 0; i < E; i += 4)
          *reinterpret_cast<f4*>(dst + i) = f4{y[i], y[i + 1], y[i + 2], y[i + 3]};
      } else {
#pragma unroll
        for (int i = 0; i < E; ++i)
          if (i < nv[u]) dst[i] = y[i];
      }
    }
  }
}

template <class SRC, int E>
hipError_t launch_row_norms(int lpr, int grid, size_t lds, const ClipArgs& a, hipStream_t s) {
  const dim3 g((unsigned)grid), b(kClipT1);
  switch (lpr) {
    case 64: hipLaunchKernelGGL((clip_row_norms<SRC, E, 64>), g, b, lds, s, a); break;
    case 32: hipLaunchKernelGGL((clip_row_norms<SRC, E, 32>), g, b, lds, s, a); break;
    case 16: hipLaunchKernelGGL((clip_row_norms<SRC, E, 16>), g, b, lds, s, a); break;
    case 8: hipLaunchKernelGGL((clip_row_norms<SRC, E, 8>), g, b, lds, s, a); break;
    case 4: hipLaunchKernelGGL((clip_row_norms<SRC, E, 4>), g, b, lds, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// Blocks of pass 1's persistent grid per CU (K doubles of LDS each): as many 4-wave blocks as
// the kernel's registers let a CU hold (122 VGPRs on fp32 items, 160 on bf16 items; with more,
// the rest would only queue behind the persistent ones).
constexpr int kClipBlocksPerCU = 4;
constexpr int kClipBlocksPerCUB16 = 3;

struct ClipWork {
  double* slab;
  double* sums;
  double* scale;
  int32_t* list;
  ClipHead* head;
};

// bytes from the first to one past the last element of a K x d matrix in its layout
inline int64_t extent(int64_t K, int64_t d, int64_t ld, int64_t W, size_t esz) {
  const int64_t n = W ? ((d + W - 1) / W - 1) * ld + K * W : (K - 1) * ld + d;
  return n * (int64_t)esz;
}

template <class SRC>
int clip_rows(const char* fn, gm_ctx* c, const SRC* X, int64_t K, int64_t d, int64_t ldx,
              int32_t layout_in, const float* centre, int32_t rule, int64_t f, double tau, float* Y,
              int64_t ldy, int32_t layout_out, double* stats, void* stream) {
  using namespace gmh;
  constexpr bool bf16 = sizeof(SRC) == 2;
  constexpr int EV = bf16 ? 8 : 4;
  auto known = [](int32_t l) { return l == GM_LAYOUT_ROWS || l == GM_LAYOUT_PANELS; };
  if (!c || !X || !Y || K < 1 || d < 0 || !known(layout_in) || !known(layout_out))
    return fail(GM_ERR_INVALID, "%s: bad args (a NULL ctx, X or Y, K < 1, d < 0 or an unknown "
                "layout)", fn);
  if (rule != GM_CLIP_STATIC && rule != GM_CLIP_ARC)
    return fail(GM_ERR_INVALID, "%s: unknown rule %d (GM_CLIP_STATIC or GM_CLIP_ARC)", fn,
                (int)rule);
  if (rule == GM_CLIP_ARC && (f < 0 || f > K - 1))
    return fail(GM_ERR_INVALID, "%s: f = %lld outside [0, %lld]", fn, (long long)f,
                (long long)(K - 1));
  if (rule == GM_CLIP_STATIC && !(tau > 0.0))
    return fail(GM_ERR_INVALID, "%s: tau = %g is not > 0", fn, tau);
  if (K > kClipMaxK)
    return fail(GM_ERR_UNSUPPORTED, "%s: K <= %d (got %lld)", fn, kClipMaxK, (long long)K);
  int64_t Wi = 0, Wo = 0;
  if (layout_in == GM_LAYOUT_PANELS) Wi = bf16 ? gm_panel_width_bf16(K) : gm_panel_width(K);
  if (layout_out == GM_LAYOUT_PANELS) Wo = gm_panel_width(K);
  if ((layout_in == GM_LAYOUT_PANELS && Wi == 0) || (layout_out == GM_LAYOUT_PANELS && Wo == 0))
    return fail(GM_ERR_UNSUPPORTED, "%s: no panel layout for K = %lld rows (pass and take them "
                "row-major)", fn, (long long)K);
  if (ldx < (Wi ? K * Wi : d) || ldy < (Wo ? K * Wo : d))
    return fail(GM_ERR_INVALID, "%s: ldx = %lld or ldy = %lld too small for its layout", fn,
                (long long)ldx, (long long)ldy);
  const bool alias = static_cast<const void*>(X) == static_cast<const void*>(Y) && ldx == ldy &&
                     layout_in == layout_out;
  if (alias && bf16)
    return fail(GM_ERR_UNSUPPORTED, "%s: bf16 rows cannot be clipped in place (Y is fp32)", fn);
  if (!alias && d > 0) {
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(X), y0 = reinterpret_cast<uintptr_t>(Y);
    const uintptr_t x1 = x0 + (uintptr_t)extent(K, d, ldx, Wi, sizeof(SRC));
    const uintptr_t y1 = y0 + (uintptr_t)extent(K, d, ldy, Wo, sizeof(float));
    if (x0 < y1 && y0 < x1)
      return fail(GM_ERR_INVALID, "%s: Y overlaps X (in place needs the same pointer, stride "
                  "and layout)", fn);
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
  const int64_t J = Wi ? (vec ? Wi : std::min<int64_t>(Wi, 64)) : 64 * E;
  const int lpr = (int)(J / E);
  const int64_t nch = (d + J - 1) / J;
  const int bpc = vec && bf16 ? kClipBlocksPerCUB16 : kClipBlocksPerCU;
  const int nb = (int)std::min<int64_t>(nch, (int64_t)c->num_cu * bpc);
  ClipWork w;
  auto lay = [&](char* base) {
    Carve cv{base};
    w.slab = cv.take<double>((size_t)K * (size_t)nb);
    w.sums = cv.take<double>(K);
    w.scale = cv.take<double>(K);
    w.list = cv.take<int32_t>(K);
    w.head = cv.take<ClipHead>(1);
    return cv.off;
  };
  int rc = grow_ws(c, lay(nullptr));
  if (rc) return rc;
  lay(c->ws);

  ClipArgs a{};
  a.X = X; a.K = K; a.d = d;
  a.rs = Wi ? Wi : ldx;
  a.cstride = Wi ? ldx : J;
  a.cps = Wi ? wshift_of(Wi / J) : 0;
  a.centre = centre; a.slab = w.slab; a.nch = nch;
  const size_t lds = (size_t)K * sizeof(double);
  HIPCHK((vec ? launch_row_norms<SRC, EV>(lpr, nb, lds, a, s)
              : launch_row_norms<SRC, 1>(lpr, nb, lds, a, s)));
  hipLaunchKernelGGL(clip_reduce, dim3((unsigned)((K + 31) / 32)), dim3(256), 0, s, w.slab, nb, K,
                     w.sums);
  HIPCHK(hipGetLastError());
  // a d-sharded context: the K sums over every rank's columns (nothing without a communicator
  // or callback)
  rc = allreduce(c, w.sums, K, s);
  if (rc) return rc;
  const int64_t rank = rule == GM_CLIP_ARC ? K - 1 - (2 * f * (K - f)) / K : 0;
  hipLaunchKernelGGL(clip_kspace, dim3(1), dim3(kClipTK), 0, s, w.sums, K, rule, rank, tau * tau,
                     w.scale, w.list, w.head, stats);
  HIPCHK(hipGetLastError());

  ApplyArgs b{};
  b.X = X; b.Y = Y; b.K = K; b.d = d;
  b.ldx = ldx; b.ldy = ldy;
  b.wsx = Wi ? wshift_of(Wi) : 0;
  b.wsy = Wo ? wshift_of(Wo) : 0;
  b.pin = Wi != 0;
  b.vy = reinterpret_cast<uintptr_t>(Y) % 16 == 0 && ldy % 4 == 0;
  b.vc = reinterpret_cast<uintptr_t>(centre) % 16 == 0;
  b.centre = centre; b.scale = w.scale;
  b.list = alias ? w.list : nullptr;
  b.head = w.head;
  // the grid covers every tile of a full list (in place the list's length is the device's)
  const int64_t per = Wi ? K * (Wi / E) : (d + E - 1) / E;
  const int64_t ct = (per + kClipTile - 1) / kClipTile;
  const int64_t ntiles = (Wi ? (d + Wi - 1) / Wi : K) * ct;
  const dim3 gb((unsigned)std::min<int64_t>(ntiles, kClipGrid2));
  if (vec)
    hipLaunchKernelGGL((clip_apply<SRC, EV>), gb, dim3(kClipT2), 0, s, b);
  else
    hipLaunchKernelGGL((clip_apply<SRC, 1>), gb, dim3(kClipT2), 0, s, b);
  HIPCHK(hipGetLastError());
  return GM_OK;
}

}  // namespace

}  // namespace gmk

extern "C" {

int gm_clip_rows_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                     int32_t layout_in, const float* centre, int32_t rule, int64_t f, double tau,
                     float* Y, int64_t ldy, int32_t layout_out, double* stats, void* stream) {
  return gmk::clip_rows("gm_clip_rows_f32", c, X, K, d, ldx, layout_in, centre, rule, f, tau, Y,
                        ldy, layout_out, stats, stream);
}

int gm_clip_rows_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                      int32_t layout_in, const float* centre, int32_t rule, int64_t f, double tau,
                      float* Y, int64_t ldy, int32_t layout_out, double* stats, void* stream) {
  return gmk::clip_rows("gm_clip_rows_bf16", c, X, K, d, ldx, layout_in, centre, rule, f, tau, Y,
                        ldy, layout_out, stats, stream);
}

}  // extern "C"
