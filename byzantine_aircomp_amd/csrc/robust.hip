// Aggregators built on the selection and Krum machinery of coordinate.hip:
//   MeaMed      (Xie, Koyejo & Gupta 2018) per column, the mean of the `keep` values nearest
//               to the column's lower median
//   Multi-Krum  (Blanchard et al. 2017) the mean of the m rows of smallest Krum score
//   Bulyan      (El Mhamdi, Guerraoui & Rouault 2018) theta rounds of Krum selection on the
//               remaining rows, then MeaMed over the selected rows
// The definitions (tie rules, summation orders) are in include/gmagg.h.
#include <algorithm>

#include "device_util.h"
#include "gmagg_internal.h"
#include "select_util.h"

namespace gmk {

// Nearest-to-median mean.  The tile is staged as col_select_st stages it (a block of NWV
// waves owns 16 columns, 64-byte row segments; rounds of SR rows go HBM -> registers -> LDS
// -> each wave's NC columns as keys in registers), with row k of the rows used read from
// row rows[k] of X when a list is given.  Per column pair the wave then
//   1. selects the lower median of the keys (select_ranks, the median's steps);
//   2. rebuilds each slot's key as the bits of dev = |x - med|: dev >= 0, so its bits are
//      ordered as unsigned integers, a NaN dev (inf - inf) lies above +inf, and a padding
//      slot's 0xFFFFFFFF above every NaN;
//   3. selects rank keep - 1 of those (the same steps): the threshold T;
//   4. sums the values with dev < T and, of those with dev == T, the first keep - #(dev < T)
//      in row order.  Lane l holds rows l, l + 64, ...: a tie's row rank is the ties of the
//      earlier slots plus those of lower lanes in its own slot (ballot + mbcnt); the branch
//      is wave-uniform and taken only when there are more ties than places.
// The sum is fp64: per lane in slot order, then the wave's xor-shuffle tree; divided by
// keep, rounded once.  One read of the rows used.
template <int R, int NC, int NWV>
__global__ void __launch_bounds__(NWV * 64) col_meamed(const float* __restrict__ X, int64_t n,
                                                       int64_t d, int64_t ldx, int ws,
                                                       const int32_t* __restrict__ rows,
                                                       int64_t keep, int vec4,
                                                       float* __restrict__ out) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  constexpr int C = NWV * NC;
  static_assert(C == 16, "64-byte row segments");
  constexpr int SR = R >= 4 ? 256 : 64 * R;        // rows per staging round
  constexpr int NRD = 64 * R / SR;                 // rounds
  constexpr int R2 = R >= 4 ? 2 : 0;
  constexpr int SLOTS = 64 * (R2 > 0 ? R2 : 1);
  // one rank per chain: select_ranks takes the counting steps, whose compaction needs 64 R2
  // slots; its histogram forms (256 bins per column) would overrun scr
  static_assert(GMK_SELECT_HIST == 0 || GMK_SELECT_HIST_NR > 1, "scr holds no histogram bins");
  constexpr int LPR = C / 4, RPI = NWV * 64 / LPR, NLD = (SR + RPI - 1) / RPI;
  static_assert(SR % 64 == 0 && (64 * R) % SR == 0, "round shape");
  __shared__ float stage[SR][C + 1];
  __shared__ uint32_t scr[NWV][NC][SLOTS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tq = threadIdx.x % LPR, tr = threadIdx.x / LPR;
  const int64_t ntiles = (d + C - 1) / C;
  const int64_t v = blockIdx.x;
  if (v >= ntiles) return;
  // blocks bid and bid + 8 share an XCD: adjacent tiles, one 128-B line's two halves
  const int64_t t = (v < ntiles / 16 * 16) ? v / 16 * 16 + (v % 8) * 2 + (v / 8) % 2 : v;
  const int64_t j0 = t * C;
  const int64_t col = j0 + 4 * tq;
  const bool vec = vec4 && col + 4 <= d;
  uint32_t key[NC][R];
  bool nan[NC];
#pragma unroll
  for (int h = 0; h < NC; ++h) nan[h] = false;
#pragma unroll
  for (int rd = 0; rd < NRD; ++rd) {
    f4 cur[NLD];
    // every load from a clamped row of the rows used, slots past n zeroed after, so the
    // loads go out back to back
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int k = rd * SR + tr + u * RPI;
      const int kc = k < (int)n ? k : (int)n - 1;
      const int64_t row = rows ? (int64_t)rows[kc] : (int64_t)kc;
      const float* src = elem(X, ldx, ws, row, col);
      f4 x = f4{0.f, 0.f, 0.f, 0.f};
      if (vec) {
        x = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = col + e < d ? src[e] : 0.f;
      }
      cur[u] = k < (int)n ? x : f4{0.f, 0.f, 0.f, 0.f};
    }
    if (rd > 0) __syncthreads();                   // the previous round's reads are done
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int r = tr + u * RPI;
      if (SR % RPI == 0 || r < SR) {
#pragma unroll
        for (int e = 0; e < 4; ++e) stage[r][4 * tq + e] = cur[u][e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NC; ++h) {
      const bool cok = j0 + w * NC + h < d;        // wave-uniform
#pragma unroll
      for (int i = 0; i < SR / 64; ++i) {
        const int row = rd * SR + lane + 64 * i;
        const bool ok = cok && row < (int)n;
        const float x = stage[lane + 64 * i][w * NC + h];
        key[h][rd * (SR / 64) + i] = slot_key<false>(x, ok);
        nan[h] |= ok && x != x;
      }
    }
  }
  auto bufc = [&](int h, int q) { return &scr[w][h][q * SLOTS]; };
  // 1. the lower median
  float med[NC];
  {
    const int64_t rk[1] = {(n - 1) / 2};
    uint32_t ans[NC][1];
    int clo[NC][1], chi[NC][1];
    select_ranks<R, NC, 1, R2, 1>(key, rk, ans, clo, chi, bufc);
#pragma unroll
    for (int h = 0; h < NC; ++h) med[h] = key_value(ans[h][0]);
  }
  // (the compaction slots are reused by the second selection)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // 2. the deviations' keys
  uint32_t dk[NC][R];
#pragma unroll
  for (int h = 0; h < NC; ++h)
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const bool ok = lane + 64 * i < (int)n;
      const float dev = __builtin_fabsf(key_value(key[h][i]) - med[h]);
      dk[h][i] = ok ? __float_as_uint(dev) : 0xFFFFFFFFu;
    }
  // 3. the threshold
  uint32_t thr[NC];
  {
    const int64_t rk[1] = {keep - 1};
    uint32_t ans[NC][1];
    int clo[NC][1], chi[NC][1];
    select_ranks<R, NC, 1, R2, 1>(dk, rk, ans, clo, chi, bufc);
#pragma unroll
    for (int h = 0; h < NC; ++h) thr[h] = ans[h][0];
  }
  // 4. the sum of what lies below the threshold and of the ties that have a place
  float res[NC];
#pragma unroll
  for (int h = 0; h < NC; ++h) {
    const uint32_t T = thr[h];
    int lt = 0, eq = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      lt += __popcll(__ballot(dk[h][i] < T));
      eq += __popcll(__ballot(dk[h][i] == T));
    }
    const int need = (int)keep - lt;               // 1 <= need <= eq
    double sv = 0.0;
    if (need >= eq) {
#pragma unroll
      for (int i = 0; i < R; ++i)
        if (dk[h][i] <= T) sv += (double)key_value(key[h][i]);
    } else {
      int base = 0;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const bool tie = dk[h][i] == T;
        const uint64_t m = __ballot(tie);
        const int pos = base + (int)__builtin_amdgcn_mbcnt_hi(
                                   (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (dk[h][i] < T || (tie && pos < need)) sv += (double)key_value(key[h][i]);
        base += __popcll(m);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sv += __shfl_xor(sv, o);
    res[h] = __ballot(nan[h]) ? __uint_as_float(0x7FC00000u) : (float)(sv / (double)keep);
  }
  if (lane == 0) {
#pragma unroll
    for (int h = 0; h < NC; ++h)
      if (j0 + w * NC + h < d) out[j0 + w * NC + h] = res[h];
  }
}

hipError_t launch_meamed(const float* X, int64_t d, int64_t ldx, int ws, const int32_t* rows,
                         int64_t n, int64_t keep, float* out, hipStream_t s) {
  if (n < 1 || n > 1024 || keep < 1 || keep > n) return hipErrorInvalidValue;
  if (d <= 0) return hipSuccess;
  const int vec4 = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 4 == 0;
  const dim3 g((unsigned)((d + 15) / 16));
#define GMK_MM(R_)                                                                              \
  hipLaunchKernelGGL((col_meamed<R_, 2, 8>), g, dim3(512), 0, s, X, n, d, ldx, ws, rows, keep,  \
                     vec4, out)
  if (n <= 64) GMK_MM(1);
  else if (n <= 128) GMK_MM(2);
  else if (n <= 256) GMK_MM(4);
  else if (n <= 512) GMK_MM(8);
  else GMK_MM(16);
#undef GMK_MM
  return hipGetLastError();
}

// a before b in the order of scores: smaller first, NaN last, ties to the lower index
__device__ __forceinline__ bool score_before(double a, int64_t i, double b, int64_t j) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? i < j : bn;
  return a < b || (a == b && i < j);
}

// flag[i] = 1 for the m rows first in the order of scores (a stable top-m), else 0.
__global__ void __launch_bounds__(256) score_top_m(const double* __restrict__ score, int64_t K,
                                                   int64_t m, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  const double si = score[i];
  int64_t rank = 0;
  for (int64_t j = 0; j < K; ++j) rank += score_before(score[j], j, si, i);
  flag[i] = rank < m;
}

// One wave: the indices i < K with flag[i] == want, increasing -> list.
__global__ void __launch_bounds__(64) flags_to_list(const int32_t* __restrict__ flag, int64_t K,
                                                    int32_t want, int32_t* __restrict__ list) {
  const int lane = threadIdx.x;
  int64_t n = 0;
  for (int64_t i0 = 0; i0 < K; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool in = i < K && flag[i] == want;
    const uint64_t b = __ballot(in);
    const int64_t pos = n + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (in) list[pos] = (int32_t)i;
    n += __popcll(b);
  }
}

// out = the mean of rows list[0 .. m-1] (increasing): per column the fp64 sum in list
// order, divided by m, rounded once.  W consecutive columns per thread as col_mean.
template <int W>
__global__ void __launch_bounds__(256) gather_mean(const float* __restrict__ X, int64_t d,
                                                   int64_t ldx, int ws,
                                                   const int32_t* __restrict__ list, int64_t m,
                                                   float* __restrict__ out) {
  typedef float fv __attribute__((ext_vector_type(W)));
  const int64_t G = W > 1 ? d / W : d;             // W > 1: d % W == 0 (checked by the launcher)
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += (int64_t)gridDim.x * blockDim.x) {
    double s[W];
    {
      const fv x = *reinterpret_cast<const fv*>(elem(X, ldx, ws, list[0], g * W));
#pragma unroll
      for (int v = 0; v < W; ++v) s[v] = (double)x[v];
    }
    for (int64_t t = 1; t < m; ++t) {
      const fv x = *reinterpret_cast<const fv*>(elem(X, ldx, ws, list[t], g * W));
#pragma unroll
      for (int v = 0; v < W; ++v) s[v] += (double)x[v];
    }
    // (m == 1: the row itself, its zero's sign included)
#pragma unroll
    for (int v = 0; v < W; ++v) out[g * W + v] = m == 1 ? (float)s[v] : (float)(s[v] / (double)m);
  }
}

hipError_t launch_score_top_m(const double* score, int64_t K, int64_t m, int32_t* flag,
                              hipStream_t s) {
  hipLaunchKernelGGL(score_top_m, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, score, K, m,
                     flag);
  return hipGetLastError();
}

hipError_t launch_flags_to_list(const int32_t* flag, int64_t K, int32_t want, int32_t* list,
                                hipStream_t s) {
  hipLaunchKernelGGL(flags_to_list, dim3(1), dim3(64), 0, s, flag, K, want, list);
  return hipGetLastError();
}

hipError_t launch_multi_krum_pick(const double* score, int64_t K, int64_t m, const float* X,
                                  int64_t d, int64_t ldx, int ws, int32_t* flag, int32_t* list,
                                  float* out, hipStream_t s) {
  (void)launch_score_top_m(score, K, m, flag, s);
  (void)launch_flags_to_list(flag, K, 1, list, s);
  return launch_gather_mean(X, d, ldx, ws, list, m, out, s);
}

// gather_mean on bf16 bit patterns: 8 consecutive columns per thread (one 16-byte load per
// listed row; VEC: base 16-byte aligned, ldx % 8 == 0), the ragged last group and the
// unaligned form one column at a time.  Per column the same fp64 sum in list order.
template <bool VEC>
__global__ void __launch_bounds__(256) gather_mean_bf16(const uint16_t* __restrict__ X, int64_t d,
                                                        int64_t ldx, int ws,
                                                        const int32_t* __restrict__ list,
                                                        int64_t m, float* __restrict__ out) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  constexpr int W = VEC ? 8 : 1;
  const int64_t G = (d + W - 1) / W;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j0 = g * W;
    if (VEC && j0 + 8 <= d) {
      double s[8];
      for (int64_t t = 0; t < m; ++t) {
        const u4 x = *reinterpret_cast<const u4*>(elem(X, ldx, ws, list[t], j0));
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const double lo = (double)__uint_as_float(x[v] << 16);
          const double hi = (double)__uint_as_float(x[v] & 0xFFFF0000u);
          s[2 * v] = t == 0 ? lo : s[2 * v] + lo;
          s[2 * v + 1] = t == 0 ? hi : s[2 * v + 1] + hi;
        }
      }
#pragma unroll
      for (int v = 0; v < 8; ++v) out[j0 + v] = m == 1 ? (float)s[v] : (float)(s[v] / (double)m);
    } else {
      for (int v = 0; v < W && j0 + v < d; ++v) {
        double s = (double)widen(*elem(X, ldx, ws, list[0], j0 + v));
        for (int64_t t = 1; t < m; ++t) s += (double)widen(*elem(X, ldx, ws, list[t], j0 + v));
        out[j0 + v] = m == 1 ? (float)s : (float)(s / (double)m);
      }
    }
  }
}

hipError_t launch_gather_mean(const uint16_t* X, int64_t d, int64_t ldx, int ws,
                              const int32_t* list, int64_t m, float* out, hipStream_t s) {
  if (d > 0) {
    const bool v8 = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 8 == 0;
    const int64_t items = v8 ? (d + 7) / 8 : d;
    const dim3 g((unsigned)std::min<int64_t>((items + 255) / 256, 4096));
    if (v8)
      hipLaunchKernelGGL(gather_mean_bf16<true>, g, dim3(256), 0, s, X, d, ldx, ws, list, m, out);
    else
      hipLaunchKernelGGL(gather_mean_bf16<false>, g, dim3(256), 0, s, X, d, ldx, ws, list, m, out);
  }
  return hipGetLastError();
}

hipError_t launch_multi_krum_pick(const double* score, int64_t K, int64_t m, const uint16_t* X,
                                  int64_t d, int64_t ldx, int ws, int32_t* flag, int32_t* list,
                                  float* out, hipStream_t s) {
  (void)launch_score_top_m(score, K, m, flag, s);
  (void)launch_flags_to_list(flag, K, 1, list, s);
  return launch_gather_mean(X, d, ldx, ws, list, m, out, s);
}

hipError_t launch_gather_mean(const float* X, int64_t d, int64_t ldx, int ws, const int32_t* list,
                              int64_t m, float* out, hipStream_t s) {
  if (d > 0) {
    const bool v4 = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 4 == 0 && d % 4 == 0;
    const int64_t items = v4 ? d / 4 : d;
    const dim3 g((unsigned)std::min<int64_t>((items + 255) / 256, 4096));
    if (v4)
      hipLaunchKernelGGL(gather_mean<4>, g, dim3(256), 0, s, X, d, ldx, ws, list, m, out);
    else
      hipLaunchKernelGGL(gather_mean<1>, g, dim3(256), 0, s, X, d, ldx, ws, list, m, out);
  }
  return hipGetLastError();
}

// A distance as an unsigned key: D >= 0, so the bits are ordered as the values; a NaN (sign
// cleared) lies above +inf, which keeps the order total whatever the input holds.
__device__ __forceinline__ unsigned long long dist_key(double x) {
  return (unsigned long long)__double_as_longlong(x) & 0x7FFFFFFFFFFFFFFFull;
}

// Bulyan, once (one block per row): ord[i][r] = the column of row i's r-th smallest distance
// by stable rank (the order krum_row_score ranks in).  The rounds below only walk this list:
// ranking the row again every round (K^2 compares per row) measured 6x the distances' time.
__global__ void __launch_bounds__(256) bulyan_row_order(const double* __restrict__ D, int64_t K,
                                                        int32_t* __restrict__ ord) {
  extern __shared__ unsigned long long skey[];
  const int64_t i = blockIdx.x;
  for (int64_t j = threadIdx.x; j < K; j += blockDim.x)
    skey[j] = dist_key(D[i <= j ? i * K + j : j * K + i]);
  __syncthreads();
  for (int64_t j = threadIdx.x; j < K; j += blockDim.x) {
    const unsigned long long x = skey[j];
    int64_t rank = 0;
    for (int64_t t = 0; t < K; ++t) rank += (skey[t] < x) || (skey[t] == x && t < j);
    ord[i * K + rank] = (int32_t)j;
  }
}

// Bulyan, one round's scores (one block per row): for a row i still in S, the sum of the kk
// smallest D[i][j], j in S (self included), by stable rank.  The kk-th entry of ord[i] that
// is still in S is the threshold (thread t counts the list's entries t P .. t P + P - 1, a
// block scan places the kk-th); the score is then summed fresh from D in krum_row_score's
// order (per thread in j order, block_sum), so identical rows give identical bits.
__global__ void __launch_bounds__(256) bulyan_score(const double* __restrict__ D,
                                                    const int32_t* __restrict__ ord, int64_t K,
                                                    int64_t kk, const int32_t* __restrict__ alive,
                                                    double* __restrict__ score) {
  __shared__ double scratch[8];
  __shared__ int wtot[4];
  __shared__ int s_thr;
  const int64_t i = blockIdx.x;
  if (!alive[i]) return;                           // (block-uniform)
  const int32_t* o = ord + i * K;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int P = (int)((K + 255) / 256);
  const int r0 = threadIdx.x * P;
  if (threadIdx.x == 0) s_thr = -1;
  int c = 0;
  for (int p = 0; p < P; ++p)
    if (r0 + p < (int)K) c += alive[o[r0 + p]] != 0;
  const int incl = wave_scan_i32(c);
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  int excl = incl - c;
  for (int q = 0; q < w; ++q) excl += wtot[q];
  if (excl < (int)kk && (int)kk <= excl + c) {     // this thread's entries hold the kk-th
    int n = excl;
    for (int p = 0; p < P; ++p)
      if (r0 + p < (int)K && alive[o[r0 + p]] != 0 && ++n == (int)kk) s_thr = o[r0 + p];
  }
  __syncthreads();
  const int64_t jt = s_thr;                        // (-1, fewer than kk rows in S: all of them)
  const unsigned long long vt =
      jt >= 0 ? dist_key(D[i <= jt ? i * K + jt : jt * K + i]) : ~0ull;
  double sc = 0.0;
  for (int64_t j = threadIdx.x; j < K; j += blockDim.x) {
    const double x = D[i <= j ? i * K + j : j * K + i];
    const unsigned long long k = dist_key(x);
    if (alive[j] != 0 && (k < vt || (k == vt && j <= jt))) sc += x;
  }
  sc = block_sum(sc, scratch);
  if (threadIdx.x == 0) score[i] = sc;
}

// Bulyan, one round's pick (one wave): the row of S first in the order of scores leaves S
// and becomes order[t].
__global__ void __launch_bounds__(64) bulyan_pick(const double* __restrict__ score, int64_t K,
                                                  int32_t* __restrict__ alive, int64_t t,
                                                  int32_t* __restrict__ order) {
  int64_t best = -1;
  double bv = 0.0;
  for (int64_t i = threadIdx.x; i < K; i += 64)
    if (alive[i] && (best < 0 || score_before(score[i], i, bv, best))) { bv = score[i]; best = i; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o);
    const int64_t oi = __shfl_xor(best, o);
    if (oi >= 0 && (best < 0 || score_before(ov, oi, bv, best))) { bv = ov; best = oi; }
  }
  if (threadIdx.x == 0 && best >= 0) {
    alive[best] = 0;
    order[t] = (int32_t)best;
  }
}

__global__ void __launch_bounds__(256) fill_i32(int32_t* __restrict__ p, int64_t n, int32_t v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

hipError_t launch_bulyan_select(const double* D, int64_t K, int64_t f, int64_t theta,
                                double* score, int32_t* ord, int32_t* alive, int32_t* order,
                                int32_t* list, hipStream_t s) {
  hipLaunchKernelGGL(fill_i32, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, alive, K, 1);
  hipLaunchKernelGGL(bulyan_row_order, dim3((unsigned)K), dim3(256), sizeof(unsigned long long) * K,
                     s, D, K, ord);
  hipError_t e = hipGetLastError();
  // (every round launches K blocks: those of rows that left S return at once)
  for (int64_t t = 0; t < theta && e == hipSuccess; ++t) {
    const int64_t kk = std::max<int64_t>(1, (K - t) - f - 1);
    hipLaunchKernelGGL(bulyan_score, dim3((unsigned)K), dim3(256), 0, s, D, ord, K, kk, alive,
                       score);
    hipLaunchKernelGGL(bulyan_pick, dim3(1), dim3(64), 0, s, score, K, alive, t, order);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flags_to_list, dim3(1), dim3(64), 0, s, alive, K, 0, list);
  return hipGetLastError();
}

}  // namespace gmk
