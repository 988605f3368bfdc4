// mean, median and trimmed_mean (coordinate.hip) on bf16 client updates: X holds bfloat16 bit
// patterns (uint16_t), rows [K][ldx] or bf16 panels [ceil(d/W)][K][W] (W =
// gm_panel_width_bf16(K), ldx = the panel stride).  The results are the fp32 kernels'
// definitions applied to the widened values (bits << 16, exact), out is fp32.  gm_mean_bf16 /
// gm_median_bf16 / gm_trimmed_mean_bf16 at the end of this file are the host side.
//
// Mean: 8 consecutive columns per thread where the base is 16-byte aligned and ldx % 8 == 0 (one
// 16-byte load per row, 8 rows' loads in flight), else one column per thread (any 2-byte
// alignment, any ldx >= d, odd d).  Each column is summed in fp64 in row order and rounded once:
// the same sum on either path and on panels.
//
// Median / trimmed mean: bit-wise selection (coordinate.hip "Order statistics") on 16-bit
// order-preserving keys, so a rank is decided in 16 counting steps instead of 32.  The key
// mapping is slot_key / order_key restated on 16 bits: -0 folded onto +0, negatives
// bit-inverted, positives with the top bit set, padding slots (rows >= K, columns >= d) 0xFFFF;
// every NaN 0xFFFF for the trimmed mean (torch's top-k order), and the median of a column that
// holds a NaN is NaN.  A block owns C = 32 columns (64-byte row segments; adjacent tiles on one
// XCD as col_select1) and never holds the tile whole: rounds of <= 256 rows go HBM ->
// registers (16-byte loads, every round's loads issued up front) -> a bf16 LDS stage (34
// halfwords per row: a column is read down the stage conflict-free, two columns per 32-bit
// read) -> each wave's NC columns as keys in registers.  A wave selects its columns in pairs.
// The median: two interleaved chains of select_util.h's select_steps on bits 15..0; at R >= 8
// keys per lane each lane counts its own keys and the two chains share one DPP wave sum (16-bit
// halves); no compaction.  The trimmed mean at R >= 4: no counting steps at all, two 256-bin
// LDS histograms per rank (ranks_hist16 below); below that, four chains of counting steps.
//   K <= 128          R = 1, 2    4 waves x 8 columns
//   K <= 512          R = 4, 8    8 waves x 4 columns
//   K <= 2048         R = 16, 32  16 waves x 2 columns
// The trimmed mean sums the keys strictly inside (lo, hi) per lane in slot order (two fp64
// accumulators, even and odd slots), then across the wave by an xor butterfly, and adds the
// boundary ties counted from the selection's final intervals: an order that depends on (K,
// column) only, so the aligned rows, the one-element rows and the panels give the same bits.
#include <algorithm>

#include "device_util.h"
#include "host_ctx.h"
#include "select_util.h"

namespace gmk {

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// Element (row k, column j): rows [K][ldx] (ws = 0) or bf16 panels with W = 2^ws, ldx = the
// panel stride.  8 columns from a multiple of 8 never straddle a panel (W % 8 == 0).
__device__ __forceinline__ const uint16_t* elem16(const uint16_t* X, int64_t ldx, int ws,
                                                  int64_t k, int64_t j) {
  return ws ? X + (j >> ws) * ldx + (k << ws) + (j & ((1 << ws) - 1)) : X + k * ldx + j;
}
__device__ __forceinline__ float widen16(uint32_t bits) { return __uint_as_float(bits << 16); }

template <bool VEC>
__global__ void __launch_bounds__(256) col_mean_bf16(const uint16_t* __restrict__ X, int64_t K,
                                                     int64_t d, int64_t ldx, int ws,
                                                     float* __restrict__ out) {
  constexpr int W = VEC ? 8 : 1, U = 8;
  const int64_t G = (d + W - 1) / W;
  const int64_t rs = ws ? ((int64_t)1 << ws) : ldx;   // row stride
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j0 = g * W;
    const uint16_t* col = elem16(X, ldx, ws, 0, j0);
    if (VEC && j0 + 8 <= d) {
      double s[8];
#pragma unroll
      for (int v = 0; v < 8; ++v) s[v] = 0.0;
      auto add = [&](const u4& x) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          s[2 * v] += (double)__uint_as_float(x[v] << 16);
          s[2 * v + 1] += (double)__uint_as_float(x[v] & 0xFFFF0000u);
        }
      };
      int64_t k = 0;
      for (; k + U <= K; k += U) {
        u4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          x[u] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(col + (k + u) * rs));
#pragma unroll
        for (int u = 0; u < U; ++u) add(x[u]);
      }
      for (; k < K; ++k) add(*reinterpret_cast<const u4*>(col + k * rs));
#pragma unroll
      for (int v = 0; v < 8; ++v) out[j0 + v] = (float)(s[v] / (double)K);
    } else {
      // one column at a time: the whole grid on the one-element path, the ragged last group
      // (d % 8 columns) on the 16-byte path
      for (int v = 0; v < W && j0 + v < d; ++v) {
        double s = 0.0;
        int64_t k = 0;
        for (; k + U <= K; k += U) {
          uint16_t x[U];
#pragma unroll
          for (int u = 0; u < U; ++u) x[u] = __builtin_nontemporal_load(col + v + (k + u) * rs);
#pragma unroll
          for (int u = 0; u < U; ++u) s += (double)widen16(x[u]);
        }
        for (; k < K; ++k) s += (double)widen16(col[v + k * rs]);
        out[j0 + v] = (float)(s / (double)K);
      }
    }
  }
}

// 16-bit order keys of bf16 bit patterns (select_util.h slot_key / key_value on 16 bits).
template <bool NANTOP>
__device__ __forceinline__ uint32_t slot_key16(uint32_t bits, bool ok) {
  const uint32_t u = bits == 0x8000u ? 0u : bits;
  uint32_t k = u ^ ((u & 0x8000u) ? 0xFFFFu : 0x8000u);
  if constexpr (NANTOP) k = (bits & 0x7FFFu) > 0x7F80u ? 0xFFFFu : k;
  return ok ? k : 0xFFFFu;
}
__device__ __forceinline__ float key_value16(uint32_t k) {
  return widen16((k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu));
}

// The ranks of one column pair from two 256-bin histograms instead of counting steps
// (use_hist16): a 16-bit key is its top byte and its low byte, so one histogram of the top
// bytes (one LDS atomic add per held key, a wave prefix scan, shared by the column's ranks)
// and, per rank, one of the low bytes of the keys inside the rank's top-byte bin decide the key
// exactly, with clo = #(keys < ans) and chi = #(keys <= ans) from the bins.  bins: this wave's
// [2][256] words.
// The trimmed mean's kernels take it from K > 128 (R >= 4): its two ranks share the first
// histogram.  The median keeps the counting steps: at K = 1000 x 2M both measured 2.93 ms (the
// adds to the few bins a column's top bytes fill serialize, as coordinate.hip found for fp32),
// and at R = 32 the bins' addressing next to 64 key registers spilled.
constexpr bool use_hist16(int mode, int R) { return mode == 1 && R >= 4; }
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The bin holding rank rr among bins whose counts this lane holds four of (hb; excl = the count
// below the lane's first bin, all wave-wide counts offset alike): its index, the count below
// it and the count up to its end.
__device__ __forceinline__ void find_bin(const int (&hb)[4], int excl, int incl, int rr, int end,
                                         int& bsel, int& blo, int& bhi) {
  const uint64_t m = __ballot(excl <= rr && rr < incl);
  const int L = __builtin_amdgcn_readfirstlane(m ? __builtin_ctzll(m) : 63);
  int lo = __builtin_amdgcn_readlane(excl, L);
  bsel = 4 * L + 3;
  blo = lo;
  bhi = end;
  bool found = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int hj = __builtin_amdgcn_readlane(hb[j], L);
    if (!found && lo + hj > rr) {
      found = true;
      bsel = 4 * L + j;
      blo = lo;
      bhi = lo + hj;
    }
    lo += hj;
  }
}
template <int R, int NR>
__device__ __forceinline__ void ranks_hist16(const uint32_t (&key)[2][R], const int (&rr)[NR],
                                             uint32_t* bins, uint32_t (&ans)[2][NR],
                                             int (&clo)[2][NR], int (&chi)[2][NR]) {
  const int lane = threadIdx.x & 63;
  wave_lds_fence();                                  // (the bins are this pair's now)
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) bins[c * 256 + 4 * lane + j] = 0u;
  wave_lds_fence();
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < R; ++i)
      __hip_atomic_fetch_add(&bins[c * 256 + (key[c][i] >> 8)], 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WAVEFRONT);
  wave_lds_fence();
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    int hb[4], sl = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hb[j] = (int)bins[c * 256 + 4 * lane + j];
      sl += hb[j];
    }
    const int incl = wave_scan_i32(sl), excl = incl - sl;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      // the bins count all 64 R keys, padding included, and rr < K <= 64 R: exactly one lane
      int bsel, blo, bhi;
      find_bin(hb, excl, incl, rr[q], 64 * R, bsel, blo, bhi);
      ans[c][q] = (uint32_t)bsel << 8;              // keys < ans: blo; keys < ans + 256: bhi
      clo[c][q] = blo;
      chi[c][q] = bhi;
    }
  }
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    wave_lds_fence();                                // the bins are consumed
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) bins[c * 256 + 4 * lane + j] = 0u;
    wave_lds_fence();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint32_t top = ans[c][q] >> 8;
#pragma unroll
      for (int i = 0; i < R; ++i)
        if ((key[c][i] >> 8) == top)
          __hip_atomic_fetch_add(&bins[c * 256 + (key[c][i] & 255u)], 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    wave_lds_fence();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      int hb[4], sl = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hb[j] = (int)bins[c * 256 + 4 * lane + j];
        sl += hb[j];
      }
      const int incl = wave_scan_i32(sl) + clo[c][q], excl = incl - sl;
      int bsel, blo, bhi;
      find_bin(hb, excl, incl, rr[q], chi[c][q], bsel, blo, bhi);
      ans[c][q] |= (uint32_t)bsel;
      clo[c][q] = blo;
      chi[c][q] = bhi;
    }
  }
}

// The order statistics of one column pair whose keys the wave holds (lane l: rows l + 64 i):
// res[h] = the median (MODE 0) or the trimmed mean (MODE 1) of column h.
template <int MODE, int R>
__device__ __forceinline__ void select_pair16(const uint32_t (&key)[2][R], const bool (&nan)[2],
                                              int64_t K, int64_t b, uint32_t* bins,
                                              float (&res)[2]) {
  constexpr int NR = MODE == 0 ? 1 : 2;
  int rr[NR];
  if constexpr (MODE == 0) {
    rr[0] = (int)((K - 1) / 2);
  } else {
    rr[0] = (int)b;
    rr[1] = (int)(K - b - 1);
  }
  uint32_t ans[2][NR];
  int clo[2][NR], chi[2][NR];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      ans[c][q] = 0;
      clo[c][q] = 0;
      chi[c][q] = 64 * R;      // padding keys (0xFFFF) count as keys: never below t
    }
  if constexpr (use_hist16(MODE, R)) {
    ranks_hist16<R, NR>(key, rr, bins, ans, clo, chi);
  } else
  select_steps<2, NR>(15, 0, ans, clo, chi, rr,
                      [&](const uint32_t (&t)[2][NR], int (&cnt)[2][NR]) {
    if constexpr (R >= 8) {
      // per-lane counts (v_cmp + v_addc per key), two chains per DPP wave sum: a count is at
      // most 64 R <= 2048, so two fit the halves of one register
      int lc[2 * NR];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          int v = 0;
#pragma unroll
          for (int i = 0; i < R; ++i) v += (int)(key[c][i] < t[c][q]);
          lc[c * NR + q] = v;
        }
#pragma unroll
      for (int p = 0; p < 2 * NR; p += 2) {
        const int s2 = wave_sum_i32(lc[p] + (lc[p + 1] << 16));
        cnt[p / NR][p % NR] = s2 & 0xFFFF;
        cnt[(p + 1) / NR][(p + 1) % NR] = s2 >> 16;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          int n = 0;
#pragma unroll
          for (int i = 0; i < R; ++i) n += __popcll(__ballot(key[c][i] < t[c][q]));
          cnt[c][q] = n;
        }
    }
  });
  if constexpr (MODE == 0) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      res[h] = __ballot(nan[h]) ? __uint_as_float(0x7FC00000u) : key_value16(ans[h][0]);
  } else {
    const int64_t n = K - 2 * b;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t lo = ans[h][0], hi = ans[h][1];
      const float vlo = key_value16(lo), vhi = key_value16(hi);
      double sum;
      if (lo == hi) {
        sum = (double)n * (double)vlo;
      } else {
        // after the last step rank b's interval is [lo, lo + 1): #(keys <= lo) = its chi, and
        // #(keys < hi) = rank K-b-1's clo (padding keys are 0xFFFF > lo and never < hi)
        double sv0 = 0.0, sv1 = 0.0;
        const int64_t le_lo = chi[h][0], lt_hi = clo[h][1];
#pragma unroll
        for (int i = 0; i < R; i += 2) {
          if (key[h][i] > lo && key[h][i] < hi) sv0 += (double)key_value16(key[h][i]);
          if (i + 1 < R && key[h][i + 1] > lo && key[h][i + 1] < hi)
            sv1 += (double)key_value16(key[h][i + 1]);
        }
        double sv = sv0 + sv1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sv += __shfl_xor(sv, o);
        sum = sv + (double)(le_lo - b) * (double)vlo + (double)((K - b) - lt_hi) * (double)vhi;
      }
      res[h] = (float)(sum / (double)n);
    }
  }
}

template <int MODE, int R, int NC, int NWV>
__global__ void __launch_bounds__(NWV * 64) col_select_bf16(const uint16_t* __restrict__ X,
                                                            int64_t K, int64_t d, int64_t ldx,
                                                            int ws, int64_t b, int vec8,
                                                            float* __restrict__ out) {
  constexpr int C = NWV * NC;
  static_assert(C == 32 && NC % 2 == 0, "64-byte row segments, columns in pairs");
  constexpr int SR = 64 * R < 256 ? 64 * R : 256;   // rows per staging round
  constexpr int NRD = 64 * R / SR;                  // rounds
  constexpr int LPR = C / 8, RPI = NWV * 64 / LPR, NLD = SR / RPI;
  static_assert(SR % RPI == 0 && NLD >= 1 && (64 * R) % SR == 0, "round shape");
  constexpr int SW = C / 2 + 1;                     // stage row stride in 32-bit words (odd)
  __shared__ uint32_t stage[SR][SW];                // bf16 pairs: columns 2m, 2m + 1 in word m
  constexpr bool HIST = use_hist16(MODE, R);
  __shared__ uint32_t bins[HIST ? NWV : 1][HIST ? 512 : 1];   // ranks_hist16's, per wave
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tq = threadIdx.x % LPR, tr = threadIdx.x / LPR;
  const int64_t ntiles = (d + C - 1) / C;
  const int64_t v = blockIdx.x;
  if (v >= ntiles) return;
  // blocks bid and bid + 8 share an XCD: adjacent tiles, one 128-B line's two halves
  const int64_t t = (v < ntiles / 16 * 16) ? v / 16 * 16 + (v % 8) * 2 + (v / 8) % 2 : v;
  const int64_t j0 = t * C;
  const int64_t col = j0 + 8 * tq;
  const bool vec = vec8 && col + 8 <= d;
  // a whole in-range, aligned tile (wave-uniform): every load issued unconditionally from a
  // clamped row and zeroed after; the edge tile and the one-element path guard each element
  const bool vec_tile = vec8 && j0 + C <= d;
  u4 buf[NRD][NLD];
#pragma unroll
  for (int rd = 0; rd < NRD; ++rd) {
    if (vec_tile) {
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const int k = rd * SR + tr + u * RPI;
        const u4 x = __builtin_nontemporal_load(
            reinterpret_cast<const u4*>(elem16(X, ldx, ws, k < (int)K ? k : (int)K - 1, col)));
        buf[rd][u] = k < (int)K ? x : u4{0u, 0u, 0u, 0u};
      }
    } else {
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const int64_t k = rd * SR + tr + (int64_t)u * RPI;
        u4 x = {0u, 0u, 0u, 0u};
        if (k < K && col < d) {
          const uint16_t* src = elem16(X, ldx, ws, k, col);
          if (vec) {
            x = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src));
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint32_t h = col + e < d ? (uint32_t)src[e] : 0u;
              x[e >> 1] |= h << (16 * (e & 1));
            }
          }
        }
        buf[rd][u] = x;
      }
    }
  }
  uint32_t key[NC][R];
  bool nan[NC];
#pragma unroll
  for (int h = 0; h < NC; ++h) nan[h] = false;
#pragma unroll
  for (int rd = 0; rd < NRD; ++rd) {
    if (rd > 0) __syncthreads();                   // the previous round's reads are done
#pragma unroll
    for (int u = 0; u < NLD; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) stage[tr + u * RPI][4 * tq + e] = buf[rd][u][e];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NC; h += 2) {
      const bool ok0 = j0 + w * NC + h < d, ok1 = j0 + w * NC + h + 1 < d;   // wave-uniform
#pragma unroll
      for (int i = 0; i < SR / 64; ++i) {
        const int row = rd * SR + lane + 64 * i;
        const bool rok = row < (int)K;
        const uint32_t x = stage[lane + 64 * i][(w * NC + h) >> 1];
        const uint32_t x0 = x & 0xFFFFu, x1 = x >> 16;
        key[h][rd * (SR / 64) + i] = slot_key16<MODE == 1>(x0, rok && ok0);
        key[h + 1][rd * (SR / 64) + i] = slot_key16<MODE == 1>(x1, rok && ok1);
        nan[h] |= rok && ok0 && (x0 & 0x7FFFu) > 0x7F80u;
        nan[h + 1] |= rok && ok1 && (x1 & 0x7FFFu) > 0x7F80u;
      }
    }
  }
#pragma unroll
  for (int h = 0; h < NC; h += 2) {
    if (j0 + w * NC + h >= d) break;               // wave-uniform
    float res[2];
    const bool np[2] = {nan[h], nan[h + 1]};
    uint32_t kp[2][R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      kp[0][i] = key[h][i];
      kp[1][i] = key[h + 1][i];
    }
    select_pair16<MODE, R>(kp, np, K, b, bins[HIST ? w : 0], res);
    if (lane == 0) {
      out[j0 + w * NC + h] = res[0];
      if (j0 + w * NC + h + 1 < d) out[j0 + w * NC + h + 1] = res[1];
    }
  }
}

int grid_cols16(int64_t groups) {
  const int64_t g = (groups + 255) / 256;
  return (int)(g < 4096 ? (g > 0 ? g : 1) : 4096);
}

// mode: -1 the mean, 0 the median, 1 the trimmed mean; fn names the entry point.
int coordinate_bf16(const char* fn, gm_ctx* c, const uint16_t* X, int64_t K, int64_t d,
                    int64_t ldx, int32_t layout, int mode, int64_t trim, float* out,
                    void* stream) {
  using namespace gmh;
  if (!c || !X || !out || K < 1 || d < 0 ||
      (layout != GM_LAYOUT_ROWS && layout != GM_LAYOUT_PANELS))
    return fail(GM_ERR_INVALID, "%s: bad args (a NULL ctx, X or out, K < 1, d < 0 or an unknown "
                "layout)", fn);
  if (mode == 1 && (trim < 0 || 2 * trim >= K))
    return fail(GM_ERR_INVALID, "%s: trim = %lld outside 0 <= 2 trim <= K - 1 = %lld", fn,
                (long long)trim, (long long)(K - 1));
  if (layout == GM_LAYOUT_ROWS && ldx < d)
    return fail(GM_ERR_INVALID, "%s: ldx = %lld < d = %lld", fn, (long long)ldx, (long long)d);
  if (mode >= 0 && K > 2048) return fail(GM_ERR_UNSUPPORTED, "%s: K <= 2048", fn);
  int ws = 0;
  if (layout == GM_LAYOUT_PANELS) {
    const int64_t W = gm_panel_width_bf16(K);
    if (W == 0)
      return fail(GM_ERR_UNSUPPORTED, "%s: no panel layout for K = %lld rows (pass them "
                  "row-major)", fn, (long long)K);
    if (ldx < K * W)
      return fail(GM_ERR_INVALID, "%s: panel stride %lld < K * W = %lld", fn, (long long)ldx,
                  (long long)(K * W));
    ws = wshift_of(W);
  }
  if (d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the 16-byte path: base and strides multiples of 8 elements (panel widths always are)
  const int vec8 = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 8 == 0;
  if (mode < 0) {
    if (vec8)
      hipLaunchKernelGGL(col_mean_bf16<true>, dim3(grid_cols16((d + 7) / 8)), dim3(256), 0, s, X,
                         K, d, ldx, ws, out);
    else
      hipLaunchKernelGGL(col_mean_bf16<false>, dim3(grid_cols16(d)), dim3(256), 0, s, X, K, d,
                         ldx, ws, out);
    HIPCHK(hipGetLastError());
    return GM_OK;
  }
  const dim3 g((unsigned)((d + 31) / 32));
#define GMK_SEL16(R_, NC_, NWV_)                                                                \
  do {                                                                                          \
    if (mode == 0)                                                                              \
      hipLaunchKernelGGL((col_select_bf16<0, R_, NC_, NWV_>), g, dim3(NWV_ * 64), 0, s, X, K, d, \
                         ldx, ws, trim, vec8, out);                                             \
    else                                                                                        \
      hipLaunchKernelGGL((col_select_bf16<1, R_, NC_, NWV_>), g, dim3(NWV_ * 64), 0, s, X, K, d, \
                         ldx, ws, trim, vec8, out);                                             \
  } while (0)
  if (K <= 64) GMK_SEL16(1, 8, 4);
  else if (K <= 128) GMK_SEL16(2, 8, 4);
  else if (K <= 256) GMK_SEL16(4, 4, 8);
  else if (K <= 512) GMK_SEL16(8, 4, 8);
  else if (K <= 1024) GMK_SEL16(16, 2, 16);
  else GMK_SEL16(32, 2, 16);
#undef GMK_SEL16
  HIPCHK(hipGetLastError());
  return GM_OK;
}

}  // namespace

}  // namespace gmk

extern "C" {

int gm_mean_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                 float* out, void* stream) {
  return gmk::coordinate_bf16("gm_mean_bf16", c, X, K, d, ldx, layout, -1, 0, out, stream);
}

int gm_median_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                   int32_t layout, float* out, void* stream) {
  return gmk::coordinate_bf16("gm_median_bf16", c, X, K, d, ldx, layout, 0, 0, out, stream);
}

int gm_trimmed_mean_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                         int32_t layout, int64_t trim, float* out, void* stream) {
  return gmk::coordinate_bf16("gm_trimmed_mean_bf16", c, X, K, d, ldx, layout, 1, trim, out,
                              stream);
}

}  // extern "C"
