// The device helpers the column-selection and Krum kernels share (coordinate.hip, robust.hip):
// element addressing for both layouts, the order-preserving keys, the bit-wise rank selection
// on keys held across one wave (its description: coordinate.hip, "Order statistics"), and the
// Krum row score.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_util.h"

namespace gmk {

// Element (row k, column j) of a client matrix: row-major [K][ldx] (ws = 0), or the
// panel layout [ceil(d/W)][K][W] with W = 2^ws and ldx = the panel stride.  A group of
// 4 columns starting at a multiple of 4 never straddles a panel (W % 4 == 0), so the
// float4 paths below read it as one vector either way.
__device__ __forceinline__ const float* elem(const float* X, int64_t ldx, int ws, int64_t k,
                                             int64_t j) {
  return ws ? X + (j >> ws) * ldx + (k << ws) + (j & ((1 << ws) - 1)) : X + k * ldx + j;
}
// The same for bf16 bit patterns (bf16 panels: W = 2^ws % 8 == 0, so 8 columns from a multiple
// of 8 never straddle a panel), and the widening to fp32 (exact).
__device__ __forceinline__ const uint16_t* elem(const uint16_t* X, int64_t ldx, int ws, int64_t k,
                                                int64_t j) {
  return ws ? X + (j >> ws) * ldx + (k << ws) + (j & ((1 << ws) - 1)) : X + k * ldx + j;
}
__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(uint16_t bits) {
  return __uint_as_float((uint32_t)bits << 16);
}

__device__ __forceinline__ uint32_t order_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (x != x) return 0xFFFFFFFFu;
  if (x == 0.f) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// The key of a held slot (round 5: 4-6 VALU, no branch; the LDS read before it is
// unconditional — padding rows hold finite garbage or zeros — so a wave's reads issue back
// to back): ok = false (a row past K, a column past d) -> 0xFFFFFFFF; -0 as +0 (x + 0);
// NaN -> 0xFFFFFFFF (above +inf: torch's order for topk) when NANTOP, else whatever key
// its bits give (the median returns NaN for a column holding one, select_pair).
template <bool NANTOP>
__device__ __forceinline__ uint32_t slot_key(float x, bool ok) {
  const uint32_t u = __float_as_uint(x + 0.0f);
  uint32_t k = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
  if constexpr (NANTOP) k = x != x ? 0xFFFFFFFFu : k;
  return ok ? k : 0xFFFFFFFFu;
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// NC columns x NR ranks selected together: independent chains interleaved, so the
// compare -> count -> decide latency of one chain hides behind the others.
// count(t, cnt): cnt[c][q] = #(keys of chain (c, q) < t[c][q]), wave-uniform.
// EXIT: stop as soon as every chain's interval holds a single key (returns the bit
// just decided: that key is the answer); -1 when the steps ran to `lo`.
template <int NC, int NR, bool EXIT = false, typename Count>
__device__ __forceinline__ int select_steps(int hi, int lo, uint32_t (&ans)[NC][NR],
                                            int (&clo)[NC][NR], int (&chi)[NC][NR],
                                            const int (&rr)[NR], Count count) {
  for (int bit = hi; bit >= lo; --bit) {
    uint32_t t[NC][NR];
    int cnt[NC][NR];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int q = 0; q < NR; ++q) t[c][q] = ans[c][q] | (1u << bit);
    count(t, cnt);
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        if (cnt[c][q] <= rr[q]) {
          ans[c][q] |= 1u << bit;
          clo[c][q] = cnt[c][q];
        } else {
          chi[c][q] = cnt[c][q];
        }
      }
    if constexpr (EXIT) {
      bool one = true;
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < NR; ++q) one = one && chi[c][q] - clo[c][q] == 1;
      if (one) return bit;
    }
  }
  return -1;
}

// Sum over the wave of a per-lane int (DPP row shifts + row broadcasts, gfx9
// family), returned wave-uniform.
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31
  return __builtin_amdgcn_readlane(v, 63);
}

// Inclusive prefix sum over the wave of a per-lane int (the DPP sequence of wave_sum_i32
// without its final read of lane 63).
__device__ __forceinline__ int wave_scan_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31
  return v;
}

// The trimmed mean's two ranks (round 4): the top byte of each chain's answer from ONE
// histogram of the keys' top bytes (256 bins in LDS, one atomic add per held key, a wave
// prefix scan), shared by the column's two ranks, instead of 8 counting steps per rank over
// every key; then, when the top byte left more candidates than the compaction takes, the
// next byte from a histogram of the keys inside each rank's top-byte bin.  K=1000 x 2M:
// 7.26 -> 6.30 ms; the median (one rank) measured slower with it, 3.81 -> 4.23 ms (the
// adds to the few bins a column's top bytes fill serialize), so it keeps the counting
// steps (profiles/r4s1_select_hist_ab.jsonl).  GMK_SELECT_HIST: 0 never, 1 the top byte
// only, 2 both bytes; applied where the chain selects >= GMK_SELECT_HIST_NR ranks.
#ifndef GMK_SELECT_HIST
#define GMK_SELECT_HIST 2
#endif
#ifndef GMK_SELECT_NBALLOT
#define GMK_SELECT_NBALLOT 0
#endif
#ifndef GMK_SELECT_HIST_NR
#define GMK_SELECT_HIST_NR 2
#endif

// Candidate compaction (round 2).  Before step `bit` a chain's answer lies in
// [L, L + 2^(bit+1)); the step's count n = #(key < L + 2^bit) is also the count
// below one end of the new interval, so the number of keys still in it (chi - clo)
// is known for free.  At two fixed points of the schedule (after bits 31..24, and
// after 23..16) the chains check it: if every chain has <= 64*R2 keys left, each
// writes those keys (a ballot + mbcnt per held value) to LDS, reads back R2 per lane,
// and the remaining steps count only them: n = c0 + #(candidate < t), c0 = the
// count below L at compaction (every dropped key is below that L or at/above the
// interval's end).  Spread data (the C3 recipe, N(0,1)) compacts after the first 8
// steps (simulated: <= 128 of 1000 keys left after ~7); clustered data after 16 or
// never, and then the loop counts every key as before.  The schedule is fixed and
// branch-free inside each run of steps: a per-step compaction check cost more than
// it saved.  buf(c, q): LDS slots of chain (c, q), STR words apart, >= 64*R2 of them.
template <int R, int NC, int NR, int R2, int STR, typename Buf>
__device__ __forceinline__ void select_ranks(const uint32_t (&key)[NC][R], const int64_t (&r)[NR],
                                             uint32_t (&ans)[NC][NR], int (&clo)[NC][NR],
                                             int (&chi)[NC][NR], Buf buf) {
  constexpr bool COMPACT = R2 > 0 && R > R2;
  int rr[NR];
#pragma unroll
  for (int q = 0; q < NR; ++q) rr[q] = (int)r[q];   // counts fit 32 bits (K <= 2048)
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      ans[c][q] = 0;
      clo[c][q] = 0;
      chi[c][q] = 64 * R;      // padding keys (0xFFFFFFFF) count as keys: never below t
    }
  // Counting every held key.  A ballot costs three instructions per key (v_cmp, a
  // scalar popcount, a scalar add) and the loop is issue-bound (one instruction per
  // wave per cycle slot), so at R >= 8 each lane counts its own keys instead (v_cmp +
  // v_addc: two) and two chains share one DPP wave sum (16-bit halves: <= 2048 each).
  // GMK_SELECT_NBALLOT (A/B knob): the first NB keys of each lane counted by ballot
  // (1 VALU + 2 SALU per key) and the rest per lane (2 VALU), to balance the two issue ports
  auto full = [&](const uint32_t (&t)[NC][NR], int (&cnt)[NC][NR]) {
    if constexpr (R >= 8) {
      constexpr int NB = GMK_SELECT_NBALLOT < R ? GMK_SELECT_NBALLOT : R - 1;
      int lc[NC * NR], sc[NC * NR];
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          int v = 0, sb = 0;
#pragma unroll
          for (int i = 0; i < NB; ++i) sb += __popcll(__ballot(key[c][i] < t[c][q]));
#pragma unroll
          for (int i = NB; i < R; ++i) v += (int)(key[c][i] < t[c][q]);
          lc[c * NR + q] = v;
          sc[c * NR + q] = sb;
        }
#pragma unroll
      for (int p = 0; p < NC * NR; p += 2) {
        if (p + 1 < NC * NR) {
          const int s2 = wave_sum_i32(lc[p] + (lc[p + 1] << 16));
          cnt[p / NR][p % NR] = (s2 & 0xFFFF) + sc[p];
          cnt[(p + 1) / NR][(p + 1) % NR] = (s2 >> 16) + sc[p + 1];
        } else {
          cnt[p / NR][p % NR] = wave_sum_i32(lc[p]) + sc[p];   // (an odd chain count: NC = NR = 1)
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          int n = 0;
#pragma unroll
          for (int i = 0; i < R; ++i) n += __popcll(__ballot(key[c][i] < t[c][q]));
          cnt[c][q] = n;
        }
    }
  };
  if constexpr (!COMPACT) {
    select_steps<NC, NR>(31, 0, ans, clo, chi, rr, full);
  } else {
    const int lane = threadIdx.x & 63;
    auto small = [&]() {
      bool ok = true;
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < NR; ++q) ok = ok && chi[c][q] - clo[c][q] <= 64 * R2;
      return ok;
    };
    // keys in [ans, ans + 2^bit) of every chain -> LDS (lane order) -> R2 per lane,
    // then steps bit-1 .. 0 on them
    auto finish_compacted = [&](int bit) {
      uint32_t ck[NC][NR][R2];
      int cbase[NC][NR];
      const uint32_t span = 1u << bit;
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          uint32_t* b = buf(c, q);
          const uint32_t lo = ans[c][q];
          int base = 0;
#pragma unroll
          for (int i = 0; i < R; ++i) {
            const bool in = key[c][i] - lo < span;
            const uint64_t m = __ballot(in);
            const int pos = base + (int)__builtin_amdgcn_mbcnt_hi(
                                       (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (in) b[pos * STR] = key[c][i];
            base += __popcll(m);
          }
          cbase[c][q] = clo[c][q];
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          const uint32_t* b = buf(c, q);
          const int nc = chi[c][q] - clo[c][q];
#pragma unroll
          for (int i = 0; i < R2; ++i) {
            const int s = lane + 64 * i;
            ck[c][q][i] = s < nc ? b[s * STR] : 0xFFFFFFFFu;
          }
        }
      // a chain whose interval holds one candidate has found its key (simulated: one
      // key left after 13-18 of the 32 steps on spread data), so the steps stop
      // when every chain is there and each takes that key
      const int stop = select_steps<NC, NR, true>(bit - 1, 0, ans, clo, chi, rr,
                           [&](const uint32_t (&t)[NC][NR], int (&cnt)[NC][NR]) {
#pragma unroll
                             for (int c = 0; c < NC; ++c)
#pragma unroll
                               for (int q = 0; q < NR; ++q) {
                                 int n = cbase[c][q];
#pragma unroll
                                 for (int i = 0; i < R2; ++i)
                                   n += __popcll(__ballot(ck[c][q][i] < t[c][q]));
                                 cnt[c][q] = n;
                               }
                           });
      if (stop > 0) {
        const uint32_t sp = 1u << stop;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int q = 0; q < NR; ++q) {
            // the first slot in range: the candidates fill slots [0, nc), the 0xFFFFFFFF
            // padding after them falls in range when the interval ends at 2^32
            uint32_t v = ans[c][q];
            bool got = false;
#pragma unroll
            for (int i = 0; i < R2; ++i) {
              const uint64_t m = __ballot(ck[c][q][i] - ans[c][q] < sp);
              if (m && !got) {
                v = __builtin_amdgcn_readlane(ck[c][q][i], __builtin_ctzll(m));
                got = true;
              }
            }
            ans[c][q] = v;
          }
      }
    };
    if constexpr (GMK_SELECT_HIST >= 1 && NR >= GMK_SELECT_HIST_NR) {
      // bins of column c: buf(c, 0)[b * STR], b < 256 (the wave's own dead tile column)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        uint32_t* h = buf(c, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) h[(4 * lane + j) * STR] = 0u;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        uint32_t* h = buf(c, 0);
#pragma unroll
        for (int i = 0; i < R; ++i)
          __hip_atomic_fetch_add(&h[(key[c][i] >> 24) * STR], 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WAVEFRONT);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint32_t* h = buf(c, 0);
        int hb[4], sl = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          hb[j] = (int)h[(4 * lane + j) * STR];
          sl += hb[j];
        }
        const int incl = wave_scan_i32(sl), excl = incl - sl;
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          // the lane whose 4 bins hold rank rr[q] (the bins count all 64 R keys, padding
          // included, and rr < K <= 64 R: exactly one lane)
          const uint64_t m = __ballot(excl <= rr[q] && rr[q] < incl);
          const int L = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
          int lo = __builtin_amdgcn_readlane(excl, L);
          int bsel = 4 * L + 3, blo = lo, bhi = 64 * R;
          bool found = false;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int hj = __builtin_amdgcn_readlane(hb[j], L);
            if (!found && lo + hj > rr[q]) {
              found = true;
              bsel = 4 * L + j;
              blo = lo;
              bhi = lo + hj;
            }
            lo += hj;
          }
          ans[c][q] = (uint32_t)bsel << 24;     // keys < ans: blo; keys < ans + 2^24: bhi
          clo[c][q] = blo;
          chi[c][q] = bhi;
        }
      }
      // (the compaction below reuses the same LDS slots: the bins are consumed)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
      select_steps<NC, NR>(31, 24, ans, clo, chi, rr, full);
    }
    if (small()) {
      finish_compacted(24);
      return;
    }
    if constexpr (GMK_SELECT_HIST >= 2 && NR >= GMK_SELECT_HIST_NR && R >= 8) {
      // bits 23..16 from a second histogram per chain: the keys inside the chain's top-byte
      // bin, binned by their next byte (slots 256 q + b of column c's dead tile column)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        uint32_t* h = buf(c, 0);
#pragma unroll
        for (int q = 0; q < NR; ++q)
#pragma unroll
          for (int j = 0; j < 4; ++j) h[(256 * q + 4 * lane + j) * STR] = 0u;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        uint32_t* h = buf(c, 0);
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          const uint32_t top = ans[c][q] >> 24;
#pragma unroll
          for (int i = 0; i < R; ++i)
            if ((key[c][i] >> 24) == top)
              __hip_atomic_fetch_add(&h[(256 * q + ((key[c][i] >> 16) & 255u)) * STR], 1u,
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint32_t* h = buf(c, 0);
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          int hb[4], sl = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            hb[j] = (int)h[(256 * q + 4 * lane + j) * STR];
            sl += hb[j];
          }
          const int incl = wave_scan_i32(sl) + clo[c][q], excl = incl - sl;
          const uint64_t m = __ballot(excl <= rr[q] && rr[q] < incl);
          const int L = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
          int lo = __builtin_amdgcn_readlane(excl, L);
          int bsel = 4 * L + 3, blo = lo, bhi = chi[c][q];
          bool found = false;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int hj = __builtin_amdgcn_readlane(hb[j], L);
            if (!found && lo + hj > rr[q]) {
              found = true;
              bsel = 4 * L + j;
              blo = lo;
              bhi = lo + hj;
            }
            lo += hj;
          }
          ans[c][q] |= (uint32_t)bsel << 16;
          clo[c][q] = blo;
          chi[c][q] = bhi;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
      select_steps<NC, NR>(23, 16, ans, clo, chi, rr, full);
    }
    if (small()) {
      finish_compacted(16);
      return;
    }
    select_steps<NC, NR>(15, 0, ans, clo, chi, rr, full);
  }
}

// The sum of the kk smallest entries of a row staged in LDS (stable rank), summed per
// thread in j order and over the block by block_sum: every Krum score — the exact path's
// and the Gram path's refined candidates' — goes through this one function, so equal rows
// give equal bits.
__device__ __forceinline__ double krum_row_score(const double* srow, int64_t K, int64_t kk,
                                                 double* scratch) {
  double sc = 0.0;
  for (int64_t j = threadIdx.x; j < K; j += blockDim.x) {
    const double x = srow[j];
    int64_t rank = 0;
    for (int64_t t = 0; t < K; ++t) rank += (srow[t] < x) || (srow[t] == x && t < j);
    if (rank < kk) sc += x;
  }
  return block_sum(sc, scratch);
}

}  // namespace gmk
