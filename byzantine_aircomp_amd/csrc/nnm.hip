// Nearest-neighbor mixing (Allouah et al., "Fixing by Mixing", AISTATS 2023, Algorithm 1), the
// pre-aggregation step Y[i] = mean of the m = K - f rows nearest to row i (itself included).
// The definition (distances, tie rule, summation) is in include/gmagg.h.
//   nnm_neighbors   D [K][K] (upper triangle, launch_krum_dist) -> the K x K membership bit
//                   mask, and on request each row's index list
//   nnm_mix         Y = W X / m from the mask, fp64 sums on the VALU
#include <algorithm>
#include <type_traits>

#include "device_util.h"
#include "gmagg_internal.h"
#include "select_util.h"

namespace gmk {

// A distance as an unsigned key in the order of score_before (robust.hip): D >= 0, so the bits
// are ordered as the values; every NaN becomes the one key above +inf, so NaNs tie and the
// index decides; the row's own entry is 0 whatever pair_dist made of x - x (inf - inf = NaN).
__device__ __forceinline__ unsigned long long nnm_key(double x, bool self) {
  if (self) return 0ull;
  if (x != x) return 0x7FF8000000000000ull;
  return (unsigned long long)__double_as_longlong(x) & 0x7FFFFFFFFFFFFFFFull;
}

// One block per row i: j is in N(i) when fewer than m entries precede (D[i][j], j) (the stable
// rank krum_row_score and bulyan_row_order compute, over the row's keys in LDS).  A wave's 64
// flags are one ballot = two mask words: mask [K][KW], KW = 2 ceil(K / 64) words per row, bit
// j & 31 of word j >> 5, the bits of j >= K zero.  list (nullable) [K][m]: the members
// increasing, placed by the running count of the ballots.
__global__ void __launch_bounds__(256) nnm_neighbors(const double* __restrict__ D, int64_t K,
                                                     int64_t m, int64_t KW,
                                                     uint32_t* __restrict__ mask,
                                                     int32_t* __restrict__ list) {
  extern __shared__ unsigned long long nkey[];
  __shared__ int wcnt[4];
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t j = threadIdx.x; j < K; j += blockDim.x)
    nkey[j] = nnm_key(D[i <= j ? i * K + j : j * K + i], j == i);
  __syncthreads();
  int64_t base = 0;
  for (int64_t j0 = 0; j0 < KW * 32; j0 += 256) {      // (block-uniform trip count)
    const int64_t jw = j0 + 64 * w, j = jw + lane;
    bool in = false;
    if (j < K) {
      const unsigned long long x = nkey[j];
      int64_t rank = 0;
      for (int64_t t = 0; t < K; ++t) rank += (nkey[t] < x) || (nkey[t] == x && t < j);
      in = rank < m;
    }
    const uint64_t b = __ballot(in);
    if (lane == 0 && jw < KW * 32) {                   // KW * 32 is a multiple of 64
      mask[i * KW + (jw >> 5)] = (uint32_t)b;
      mask[i * KW + (jw >> 5) + 1] = (uint32_t)(b >> 32);
    }
    if (list) {                                        // (block-uniform)
      if (lane == 0) wcnt[w] = __popcll(b);
      __syncthreads();
      int64_t pos = base + (int64_t)__builtin_amdgcn_mbcnt_hi(
                               (uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
      for (int q = 0; q < w; ++q) pos += wcnt[q];
      if (in) list[i * m + pos] = (int32_t)j;
      base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
      __syncthreads();
    }
  }
}

// The mixing pass.  A block of 8 waves owns 8 R output rows (a "sweep": wave w rows
// i0 + w R .. + R - 1) x 256 columns (lane l columns 4 l .. 4 l + 3) and streams all K rows of
// that column tile through LDS, 32 rows per stage = one mask word per output row; the stage is
// widened to fp64 once, on its way into LDS.  Every lane of a wave works on the same output
// rows, so a neighbour bit is wave-uniform: the mask words sit in SGPRs, the test is a scalar
// branch, and only members cost VALU work, 4 v_add_f64 each (a staged row that no row of the
// wave holds is not even read).  acc starts at -0.0, the exact identity of IEEE addition, and
// takes the members in increasing k: the order is a function of N alone.  No product is
// formed, so an excluded row's inf or NaN never reaches a sum.
// The next stage's tile and mask words are loaded into registers before this stage's
// arithmetic (pair_dist's prefetch); two blocks share a CU (64 KB of LDS each), so one
// block's barriers and staging hide behind the other's additions (67.3 -> 62.7 ms against
// one 16-wave block per CU).  Blocks are numbered so that the sweeps of one
// column tile are consecutive on ONE XCD (workgroups go round-robin over the 8 XCDs): the tile
// is read from HBM once per XCD that holds one of its sweeps and otherwise from that XCD's L2.
constexpr int kMixT = 512;            // threads per block
constexpr int kMixW = kMixT / 64;     // waves per block
constexpr int kMixC = 256;            // columns per block
constexpr int kMixS = 32;             // rows of X per stage
constexpr int kMixQ = kMixS * 64 / kMixT;   // float4 groups of a stage per thread

// T: float, or uint16_t = bf16 bit patterns, which differ in the staging only: a thread loads
// two 16-byte groups of 8 columns per stage (VEC: base 16-byte aligned, ldx % 8 == 0; else by
// element) and widens them (exact) on the way into the same fp64 LDS stage.
template <typename T, int R, bool VEC>
__global__ void __launch_bounds__(kMixT, 2)
nnm_mix(const T* __restrict__ X, int64_t K, int64_t d, int64_t ldx, int ws,
        const uint32_t* __restrict__ mask, int64_t KW, int64_t m, int64_t nsw, int64_t nblk,
        float* __restrict__ Y, int64_t ldy, int wsy, int vecy) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  constexpr bool B16 = std::is_same<T, uint16_t>::value;
  // the stage widened once, [row][column pair of the lane][lane]: a wave's 16-byte reads and
  // writes are contiguous across lanes
  __shared__ __attribute__((aligned(16))) d2 sX[kMixS][2][64];
  const int64_t per = gridDim.x / 8;                   // (the grid is a multiple of 8)
  const int64_t L = ((int64_t)blockIdx.x % 8) * per + (int64_t)blockIdx.x / 8;
  if (L >= nblk) return;                               // (block-uniform)
  const int64_t tile = L / nsw, sweep = L - tile * nsw;
  const int64_t j0 = tile * kMixC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = sweep * (kMixW * R) + (int64_t)w * R;
  const int64_t nst = (K + kMixS - 1) / kMixS;

  double acc[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = -0.0;

  f4 pre[kMixQ];
  u4 pre16[kMixQ / 2];
  auto load_stage = [&](int64_t st) {
    if constexpr (B16) {
#pragma unroll
      for (int q = 0; q < kMixQ / 2; ++q) {
        const int idx = threadIdx.x + kMixT * q, r = idx >> 5, cg = idx & 31;
        const int64_t row = st * kMixS + r, col = j0 + 8 * cg;
        u4 v = {0u, 0u, 0u, 0u};
        if (row < K && col < d) {
          const uint16_t* src = elem(X, ldx, ws, row, col);
          if (VEC && col + 8 <= d) {
            v = *reinterpret_cast<const u4*>(src);
          } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const uint32_t h = col + u < d ? (uint32_t)src[u] : 0u;
              v[u >> 1] |= h << (16 * (u & 1));
            }
          }
        }
        pre16[q] = v;
      }
    } else {
#pragma unroll
    for (int q = 0; q < kMixQ; ++q) {
      const int idx = threadIdx.x + kMixT * q, r = idx >> 6, cg = idx & 63;
      const int64_t row = st * kMixS + r, col = j0 + 4 * cg;
      f4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < K && col < d) {
        const float* src = elem(X, ldx, ws, row, col);
        if (VEC && col + 4 <= d) {
          v = *reinterpret_cast<const f4*>(src);
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = col + u < d ? src[u] : 0.f;
        }
      }
      pre[q] = v;
    }
    }
  };
  // this wave's rows' mask words of stage st, row i0 + r in lane r (rows past K: no members)
  uint32_t nxt = 0u;
  auto load_words = [&](int64_t st) {
    nxt = lane < R && i0 + lane < K ? mask[(i0 + lane) * KW + st] : 0u;
  };
  load_stage(0);
  load_words(0);
  for (int64_t st = 0; st < nst; ++st) {
    __syncthreads();                                   // the previous stage's reads are done
    if constexpr (B16) {
#pragma unroll
      for (int q = 0; q < kMixQ / 2; ++q) {
        const int idx = threadIdx.x + kMixT * q, r = idx >> 5, cg = idx & 31;
#pragma unroll
        for (int h = 0; h < 4; ++h)                    // word h: columns 8 cg + 2 h, + 1
          sX[r][h & 1][2 * cg + (h >> 1)] =
              d2{(double)__uint_as_float(pre16[q][h] << 16),
                 (double)__uint_as_float(pre16[q][h] & 0xFFFF0000u)};
      }
    } else {
#pragma unroll
    for (int q = 0; q < kMixQ; ++q) {
      const int idx = threadIdx.x + kMixT * q;
      sX[idx >> 6][0][idx & 63] = d2{(double)pre[q][0], (double)pre[q][1]};
      sX[idx >> 6][1][idx & 63] = d2{(double)pre[q][2], (double)pre[q][3]};
    }
    }
    __syncthreads();
    uint32_t wb[R], any = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      wb[r] = __builtin_amdgcn_readlane(nxt, r);
      any |= wb[r];
    }
    if (st + 1 < nst) {
      load_stage(st + 1);
      load_words(st + 1);
    }
    if (any == 0u) continue;                           // (wave-uniform)
#pragma unroll
    for (int kk = 0; kk < kMixS; ++kk) {
      if (!((any >> kk) & 1u)) continue;
      const d2 x0 = sX[kk][0][lane], x1 = sX[kk][1][lane];
      const double xd[4] = {x0[0], x0[1], x1[0], x1[1]};
#pragma unroll
      for (int r = 0; r < R; ++r)
        if ((wb[r] >> kk) & 1u) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[r][e] += xd[e];
        }
    }
  }
  const int64_t col = j0 + 4 * lane;
  if (col >= d) return;
  const double dm = (double)m;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = i0 + r;
    if (i >= K) break;
    float* dst = const_cast<float*>(elem(Y, ldy, wsy, i, col));
    f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)(acc[r][e] / dm);
    if (vecy && col + 4 <= d) {
      *reinterpret_cast<f4*>(dst) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < d) dst[e] = o[e];
    }
  }
}

int64_t nnm_mask_words(int64_t K) { return K * 2 * ((K + 63) / 64); }

hipError_t launch_nnm_neighbors(const double* D, int64_t K, int64_t m, uint32_t* mask,
                                int32_t* list, hipStream_t s) {
  if (K < 1 || K > 4096 || m < 1 || m > K) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nnm_neighbors, dim3((unsigned)K), dim3(256), sizeof(unsigned long long) * K,
                     s, D, K, m, 2 * ((K + 63) / 64), mask, list);
  return hipGetLastError();
}

template <typename T>
static hipError_t nnm_mix_t(const T* X, int64_t K, int64_t d, int64_t ldx, int ws,
                            const uint32_t* mask, int64_t m, float* Y, int64_t ldy, int wsy,
                            hipStream_t s) {
  if (K < 1 || K > 4096 || m < 1 || m > K) return hipErrorInvalidValue;
  if (d <= 0) return hipSuccess;
  // rows per wave: the fewest that cover K in one sweep, 8 from K = 33 up
  const int R = K <= kMixW ? 1 : K <= 2 * kMixW ? 2 : K <= 4 * kMixW ? 4 : 8;
  const int64_t nsw = (K + kMixW * R - 1) / (kMixW * R);
  const int64_t nblk = (d + kMixC - 1) / kMixC * nsw;
  if (nblk > 0x7FFFFFF0ll) return hipErrorInvalidValue;
  const dim3 g((unsigned)((nblk + 7) / 8 * 8));
  const int64_t KW = 2 * ((K + 63) / 64);
  const bool vec = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % (16 / sizeof(T)) == 0;
  const int vecy = reinterpret_cast<uintptr_t>(Y) % 16 == 0 && ldy % 4 == 0;
#define GMK_MIX(R_)                                                                            \
  do {                                                                                         \
    if (vec)                                                                                   \
      hipLaunchKernelGGL((nnm_mix<T, R_, true>), g, dim3(kMixT), 0, s, X, K, d, ldx, ws, mask, KW, m, \
                         nsw, nblk, Y, ldy, wsy, vecy);                                        \
    else                                                                                       \
      hipLaunchKernelGGL((nnm_mix<T, R_, false>), g, dim3(kMixT), 0, s, X, K, d, ldx, ws, mask, KW, \
                         m, nsw, nblk, Y, ldy, wsy, vecy);                                     \
  } while (0)
  if (R == 1) GMK_MIX(1);
  else if (R == 2) GMK_MIX(2);
  else if (R == 4) GMK_MIX(4);
  else GMK_MIX(8);
#undef GMK_MIX
  return hipGetLastError();
}

hipError_t launch_nnm_mix(const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                          const uint32_t* mask, int64_t m, float* Y, int64_t ldy, int wsy,
                          hipStream_t s) {
  return nnm_mix_t(X, K, d, ldx, ws, mask, m, Y, ldy, wsy, s);
}
hipError_t launch_nnm_mix(const uint16_t* X, int64_t K, int64_t d, int64_t ldx, int ws,
                          const uint32_t* mask, int64_t m, float* Y, int64_t ldy, int wsy,
                          hipStream_t s) {
  return nnm_mix_t(X, K, d, ldx, ws, mask, m, Y, ldy, wsy, s);
}

}  // namespace gmk
