// s-bucketing (Karimireddy, He & Jaggi, "Byzantine-Robust Learning on Heterogeneous Datasets
// via Bucketing", ICLR 2022): the K client rows are permuted and every s consecutive rows
// averaged; the aggregator then sees the Kb = ceil(K / s) bucket means.  Bucket i holds rows
// perm[i s] ... perm[min(K, (i + 1) s) - 1] (perm == nullptr: the identity), and
//   y[i][j] = (float)(sum over the bucket, in that order, of (double)x[row][j]) / count_i)
// an fp64 sum in bucket order, rounded once (coordinate.hip's rule), NaN and infinities by
// IEEE rules.  The order is fixed, so every layout and alignment path gives the same bits.
//
// One memory-bound pass: K d elements read, Kb d floats written, nothing reused (nontemporal
// loads and stores).  A thread item is 4 columns of one row, 16 bytes of fp32 or 8 of bf16 in
// and 16 bytes out (a group of 4 columns starting at a multiple of 4 never straddles a panel
// of either layout); consecutive threads walk the
// groups of one OUTPUT row segment (a panel row, or 1024 columns of a row-major row), then
// the next bucket, then the next panel, so a wave's stores are contiguous and each of its s
// loads covers whole row segments.  An output row depends on s input rows only, so a
// row-major input is read along its rows: the 128-byte row segments that bind the row-major
// streaming pass do not arise.  The s loads of an item are issued back to
// back (8 at a time beyond s = 8) before the fp64 adds.
#include "gmagg_internal.h"

namespace gmk {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// One item: E = 4 columns of one row.
template <class SRC>
struct Item;
template <>
struct Item<float> {
  static constexpr int E = 4;
  f4 v;
  __device__ __forceinline__ void load(const float* p) {
    v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
  }
  __device__ __forceinline__ void add(double* acc) const {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] += (double)v[c];
  }
};
// bf16: 4 columns too, an 8-byte load.  With 16-byte loads (8 columns) a lane owns 32 bytes of
// output, so each of its two 16-byte stores leaves every other 16 bytes of the wave's range
// to the other instruction; measured at K = 1000 x d = 2M into panels, that form took 2,030 µs
// at s = 2 and 1,251 at s = 4 against 1,524 and 1,172 for this one, whose every store
// instruction writes 1 KiB contiguously (profiles/bucketing_bf16_item_ab.jsonl).
template <>
struct Item<uint16_t> {
  static constexpr int E = 4;
  u2 v;
  __device__ __forceinline__ void load(const uint16_t* p) {
    v = __builtin_nontemporal_load(reinterpret_cast<const u2*>(p));
  }
  __device__ __forceinline__ void add(double* acc) const {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      acc[2 * c] += (double)__uint_as_float(v[c] << 16);
      acc[2 * c + 1] += (double)__uint_as_float(v[c] & 0xffff0000u);
    }
  }
};

struct BucketKArgs {
  const void* X;
  int64_t K, d, ldx;      // ldx: the row stride, or the panel stride (wsi > 0)
  int wsi;                // log2 of the input panel width; 0: row-major
  const int32_t* perm;    // nullable
  int64_t s, Kb;          // s <= K
  float* Y;
  int64_t ldy;
  int wso;                // log2 of the output panel width; 0: row-major
  int wws;                // log2 of the walk width: the output panel's, or 1024 columns
};

__device__ __forceinline__ int64_t row_of(const BucketKArgs& a, int64_t slot) {
  return a.perm ? (int64_t)a.perm[slot] : slot;
}

// Rows slot0 ... slot0 + N - 1 of the bucket added to acc in that order: the N loads first.
template <class SRC, bool VEC, int N>
__device__ __forceinline__ void add_rows(const BucketKArgs& a, const SRC* base, int64_t rs,
                                         int64_t slot0, double* acc) {
  if constexpr (VEC) {
    Item<SRC> x[N];
    int64_t r[N];
#pragma unroll
    for (int u = 0; u < N; ++u) r[u] = row_of(a, slot0 + u);
#pragma unroll
    for (int u = 0; u < N; ++u) x[u].load(base + r[u] * rs);
#pragma unroll
    for (int u = 0; u < N; ++u) x[u].add(acc);
  } else {
    SRC x[N];
    int64_t r[N];
#pragma unroll
    for (int u = 0; u < N; ++u) r[u] = row_of(a, slot0 + u);
#pragma unroll
    for (int u = 0; u < N; ++u) x[u] = __builtin_nontemporal_load(base + r[u] * rs);
#pragma unroll
    for (int u = 0; u < N; ++u) acc[0] += (double)widen(x[u]);
  }
}

// The bucket's sum at `base` (the address of row 0's first column of the group).
template <class SRC, bool VEC>
__device__ __forceinline__ void bucket_sum(const BucketKArgs& a, const SRC* base, int64_t rs,
                                           int64_t slot0, int64_t cnt, double* acc) {
  int64_t t = 0;
  for (; t + 8 <= cnt; t += 8) add_rows<SRC, VEC, 8>(a, base, rs, slot0 + t, acc);
  switch (cnt - t) {
    case 1: add_rows<SRC, VEC, 1>(a, base, rs, slot0 + t, acc); break;
    case 2: add_rows<SRC, VEC, 2>(a, base, rs, slot0 + t, acc); break;
    case 3: add_rows<SRC, VEC, 3>(a, base, rs, slot0 + t, acc); break;
    case 4: add_rows<SRC, VEC, 4>(a, base, rs, slot0 + t, acc); break;
    case 5: add_rows<SRC, VEC, 5>(a, base, rs, slot0 + t, acc); break;
    case 6: add_rows<SRC, VEC, 6>(a, base, rs, slot0 + t, acc); break;
    case 7: add_rows<SRC, VEC, 7>(a, base, rs, slot0 + t, acc); break;
    default: break;
  }
}

// sum / cnt rounded once.  A power-of-two cnt multiplies by its exact reciprocal, which is
// the quotient bit for bit (no fp64 sum of fp32 terms is near the subnormal range) and
// spares the fp64 division's ~20 instructions per column at the usual s = 2, 4.
struct Divisor {
  double cnt, inv;   // inv: 1 / cnt where that is exact, else 0
  __device__ __forceinline__ explicit Divisor(int64_t c)
      : cnt((double)c), inv((c & (c - 1)) == 0 ? ldexp(1.0, 1 - __ffsll((long long)c)) : 0.0) {}
  __device__ __forceinline__ float mean(double sum) const {
    return inv != 0.0 ? (float)(sum * inv) : (float)(sum / cnt);
  }
};

template <class SRC, bool VEC>
__global__ void __launch_bounds__(256) bucket_means(const BucketKArgs a) {
  constexpr int E = VEC ? Item<SRC>::E : 1;
  constexpr int ES = VEC ? 2 : 0;                  // log2 E
  const SRC* X = static_cast<const SRC*>(a.X);
  const int prs = a.wws - ES;                      // log2 items per (panel, bucket)
  const int64_t npan = (a.d + ((int64_t)1 << a.wws) - 1) >> a.wws;
  const int64_t nseg = npan * a.Kb;
  const int64_t n = nseg << prs;
  const bool small = nseg <= 0xffffffffll;         // 32-bit division of the segment index
  const int64_t rs = a.wsi ? ((int64_t)1 << a.wsi) : a.ldx;   // input row stride
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = e & (((int64_t)1 << prs) - 1), seg = e >> prs;
    int64_t p, i;
    if (small) {
      const uint32_t sg = (uint32_t)seg, kb = (uint32_t)a.Kb;
      p = sg / kb;
      i = sg % kb;
    } else {
      p = seg / a.Kb;
      i = seg % a.Kb;
    }
    const int64_t col = (p << a.wws) + q * E;
    if (col >= a.d) continue;
    const int64_t slot0 = i * a.s;
    const int64_t cnt = a.K - slot0 < a.s ? a.K - slot0 : a.s;
    const Divisor dv(cnt);
    // row 0's address of this column group; a row is rs elements further in both layouts
    const SRC* base = a.wsi ? X + (col >> a.wsi) * a.ldx + (col & (((int64_t)1 << a.wsi) - 1))
                            : X + col;
    float* dst = a.wso ? a.Y + (col >> a.wso) * a.ldy + (i << a.wso) +
                             (col & (((int64_t)1 << a.wso) - 1))
                       : a.Y + i * a.ldy + col;
    if (!VEC || col + E <= a.d) {
      double acc[E];
#pragma unroll
      for (int c = 0; c < E; ++c) acc[c] = 0.0;
      bucket_sum<SRC, VEC>(a, base, rs, slot0, cnt, acc);
      if constexpr (VEC) {
#pragma unroll
        for (int c = 0; c < E; c += 4) {
          const f4 o = {dv.mean(acc[c]), dv.mean(acc[c + 1]), dv.mean(acc[c + 2]),
                        dv.mean(acc[c + 3])};
          __builtin_nontemporal_store(o, reinterpret_cast<f4*>(dst + c));
        }
      } else {
        __builtin_nontemporal_store(dv.mean(acc[0]), dst);
      }
    } else {
      // the ragged last group of a row: its columns < d one at a time, the same sums
      for (int c = 0; col + c < a.d; ++c) {
        double acc = 0.0;
        bucket_sum<SRC, false>(a, base + c, rs, slot0, cnt, &acc);
        dst[c] = dv.mean(acc);
      }
    }
  }
}

}  // namespace

hipError_t launch_bucket_means(const void* X, bool bf16, int64_t K, int64_t d, int64_t ldx,
                               int64_t Wi, const int32_t* perm, int64_t s, float* Y, int64_t ldy,
                               int64_t Wo, hipStream_t stream) {
  auto shift = [](int64_t W) {
    int ws = 0;
    while (((int64_t)1 << ws) < W) ++ws;
    return ws;
  };
  BucketKArgs a{};
  a.X = X; a.K = K; a.d = d; a.ldx = ldx; a.wsi = shift(Wi); a.perm = perm;
  a.s = s < K ? s : K;                     // one bucket of K rows for every s >= K
  a.Kb = (K + a.s - 1) / a.s;
  a.Y = Y; a.ldy = ldy; a.wso = shift(Wo);
  a.wws = Wo ? a.wso : 10;
  // 4-column items: the input's base and row / panel stride (16 bytes fp32, 8 bf16), the
  // output's base and stride (16 bytes); panel widths are multiples of 16 elements and column
  // groups start at multiples of 4
  const int64_t esz = bf16 ? 2 : 4, E = 4;
  const bool vec = reinterpret_cast<uintptr_t>(X) % (E * esz) == 0 && ldx % E == 0 &&
                   reinterpret_cast<uintptr_t>(Y) % 16 == 0 && ldy % 4 == 0 &&
                   (Wi == 0 || Wi % E == 0) && (Wo == 0 || Wo % E == 0);
  const int64_t W = (int64_t)1 << a.wws;
  const int64_t items = ((d + W - 1) / W) * a.Kb * (vec ? W / E : W);
  int64_t grid = (items + 255) / 256;
  if (grid > 16384) grid = 16384;
  if (grid < 1) grid = 1;
  const dim3 g((unsigned)grid), b(256);
  if (bf16 && vec)
    hipLaunchKernelGGL((bucket_means<uint16_t, true>), g, b, 0, stream, a);
  else if (bf16)
    hipLaunchKernelGGL((bucket_means<uint16_t, false>), g, b, 0, stream, a);
  else if (vec)
    hipLaunchKernelGGL((bucket_means<float, true>), g, b, 0, stream, a);
  else
    hipLaunchKernelGGL((bucket_means<float, false>), g, b, 0, stream, a);
  return hipGetLastError();
}

}  // namespace gmk
