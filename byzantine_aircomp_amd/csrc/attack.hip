// Omniscient model-poisoning attacks, in place on the client matrix: per-column statistics of
// the H = K - B honest rows 0 .. H-1, then one malicious row written to rows H .. K-1.
//   affine   y_j = a mu_j + b sigma_j: "A Little Is Enough" (Baruch, Baruch & Goldberg 2019;
//            a = 1, b = -z) and inner-product manipulation (Xie, Koyejo & Gupta 2019;
//            a = -epsilon, b = 0)
//   min-max / min-sum (Shejwalkar & Houmansadr 2021): m = mu - gamma p with the largest gamma
//            that keeps m within the honest rows' own spread, in closed form
// The definitions are in include/gmagg.h.  Per column, in fp64 and in row order:
//   s = sum x_k                          mu    = s / H
//   u = sum (x_k - x_0), v = sum (x_k - x_0)^2
//                                        sigma = sqrt(max(0, v - u^2 / H) / (H - 1))
// The shift by the column's first row makes an all-equal column give u = v = 0, so sigma is
// exactly 0 (and mu exactly the value: H <= 2^12 copies of an fp32 value sum exactly).  The
// order is fixed, so every layout and alignment path gives the same bits.
//
// attack_columns is the hot path, one memory-bound pass shaped as bucket.hip's: H d elements
// read once, B d written, nothing reused (nontemporal loads and stores).  A thread item is 4
// columns (16 bytes of fp32, 8 of bf16; a group starting at a multiple of 4 never straddles a
// panel of either layout); its H loads are issued 8 rows at a time before the fp64
// arithmetic, and the same thread then stores its 4 values to the B Byzantine rows.  Only
// columns < d of rows >= H are ever written.
#include <algorithm>

#include "device_util.h"
#include "gmagg_internal.h"

namespace gmk {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// y rounded once to the storage type.  bf16: fp64 -> fp32 rounded to odd (the truncated
// value with its last bit set when inexact; an fp32 overflow steps back to the largest finite
// value), then to nearest even on the 16 bits dropped: fp32 keeps 16 bits more than bf16, so
// the two steps round as one.
__device__ __forceinline__ float narrow_f32(double y) { return (float)y; }
__device__ __forceinline__ uint16_t narrow_bf16(double y) {
  if (y != y) return 0x7FC0;
  const float f = (float)y;
  uint32_t u = __float_as_uint(f);
  if ((double)f != y) {
    if (fabs((double)f) > fabs(y)) --u;
    u |= 1u;
  }
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// One item: 4 columns of one row.
template <class SRC>
struct Item;
template <>
struct Item<float> {
  f4 v;
  __device__ __forceinline__ void load(const float* p) {
    v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
  }
  __device__ __forceinline__ float get(int c) const { return v[c]; }
  static __device__ __forceinline__ Item pack(const double* y) {
    Item o;
    o.v = f4{narrow_f32(y[0]), narrow_f32(y[1]), narrow_f32(y[2]), narrow_f32(y[3])};
    return o;
  }
  __device__ __forceinline__ void store(float* p) const {
    __builtin_nontemporal_store(v, reinterpret_cast<f4*>(p));
  }
};
template <>
struct Item<uint16_t> {
  u2 v;
  __device__ __forceinline__ void load(const uint16_t* p) {
    v = __builtin_nontemporal_load(reinterpret_cast<const u2*>(p));
  }
  __device__ __forceinline__ float get(int c) const {
    return __uint_as_float((c & 1) ? v[c >> 1] & 0xffff0000u : v[c >> 1] << 16);
  }
  static __device__ __forceinline__ Item pack(const double* y) {
    Item o;
    o.v = u2{(uint32_t)narrow_bf16(y[0]) | ((uint32_t)narrow_bf16(y[1]) << 16),
             (uint32_t)narrow_bf16(y[2]) | ((uint32_t)narrow_bf16(y[3]) << 16)};
    return o;
  }
  __device__ __forceinline__ void store(uint16_t* p) const {
    __builtin_nontemporal_store(v, reinterpret_cast<u2*>(p));
  }
};

__device__ __forceinline__ void narrow_to(double y, float* o) { *o = narrow_f32(y); }
__device__ __forceinline__ void narrow_to(double y, uint16_t* o) { *o = narrow_bf16(y); }

// The sums of one column: s plain, u and v shifted by the first row's value x0.
struct ColSums {
  double x0, s, u, v;
  __device__ __forceinline__ void start(float first) {
    x0 = (double)first;
    s = u = v = 0.0;
  }
  __device__ __forceinline__ void add(float x) {
    const double xd = (double)x, t = xd - x0;
    s += xd;
    u += t;
    v = fma(t, t, v);
  }
  __device__ __forceinline__ double mean(double H) const { return s / H; }
  // (the comparison keeps a NaN variance)
  __device__ __forceinline__ double sigma(double H) const {
    const double var = fma(-u, u / H, v) / (H - 1.0);
    return sqrt(var < 0.0 ? 0.0 : var);
  }
};

// The honest rows' sums of E columns at `base` (row 0's address; a row is rs elements on).
template <class SRC, bool VEC>
__device__ __forceinline__ void column_sums(const SRC* base, int64_t rs, int64_t H,
                                            ColSums* cs) {
  constexpr int U = 8;
  int64_t k = 0;
  if constexpr (VEC) {
    Item<SRC> x[U];
    x[0].load(base);
#pragma unroll
    for (int c = 0; c < 4; ++c) cs[c].start(x[0].get(c));
    for (; k + U <= H; k += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) x[u].load(base + (k + u) * rs);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) cs[c].add(x[u].get(c));
    }
    for (; k < H; ++k) {
      x[0].load(base + k * rs);
#pragma unroll
      for (int c = 0; c < 4; ++c) cs[c].add(x[0].get(c));
    }
  } else {
    SRC x[U];
    cs[0].start(widen(__builtin_nontemporal_load(base)));
    for (; k + U <= H; k += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = __builtin_nontemporal_load(base + (k + u) * rs);
#pragma unroll
      for (int u = 0; u < U; ++u) cs[0].add(widen(x[u]));
    }
    for (; k < H; ++k) cs[0].add(widen(__builtin_nontemporal_load(base + k * rs)));
  }
}

// y (E values) rounded once and stored to rows H .. K-1 of the columns at `base`.
template <class SRC, bool VEC>
__device__ __forceinline__ void store_rows(SRC* base, int64_t rs, int64_t H, int64_t K,
                                           const double* y) {
  if constexpr (VEC) {
    const Item<SRC> o = Item<SRC>::pack(y);
    for (int64_t k = H; k < K; ++k) o.store(base + k * rs);
  } else {
    SRC o;
    narrow_to(y[0], &o);
    for (int64_t k = H; k < K; ++k) base[k * rs] = o;
  }
}

struct AttackKArgs {
  void* X;
  int64_t K, H, d, ldx;   // ldx: the row stride, or the panel stride (ws > 0)
  int ws;                 // log2 of the panel width; 0: row-major
  double a, b;            // the affine attack's coefficients
  double* mu;             // statistics only (min-max / min-sum): mu [d] and p [d]
  double* p;
  int dev;                // p: 0 sigma, 1 mu (the unit direction, gamma rescaled), 2 sign(mu)
};

// E columns from their sums: the affine row into X, or mu and p into the workspace.
template <class SRC, bool VEC, bool STATS>
__device__ __forceinline__ void emit(const AttackKArgs& a, SRC* base, int64_t rs, int64_t col,
                                     const ColSums* cs) {
  constexpr int E = VEC ? 4 : 1;
  const double H = (double)a.H;
  if constexpr (STATS) {
#pragma unroll
    for (int c = 0; c < E; ++c) {
      const double mu = cs[c].mean(H);
      a.mu[col + c] = mu;
      a.p[col + c] = a.dev == 0 ? cs[c].sigma(H)
                   : a.dev == 1 ? mu
                                : (mu != mu ? mu : (double)((mu > 0.0) - (mu < 0.0)));
    }
  } else {
    double y[E];
#pragma unroll
    for (int c = 0; c < E; ++c) {
      y[c] = a.a * cs[c].mean(H);
      // b == 0: the sigma term is not formed (no 0 * NaN)
      if (a.b != 0.0) y[c] = fma(a.b, cs[c].sigma(H), y[c]);
    }
    store_rows<SRC, VEC>(base, rs, a.H, a.K, y);
  }
}

__device__ __forceinline__ int64_t col_offset(int64_t col, int64_t ldx, int ws) {
  return ws ? (col >> ws) * ldx + (col & (((int64_t)1 << ws) - 1)) : col;
}

template <class SRC, bool VEC, bool STATS>
__global__ void __launch_bounds__(256) attack_columns(const AttackKArgs a) {
  constexpr int E = VEC ? 4 : 1;
  SRC* X = static_cast<SRC*>(a.X);
  const int64_t rs = a.ws ? ((int64_t)1 << a.ws) : a.ldx;    // row stride
  const int64_t n = (a.d + E - 1) / E;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = e * E;
    SRC* base = X + col_offset(col, a.ldx, a.ws);
    if (!VEC || col + E <= a.d) {
      ColSums cs[E];
      column_sums<SRC, VEC>(base, rs, a.H, cs);
      emit<SRC, VEC, STATS>(a, base, rs, col, cs);
    } else {
      // the ragged last group: its columns < d one at a time, the same sums
      for (int c = 0; col + c < a.d; ++c) {
        ColSums cs;
        column_sums<SRC, false>(base + c, rs, a.H, &cs);
        emit<SRC, false, STATS>(a, base + c, rs, col + c, &cs);
      }
    }
  }
}

// 4-column items need the base and the row / panel stride on 16 bytes (fp32) or 8 (bf16);
// panel widths are multiples of 16 elements
bool vector_items(const void* X, int64_t ldx, int64_t esz) {
  return reinterpret_cast<uintptr_t>(X) % (4 * esz) == 0 && ldx % 4 == 0;
}

dim3 column_grid(int64_t d, bool vec) {
  const int64_t items = vec ? (d + 3) / 4 : d;
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 16384)));
}

// ---- min-max / min-sum -------------------------------------------------------------------

// Tree reduction over the block's 256 threads in a fixed order; every thread gets the result.
template <class OP>
__device__ __forceinline__ double block_reduce(double v, double* red, OP op) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}
// (a NaN wins both, so it reaches gamma)
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double add(double a, double b) { return a + b; }

// Block b owns columns [b chunk, (b + 1) chunk); wave w of its 4 the honest rows w, w + 4, ...
// Per row i the slice's share of a_i = ||mu - x_i||^2 and b_i = p . (mu - x_i), fp64 per lane
// and over the wave, to slab[b][i] and slab[b][H + i]; the slice's share of c = ||p||^2 to
// slab[b][2H].  attack_terms_reduce sums the slices in slice order (no atomics).
template <int G>
__global__ void __launch_bounds__(256) attack_row_terms(const float* __restrict__ X, int64_t H,
                                                        int64_t d, int64_t ldx, int ws,
                                                        int64_t chunk,
                                                        const double* __restrict__ mu,
                                                        const double* __restrict__ p,
                                                        double* __restrict__ slab) {
  __shared__ double red[256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * chunk, c1 = c0 + chunk < d ? c0 + chunk : d;
  const int64_t rs = ws ? ((int64_t)1 << ws) : ldx;
  double* out = slab + (int64_t)blockIdx.x * (2 * H + 1);
  for (int64_t i = w; i < H; i += 4) {
    double sa = 0.0, sb = 0.0;
    for (int64_t col = c0 + (int64_t)lane * G; col < c1; col += 64 * G) {
      const float* src = X + col_offset(col, ldx, ws) + i * rs;
      if (G == 4 && col + 4 <= c1) {
        const f4 x = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double t = mu[col + c] - (double)x[c];
          sa = fma(t, t, sa);
          sb = fma(p[col + c], t, sb);
        }
      } else {
        for (int c = 0; c < G && col + c < c1; ++c) {
          const double t = mu[col + c] - (double)src[c];
          sa = fma(t, t, sa);
          sb = fma(p[col + c], t, sb);
        }
      }
    }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    if (lane == 0) {
      out[i] = sa;
      out[H + i] = sb;
    }
  }
  double sc = 0.0;
  for (int64_t col = c0 + threadIdx.x; col < c1; col += 256) sc = fma(p[col], p[col], sc);
  sc = block_reduce(sc, red, add);
  if (threadIdx.x == 0) out[2 * H] = sc;
}

__global__ void __launch_bounds__(256) attack_terms_reduce(const double* __restrict__ slab,
                                                           int nb, int64_t S,
                                                           double* __restrict__ sums) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += slab[(int64_t)b * S + e];
  sums[e] = s;
}

// One block per honest row i over D [H][H] (upper triangle): rule 0 max_j D_ij, rule 1
// sum_j D_ij.
__global__ void __launch_bounds__(256) attack_row_bound(const double* __restrict__ D, int64_t H,
                                                        int rule, double* __restrict__ rb) {
  __shared__ double red[256];
  const int64_t i = blockIdx.x;
  double v = 0.0;
  for (int64_t j = threadIdx.x; j < H; j += 256) {
    const double x = D[i <= j ? i * H + j : j * H + i];
    v = rule ? v + x : nan_max(v, x);
  }
  v = rule ? block_reduce(v, red, add) : block_reduce(v, red, nan_max);
  if (threadIdx.x == 0) rb[i] = v;
}

// One block: the bound D* (rule 0) or S* (rule 1) = max_i rb[i], then the largest gamma that
// meets it, from sums = {a [H], b [H], c}:
//   rule 0   min_i (b_i + sqrt(b_i^2 + c (D* - a_i))) / c
//   rule 1   sqrt((S* - sum_i a_i) / (H c))
// and 0 when c == 0.  gam[0]: gamma for the p the kernels hold; gam[1]: gamma of the
// definition's p (dev 1: p = mu / ||mu||, so gamma ||mu||).
__global__ void __launch_bounds__(256) attack_gamma(const double* __restrict__ sums,
                                                    const double* __restrict__ rb, int64_t H,
                                                    int rule, int dev, double* __restrict__ gam) {
  __shared__ double red[256];
  const double* A = sums;
  const double* Bv = sums + H;
  const double c = sums[2 * H];
  double bound = 0.0;
  for (int64_t i = threadIdx.x; i < H; i += 256) bound = nan_max(bound, rb[i]);
  bound = block_reduce(bound, red, nan_max);
  double g;
  if (rule == 0) {
    g = INFINITY;
    for (int64_t i = threadIdx.x; i < H; i += 256) {
      const double q = fma(Bv[i], Bv[i], c * (bound - A[i]));
      g = nan_min(g, (Bv[i] + sqrt(q < 0.0 ? 0.0 : q)) / c);
    }
    g = block_reduce(g, red, nan_min);
  } else {
    double sa = 0.0;
    for (int64_t i = threadIdx.x; i < H; i += 256) sa += A[i];
    sa = block_reduce(sa, red, add);
    const double q = (bound - sa) / ((double)H * c);
    g = sqrt(q < 0.0 ? 0.0 : q);
  }
  if (c == 0.0) g = 0.0;
  if (threadIdx.x == 0) {
    gam[0] = g;
    gam[1] = dev == 1 ? g * sqrt(c) : g;
  }
}

// fp32(mu_j - gamma p_j) to rows H .. K-1, gamma read from device memory.
template <bool VEC>
__global__ void __launch_bounds__(256) attack_write_row(const AttackKArgs a,
                                                        const double* __restrict__ gam) {
  constexpr int E = VEC ? 4 : 1;
  float* X = static_cast<float*>(a.X);
  const int64_t rs = a.ws ? ((int64_t)1 << a.ws) : a.ldx;
  const int64_t n = (a.d + E - 1) / E;
  const double g = gam[0];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = e * E;
    float* base = X + col_offset(col, a.ldx, a.ws);
    if (!VEC || col + E <= a.d) {
      double y[E];
#pragma unroll
      for (int c = 0; c < E; ++c) y[c] = fma(-g, a.p[col + c], a.mu[col + c]);
      store_rows<float, VEC>(base, rs, a.H, a.K, y);
    } else {
      for (int c = 0; col + c < a.d; ++c) {
        const double y = fma(-g, a.p[col + c], a.mu[col + c]);
        store_rows<float, false>(base + c, rs, a.H, a.K, &y);
      }
    }
  }
}

}  // namespace

hipError_t launch_attack_affine(void* X, bool bf16, int64_t K, int64_t H, int64_t d, int64_t ldx,
                                int ws, double a, double b, hipStream_t stream) {
  AttackKArgs k{};
  k.X = X; k.K = K; k.H = H; k.d = d; k.ldx = ldx; k.ws = ws; k.a = a; k.b = b;
  const bool vec = vector_items(X, ldx, bf16 ? 2 : 4);
  const dim3 g = column_grid(d, vec), blk(256);
  if (bf16 && vec)
    hipLaunchKernelGGL((attack_columns<uint16_t, true, false>), g, blk, 0, stream, k);
  else if (bf16)
    hipLaunchKernelGGL((attack_columns<uint16_t, false, false>), g, blk, 0, stream, k);
  else if (vec)
    hipLaunchKernelGGL((attack_columns<float, true, false>), g, blk, 0, stream, k);
  else
    hipLaunchKernelGGL((attack_columns<float, false, false>), g, blk, 0, stream, k);
  return hipGetLastError();
}

int attack_term_blocks(int64_t d) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((d + 1023) / 1024, 512));
}

hipError_t launch_attack_minmax(float* X, int64_t K, int64_t H, int64_t d, int64_t ldx, int ws,
                                int rule, int dev, const double* D, double* mu, double* p,
                                double* slab, int nb, double* sums, double* rb, double* gam,
                                hipStream_t stream) {
  AttackKArgs k{};
  k.X = X; k.K = K; k.H = H; k.d = d; k.ldx = ldx; k.ws = ws; k.mu = mu; k.p = p; k.dev = dev;
  const bool vec = vector_items(X, ldx, 4);
  const dim3 g = column_grid(d, vec), blk(256);
  if (vec)
    hipLaunchKernelGGL((attack_columns<float, true, true>), g, blk, 0, stream, k);
  else
    hipLaunchKernelGGL((attack_columns<float, false, true>), g, blk, 0, stream, k);
  // slices of whole 4-column groups (a multiple of 256 columns)
  const int64_t chunk = ((d + nb - 1) / nb + 255) / 256 * 256;
  if (vec)
    hipLaunchKernelGGL(attack_row_terms<4>, dim3(nb), blk, 0, stream, X, H, d, ldx, ws, chunk, mu,
                       p, slab);
  else
    hipLaunchKernelGGL(attack_row_terms<1>, dim3(nb), blk, 0, stream, X, H, d, ldx, ws, chunk, mu,
                       p, slab);
  const int64_t S = 2 * H + 1;
  hipLaunchKernelGGL(attack_terms_reduce, dim3((unsigned)((S + 255) / 256)), blk, 0, stream, slab,
                     nb, S, sums);
  hipLaunchKernelGGL(attack_row_bound, dim3((unsigned)H), blk, 0, stream, D, H, rule, rb);
  hipLaunchKernelGGL(attack_gamma, dim3(1), blk, 0, stream, sums, rb, H, rule, dev, gam);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (vec)
    hipLaunchKernelGGL(attack_write_row<true>, g, blk, 0, stream, k, gam);
  else
    hipLaunchKernelGGL(attack_write_row<false>, g, blk, 0, stream, k, gam);
  return hipGetLastError();
}

}  // namespace gmk
