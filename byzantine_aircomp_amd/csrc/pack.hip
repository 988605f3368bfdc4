// Row f2: the caller-side packing.  The reference stacks the K
// flattened client vectors row-major (flatten_list, MNIST_Air_weight.py:206-209);
// the streaming pass reads them fastest in the panel layout [ceil(d/W)][K][W]
// (DESIGN.md §1).  One kernel converts: thread e moves one float4 (or one float),
// consecutive threads walk the W/4 groups of one row segment, then the next row,
// then the next panel, so a wave reads 8 row segments of 128 B (W = 32) and
// writes 1 KiB contiguously.  Padding columns (>= d) of the last panel are left
// as they are (ClientPanels allocates them zeroed).  rows_to_panels_bf16 writes the bf16
// panels of gm_weiszfeld_bf16 the same way, from fp32 (rounding) or bf16 rows.
#include "gmagg_internal.h"

namespace gmk {

template <bool VEC4>
__global__ void __launch_bounds__(256) rows_to_panels(const float* __restrict__ X, int64_t K,
                                                      int64_t d, int64_t ldx,
                                                      float* __restrict__ P, int64_t W,
                                                      int64_t pstride) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  constexpr int E = VEC4 ? 4 : 1;                 // floats per thread-item
  const int64_t per_row = W / E;                  // items per (panel, row)
  const int64_t npan = (d + W - 1) / W;
  const int64_t n = npan * K * per_row;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = e % per_row, rk = e / per_row;
    const int64_t k = rk % K, p = rk / K;
    const int64_t col = p * W + q * E;
    if (col >= d) continue;
    float* dst = P + p * pstride + k * W + q * E;
    const float* src = X + k * ldx + col;
    if constexpr (VEC4) {
      if (col + 4 <= d) {
        __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const f4*>(src)),
                                    reinterpret_cast<f4*>(dst));
      } else {
        for (int u = 0; col + u < d; ++u) dst[u] = src[u];
      }
    } else {
      *dst = *src;
    }
  }
}

hipError_t launch_rows_to_panels(const float* X, int64_t K, int64_t d, int64_t ldx, float* P,
                                 int64_t W, int64_t pstride, hipStream_t s) {
  const bool vec4 = reinterpret_cast<uintptr_t>(X) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(P) % 16 == 0 && ldx % 4 == 0 && W % 4 == 0 &&
                    pstride % 4 == 0;
  const int64_t items = ((d + W - 1) / W) * K * (vec4 ? W / 4 : W);
  int64_t grid = (items + 255) / 256;
  if (grid > 16384) grid = 16384;
  if (grid < 1) grid = 1;
  if (vec4)
    hipLaunchKernelGGL(rows_to_panels<true>, dim3((unsigned)grid), dim3(256), 0, s, X, K, d, ldx,
                       P, W, pstride);
  else
    hipLaunchKernelGGL(rows_to_panels<false>, dim3((unsigned)grid), dim3(256), 0, s, X, K, d, ldx,
                       P, W, pstride);
  return hipGetLastError();
}

// bf16 panels (gm_weiszfeld_bf16's layout) from row-major fp32 or bf16 rows: the thread
// walk of rows_to_panels with 8 columns = 16 bytes of panel per item.  fp32 is rounded to
// nearest even, the bits of torch's .to(torch.bfloat16) (NaN -> 0x7FC0).
__device__ __forceinline__ uint32_t bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if (f != f) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint16_t to_bf16(float f) { return (uint16_t)bf16_rne(f); }
__device__ __forceinline__ uint16_t to_bf16(uint16_t b) { return b; }

template <class SRC, bool VEC8>
__global__ void __launch_bounds__(256) rows_to_panels_bf16(const SRC* __restrict__ X, int64_t K,
                                                           int64_t d, int64_t ldx,
                                                           uint16_t* __restrict__ P, int64_t W,
                                                           int64_t pstride) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  constexpr int E = VEC8 ? 8 : 1;
  const int64_t per_row = W / E;
  const int64_t npan = (d + W - 1) / W;
  const int64_t n = npan * K * per_row;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = e % per_row, rk = e / per_row;
    const int64_t k = rk % K, p = rk / K;
    const int64_t col = p * W + q * E;
    if (col >= d) continue;
    uint16_t* dst = P + p * pstride + k * W + q * E;
    const SRC* src = X + k * ldx + col;
    if constexpr (VEC8) {
      if (col + 8 <= d) {
        u4 o;
        if constexpr (sizeof(SRC) == 4) {
          const f4 a = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src));
          const f4 b = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src) + 1);
          o = u4{bf16_rne(a[0]) | bf16_rne(a[1]) << 16, bf16_rne(a[2]) | bf16_rne(a[3]) << 16,
                 bf16_rne(b[0]) | bf16_rne(b[1]) << 16, bf16_rne(b[2]) | bf16_rne(b[3]) << 16};
        } else {
          o = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src));
        }
        __builtin_nontemporal_store(o, reinterpret_cast<u4*>(dst));
      } else {
        for (int u = 0; col + u < d; ++u) dst[u] = to_bf16(src[u]);
      }
    } else {
      *dst = to_bf16(*src);
    }
  }
}

hipError_t launch_rows_to_panels_bf16(const void* X, bool src_f32, int64_t K, int64_t d,
                                      int64_t ldx, uint16_t* P, int64_t W, int64_t pstride,
                                      hipStream_t s) {
  // 16-byte items: the source row segments (fp32: two float4, ldx % 4; bf16: ldx % 8) and
  // the panel's
  const bool vec8 = reinterpret_cast<uintptr_t>(X) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(P) % 16 == 0 && ldx % (src_f32 ? 4 : 8) == 0 &&
                    W % 8 == 0 && pstride % 8 == 0;
  const int64_t items = ((d + W - 1) / W) * K * (vec8 ? W / 8 : W);
  int64_t grid = (items + 255) / 256;
  if (grid > 16384) grid = 16384;
  if (grid < 1) grid = 1;
  const dim3 g((unsigned)grid), b(256);
  const float* Xf = static_cast<const float*>(X);
  const uint16_t* Xh = static_cast<const uint16_t*>(X);
  if (src_f32 && vec8)
    hipLaunchKernelGGL((rows_to_panels_bf16<float, true>), g, b, 0, s, Xf, K, d, ldx, P, W, pstride);
  else if (src_f32)
    hipLaunchKernelGGL((rows_to_panels_bf16<float, false>), g, b, 0, s, Xf, K, d, ldx, P, W, pstride);
  else if (vec8)
    hipLaunchKernelGGL((rows_to_panels_bf16<uint16_t, true>), g, b, 0, s, Xh, K, d, ldx, P, W, pstride);
  else
    hipLaunchKernelGGL((rows_to_panels_bf16<uint16_t, false>), g, b, 0, s, Xh, K, d, ldx, P, W, pstride);
  return hipGetLastError();
}

}  // namespace gmk
