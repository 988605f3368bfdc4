// The K simulated clients' stochastic gradients of one federated step in gradient space,
// folded into their momenta, as ONE kernel: the worker-momentum loop of Karimireddy, He &
// Jaggi (ICML 2021, Algorithm 1; "robust D-SHB" in Farhadkhani et al., ICML 2022).
//
// Every client evaluates the SAME model theta = [W (C*F, row-major), b (C)] (flatten_list
// order) on its own batch:
//   g_k = grad_theta meanCE(theta; batch k) + weight_decay * theta
//   M_k <- beta * M_k + (1 - beta) * g_k
// so, unlike clients.hip's chain (client k starts from client k-1's update), the clients are
// independent: one workgroup per client, grid = K.  W and b are read only (every block reads
// the same C*F + C floats from L2); row k of M depends on (W, b, batch k, k >= honest, M_k)
// alone, so its bits do not depend on K, on the grid's schedule or on M's layout.
//
// The model, the batches (rows idx[k][0..B) of the training set) and the Byzantine clients'
// flips (classflip C-1-y, dataflip 1-x) are clients.hip's, and so is the arithmetic of a
// client: the workgroup's shape (512 threads, the wave's batch tile in registers, dz in LDS,
// the B x F tile staged in LDS where it fits) and its phases
//   A  logits z[s][c] = x_s . W_c + b_c (wave = samples w + 8 i, lane = features
//      lane + 64 j, classes in groups of 4, one transpose-reduce per group),
//   B  dz = d meanCE / dz in torch's log_softmax backward order,
//   C  gW[c][f] = sum_s dz[s][c] x[s][f], s ascending (thread = features f, f + 512),
// are kept as they are there (that file's header has the reasons); phase C ends in the
// momentum update instead of the SGD step.  clients.hip itself is untouched: the chain
// kernel's registers and code stay what the e2e fixtures pin.
#include "device_util.h"
#include "gmagg_internal.h"

namespace gmk {

constexpr int kCgThreads = 512;
constexpr int kCgWaves = kCgThreads / 64;
constexpr int kCgSpw = 8;        // samples per wave in phase A (B <= 64)
constexpr int kCgCg = 4;         // classes per phase-A group
constexpr int kCgFpt = 2;        // features per thread in phase C
constexpr int kCgNj = 13;        // features per lane in phase A: F <= 832
constexpr int kCgCgC = 16;       // classes per phase-C group (CGC: 10 when C <= 10)
constexpr int kCgMaxC = 64;
// dz row stride for phase C's class groups of CGC: every column a group reads, rounded up
// to 16 bytes
__host__ __device__ constexpr int cg_zs(int cgc) { return cgc == 10 ? 12 : 64; }
constexpr int kCgMaxB = kCgWaves * kCgSpw;

// element jj of client k's row of M (rows: any ldx >= d; panels: never a padding column,
// jj < d)
__device__ __forceinline__ int64_t cg_at(const ClientGradArgs& a, int64_t k, int64_t jj) {
  if (a.pstride > 0)
    return (jj >> a.wshift) * a.pstride + k * ((int64_t)1 << a.wshift) +
           (jj & (((int64_t)1 << a.wshift) - 1));
  return k * a.ldx + jj;
}

// fp32 max over the wave, every lane the result (clients.hip's cc_wave_max)
__device__ __forceinline__ float cg_wave_max(float v) {
  auto sw = [&](auto r) { v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1])); };
  sw(__builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false));
  sw(__builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false));
  v = fmaxf(v, xlane_partner<8>(v));
  v = fmaxf(v, xlane_partner<4>(v));
  v = fmaxf(v, xlane_partner<2>(v));
  v = fmaxf(v, xlane_partner<1>(v));
  return v;
}

// NJ = features per lane in phase A (F <= 64 * NJ).  Dynamic LDS: dz [B][ZS], then the
// client's batch tile x[B][F] when B * F * 4 bytes fit beside it (a.stage); else phase C
// reads the rows from global memory.
template <int NJ, int CGC>
__global__ void __launch_bounds__(kCgThreads, 1) client_grads(ClientGradArgs a) {
  __shared__ int s_row[kCgMaxB];                  // dataset rows of the client's batch
  __shared__ int s_lab[kCgMaxB];                  // (relabelled) targets
  __shared__ float s_b[kCgMaxC];                  // the bias
  extern __shared__ float s_dyn[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = (int)a.F, C = (int)a.C, B = (int)a.B;
  const float invB = 1.0f / (float)B;
  constexpr int ZS = cg_zs(CGC);
  float* s_z = s_dyn;
  float* s_x = s_dyn + B * ZS;

  const int64_t k = blockIdx.x;
  const bool byz = k >= a.honest;
  const bool flip_x = byz && a.attack == 2;
  if (tid < B) {
    const int r = a.idx[k * B + tid];
    s_row[tid] = r;
    const int y = (int)a.labels[r];
    s_lab[tid] = (byz && a.attack == 1) ? (C - 1 - y) : y;
  }
  if (tid < C) s_b[tid] = a.b[tid];
  __syncthreads();

  // ---- A: logits on the wave's batch tile: samples w + 8 i, features lane + 64 j (every
  // load issued at a clamped address, masked after; 0 outside the batch)
  float xr[kCgSpw][NJ];
  {
    int rows[kCgSpw];
#pragma unroll
    for (int i = 0; i < kCgSpw; ++i) {
      const int s = w + kCgWaves * i;
      rows[i] = s < B ? s_row[s] : s_row[0];
    }
#pragma unroll
    for (int i = 0; i < kCgSpw; ++i) {
      const float* row = a.data + (int64_t)rows[i] * a.ldd;
#pragma unroll
      for (int j = 0; j < NJ; ++j) xr[i][j] = row[min(lane + 64 * j, F - 1)];
    }
#pragma unroll
    for (int i = 0; i < kCgSpw; ++i) {
      const bool sv = w + kCgWaves * i < B;
#pragma unroll
      for (int j = 0; j < NJ; ++j) xr[i][j] = (sv && lane + 64 * j < F) ? xr[i][j] : 0.f;
    }
  }
  if (flip_x) {
#pragma unroll
    for (int i = 0; i < kCgSpw; ++i) {
      const int s = w + kCgWaves * i;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (s < B && lane + 64 * j < F) xr[i][j] = 1.0f - xr[i][j];
    }
  }
  if (a.stage) {
#pragma unroll
    for (int i = 0; i < kCgSpw; ++i) {
      const int s = w + kCgWaves * i;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int f = lane + 64 * j;
        if (s < B && f < F) s_x[s * F + f] = xr[i][j];
      }
    }
  }
  auto logits = [&](const int c0) {
    float e[kCgSpw * kCgCg];                            // value i * CG + cc
#pragma unroll
    for (int q = 0; q < kCgSpw * kCgCg; ++q) e[q] = 0.f;
#pragma unroll
    for (int cc = 0; cc < kCgCg; ++cc) {
      const int c = c0 + cc < C ? c0 + cc : C - 1;      // (a padding class repeats C-1)
      const float* wc = a.W + (int64_t)c * F;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int f = lane + 64 * j;
        const float wv = f < F ? wc[f] : 0.f;
#pragma unroll
        for (int i = 0; i < kCgSpw; ++i) e[i * kCgCg + cc] = fmaf(xr[i][j], wv, e[i * kCgCg + cc]);
      }
    }
    xlane_transpose64<kCgSpw * kCgCg>(e, lane);
    // lanes 2v and 2v + 1 hold value row_of_lane(lane) (32 values over 64 lanes)
    if ((lane & 1) == 0) {
      const int v = row_of_lane<64, kCgSpw * kCgCg>(lane);
      const int i = v / kCgCg, cc = v % kCgCg;
      const int s = w + kCgWaves * i, c = c0 + cc;
      if (s < B && c < C) s_z[s * ZS + c] = e[0] + s_b[c];
    }
  };
  if constexpr (CGC == 10) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
      if (g * kCgCg < C) logits(g * kCgCg);
  } else {
    for (int c0 = 0; c0 < C; c0 += kCgCg) logits(c0);
  }
  __syncthreads();

  // ---- B: dz = d mean CE / dz, torch's log_softmax backward order.  C <= 10: four samples
  // per wave, one 16-lane DPP row each
  if constexpr (CGC == 10) {
    const int q = lane >> 4, cl = lane & 15;
    for (int s0 = 4 * w; s0 < B; s0 += 4 * kCgWaves) {
      const int s = s0 + q;
      const bool cv = cl < C && s < B;
      const float z = cv ? s_z[s * ZS + cl] : -INFINITY;
      float m = z;
      m = fmaxf(m, xlane_partner<8>(m));
      m = fmaxf(m, xlane_partner<4>(m));
      m = fmaxf(m, xlane_partner<2>(m));
      m = fmaxf(m, xlane_partner<1>(m));
      float sum = cv ? expf(z - m) : 0.f;
      sum += xlane_partner<8>(sum);
      sum += xlane_partner<4>(sum);
      sum += xlane_partner<2>(sum);
      sum += xlane_partner<1>(sum);
      const float logp = (z - m) - logf(sum);
      const float gout = (cv && cl == s_lab[s]) ? -invB : 0.f;
      if (cv) s_z[s * ZS + cl] = gout - expf(logp) * (-invB);
    }
  } else
  for (int s = w; s < B; s += kCgWaves) {
    const bool cv = lane < C;
    const float z = cv ? s_z[s * ZS + lane] : -INFINITY;
    const float m = cg_wave_max(z);
    const float sum = xlane_wave_sum_f32(cv ? expf(z - m) : 0.f);
    const float logp = (z - m) - logf(sum);
    const float gout = (lane == s_lab[s]) ? -invB : 0.f;
    if (cv) s_z[s * ZS + lane] = gout - expf(logp) * (-invB);
  }
  __syncthreads();

  // ---- C: gradient and momentum update; thread = 2 features, classes in groups of CGC.
  // beta == 0: M is write-only (its old value, NaN included, is never loaded)
  const float beta = a.beta, omb = 1.0f - a.beta;
  const bool keep = beta != 0.f;
  for (int c0 = 0; c0 < C; c0 += CGC) {
    // the parameters and the old momenta of this thread's columns, loaded before the sample
    // loop (their latency hides behind it): clamped addresses, no branches
    float par[kCgFpt][CGC], mold[kCgFpt][CGC];
#pragma unroll
    for (int h = 0; h < kCgFpt; ++h)
#pragma unroll
      for (int cc = 0; cc < CGC; ++cc) {
        const int f = min(tid + kCgThreads * h, F - 1), c = min(c0 + cc, C - 1);
        par[h][cc] = a.W[(int64_t)c * F + f];
        mold[h][cc] = keep ? a.M[cg_at(a, k, (int64_t)c * F + f)] : 0.f;
      }
    float g[kCgFpt][CGC], gb[CGC];   // gb: the bias gradient (used by thread 0)
#pragma unroll
    for (int cc = 0; cc < CGC; ++cc) {
      gb[cc] = 0.f;
#pragma unroll
      for (int h = 0; h < kCgFpt; ++h) g[h][cc] = 0.f;
    }
#pragma unroll 2
    for (int s = 0; s < B; ++s) {
      float xv[kCgFpt];
      if (a.stage) {
#pragma unroll
        for (int h = 0; h < kCgFpt; ++h) {
          const int f = tid + kCgThreads * h;
          xv[h] = f < F ? s_x[s * F + f] : 0.f;             // (flipped when staged)
        }
      } else {
        const float* row = a.data + (int64_t)s_row[s] * a.ldd;
#pragma unroll
        for (int h = 0; h < kCgFpt; ++h) {
          const int f = tid + kCgThreads * h;
          xv[h] = f < F ? row[f] : 0.f;
          if (flip_x) xv[h] = 1.0f - xv[h];
        }
      }
#pragma unroll
      for (int cc = 0; cc < CGC; ++cc) {
        const float dz = s_z[s * ZS + c0 + cc];        // (columns >= C: never stored)
        gb[cc] += dz;
#pragma unroll
        for (int h = 0; h < kCgFpt; ++h) g[h][cc] = fmaf(dz, xv[h], g[h][cc]);
      }
    }
#pragma unroll
    for (int h = 0; h < kCgFpt; ++h) {
      const int f = tid + kCgThreads * h;
      if (f < F) {
#pragma unroll
        for (int cc = 0; cc < CGC; ++cc) {
          const int c = c0 + cc;
          if (c < C)
            a.M[cg_at(a, k, (int64_t)c * F + f)] =
                fmaf(beta, mold[h][cc], omb * (g[h][cc] + a.wd * par[h][cc]));
        }
      }
    }
    if (tid == 0) {   // the bias: sum over s ascending, as the weights' gradients
#pragma unroll
      for (int cc = 0; cc < CGC; ++cc) {
        const int c = c0 + cc;
        if (c < C) {
          const int64_t at = cg_at(a, k, (int64_t)C * F + c);
          const float mo = keep ? a.M[at] : 0.f;
          a.M[at] = fmaf(beta, mo, omb * (gb[cc] + a.wd * s_b[c]));
        }
      }
    }
  }
}

bool client_grads_supported(int64_t F, int64_t C, int64_t B) {
  return F >= 1 && F <= 64 * kCgNj && F <= kCgThreads * kCgFpt && C >= 1 && C <= kCgMaxC &&
         B >= 1 && B <= kCgMaxB;
}

hipError_t launch_client_grads(const ClientGradArgs& a, hipStream_t s) {
  // clients.hip's two instances (phase C's class groups: exactly 10 for MNIST's classifier,
  // 16 otherwise) and its LDS plan: dz [B][ZS] and, when it fits beside it in the CU's
  // 160 KB, the batch tile [B][F] (B = 50, F = 784: 157 KB + 2.4 KB of dz at C <= 10, one
  // workgroup per CU; C = 62 leaves no room and reads the rows from L2 in phase C)
  constexpr size_t kLdsMax =   // (s_row, s_lab, s_b static)
      (160u << 10) - 2 * kCgMaxB * sizeof(int) - kCgMaxC * sizeof(float);
  auto raise = [](const void* fn) {   // the kernel's dynamic-LDS limit, once per process
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) ==
           hipSuccess;
  };
  static const bool ok10 = raise(reinterpret_cast<const void*>(&client_grads<kCgNj, 10>));
  static const bool ok16 = raise(reinterpret_cast<const void*>(&client_grads<kCgNj, kCgCgC>));
  const bool c10 = a.C <= 10;
  const size_t dz = (size_t)a.B * (size_t)cg_zs(c10 ? 10 : kCgCgC) * sizeof(float);
  const size_t tile = (size_t)a.B * (size_t)a.F * sizeof(float);
  ClientGradArgs b = a;
  b.stage = (c10 ? ok10 : ok16) && dz + tile <= kLdsMax ? 1 : 0;
  const size_t lds = dz + (b.stage ? tile : 0);
  const dim3 grid((unsigned)a.K);
  if (c10)
    hipLaunchKernelGGL((client_grads<kCgNj, 10>), grid, dim3(kCgThreads), lds, s, b);
  else
    hipLaunchKernelGGL((client_grads<kCgNj, kCgCgC>), grid, dim3(kCgThreads), lds, s, b);
  return hipGetLastError();
}

}  // namespace gmk
