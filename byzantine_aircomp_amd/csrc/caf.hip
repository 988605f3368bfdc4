// CAF, the covariance filter (the down-weighting filter of Diakonikolas et al., "Being Robust
// (in High Dimensions) Can Be Practical", ICML 2017; ByzFL's Covariance-bound Agnostic Filter),
// solved in K-space.  The definition (the rounds, the start vector, the stopping rule, the order
// of every sum) is in include/gmagg.h; the host loop is gm_caf_f32 (api.hip).  The filter only
// ever needs inner products of centred rows, and with a = D p, q = p.a / 2, rho = a - q those
// are u_i . u_j = (rho_i + rho_j - D_ij) / 2 on the squared distances D of launch_krum_dist: the
// solver below never touches X.  Per call:
//   caf_mirror   D's lower triangle from its upper one, once
//   caf_init     c = 1, S = K, p = 1 / K and the fresh state
// per round:
//   caf_matvec   a = D p                                         (many blocks)
//   caf_start    q, rho, the start row r, w_0 = M e_r / ||.||, z = sqrt(p) o w_0, 1.z and rho.z
//   power_iters times, no-ops once the state says the iteration has ended:
//     caf_matvec   y = D z                                       (many blocks)
//     caf_finish   M w = sqrt(p) o (rho (1.z) + 1 (rho.z) - y) / 2, its norm, the new unit
//                  iterate, its movement, z, 1.z, rho.z and the state
//   caf_matvec   y = D z of the last iterate
//   caf_end      lambda = w.Mw, the strict-less record of (c, S, t), g = G z, tau_max, the new
//                c, S, p and whether another round runs
// then caf_compact (the rows with c* > 0 and their c*_k / S*) and caf_weighted_mean over X.
//
// D is mirrored, not read symmetrically: launch_krum_dist fills the upper triangle only, and a
// product that read D_ij for j < i as D_ji would walk a column, K doubles apart, in every one of
// the ~10^4 products of a call; the mirror costs one pass over D and every product then reads
// whole rows, one wave per row, 512 contiguous bytes per load instruction.
// Blocks combine at launch boundaries only: the product is one launch, the O(K) work that
// needs all of it is a one-block launch behind it.  No block waits on another and nothing is
// counted across blocks.  Every sum has a fixed order that depends on K alone (caf_sum: thread t
// of 1024 takes k = t, t + 1024, ... in order, then block_sum; a row of the product: lane l takes
// j = l, l + 64, ... in order, then the wave butterfly), so every result is a function of D.
#include <algorithm>

#include "device_util.h"
#include "gmagg_internal.h"
#include "select_util.h"

namespace gmk {

namespace {

constexpr int kCafT = 1024;           // threads of the one-block kernels (K <= 4096: 4 rows each)
constexpr int kCafR = 4;              // rows per thread of a one-block kernel: K <= kCafR * kCafT
constexpr int kCafMV = 256;           // threads per block of the product: 4 waves, a row each

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool caf_finite(double x) { return x - x == 0.0; }

// sum_k f(k) over k < K in the one order every K-space sum of this file uses
template <class F>
__device__ __forceinline__ double caf_sum(int64_t K, double* scratch, F f) {
  double a = 0.0;
  for (int64_t k = threadIdx.x; k < K; k += kCafT) a += f(k);
  return block_sum(a, scratch);
}

// a before b in the order the start row is chosen in: NaN first, then larger first, ties to the
// lower index (a total order: the result of a reduction does not depend on its shape)
__device__ __forceinline__ bool caf_before(double a, int64_t i, double b, int64_t j) {
  if (i < 0 || j < 0) return j < 0 && i >= 0;
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? i < j : an;
  return a > b || (a == b && i < j);
}

__global__ void __launch_bounds__(256) caf_mirror(double* __restrict__ D, int64_t K) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= K * K) return;
  const int64_t i = e / K, j = e - i * K;
  if (i > j) D[e] = D[j * K + i];
}

__global__ void __launch_bounds__(kCafT) caf_init(const CafWork w, int64_t K, int64_t f) {
  const double p = 1.0 / (double)K;
  for (int64_t k = threadIdx.x; k < K; k += kCafT) {
    w.c[k] = 1.0;
    w.p[k] = p;
    w.sp[k] = sqrt(p);
  }
  if (threadIdx.x != 0) return;
  CafState st{};
  st.S = (double)K;
  st.best = __builtin_inf();
  st.Sbest = (double)K;
  st.lambda = __builtin_nan("");
  st.loop_done = !(st.S > (double)(K - 2 * f));
  *w.st = st;
}

// y = D x, one wave per row.  force: run whatever the iteration's state says (a = D p at the
// round's start, y = D z of the last iterate at its end).
__global__ void __launch_bounds__(kCafMV) caf_matvec(const double* __restrict__ D, int64_t K,
                                                     const double* __restrict__ x,
                                                     const CafState* __restrict__ st, int force,
                                                     double* __restrict__ y) {
  if (st->loop_done || (!force && st->it_done)) return;   // (grid-uniform)
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * (kCafMV / 64) + (threadIdx.x >> 6);
  if (k >= K) return;
  const double* row = D + k * K;
  double acc = 0.0;
  int64_t j = lane;
  for (; j + 192 < K; j += 256) {
    const double d0 = row[j], d1 = row[j + 64], d2 = row[j + 128], d3 = row[j + 192];
    const double x0 = x[j], x1 = x[j + 64], x2 = x[j + 128], x3 = x[j + 192];
    acc = fma(d0, x0, acc);
    acc = fma(d1, x1, acc);
    acc = fma(d2, x2, acc);
    acc = fma(d3, x3, acc);
  }
  for (; j < K; j += 64) acc = fma(row[j], x[j], acc);
  acc = wave_sum(acc);
  if (lane == 0) y[k] = acc;
}

// One block: q, rho, the start row and w_0, and the round's fresh iteration state.
__global__ void __launch_bounds__(kCafT) caf_start(const CafWork w, int64_t K) {
  __shared__ double scratch[kCafT / 64];
  __shared__ double sv[kCafT];
  __shared__ int32_t si[kCafT];
  CafState* st = w.st;
  if (st->loop_done) return;                         // (block-uniform: written at the end)
  const double q = 0.5 * caf_sum(K, scratch, [&](int64_t k) { return w.p[k] * w.y[k]; });
  int64_t best = -1;
  double bv = 0.0;
  for (int64_t k = threadIdx.x; k < K; k += kCafT) {
    const double rho = w.y[k] - q;
    w.rho[k] = rho;
    const double m = w.p[k] * rho;                   // M_kk
    if (caf_before(m, k, bv, best)) { bv = m; best = k; }
  }
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = (int32_t)best;
  __syncthreads();
  for (int s = kCafT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s &&
        caf_before(sv[threadIdx.x + s], si[threadIdx.x + s], sv[threadIdx.x], si[threadIdx.x])) {
      sv[threadIdx.x] = sv[threadIdx.x + s];
      si[threadIdx.x] = si[threadIdx.x + s];
    }
    __syncthreads();
  }
  const int64_t r = si[0];
  const double* Dr = w.D + r * K;
  const double spr = w.sp[r], rr = w.rho[r];         // (rho[r]: written above by this block,
  __syncthreads();                                   //  read after the reduction's barriers)
  // column r of M
  auto col = [&](int64_t k) { return w.sp[k] * spr * (0.5 * (w.rho[k] + rr - Dr[k])); };
  const double nrm = sqrt(caf_sum(K, scratch, [&](int64_t k) { const double m = col(k); return m * m; }));
  const bool ok = nrm > 0.0 && caf_finite(nrm);
  for (int64_t k = threadIdx.x; k < K; k += kCafT) {
    const double x = ok ? col(k) / nrm : 0.0;
    w.w[k] = x;
    w.z[k] = w.sp[k] * x;
  }
  __syncthreads();
  const double sz = caf_sum(K, scratch, [&](int64_t k) { return w.z[k]; });
  const double rz = caf_sum(K, scratch, [&](int64_t k) { return w.rho[k] * w.z[k]; });
  if (threadIdx.x != 0) return;
  st->it_done = !ok;
  st->degenerate = nrm == 0.0;
  st->failed = !ok && nrm != 0.0;
  st->converged = nrm == 0.0;
  st->iters = 0;
  st->r = (int32_t)r;
  st->q = q;
  st->sz = sz;
  st->rz = rz;
  st->nrm = nrm;
  st->movement = 0.0;
}

// One block: the state after one application of M (y = D z is the product's launch).  A thread
// keeps its rows' M w (K <= 4096: at most kCafR) in registers over the two reductions, the norm
// with the next iterate's 1.z and rho.z (sums of sqrt(p) o M w, divided by the norm afterwards),
// then the movement: this launch sits between every two products of a call.
__global__ void __launch_bounds__(kCafT) caf_finish(const CafWork w, int64_t K, double tol) {
  __shared__ double scratch[3][kCafT / 64];
  CafState* st = w.st;
  if (st->loop_done || st->it_done) return;          // (block-uniform: written at the end)
  const double sz = st->sz, rz = st->rz;
  double m[kCafR], sp[kCafR], a3[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < kCafR; ++i) {
    const int64_t k = threadIdx.x + (int64_t)i * kCafT;
    m[i] = sp[i] = 0.0;
    if (k < K) {
      const double rho = w.rho[k];
      sp[i] = w.sp[k];
      m[i] = sp[i] * (0.5 * (rho * sz + rz - w.y[k]));
      a3[0] += m[i] * m[i];
      a3[1] += sp[i] * m[i];
      a3[2] += rho * (sp[i] * m[i]);
    }
  }
  // the three sums at once, each in caf_sum's order
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    a3[j] = wave_sum(a3[j]);
    if (lane == 0) scratch[j][wv] = a3[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double s = 0.0;
    for (int i = 0; i < kCafT / 64; ++i) s += scratch[j][i];
    a3[j] = s;
  }
  const double nrm = sqrt(a3[0]);
  const bool ok = nrm > 0.0 && caf_finite(nrm);
  double mov = 0.0;
  if (ok) {
    double am = 0.0;
#pragma unroll
    for (int i = 0; i < kCafR; ++i) {
      const int64_t k = threadIdx.x + (int64_t)i * kCafT;
      if (k < K) {
        const double x = m[i] / nrm, dl = x - w.w[k];
        am += dl * dl;
        w.w[k] = x;
        w.z[k] = sp[i] * x;
      }
    }
    mov = sqrt(block_sum(am, scratch[0]));
  }
  const double sz1 = a3[1] / nrm, rz1 = a3[2] / nrm;
  if (threadIdx.x != 0) return;
  st->iters += 1;
  st->nrm = nrm;
  if (!ok) {                                         // (a zero norm cannot be normalised either)
    st->it_done = 1;
    st->failed = 1;
    return;
  }
  st->sz = sz1;
  st->rz = rz1;
  st->movement = mov;
  if (mov <= tol) {
    st->it_done = 1;
    st->converged = 1;
  }
}

// One block: steps 2 (lambda), 3 and 4 of the round on y = D z of the last iterate, and the
// next round's weights.
__global__ void __launch_bounds__(kCafT) caf_end(const CafWork w, int64_t K, int64_t f) {
  __shared__ double scratch[kCafT / 64];
  __shared__ double smax[kCafT];
  __shared__ int32_t snan[kCafT];
  CafState* st = w.st;
  if (st->loop_done) return;                         // (block-uniform: written at the end)
  const double sz = st->sz, rz = st->rz, S = st->S, best = st->best;
  const bool degenerate = st->degenerate != 0, it_failed = st->failed != 0;
  const int32_t recorded = st->recorded, round = st->round;
  __syncthreads();                                   // (every read of the state is above)
  auto g = [&](int64_t k) { return 0.5 * (w.rho[k] * sz + rz - w.y[k]); };
  double lambda = 0.0;
  if (!degenerate && !it_failed)
    lambda = caf_sum(K, scratch, [&](int64_t k) { return w.w[k] * (w.sp[k] * g(k)); });
  const bool failed = it_failed || !caf_finite(lambda);
  if (failed) {                                      // the loop ends at once
    if (!recorded)
      for (int64_t k = threadIdx.x; k < K; k += kCafT) w.cbest[k] = w.c[k];
    if (threadIdx.x != 0) return;
    if (!recorded) {
      st->recorded = 1;
      st->Sbest = S;
      st->best_round = round;
      st->lambda = __builtin_nan("");
    }
    st->loop_done = 1;
    return;
  }
  const bool better = lambda < best;
  if (better)
    for (int64_t k = threadIdx.x; k < K; k += kCafT) w.cbest[k] = w.c[k];
  // tau_max over the rows of positive weight (a NaN score makes it NaN)
  double tm = 0.0;
  int32_t tn = 0;
  if (!degenerate)
    for (int64_t k = threadIdx.x; k < K; k += kCafT)
      if (w.c[k] > 0.0) {
        const double gk = g(k), tau = gk * gk;
        if (tau != tau) tn = 1;
        else if (tau > tm) tm = tau;
      }
  smax[threadIdx.x] = tm;
  snan[threadIdx.x] = tn;
  __syncthreads();
  for (int s = kCafT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
      snan[threadIdx.x] |= snan[threadIdx.x + s];
    }
    __syncthreads();
  }
  const double tau_max = smax[0];
  const bool step4 = !degenerate && !snan[0] && tau_max > 0.0 && caf_finite(tau_max);
  double S1 = S;
  if (step4) {
    for (int64_t k = threadIdx.x; k < K; k += kCafT) {
      const double ck = w.c[k];
      if (ck > 0.0) {
        const double gk = g(k);
        w.c[k] = ck * (1.0 - gk * gk / tau_max);
      }
    }
    __syncthreads();
    S1 = caf_sum(K, scratch, [&](int64_t k) { return w.c[k]; });
  }
  const bool again = step4 && S1 > (double)(K - 2 * f);
  if (again)
    for (int64_t k = threadIdx.x; k < K; k += kCafT) {
      const double p = w.c[k] / S1;
      w.p[k] = p;
      w.sp[k] = sqrt(p);
    }
  if (threadIdx.x != 0) return;
  st->lambda = lambda;
  st->rounds += 1;
  if (better) {
    st->best = lambda;
    st->Sbest = S;
    st->best_round = round;
    st->recorded = 1;
  }
  st->S = S1;
  st->round = round + 1;
  st->loop_done = !again;
}

// One block: S = sum c_k (caf_sum's order, the order every round's S is formed in), then the
// first wave lists the rows with c_k > 0, increasing, with c_k / S (flags_to_list's ballot walk).
__global__ void __launch_bounds__(kCafT) caf_compact(const double* __restrict__ c, int64_t K,
                                                     double* __restrict__ coef,
                                                     int32_t* __restrict__ list,
                                                     CafHead* __restrict__ head) {
  __shared__ double scratch[kCafT / 64];
  const double S = caf_sum(K, scratch, [&](int64_t k) { return c[k] > 0.0 ? c[k] : 0.0; });
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  int64_t n = 0;
  for (int64_t i0 = 0; i0 < K; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool in = i < K && c[i < K ? i : 0] > 0.0;
    const uint64_t b = __ballot(in);
    const int64_t pos = n + (int64_t)__builtin_amdgcn_mbcnt_hi(
                                (uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (in) {
      list[pos] = (int32_t)i;
      coef[pos] = c[i] / S;
    }
    n += __popcll(b);
  }
  if (lane == 0) {
    head->S = S;
    head->m = (int32_t)n;
    head->pad = 0;
  }
}

constexpr int kCafU = 4;              // rows in flight per thread in the weighted mean

// out_j = float(sum_t coef[t] x_{list[t] j}), t < head->m in order: a thread owns E columns
// (E = 4: one 16-byte load per row) and walks the listed rows; rows not listed are not read.
template <int E>
__global__ void __launch_bounds__(256) caf_weighted_mean(const float* __restrict__ X, int64_t d,
                                                         int64_t ldx, int ws,
                                                         const double* __restrict__ coef,
                                                         const int32_t* __restrict__ list,
                                                         const CafHead* __restrict__ head,
                                                         float* __restrict__ out) {
  const int64_t m = head->m;
  const int64_t rs = ws ? (int64_t)1 << ws : ldx;    // elements between rows
  const int64_t G = (d + E - 1) / E;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < G;
       gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = gi * E;
    const int nv = d - col >= E ? E : (int)(d - col);
    const float* base = elem(X, ldx, ws, 0, col);
    double acc[E];
#pragma unroll
    for (int i = 0; i < E; ++i) acc[i] = 0.0;
    if (nv == E) {
      int64_t t = 0;
      for (; t + kCafU <= m; t += kCafU) {
        float x[kCafU][E];
        double cf[kCafU];
#pragma unroll
        for (int u = 0; u < kCafU; ++u) {
          const float* src = base + (int64_t)list[t + u] * rs;
          if constexpr (E == 4) {
            const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src));
#pragma unroll
            for (int i = 0; i < 4; ++i) x[u][i] = v[i];
          } else {
            x[u][0] = __builtin_nontemporal_load(src);
          }
          cf[u] = coef[t + u];
        }
#pragma unroll
        for (int u = 0; u < kCafU; ++u)
#pragma unroll
          for (int i = 0; i < E; ++i) acc[i] = fma(cf[u], (double)x[u][i], acc[i]);
      }
      for (; t < m; ++t) {
        const float* src = base + (int64_t)list[t] * rs;
        const double cf = coef[t];
#pragma unroll
        for (int i = 0; i < E; ++i) acc[i] = fma(cf, (double)src[i], acc[i]);
      }
#pragma unroll
      for (int i = 0; i < E; ++i) out[col + i] = (float)acc[i];
    } else {
      // the ragged last group: its columns < d one at a time, the same sums
      for (int i = 0; i < nv; ++i) {
        double s = 0.0;
        for (int64_t t = 0; t < m; ++t)
          s = fma(coef[t], (double)base[(int64_t)list[t] * rs + i], s);
        out[col + i] = (float)s;
      }
    }
  }
}

}  // namespace

size_t caf_layout(char* base, int64_t K, CafWork* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off = (off + bytes + 255) / 256 * 256;
    return p;
  };
  const size_t kd = sizeof(double) * (size_t)K;
  w->st = reinterpret_cast<CafState*>(take(sizeof(CafState)));
  w->head = reinterpret_cast<CafHead*>(take(sizeof(CafHead)));
  w->c = reinterpret_cast<double*>(take(kd));
  w->cbest = reinterpret_cast<double*>(take(kd));
  w->p = reinterpret_cast<double*>(take(kd));
  w->sp = reinterpret_cast<double*>(take(kd));
  w->rho = reinterpret_cast<double*>(take(kd));
  w->w = reinterpret_cast<double*>(take(kd));
  w->z = reinterpret_cast<double*>(take(kd));
  w->y = reinterpret_cast<double*>(take(kd));
  w->coef = reinterpret_cast<double*>(take(kd));
  w->list = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)K));
  return off;
}

static unsigned caf_mv_grid(int64_t K) { return (unsigned)((K + kCafMV / 64 - 1) / (kCafMV / 64)); }

hipError_t launch_caf_begin(const CafWork& w, int64_t K, int64_t f, hipStream_t s) {
  if (w.D)
    hipLaunchKernelGGL(caf_mirror, dim3((unsigned)((K * K + 255) / 256)), dim3(256), 0, s, w.D, K);
  hipLaunchKernelGGL(caf_init, dim3(1), dim3(kCafT), 0, s, w, K, f);
  return hipGetLastError();
}

hipError_t launch_caf_round(const CafWork& w, int64_t K, int64_t f, int64_t power_iters,
                            double tol, hipStream_t s) {
  const dim3 g(caf_mv_grid(K)), b(kCafMV);
  hipLaunchKernelGGL(caf_matvec, g, b, 0, s, w.D, K, w.p, w.st, 1, w.y);
  hipLaunchKernelGGL(caf_start, dim3(1), dim3(kCafT), 0, s, w, K);
  for (int64_t i = 0; i < power_iters; ++i) {
    hipLaunchKernelGGL(caf_matvec, g, b, 0, s, w.D, K, w.z, w.st, 0, w.y);
    hipLaunchKernelGGL(caf_finish, dim3(1), dim3(kCafT), 0, s, w, K, tol);
  }
  hipLaunchKernelGGL(caf_matvec, g, b, 0, s, w.D, K, w.z, w.st, 1, w.y);
  hipLaunchKernelGGL(caf_end, dim3(1), dim3(kCafT), 0, s, w, K, f);
  return hipGetLastError();
}

hipError_t launch_caf_weighted_mean(const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                                    const double* c, const CafWork& w, float* out,
                                    hipStream_t s) {
  hipLaunchKernelGGL(caf_compact, dim3(1), dim3(kCafT), 0, s, c, K, w.coef, w.list, w.head);
  const bool vec = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 4 == 0;
  const int E = vec ? 4 : 1;
  const int64_t items = (d + E - 1) / E;
  const dim3 g((unsigned)std::min<int64_t>((items + 255) / 256, 2048));
  if (vec)
    hipLaunchKernelGGL(caf_weighted_mean<4>, g, dim3(256), 0, s, X, d, ldx, ws, w.coef, w.list,
                       w.head, out);
  else
    hipLaunchKernelGGL(caf_weighted_mean<1>, g, dim3(256), 0, s, X, d, ldx, ws, w.coef, w.list,
                       w.head, out);
  return hipGetLastError();
}

}  // namespace gmk
