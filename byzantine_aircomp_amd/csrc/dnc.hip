// Divide-and-Conquer (Shejwalkar & Houmansadr, "Manipulating the Byzantine", NDSS 2021,
// Algorithm 2): spectral filtering on a sample of n columns.  The definition (centring, the
// stopping rule, the scores, the order of every sum) is in include/gmagg.h; the host loop is
// gm_dnc_f32 (api.hip).  Per round:
//   dnc_gather     G[k][t] = X[k][cols[t]], the K x n sub-matrix as the fp32 values themselves
//   dnc_center     mu[t], the fp64 column sums in row order
//   dnc_rowdot     p[k] = ||c_k||^2 (the start) or c_k . v, one block per row
//   dnc_pick_start / dnc_init_v   v_0 = the centred row of largest norm, normalised
//   dnc_colacc     part[s][j] = sum over the rows of slice s of c_kj p_k
//   dnc_reduce     w = the slices' sum in slice order, block partials of ||w||^2
//   dnc_scale      v <- w / ||w||, block partials of the movement
//   dnc_finish     the state: iteration count, movement test, a degenerate norm
//   dnc_scores     score[k] = (c_k . v)^2
// A centred element is formed where it is used, (double)G[k][j] - mu[j]: the sub-matrix stays
// 4 bytes per element (41 MB at K = 1000, n = 10,000: it stays in the last-level cache between
// the passes) and every product and sum is fp64.  C v and C^T p are two streaming passes over
// G; a K x K Gram form would cost K^2 n / 2 fp64 FMAs up front (5e9 at that shape) to save
// passes that each move 41 MB on chip, and the iteration ends after a handful of them.
// Every reduction has a fixed order that depends on (K, n) alone, and G holds the same values
// whatever X's layout or alignment: the results are bit-identical across them.
#include <algorithm>

#include "device_util.h"
#include "gmagg_internal.h"
#include "select_util.h"

namespace gmk {

constexpr int kDncT = 256;            // threads per block of every kernel below
constexpr int kDncGR = 8;             // rows per block of the gather

__global__ void __launch_bounds__(kDncT) dnc_gather(const float* __restrict__ X, int64_t K,
                                                    int64_t ldx, int ws,
                                                    const int64_t* __restrict__ cols, int64_t n,
                                                    float* __restrict__ G) {
  const int64_t t = (int64_t)blockIdx.x * kDncT + threadIdx.x;
  if (t >= n) return;
  const int64_t j = cols[t];
  const int64_t k0 = (int64_t)blockIdx.y * kDncGR;
  float x[kDncGR];
#pragma unroll
  for (int r = 0; r < kDncGR; ++r) x[r] = k0 + r < K ? *elem(X, ldx, ws, k0 + r, j) : 0.f;
#pragma unroll
  for (int r = 0; r < kDncGR; ++r)
    if (k0 + r < K) G[(k0 + r) * n + t] = x[r];
}

// mu[t] = (sum_k G[k][t]) / K, in row order from 0.0 (8 rows' loads in flight, as col_mean)
__global__ void __launch_bounds__(kDncT) dnc_center(const float* __restrict__ G, int64_t K,
                                                    int64_t n, double* __restrict__ mu) {
  const int64_t t = (int64_t)blockIdx.x * kDncT + threadIdx.x;
  if (t >= n) return;
  const float* col = G + t;
  double s = 0.0;
  int64_t k = 0;
  for (; k + 8 <= K; k += 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = col[(k + u) * n];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (double)x[u];
  }
  for (; k < K; ++k) s += (double)col[k * n];
  mu[t] = s / (double)K;
}

// One block per row k: p[k] = sum_j c_kj^2 (SELF) or sum_j c_kj v_j; thread t takes columns
// t, t + 256, ... in order, then block_sum.  force: run whatever the state says (the scores'
// pass after the iteration has ended).
template <bool SELF>
__global__ void __launch_bounds__(kDncT) dnc_rowdot(const float* __restrict__ G, int64_t n,
                                                    const double* __restrict__ mu,
                                                    const double* __restrict__ v,
                                                    const DncState* __restrict__ st, int force,
                                                    double* __restrict__ p) {
  __shared__ double scratch[kDncT / 64];
  if (!force && st->done) return;                    // (block-uniform)
  const float* g = G + (int64_t)blockIdx.x * n;
  double acc = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += kDncT) {
    const double c = (double)g[j] - mu[j];
    acc += SELF ? c * c : c * v[j];
  }
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) p[blockIdx.x] = acc;
}

// a before b in the order the start row is chosen in: NaN first, then larger first, ties to the
// lower index (a NaN norm anywhere ends the round with NaN scores)
__device__ __forceinline__ bool start_before(double a, int64_t i, double b, int64_t j) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? i < j : an;
  return a > b || (a == b && i < j);
}

// One block: the start row and the round's fresh state.
__global__ void __launch_bounds__(kDncT) dnc_pick_start(const double* __restrict__ r2, int64_t K,
                                                        DncState* __restrict__ st) {
  __shared__ double sv[kDncT];
  __shared__ int64_t si[kDncT];
  int64_t best = -1;
  double bv = 0.0;
  for (int64_t i = threadIdx.x; i < K; i += kDncT)
    if (best < 0 || start_before(r2[i], i, bv, best)) { bv = r2[i]; best = i; }
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int t = 1; t < kDncT; ++t)
    if (si[t] >= 0 && start_before(sv[t], si[t], bv, best)) { bv = sv[t]; best = si[t]; }
  const double nrm = sqrt(bv);
  const bool ok = nrm > 0.0 && nrm < __builtin_inf();
  st->done = !ok;
  st->degenerate = !ok;
  st->converged = nrm == 0.0;
  st->iters = 0;
  st->kstar = best;
  st->val = nrm;                                     // ok: the start row's norm
  st->movement = 0.0;
}

__global__ void __launch_bounds__(kDncT) dnc_init_v(const float* __restrict__ G, int64_t n,
                                                    const double* __restrict__ mu,
                                                    const DncState* __restrict__ st,
                                                    double* __restrict__ v) {
  const int64_t j = (int64_t)blockIdx.x * kDncT + threadIdx.x;
  if (j >= n) return;
  v[j] = st->degenerate ? 0.0 : ((double)G[st->kstar * n + j] - mu[j]) / st->val;
}

// Block (x, s): columns 256 x .. 256 x + 255 over the rows of slice s, in row order.
__global__ void __launch_bounds__(kDncT) dnc_colacc(const float* __restrict__ G, int64_t K,
                                                    int64_t n, const double* __restrict__ mu,
                                                    const double* __restrict__ p, int64_t R,
                                                    const DncState* __restrict__ st,
                                                    double* __restrict__ part) {
  if (st->done) return;
  const int64_t j = (int64_t)blockIdx.x * kDncT + threadIdx.x;
  if (j >= n) return;
  const int64_t k0 = (int64_t)blockIdx.y * R, k1 = k0 + R < K ? k0 + R : K;
  const double m = mu[j];
  const float* col = G + j;
  double acc = 0.0;
  int64_t k = k0;
  for (; k + 8 <= k1; k += 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = col[(k + u) * n];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += ((double)x[u] - m) * p[k + u];
  }
  for (; k < k1; ++k) acc += ((double)col[k * n] - m) * p[k];
  part[(int64_t)blockIdx.y * n + j] = acc;
}

// The sum of a [nb] array of block partials, nb <= kDncBlocks, in one order for every caller.
__device__ __forceinline__ double dnc_sum_blocks(const double* __restrict__ b, int nb,
                                                 double* scratch) {
  double a = 0.0;
  for (int i = threadIdx.x; i < nb; i += kDncT) a += b[i];
  return block_sum(a, scratch);
}

__global__ void __launch_bounds__(kDncT) dnc_reduce(const double* __restrict__ part, int64_t S,
                                                    int64_t n, const DncState* __restrict__ st,
                                                    double* __restrict__ w,
                                                    double* __restrict__ bn) {
  __shared__ double scratch[kDncT / 64];
  if (st->done) return;                              // (block-uniform)
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kDncT + threadIdx.x; j < n;
       j += (int64_t)gridDim.x * kDncT) {
    double x = part[j];
    for (int64_t s = 1; s < S; ++s) x += part[s * n + j];
    w[j] = x;
    acc += x * x;
  }
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) bn[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(kDncT) dnc_scale(const double* __restrict__ w, int64_t n,
                                                   const double* __restrict__ bn,
                                                   const DncState* __restrict__ st,
                                                   double* __restrict__ v,
                                                   double* __restrict__ bm) {
  __shared__ double scratch[kDncT / 64];
  if (st->done) return;                              // (block-uniform)
  const double nrm = sqrt(dnc_sum_blocks(bn, (int)gridDim.x, scratch));
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kDncT + threadIdx.x; j < n;
       j += (int64_t)gridDim.x * kDncT) {
    const double x = w[j] / nrm, dl = x - v[j];
    acc += dl * dl;
    v[j] = x;
  }
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) bm[blockIdx.x] = acc;
}

// One block: the state after this application.
__global__ void __launch_bounds__(kDncT) dnc_finish(const double* __restrict__ bn,
                                                    const double* __restrict__ bm, int nb,
                                                    double tol, DncState* __restrict__ st) {
  __shared__ double scratch[kDncT / 64];
  if (st->done) return;                              // (block-uniform: written below, after the sums)
  const double nrm = sqrt(dnc_sum_blocks(bn, nb, scratch));
  const double mov = sqrt(dnc_sum_blocks(bm, nb, scratch));
  if (threadIdx.x != 0) return;
  st->iters += 1;
  if (!(nrm > 0.0 && nrm < __builtin_inf())) {
    st->done = 1;
    st->degenerate = 1;
    st->converged = nrm == 0.0;
    st->val = nrm;
    return;
  }
  st->movement = mov;
  if (mov <= tol) {
    st->done = 1;
    st->converged = 1;
  }
}

__global__ void __launch_bounds__(kDncT) dnc_scores(const double* __restrict__ p, int64_t K,
                                                    const DncState* __restrict__ st,
                                                    double* __restrict__ score) {
  const int64_t k = (int64_t)blockIdx.x * kDncT + threadIdx.x;
  if (k < K) score[k] = st->degenerate ? st->val : p[k] * p[k];
}

__global__ void __launch_bounds__(kDncT) dnc_and_flags(int32_t* __restrict__ good,
                                                       const int32_t* __restrict__ flag, int64_t K,
                                                       int first) {
  const int64_t k = (int64_t)blockIdx.x * kDncT + threadIdx.x;
  if (k < K) good[k] = first ? flag[k] : (good[k] & flag[k]);
}

static unsigned dnc_cols_grid(int64_t n) { return (unsigned)((n + kDncT - 1) / kDncT); }
static unsigned dnc_red_grid(int64_t n) {
  return (unsigned)std::min<int64_t>((n + kDncT - 1) / kDncT, kDncBlocks);
}

void dnc_slices(int64_t K, int64_t n, int64_t* slices, int64_t* slice_rows) {
  // about 2048 blocks in the C^T p pass, at most 64 slices, at least 8 rows each
  const int64_t nbx = (n + kDncT - 1) / kDncT;
  int64_t S = std::min<int64_t>(64, (2048 + nbx - 1) / nbx);
  S = std::max<int64_t>(1, std::min<int64_t>(S, K / 8));
  const int64_t R = (K + S - 1) / S;
  *slice_rows = R;
  *slices = (K + R - 1) / R;
}

hipError_t launch_dnc_gather(const float* X, int64_t K, int64_t ldx, int ws, const int64_t* cols,
                             int64_t n, float* G, hipStream_t s) {
  const dim3 g(dnc_cols_grid(n), (unsigned)((K + kDncGR - 1) / kDncGR));
  hipLaunchKernelGGL(dnc_gather, g, dim3(kDncT), 0, s, X, K, ldx, ws, cols, n, G);
  return hipGetLastError();
}

hipError_t launch_dnc_center(const DncWork& w, int64_t K, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(dnc_center, dim3(dnc_cols_grid(n)), dim3(kDncT), 0, s, w.G, K, n, w.mu);
  return hipGetLastError();
}

hipError_t launch_dnc_start(const DncWork& w, int64_t K, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(dnc_rowdot<true>, dim3((unsigned)K), dim3(kDncT), 0, s, w.G, n, w.mu, w.v,
                     w.st, 1, w.p);
  hipLaunchKernelGGL(dnc_pick_start, dim3(1), dim3(kDncT), 0, s, w.p, K, w.st);
  hipLaunchKernelGGL(dnc_init_v, dim3(dnc_cols_grid(n)), dim3(kDncT), 0, s, w.G, n, w.mu, w.st,
                     w.v);
  return hipGetLastError();
}

hipError_t launch_dnc_iterate(const DncWork& w, int64_t K, int64_t n, double tol, int64_t count,
                              hipStream_t s) {
  const unsigned nb = dnc_red_grid(n);
  const dim3 gc(dnc_cols_grid(n), (unsigned)w.slices);
  for (int64_t i = 0; i < count; ++i) {
    hipLaunchKernelGGL(dnc_rowdot<false>, dim3((unsigned)K), dim3(kDncT), 0, s, w.G, n, w.mu, w.v,
                       w.st, 0, w.p);
    hipLaunchKernelGGL(dnc_colacc, gc, dim3(kDncT), 0, s, w.G, K, n, w.mu, w.p, w.slice_rows,
                       w.st, w.part);
    hipLaunchKernelGGL(dnc_reduce, dim3(nb), dim3(kDncT), 0, s, w.part, w.slices, n, w.st, w.w,
                       w.bn);
    hipLaunchKernelGGL(dnc_scale, dim3(nb), dim3(kDncT), 0, s, w.w, n, w.bn, w.st, w.v, w.bm);
    hipLaunchKernelGGL(dnc_finish, dim3(1), dim3(kDncT), 0, s, w.bn, w.bm, (int)nb, tol, w.st);
  }
  return hipGetLastError();
}

hipError_t launch_dnc_scores(const DncWork& w, int64_t K, int64_t n, double* score, hipStream_t s) {
  hipLaunchKernelGGL(dnc_rowdot<false>, dim3((unsigned)K), dim3(kDncT), 0, s, w.G, n, w.mu, w.v,
                     w.st, 1, w.p);
  hipLaunchKernelGGL(dnc_scores, dim3((unsigned)((K + kDncT - 1) / kDncT)), dim3(kDncT), 0, s, w.p,
                     K, w.st, score);
  return hipGetLastError();
}

hipError_t launch_dnc_and_flags(int32_t* good, const int32_t* flag, int64_t K, bool first,
                                hipStream_t s) {
  hipLaunchKernelGGL(dnc_and_flags, dim3((unsigned)((K + kDncT - 1) / kDncT)), dim3(kDncT), 0, s,
                     good, flag, K, first ? 1 : 0);
  return hipGetLastError();
}

}  // namespace gmk
