// C ABI of libgmagg.so (include/gmagg.h): contexts, the coordinate-wise aggregators, Krum's
// host side, MeaMed / Multi-Krum / Bulyan, nearest-neighbor mixing, DnC's and the covariance
// filter's host loops, OMA, the synthetic fills,
// the panel pack, s-bucketing,
// the omniscient attacks and the client chain.  The Weiszfeld
// entry points are in host_weiszfeld.hip and host_batched.hip; what the three share is in
// host_ctx.h.
#include <cstring>

#include "host_ctx.h"

using namespace gmh;

extern "C" {

const char* gm_last_error(void) { return g_err.c_str(); }
int gm_abi_version(void) { return GMAGG_ABI_VERSION; }

int64_t gm_panel_width(int64_t K) {
  PassCfg cfg{};
  return K >= 1 && pick_cfg(K, 4, 1, &cfg, true) ? (int64_t)cfg.LPR * cfg.V : 0;
}

int64_t gm_panel_width_bf16(int64_t K) {
  PassCfg cfg{};
  return K >= 1 && pick_cfg(K, 8, 1, &cfg, true, true) ? (int64_t)cfg.LPR * cfg.V : 0;
}

int gm_ctx_create(int device, gm_ctx** out) {
  if (!out) return fail(GM_ERR_INVALID, "gm_ctx_create: out is NULL");
  *out = nullptr;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n)
    return fail(GM_ERR_INVALID, "gm_ctx_create: device %d of %d", device, n);
  gm_ctx* c = new gm_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    c->num_cu = prop.multiProcessorCount;
  *out = c;
  return GM_OK;
}

int gm_ctx_destroy(gm_ctx* c) {
  if (!c) return GM_OK;
  (void)hipSetDevice(c->device);
  if (c->comm) ncclCommDestroy(c->comm);
  if (c->ws) (void)hipFree(c->ws);
  if (c->stage) (void)hipFree(c->stage);
  if (c->shadow) (void)hipFree(c->shadow);
  if (c->host) (void)hipHostFree(c->host);
  if (c->dist_flag) (void)hipHostFree(c->dist_flag);
  for (auto e : c->poll_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto e : c->ev_free) (void)hipEventDestroy(e);
  for (auto& p : c->ev_used) {
    (void)hipEventDestroy(p.first);
    (void)hipEventDestroy(p.second);
  }
  delete c;
  return GM_OK;
}

int gm_ctx_set_shard(gm_ctx* c, int64_t d_total, int64_t d_offset) {
  if (!c || d_total < -1 || d_offset < 0) return fail(GM_ERR_INVALID, "gm_ctx_set_shard: bad args");
  c->d_total = d_total;
  c->d_offset = d_offset;
  return GM_OK;
}

int gm_ctx_set_allreduce(gm_ctx* c, gm_allreduce_cb fn, void* user) {
  if (!c) return fail(GM_ERR_INVALID, "gm_ctx_set_allreduce: ctx is NULL");
  c->ar_fn = fn;
  c->ar_user = user;
  return GM_OK;
}

int gm_rccl_get_unique_id(void* uid) {
  if (!uid) return fail(GM_ERR_INVALID, "gm_rccl_get_unique_id: NULL");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) return fail(GM_ERR_COMM, "ncclGetUniqueId: %s", ncclGetErrorString(r));
  memcpy(uid, &id, sizeof id);
  return GM_OK;
}

int gm_ctx_init_rccl(gm_ctx* c, const void* uid, int nranks, int rank) {
  if (!c || !uid || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(GM_ERR_INVALID, "gm_ctx_init_rccl: bad args");
  HIPCHK(hipSetDevice(c->device));
  ncclUniqueId id;
  memcpy(&id, uid, sizeof id);
  ncclResult_t r = ncclCommInitRank(&c->comm, nranks, id, rank);
  if (r != ncclSuccess) {
    c->comm = nullptr;
    return fail(GM_ERR_COMM, "ncclCommInitRank: %s", ncclGetErrorString(r));
  }
  return GM_OK;
}

int gm_ctx_pass_timing(gm_ctx* c, int enable, double* total_ms, int64_t* launches) {
  if (!c) return fail(GM_ERR_INVALID, "gm_ctx_pass_timing: ctx is NULL");
  double tot = 0.0;
  int64_t n = 0;
  for (auto& p : c->ev_used) {
    HIPCHK(hipEventSynchronize(p.second));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
    tot += ms;
    ++n;
    c->ev_free.push_back(p.first);
    c->ev_free.push_back(p.second);
  }
  c->ev_used.clear();
  if (total_ms) *total_ms = tot;
  if (launches) *launches = n;
  c->timing = enable != 0;
  return GM_OK;
}

int gm_mean_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, float* out,
                void* stream) {
  if (!c || !X || !out || K < 1 || d < 0 || ldx < d) return fail(GM_ERR_INVALID, "gm_mean_f32: bad args");
  if (d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_col_mean(X, K, d, ldx, out, reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

// The coordinate-wise aggregators on client updates in the panel layout: the same
// kernels with panel addressing (W = gm_panel_width(K) = 2^ws, ldx = panel_stride);
// results identical to the row-major calls (same per-column reductions).
static int panel_shift(int64_t K, int64_t panel_stride, int* ws) {
  const int64_t W = gm_panel_width(K);
  if (W == 0 || panel_stride < K * W) return GM_ERR_INVALID;
  *ws = wshift_of(W);
  return GM_OK;
}

// Median (mode 0) / trimmed mean (mode 1) of validated arguments; fn names the entry point.
static int col_select(const char* fn, gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                      int ws, int mode, int64_t trim, float* out, void* stream) {
  if (K > 2048) return fail(GM_ERR_UNSUPPORTED, "%s: K <= 2048", fn);
  if (d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_col_select(X, K, d, ldx, mode, trim, out, reinterpret_cast<hipStream_t>(stream),
                           ws));
  return GM_OK;
}

int gm_mean_panels_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t panel_stride,
                       float* out, void* stream) {
  int ws = 0;
  if (!c || !X || !out || K < 1 || d < 0 || panel_shift(K, panel_stride, &ws))
    return fail(GM_ERR_INVALID, "gm_mean_panels_f32: bad args");
  if (d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_col_mean(X, K, d, panel_stride, out, reinterpret_cast<hipStream_t>(stream), ws));
  return GM_OK;
}

int gm_median_panels_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t panel_stride,
                         float* out, void* stream) {
  int ws = 0;
  if (!c || !X || !out || K < 1 || d < 0 || panel_shift(K, panel_stride, &ws))
    return fail(GM_ERR_INVALID, "gm_median_panels_f32: bad args");
  return col_select("gm_median_panels_f32", c, X, K, d, panel_stride, ws, 0, 0, out, stream);
}

int gm_trimmed_mean_panels_f32(gm_ctx* c, const float* X, int64_t K, int64_t d,
                               int64_t panel_stride, int64_t trim, float* out, void* stream) {
  int ws = 0;
  if (!c || !X || !out || K < 1 || d < 0 || trim < 0 || 2 * trim >= K ||
      panel_shift(K, panel_stride, &ws))
    return fail(GM_ERR_INVALID, "gm_trimmed_mean_panels_f32: bad args");
  return col_select("gm_trimmed_mean_panels_f32", c, X, K, d, panel_stride, ws, 1, trim, out,
                    stream);
}

// getVarience (M:127-129) on rows (wshift 0) or panels (ldx = the panel stride)
static int honest_variance(gm_ctx* c, const float* X, int64_t honest, int64_t d, int64_t ldx,
                           int wshift, float* out, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  const int nb = honest_var_blocks(d, c->num_cu);
  Workspace w;
  const int rc = ensure_ws(c, 1, 1, nb, &w);
  if (rc) return rc;
  HIPCHK(launch_honest_var(X, honest, d, ldx, wshift, nb, w.slab, out, s));
  return GM_OK;
}

int gm_honest_variance_f32(gm_ctx* c, const float* X, int64_t honest, int64_t d, int64_t ldx,
                           float* out, void* stream) {
  if (!c || !X || !out || honest < 1 || d < 1 || ldx < d)
    return fail(GM_ERR_INVALID, "gm_honest_variance_f32: bad args");
  return honest_variance(c, X, honest, d, ldx, 0, out, stream);
}

int gm_honest_variance_panels_f32(gm_ctx* c, const float* X, int64_t K, int64_t honest, int64_t d,
                                  int64_t panel_stride, float* out, void* stream) {
  const int64_t W = gm_panel_width(K);
  if (!c || !X || !out || honest < 1 || honest > K || d < 1 || W == 0 || panel_stride < K * W)
    return fail(GM_ERR_INVALID, "gm_honest_variance_panels_f32: bad args");
  return honest_variance(c, X, honest, d, panel_stride, wshift_of(W), out, stream);
}

int gm_median_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, float* out,
                  void* stream) {
  if (!c || !X || !out || K < 1 || d < 0 || ldx < d) return fail(GM_ERR_INVALID, "gm_median_f32: bad args");
  return col_select("gm_median_f32", c, X, K, d, ldx, 0, 0, 0, out, stream);
}

int gm_trimmed_mean_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                        int64_t trim, float* out, void* stream) {
  if (!c || !X || !out || K < 1 || d < 0 || ldx < d || trim < 0 || 2 * trim >= K)
    return fail(GM_ERR_INVALID, "gm_trimmed_mean_f32: bad args");
  return col_select("gm_trimmed_mean_f32", c, X, K, d, ldx, 0, 1, trim, out, stream);
}

static int krum_impl(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                     int64_t honest, float* out, int64_t* index, void* stream);

int gm_krum_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int64_t honest,
                float* out, int64_t* index, void* stream) {
  if (!c || !X || !out || K < 1 || d < 0 || ldx < d || honest < 2 || honest - 1 > K)
    return fail(GM_ERR_INVALID, "gm_krum_f32: bad args (needs 2 <= honestSize <= K+1)");
  if (K > 4096) return fail(GM_ERR_UNSUPPORTED, "gm_krum_f32: K <= 4096");
  return krum_impl(c, X, K, d, ldx, 0, honest, out, index, stream);
}

int gm_krum_panels_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t panel_stride,
                       int64_t honest, float* out, int64_t* index, void* stream) {
  int ws = 0;
  if (!c || !X || !out || K < 1 || d < 0 || honest < 2 || honest - 1 > K ||
      panel_shift(K, panel_stride, &ws))
    return fail(GM_ERR_INVALID, "gm_krum_panels_f32: bad args (needs 2 <= honestSize <= K+1)");
  if (K > 4096) return fail(GM_ERR_UNSUPPORTED, "gm_krum_panels_f32: K <= 4096");
  return krum_impl(c, X, K, d, panel_stride, ws, honest, out, index, stream);
}

// Krum through the Gram MFMA kernel (coordinate.hip krum_gram_bounds: the bounds, the
// candidates, the exact recomputation).  epsg bounds the relative error |G~_ij - G_ij| /
// (n_i n_j) of the scaled-f16 split (gram.hip): the split's dropped terms (<= 3 * 2^-22),
// the fp32 chain of one flush period (kH16Flush stages x 64 columns = 8192 columns, 3
// products: <= 768 accumulator roundings + the 32-term MFMA sums + the fp32 partial,
// <= 800 * 2^-24) and the centring rounding (2^-24 each side), rounded up to 6e-5.  The f16
// subnormal floor is an ABSOLUTE error set by each column block's shared scale (one large
// row raises it for every row of the block): krum_gram_bounds adds it from the exponents
// the Gram kernel exports (a per-row bound was assumed here before).
static double krum_gram_eps() { return 6e-5; }

// GMAGG_KRUM: 0 exact pair distances only, 1 the Gram path wherever it is eligible, 2
// (default) AUTO: the Gram path at K >= 64 and K^2 d >= 2^29 (it measured faster on every
// shape from 64 x 131,072 up, profiles/r5s2_krum_ab.jsonl).  Read per call (the tests
// switch it).
static int krum_mode() {
  const char* e = getenv("GMAGG_KRUM");
  return e ? atoi(e) : 2;
}

// Returns GM_OK with *done = false when the exact path must run (not eligible, a
// non-finite Gram, too many candidates), c->krum_info saying why.
static int krum_gram(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                     int64_t honest, float* out, int64_t* index, hipStream_t s, bool* done) {
  *done = false;
  const int KT = gram_kt(K), KP = 32 * KT;
  const int64_t kk = honest - 1;
  const GramGrid gg = gram_grid(d, GramKind::H16, c->num_cu);
  const int64_t S = krum_slices(K, d);
  const int64_t RC = krum_refine_max();
  const int64_t maxc = 4 * RC;
  // slab: the Gram partials, then (after gram_reduce has consumed them) the refinement's
  // [S][RC][K] fp64 partials + Dc [RC][K]; behind both the candidate list (int64)
  size_t body = std::max(gram_slab_floats(KT, gg), (size_t)2 * (size_t)(S * RC * K + RC * K));
  body = (body + 1) / 2 * 2;
  Workspace w;
  int rc = ensure_ws(c, K, d, 1, &w, body + 2 * (size_t)(maxc + 2), KP);
  if (rc) return rc;
  rc = ensure_host(c, sizeof(KState) + 2 * sizeof(int64_t));
  if (rc) return rc;
  double* part = reinterpret_cast<double*>(w.gslab);
  double* Dc = part + (size_t)S * RC * K;
  int64_t* cand = reinterpret_cast<int64_t*>(w.gslab + body);
  int64_t* didx = reinterpret_cast<int64_t*>(w.r);
  KState* hst = host_state(c);
  int64_t* hcand = host_after_states<int64_t>(c);
  const int64_t W = ws ? (int64_t)1 << ws : 0;
  // The bounds scale with the rows' distances from the centre p: row 0 first (honest in
  // the reference's layout, M:292); when it leaves too many candidates (a Byzantine row 0,
  // far from the honest cluster) once more from the row of the smallest upper bound.
  int64_t n = 0, centre = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    float* p = w.g[1];
    HIPCHK(launch_copy_row_k(X, d, ldx, ws, centre, p, s));
    HIPCHK(hipMemsetAsync(w.st, 0, sizeof(KState), s));
    HIPCHK(launch_gram(X, K, d, ws ? W : ldx, p, GramKind::H16, gg, w.gslab, w.G, w.st, s,
                       ws ? ldx : 0, ws));
    HIPCHK(launch_gram_check(w.G, KP, w.st, s));
    HIPCHK(launch_krum_gram_select(w.G, KP, K, kk, krum_gram_eps(),
                                   gram_block_exp(w.gslab, KT, gg), gg.nb, d, w.alpha, w.u, maxc,
                                   cand, s));
    HIPCHK(hipMemcpyAsync(hst, w.st, sizeof(KState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hcand, cand, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hcand + 1, cand + maxc + 1, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (hst->gram_bad) {
      c->krum_info[2] = GM_KRUM_REASON_GRAM_NONFINITE;
      return GM_OK;
    }
    n = hcand[0];
    if (n != -2 || hcand[1] == centre) break;
    centre = hcand[1];
  }
  if (n < 1) {
    c->krum_info[2] = GM_KRUM_REASON_CANDIDATES;
    return GM_OK;
  }
  for (int64_t q = 0; q < n; q += RC) {
    const int m = (int)std::min<int64_t>(RC, n - q);
    HIPCHK(launch_krum_refine(X, K, d, ldx, ws, cand + 1 + q, m, kk, part, Dc, w.sums + q, s));
  }
  HIPCHK(launch_krum_pick(w.sums, cand + 1, n, X, d, ldx, ws, didx, out, s));
  if (index) {
    HIPCHK(hipMemcpyAsync(index, didx, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  c->krum_info[0] = GM_KRUM_GRAM;
  c->krum_info[1] = n;
  c->krum_info[2] = GM_KRUM_REASON_OK;
  *done = true;
  return GM_OK;
}

int gm_delta_last_info(gm_ctx* c, int64_t* info) {
  if (!c || !info) return fail(GM_ERR_INVALID, "gm_delta_last_info: bad args");
  for (int i = 0; i < 3; ++i) info[i] = c->delta_info[i];
  return GM_OK;
}

int gm_krum_last_info(gm_ctx* c, int64_t* info) {
  if (!c || !info) return fail(GM_ERR_INVALID, "gm_krum_last_info: bad args");
  for (int i = 0; i < 3; ++i) info[i] = c->krum_info[i];
  return GM_OK;
}

static int krum_impl(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                     int64_t honest, float* out, int64_t* index, void* stream) {
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  c->krum_info[0] = GM_KRUM_EXACT;
  c->krum_info[1] = 0;
  c->krum_info[2] = GM_KRUM_REASON_NOT_CHOSEN;
  // the Gram kernel's inputs: K <= 256; rows 16-byte aligned with d, ldx multiples of 4
  // (float4 stages); panels of width 64 / 128 / 256 (a power of two, multiple of 64)
  const bool eligible =
      gram_kt(K) > 0 && d > 0 && honest - 1 <= K &&
      (ws ? (ws >= 6 && ws <= 8 && K * ((int64_t)1 << ws) * 4 <= 0x7fffffff)
          : (d % 4 == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 &&
             ldx < ((int64_t)1 << 26)));
  const int mode = krum_mode();
  const bool want = mode == 1 || (mode == 2 && K >= 64 && (double)K * K * d >= 536870912.0);
  if (want && !eligible) c->krum_info[2] = GM_KRUM_REASON_NOT_ELIGIBLE;
  if (want && eligible) {
    bool done = false;
    const int rc = krum_gram(c, X, K, d, ldx, ws, honest, out, index, s, &done);
    if (rc || done) return rc;
  }
  Workspace w;
  // G area holds the K x K distances; the float slab holds the per-slice fp64 partials
  const size_t part_doubles = (size_t)krum_slices(K, d) * (size_t)(K * K);
  int rc = ensure_ws(c, K, 1, 1, &w, 2 * part_doubles, (int)K);
  if (rc) return rc;
  int64_t* didx = reinterpret_cast<int64_t*>(w.u);
  HIPCHK(launch_krum(X, K, d, ldx, honest - 1, w.G, reinterpret_cast<double*>(w.gslab), w.alpha,
                     out, didx, s, ws));
  if (index) {
    HIPCHK(hipMemcpyAsync(index, didx, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return GM_OK;
}

// ---- MeaMed, Multi-Krum, Bulyan (robust.hip) ------------------------------------------------

// The panel shift of a validated layout (0 for rows) after the stride check.
static int robust_shift(const char* fn, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                        int* ws) {
  *ws = 0;
  if (layout == GM_LAYOUT_ROWS) {
    if (ldx < d) return fail(GM_ERR_INVALID, "%s: ldx = %lld < d", fn, (long long)ldx);
    return GM_OK;
  }
  const int64_t W = gm_panel_width(K);
  if (W == 0)
    return fail(GM_ERR_UNSUPPORTED, "%s: no panel layout for K = %lld rows (pass them row-major)",
                fn, (long long)K);
  if (ldx < K * W)
    return fail(GM_ERR_INVALID, "%s: panel stride %lld < K * W = %lld", fn, (long long)ldx,
                (long long)(K * W));
  *ws = wshift_of(W);
  return GM_OK;
}

static bool known_layout(int32_t l) { return l == GM_LAYOUT_ROWS || l == GM_LAYOUT_PANELS; }

int gm_meamed_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                  const int32_t* rows, int64_t n_rows, int64_t keep, float* out, void* stream) {
  if (!c || !X || !out || K < 1 || d < 0 || !known_layout(layout) || n_rows < 1 || n_rows > K ||
      (!rows && n_rows != K) || keep < 1 || keep > n_rows)
    return fail(GM_ERR_INVALID, "gm_meamed_f32: bad args (a NULL ctx, X or out, K < 1, d < 0, an "
                "unknown layout, n_rows outside [1, K] or != K without rows, keep outside "
                "[1, n_rows])");
  if (K > 1024) return fail(GM_ERR_UNSUPPORTED, "gm_meamed_f32: K <= 1024 (got %lld)", (long long)K);
  int ws = 0;
  const int rc = robust_shift("gm_meamed_f32", K, d, ldx, layout, &ws);
  if (rc) return rc;
  if (d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_meamed(X, d, ldx, ws, rows, n_rows, keep, out,
                       reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

// The exact path's distances into w->G (Krum's workspace layout: the slices' partials in the
// float slab); int32 scratch: w->u holds 2K, w->r 2K.
static int krum_distances(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                          Workspace* w, hipStream_t s) {
  const size_t part_doubles = (size_t)krum_slices(K, d) * (size_t)(K * K);
  const int rc = ensure_ws(c, K, 1, 1, w, 2 * part_doubles, (int)K);
  if (rc) return rc;
  HIPCHK(launch_krum_dist(X, K, d, ldx, ws, w->G, reinterpret_cast<double*>(w->gslab), s));
  return GM_OK;
}

static int copy_selected(int32_t* selected, const int32_t* dev, int64_t n, hipStream_t s) {
  if (!selected) return GM_OK;
  HIPCHK(hipMemcpyAsync(selected, dev, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return GM_OK;
}

int gm_multi_krum_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                      int64_t honest, int64_t m, float* out, int32_t* selected, void* stream) {
  if (!c || !X || !out || K < 1 || d < 0 || !known_layout(layout) || honest < 2 ||
      honest - 1 > K || m < 1 || m > K)
    return fail(GM_ERR_INVALID, "gm_multi_krum_f32: bad args (a NULL ctx, X or out, K < 1, d < 0, "
                "an unknown layout; needs 2 <= honestSize <= K+1 and 1 <= m <= K)");
  if (K > 4096)
    return fail(GM_ERR_UNSUPPORTED, "gm_multi_krum_f32: K <= 4096 (got %lld)", (long long)K);
  int ws = 0;
  int rc = robust_shift("gm_multi_krum_f32", K, d, ldx, layout, &ws);
  if (rc) return rc;
  if (d == 0) return GM_OK;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  Workspace w;
  rc = krum_distances(c, X, K, d, ldx, ws, &w, s);
  if (rc) return rc;
  HIPCHK(launch_krum_scores(w.G, K, honest - 1, w.alpha, s));
  int32_t* flag = reinterpret_cast<int32_t*>(w.u);
  int32_t* list = flag + K;
  HIPCHK(launch_multi_krum_pick(w.alpha, K, m, X, d, ldx, ws, flag, list, out, s));
  return copy_selected(selected, list, m, s);
}

int gm_bulyan_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                  int64_t honest, float* out, int32_t* selected, void* stream) {
  const int64_t f = K - honest;
  if (!c || !X || !out || K < 1 || d < 0 || !known_layout(layout) || honest < 1 || f < 0 ||
      K < 4 * f + 3)
    return fail(GM_ERR_INVALID, "gm_bulyan_f32: bad args (a NULL ctx, X or out, K < 1, d < 0, an "
                "unknown layout; needs f = K - honestSize >= 0 and K >= 4f + 3)");
  if (K > 1024) return fail(GM_ERR_UNSUPPORTED, "gm_bulyan_f32: K <= 1024 (got %lld)", (long long)K);
  int ws = 0;
  int rc = robust_shift("gm_bulyan_f32", K, d, ldx, layout, &ws);
  if (rc) return rc;
  if (d == 0) return GM_OK;
  const int64_t theta = K - 2 * f, beta = theta - 2 * f;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  Workspace w;
  rc = krum_distances(c, X, K, d, ldx, ws, &w, s);
  if (rc) return rc;
  int32_t* alive = reinterpret_cast<int32_t*>(w.u);
  int32_t* list = alive + K;
  int32_t* picked = reinterpret_cast<int32_t*>(w.r);
  // (the slices' partials are dead once D is reduced: the float slab holds >= 2 K^2 words)
  int32_t* ord = reinterpret_cast<int32_t*>(w.gslab);
  HIPCHK(launch_bulyan_select(w.G, K, f, theta, w.alpha, ord, alive, picked, list, s));
  HIPCHK(launch_meamed(X, d, ldx, ws, list, theta, beta, out, s));
  return copy_selected(selected, picked, theta, s);
}

// GMAGG_NNM_STOP (read per call; tools/nnm_bench.py times the steps apart with it): 1 returns
// after the distances, 2 after the neighbours; anything else runs the whole call.
static int nnm_stop() { return env_int("GMAGG_NNM_STOP", 0); }

int gm_nnm_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout_in,
               int64_t f, float* Y, int64_t ldy, int32_t layout_out, int32_t* neighbors,
               void* stream) {
  if (!c || !X || !Y || K < 1 || d < 0 || f < 0 || f > K - 1 || !known_layout(layout_in) ||
      !known_layout(layout_out))
    return fail(GM_ERR_INVALID, "gm_nnm_f32: bad args (a NULL ctx, X or Y, K < 1, d < 0, f outside "
                "[0, K - 1] or an unknown layout)");
  if (K > 4096) return fail(GM_ERR_UNSUPPORTED, "gm_nnm_f32: K <= 4096 (got %lld)", (long long)K);
  int ws = 0, wsy = 0;
  int rc = robust_shift("gm_nnm_f32", K, d, ldx, layout_in, &ws);
  if (rc) return rc;
  rc = robust_shift("gm_nnm_f32", K, d, ldy, layout_out, &wsy);
  if (rc) return rc;
  if (d == 0) return GM_OK;
  if (c->d_total > 0 || c->comm || c->ar_fn)
    return fail(GM_ERR_UNSUPPORTED, "gm_nnm_f32: a d-sharded or collective context (the distances would need a "
                "K x K all-reduce)");
  const int64_t m = K - f;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  // Krum's workspace (D in the G area, the slices' partials in the float slab); the partials
  // are dead once D is reduced, and the slab then holds the mask
  const size_t part_doubles = (size_t)krum_slices(K, d) * (size_t)(K * K);
  Workspace w;
  rc = ensure_ws(c, K, 1, 1, &w, std::max(2 * part_doubles, (size_t)nnm_mask_words(K)), (int)K);
  if (rc) return rc;
  HIPCHK(launch_krum_dist(X, K, d, ldx, ws, w.G, reinterpret_cast<double*>(w.gslab), s));
  const int stop = nnm_stop();
  if (stop == 1) return GM_OK;
  uint32_t* mask = reinterpret_cast<uint32_t*>(w.gslab);
  HIPCHK(launch_nnm_neighbors(w.G, K, m, mask, neighbors, s));
  if (stop == 2) return GM_OK;
  HIPCHK(launch_nnm_mix(X, K, d, ldx, ws, mask, m, Y, ldy, wsy, s));
  return GM_OK;
}

// GMAGG_DNC_STOP (read per call; tools/dnc_bench.py times the stages apart with it): 1 returns
// after the first round's gather, 2 after the last round's selection (before the final mean);
// anything else runs the whole call.
static int dnc_stop() { return env_int("GMAGG_DNC_STOP", 0); }

// The most elements of a sampled sub-matrix (512 MiB of workspace as fp32).
constexpr int64_t kDncMaxElems = (int64_t)1 << 27;

int gm_dnc_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
               const int64_t* columns, int64_t n, int64_t iters, int64_t remove,
               int64_t power_iters, double power_tol, float* out, double* scores, int32_t* good,
               int64_t* n_good, int32_t* niter, int32_t* converged, void* stream) {
  if (!c || !X || !out || !scores || !good || !n_good || !niter || !converged ||
      (remove > 0 && !columns))
    return fail(GM_ERR_INVALID, "gm_dnc_f32: a NULL ctx, X, out, scores, good, n_good, niter or "
                "converged, or NULL columns with remove > 0");
  if (K < 2 || d < 0 || !known_layout(layout) || iters < 1 || remove < 0 || remove >= K ||
      (remove > 0 && iters > (K - 1) / remove) || power_iters < 1 || !(power_tol >= 0) ||
      (remove > 0 && (n < 1 || n > d)))
    return fail(GM_ERR_INVALID, "gm_dnc_f32: bad args (K < 2, d < 0, an unknown layout, iters < 1, "
                "remove < 0, remove * iters >= K, power_iters < 1, power_tol not >= 0, n outside "
                "[1, d])");
  if (K > 4096) return fail(GM_ERR_UNSUPPORTED, "gm_dnc_f32: K <= 4096 (got %lld)", (long long)K);
  if (remove > 0 && n > kDncMaxElems / K)
    return fail(GM_ERR_UNSUPPORTED, "gm_dnc_f32: K * n = %lld x %lld sampled elements exceed %lld",
                (long long)K, (long long)n, (long long)kDncMaxElems);
  int ws = 0;
  int rc = robust_shift("gm_dnc_f32", K, d, ldx, layout, &ws);
  if (rc) return rc;
  if (c->d_total > 0 || c->comm || c->ar_fn)
    return fail(GM_ERR_UNSUPPORTED, "gm_dnc_f32: a d-sharded or collective context (the sampled "
                "columns and the final mean would span the shards)");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (remove == 0) {       // nothing is filtered: the column mean, gm_mean_f32's launch
    HIPCHK(hipSetDevice(c->device));
    if (d > 0) HIPCHK(launch_col_mean(X, K, d, ldx, out, s, ws));
    HIPCHK(hipMemsetAsync(scores, 0, sizeof(double) * (size_t)(iters * K), s));
    for (int64_t t = 0; t < iters; ++t) { niter[t] = 0; converged[t] = 1; }
    for (int64_t k = 0; k < K; ++k) good[k] = (int32_t)k;
    *n_good = K;
    return GM_OK;
  }
  WsOrder order(c, s);
  HIPCHK(order.err);
  DncWork w{};
  dnc_slices(K, n, &w.slices, &w.slice_rows);
  int32_t *flag = nullptr, *goodf = nullptr, *list = nullptr;
  auto lay = [&](char* base) {
    Carve cv{base};
    w.st = cv.take<DncState>(1);
    w.G = cv.take<float>((size_t)(K * n));
    w.mu = cv.take<double>(n);
    w.v = cv.take<double>(n);
    w.w = cv.take<double>(n);
    w.part = cv.take<double>((size_t)(w.slices * n));
    w.p = cv.take<double>(K);
    w.bn = cv.take<double>(kDncBlocks);
    w.bm = cv.take<double>(kDncBlocks);
    flag = cv.take<int32_t>(K);
    goodf = cv.take<int32_t>(K);
    list = cv.take<int32_t>(K);
    return cv.off;
  };
  rc = grow_ws(c, lay(nullptr));
  if (rc) return rc;
  lay(c->ws);
  // the pinned buffer: DncState | pad to 256 | int32 flags[K]
  rc = ensure_host(c, 256 + sizeof(int32_t) * (size_t)K);
  if (rc) return rc;
  DncState* hst = reinterpret_cast<DncState*>(c->host);
  int32_t* hflag = reinterpret_cast<int32_t*>(c->host + 256);
  const int stop = dnc_stop();
  for (int64_t t = 0; t < iters; ++t) {
    HIPCHK(launch_dnc_gather(X, K, ldx, ws, columns + t * n, n, w.G, s));
    if (stop == 1) return GM_OK;
    HIPCHK(launch_dnc_center(w, K, n, s));
    HIPCHK(launch_dnc_start(w, K, n, s));
    // the iteration runs ahead in chunks; the state is polled between them
    for (int64_t it = 0; it < power_iters;) {
      const int64_t chunk = std::min<int64_t>(it == 0 ? 8 : 16, power_iters - it);
      HIPCHK(launch_dnc_iterate(w, K, n, power_tol, chunk, s));
      it += chunk;
      HIPCHK(hipMemcpyAsync(hst, w.st, sizeof(DncState), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (hst->done) break;
    }
    niter[t] = hst->iters;
    converged[t] = hst->converged;
    double* sc = scores + t * K;
    HIPCHK(launch_dnc_scores(w, K, n, sc, s));
    HIPCHK(launch_score_top_m(sc, K, K - remove, flag, s));
    HIPCHK(launch_dnc_and_flags(goodf, flag, K, t == 0, s));
  }
  HIPCHK(launch_flags_to_list(goodf, K, 1, list, s));
  HIPCHK(hipMemcpyAsync(hflag, goodf, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int64_t m = 0;
  for (int64_t k = 0; k < K; ++k)
    if (hflag[k]) good[m++] = (int32_t)k;
  *n_good = m;                                       // >= K - remove * iters >= 1
  if (stop == 2) return GM_OK;
  HIPCHK(launch_gather_mean(X, d, ldx, ws, list, m, out, s));
  return GM_OK;
}

// GMAGG_CAF_STOP (read per call; tools/caf_bench.py times the stages apart with it): 1 returns
// after the distances, 2 after the last round (before the weighted mean); anything else runs the
// whole call.
static int caf_stop() { return env_int("GMAGG_CAF_STOP", 0); }

int gm_caf_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
               int64_t f, int64_t power_iters, double power_tol, float* out, double* weights,
               double* eigenvalue, double* weight, int32_t* rounds, int32_t* best_round,
               int32_t* niter, int32_t* converged, void* stream) {
  if (!c || !X || !out) return fail(GM_ERR_INVALID, "gm_caf_f32: a NULL ctx, X or out");
  if (K < 2 || d < 0 || !known_layout(layout) || f < 0 || 2 * f >= K || power_iters < 1 ||
      !(power_tol >= 0))
    return fail(GM_ERR_INVALID, "gm_caf_f32: bad args (K < 2, d < 0, an unknown layout, f < 0, "
                "2f >= K, power_iters < 1, power_tol not >= 0)");
  if (K > 4096) return fail(GM_ERR_UNSUPPORTED, "gm_caf_f32: K <= 4096 (got %lld)", (long long)K);
  int ws = 0;
  int rc = robust_shift("gm_caf_f32", K, d, ldx, layout, &ws);
  if (rc) return rc;
  if (c->d_total > 0 || c->comm || c->ar_fn)
    return fail(GM_ERR_UNSUPPORTED, "gm_caf_f32: a d-sharded or collective context (the distances "
                "would need a K x K all-reduce)");
  if (d == 0) return GM_OK;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  CafWork cw{};
  const size_t need = caf_layout(nullptr, K, &cw);
  const double nan = std::nan("");
  if (f == 0) {            // no round runs: the column mean, gm_mean_f32's launch, and c* = 1
    HIPCHK(launch_col_mean(X, K, d, ldx, out, s, ws));
    if (weights) {
      rc = grow_ws(c, need);
      if (rc) return rc;
      caf_layout(c->ws, K, &cw);
      HIPCHK(launch_caf_begin(cw, K, 0, s));
      HIPCHK(hipMemcpyAsync(weights, cw.c, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, s));
    }
    if (eigenvalue) *eigenvalue = nan;
    if (weight) *weight = (double)K;
    if (rounds) *rounds = 0;
    if (best_round) *best_round = 0;
    return GM_OK;
  }
  // Krum's workspace (D in the G area, the slices' partials in the float slab); the partials
  // are dead once D is reduced, and the slab then holds the solver's O(K) state
  const size_t part_doubles = (size_t)krum_slices(K, d) * (size_t)(K * K);
  Workspace w;
  rc = ensure_ws(c, K, 1, 1, &w, std::max(2 * part_doubles, (need + 3) / 4), (int)K);
  if (rc) return rc;
  rc = ensure_host(c, sizeof(CafState));
  if (rc) return rc;
  HIPCHK(launch_krum_dist(X, K, d, ldx, ws, w.G, reinterpret_cast<double*>(w.gslab), s));
  const int stop = caf_stop();
  if (stop == 1) return GM_OK;
  caf_layout(reinterpret_cast<char*>(w.gslab), K, &cw);
  cw.D = w.G;
  HIPCHK(launch_caf_begin(cw, K, f, s));
  CafState* hst = reinterpret_cast<CafState*>(c->host);
  std::vector<int32_t> nit, cv;
  // every completed round zeroes a positive weight: at most K rounds; the state is read once
  // per round, the round's power_iters applications are queued without looking
  for (int64_t t = 0; t < K; ++t) {
    HIPCHK(launch_caf_round(cw, K, f, power_iters, power_tol, s));
    HIPCHK(hipMemcpyAsync(hst, cw.st, sizeof(CafState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (hst->rounds > (int32_t)nit.size()) {
      nit.push_back(hst->iters);
      cv.push_back(hst->converged);
    }
    if (hst->loop_done) break;
  }
  if (stop == 2) return GM_OK;
  HIPCHK(launch_caf_weighted_mean(X, K, d, ldx, ws, cw.cbest, cw, out, s));
  if (weights)
    HIPCHK(hipMemcpyAsync(weights, cw.cbest, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, s));
  if (eigenvalue) *eigenvalue = hst->rounds > 0 ? hst->best : nan;
  if (weight) *weight = hst->Sbest;
  if (rounds) *rounds = hst->rounds;
  if (best_round) *best_round = hst->best_round;
  for (size_t t = 0; t < nit.size(); ++t) {
    if (niter) niter[t] = nit[t];
    if (converged) converged[t] = cv[t];
  }
  return GM_OK;
}

int gm_weighted_mean_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                         int32_t layout, const double* weights, float* out, void* stream) {
  if (!c || !X || !weights || !out || K < 1 || d < 0 || !known_layout(layout))
    return fail(GM_ERR_INVALID, "gm_weighted_mean_f32: bad args (a NULL ctx, X, weights or out, "
                "K < 1, d < 0 or an unknown layout)");
  if (K > 4096)
    return fail(GM_ERR_UNSUPPORTED, "gm_weighted_mean_f32: K <= 4096 (got %lld)", (long long)K);
  int ws = 0;
  int rc = robust_shift("gm_weighted_mean_f32", K, d, ldx, layout, &ws);
  if (rc) return rc;
  if (d == 0) return GM_OK;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  CafWork cw{};
  rc = grow_ws(c, caf_layout(nullptr, K, &cw));
  if (rc) return rc;
  caf_layout(c->ws, K, &cw);
  HIPCHK(launch_caf_weighted_mean(X, K, d, ldx, ws, weights, cw, out, s));
  return GM_OK;
}

int gm_oma_philox_f32(gm_ctx* c, float* X, int64_t K, int64_t d, int64_t ldx, double noise_var,
                      uint64_t seed, void* stream) {
  if (!c || !X || K < 0 || d < 0 || ldx < d || noise_var < 0)
    return fail(GM_ERR_INVALID, "gm_oma_philox_f32: bad args");
  if (K == 0 || d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  const int64_t d_total = c->d_total > 0 ? c->d_total : d;
  const int64_t col_off = c->d_total > 0 ? c->d_offset : 0;
  HIPCHK(launch_oma_philox(X, K, d, ldx, d_total, col_off, (float)std::sqrt(noise_var), seed,
                           reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_oma_philox_batched_f32(gm_ctx* c, float* X, int64_t P, int64_t K, int64_t d, int64_t ldx,
                              int64_t pstride, double noise_var, uint64_t seed, void* stream) {
  if (!c || !X || P < 0 || K < 0 || d < 0 || ldx < d || noise_var < 0 ||
      (P > 1 && pstride < K * ldx))
    return fail(GM_ERR_INVALID, "gm_oma_philox_batched_f32: bad args");
  if (P == 0 || K == 0 || d == 0) return GM_OK;
  if (c->d_total > 0)
    return fail(GM_ERR_UNSUPPORTED, "gm_oma_philox_batched_f32: not on a d-sharded context");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_oma_philox(X, K, d, ldx, d, 0, (float)std::sqrt(noise_var), seed,
                           reinterpret_cast<hipStream_t>(stream), 0, P, P > 1 ? pstride : 0));
  return GM_OK;
}

int gm_oma_philox_batched_panels_f32(gm_ctx* c, float* X, int64_t P, int64_t K, int64_t d,
                                     int64_t panel_stride, int64_t pstride, double noise_var,
                                     uint64_t seed, void* stream) {
  const int64_t W = gm_panel_width(K);
  if (!c || !X || P < 0 || K < 0 || d < 0 || noise_var < 0 || (K > 0 && W == 0) ||
      panel_stride < K * W || (P > 1 && pstride < (d + W - 1) / W * panel_stride))
    return fail(GM_ERR_INVALID, "gm_oma_philox_batched_panels_f32: bad args");
  if (P == 0 || K == 0 || d == 0) return GM_OK;
  if (c->d_total > 0)
    return fail(GM_ERR_UNSUPPORTED, "gm_oma_philox_batched_panels_f32: not on a d-sharded context");
  HIPCHK(hipSetDevice(c->device));
  const int wshift = wshift_of(W);
  HIPCHK(launch_oma_philox(X, K, d, panel_stride, d, 0, (float)std::sqrt(noise_var), seed,
                           reinterpret_cast<hipStream_t>(stream), wshift, P, P > 1 ? pstride : 0));
  return GM_OK;
}

int gm_oma_philox_panels_f32(gm_ctx* c, float* X, int64_t K, int64_t d, int64_t panel_stride,
                             double noise_var, uint64_t seed, void* stream) {
  const int64_t W = gm_panel_width(K);
  if (!c || !X || K < 0 || d < 0 || noise_var < 0 || (K > 0 && W == 0) || panel_stride < K * W)
    return fail(GM_ERR_INVALID, "gm_oma_philox_panels_f32: bad args");
  if (K == 0 || d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  const int64_t d_total = c->d_total > 0 ? c->d_total : d;
  const int64_t col_off = c->d_total > 0 ? c->d_offset : 0;
  const int wshift = wshift_of(W);
  HIPCHK(launch_oma_philox(X, K, d, panel_stride, d_total, col_off, (float)std::sqrt(noise_var),
                           seed, reinterpret_cast<hipStream_t>(stream), wshift));
  return GM_OK;
}

int gm_rows_to_panels_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                          float* P, int64_t W, int64_t panel_stride, void* stream) {
  if (!c || !X || !P || K < 0 || d < 0 || ldx < d || W < 1 || panel_stride < K * W)
    return fail(GM_ERR_INVALID, "gm_rows_to_panels_f32: bad args");
  if (K == 0 || d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_rows_to_panels(X, K, d, ldx, P, W, panel_stride,
                               reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

static int pack_bf16(gm_ctx* c, const void* X, bool src_f32, int64_t K, int64_t d, int64_t ldx,
                     uint16_t* P, int64_t W, int64_t panel_stride, void* stream, const char* who) {
  if (!c || !X || !P || K < 0 || d < 0 || ldx < d || W < 1 || panel_stride < K * W)
    return fail(GM_ERR_INVALID, "%s: bad args", who);
  if (K == 0 || d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_rows_to_panels_bf16(X, src_f32, K, d, ldx, P, W, panel_stride,
                                    reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_rows_to_panels_bf16_from_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                                    uint16_t* P, int64_t W, int64_t panel_stride, void* stream) {
  return pack_bf16(c, X, true, K, d, ldx, P, W, panel_stride, stream,
                   "gm_rows_to_panels_bf16_from_f32");
}

int gm_rows_to_panels_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                           uint16_t* P, int64_t W, int64_t panel_stride, void* stream) {
  return pack_bf16(c, X, false, K, d, ldx, P, W, panel_stride, stream, "gm_rows_to_panels_bf16");
}

// s-bucketing of validated pointers: the layouts' panel widths (0 for rows) and strides
static int bucket_means(const char* fn, gm_ctx* c, const void* X, bool bf16, int64_t K, int64_t d,
                        int64_t ldx, int32_t lin, const int32_t* perm, int64_t s, float* Y,
                        int64_t ldy, int32_t lout, void* stream) {
  auto known = [](int32_t l) { return l == GM_LAYOUT_ROWS || l == GM_LAYOUT_PANELS; };
  if (!c || !X || !Y || K < 1 || d < 0 || s < 1 || !known(lin) || !known(lout))
    return fail(GM_ERR_INVALID, "%s: bad args (a NULL ctx, X or Y, K < 1, d < 0, s < 1 or an "
                "unknown layout)", fn);
  const int64_t Kb = s >= K ? 1 : (K + s - 1) / s;
  int64_t Wi = 0, Wo = 0;
  if (lin == GM_LAYOUT_PANELS) {
    Wi = bf16 ? gm_panel_width_bf16(K) : gm_panel_width(K);
    if (Wi == 0)
      return fail(GM_ERR_UNSUPPORTED, "%s: no panel layout for K = %lld input rows (pass them "
                  "row-major)", fn, (long long)K);
  } else if (K > 0x7fffffffll) {
    return fail(GM_ERR_INVALID, "%s: K = %lld exceeds the int32 row indices", fn, (long long)K);
  }
  if (lout == GM_LAYOUT_PANELS) {
    Wo = gm_panel_width(Kb);
    if (Wo == 0)
      return fail(GM_ERR_UNSUPPORTED, "%s: no panel layout for the %lld bucket means (take them "
                  "row-major)", fn, (long long)Kb);
  }
  if (ldx < (Wi ? K * Wi : d) || ldy < (Wo ? Kb * Wo : d))
    return fail(GM_ERR_INVALID, "%s: ldx = %lld or ldy = %lld too small for its layout", fn,
                (long long)ldx, (long long)ldy);
  if (d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_bucket_means(X, bf16, K, d, ldx, Wi, perm, s, Y, ldy, Wo,
                             reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_bucket_means_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                        int32_t layout_in, const int32_t* perm, int64_t s, float* Y, int64_t ldy,
                        int32_t layout_out, void* stream) {
  return bucket_means("gm_bucket_means_f32", c, X, false, K, d, ldx, layout_in, perm, s, Y, ldy,
                      layout_out, stream);
}

int gm_bucket_means_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                         int32_t layout_in, const int32_t* perm, int64_t s, float* Y, int64_t ldy,
                         int32_t layout_out, void* stream) {
  return bucket_means("gm_bucket_means_bf16", c, X, true, K, d, ldx, layout_in, perm, s, Y, ldy,
                      layout_out, stream);
}

// ---- the omniscient attacks (attack.hip) ------------------------------------------------------

// The common refusals of the attack entry points, then the panel shift (0 for rows).
static int attack_shift(const char* fn, gm_ctx* c, const void* X, bool bf16, int64_t K, int64_t d,
                        int64_t ldx, int32_t layout, int64_t byz, int* ws) {
  if (!c || !X || K < 1 || d < 0 || !known_layout(layout) || byz < 1 || K - byz < 2)
    return fail(GM_ERR_INVALID, "%s: bad args (a NULL ctx or X, K < 1, d < 0, an unknown layout, "
                "byz < 1 or fewer than 2 honest rows)", fn);
  if (!bf16 || layout == GM_LAYOUT_ROWS) return robust_shift(fn, K, d, ldx, layout, ws);
  const int64_t W = gm_panel_width_bf16(K);
  if (W == 0)
    return fail(GM_ERR_UNSUPPORTED, "%s: no bf16 panel layout for K = %lld rows (pass them "
                "row-major)", fn, (long long)K);
  if (ldx < K * W)
    return fail(GM_ERR_INVALID, "%s: panel stride %lld < K * W = %lld (W = gm_panel_width_bf16)",
                fn, (long long)ldx, (long long)(K * W));
  *ws = wshift_of(W);
  return GM_OK;
}

static int attack_affine(const char* fn, gm_ctx* c, void* X, bool bf16, int64_t K, int64_t d,
                         int64_t ldx, int32_t layout, int64_t byz, double a, double b,
                         void* stream) {
  int ws = 0;
  const int rc = attack_shift(fn, c, X, bf16, K, d, ldx, layout, byz, &ws);
  if (rc) return rc;
  if (d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_attack_affine(X, bf16, K, K - byz, d, ldx, ws, a, b,
                              reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_attack_affine_f32(gm_ctx* c, float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                         int64_t byz, double a, double b, void* stream) {
  return attack_affine("gm_attack_affine_f32", c, X, false, K, d, ldx, layout, byz, a, b, stream);
}

int gm_attack_affine_bf16(gm_ctx* c, uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                          int32_t layout, int64_t byz, double a, double b, void* stream) {
  return attack_affine("gm_attack_affine_bf16", c, X, true, K, d, ldx, layout, byz, a, b, stream);
}

int gm_attack_minmax_f32(gm_ctx* c, float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                         int64_t byz, int32_t rule, int32_t dev, double* gamma, void* stream) {
  const char* fn = "gm_attack_minmax_f32";
  int ws = 0;
  int rc = attack_shift(fn, c, X, false, K, d, ldx, layout, byz, &ws);
  if (rc) return rc;
  if (rule < 0 || rule > 1 || dev < 0 || dev > 2)
    return fail(GM_ERR_INVALID, "%s: rule %d (0 max, 1 sum) or dev %d (0 std, 1 unit, 2 sign)", fn,
                rule, dev);
  if (K > 4096) return fail(GM_ERR_UNSUPPORTED, "%s: K <= 4096 (got %lld)", fn, (long long)K);
  if (d == 0) {
    if (gamma) *gamma = 0.0;
    return GM_OK;
  }
  const int64_t H = K - byz;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  // Krum's workspace on H rows (D in the G area, the slices' partials in the float slab), the
  // iterate area as mu [d] and p [d] fp64, the slab as the row terms' slices
  const int nb = attack_term_blocks(d);
  const size_t part_doubles = (size_t)krum_slices(H, d) * (size_t)(H * H);
  Workspace w;
  rc = ensure_ws(c, H, 4 * d, nb, &w, 2 * part_doubles, (int)H);
  if (rc) return rc;
  double* mu = reinterpret_cast<double*>(w.g[0]);
  // the panel shift and stride are K's: a row's address does not depend on the row count
  HIPCHK(launch_krum_dist(X, H, d, ldx, ws, w.G, reinterpret_cast<double*>(w.gslab), s));
  HIPCHK(launch_attack_minmax(X, K, H, d, ldx, ws, rule, dev, w.G, mu, mu + d, w.slab, nb, w.sums,
                              w.alpha, w.r, s));
  if (gamma) {
    HIPCHK(hipMemcpyAsync(gamma, w.r + 1, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return GM_OK;
}

int gm_client_chain_f32(gm_ctx* c, const float* data, int64_t ldd, const int64_t* labels,
                        int64_t F, int64_t C, const int32_t* idx, int64_t K, int64_t B,
                        int64_t honest, int32_t attack, float gamma, float weight_decay,
                        float* W, float* b, float* X, int64_t ldx, int32_t layout, void* stream) {
  if (!c || !data || !labels || !idx || !W || !b || !X || K < 0 || honest < 0 || ldd < F ||
      attack < 0 || attack > 2 || (layout != GM_LAYOUT_ROWS && layout != GM_LAYOUT_PANELS))
    return fail(GM_ERR_INVALID, "gm_client_chain_f32: bad args");
  if (!client_chain_supported(F, C, B))
    return fail(GM_ERR_UNSUPPORTED, "gm_client_chain_f32: needs F <= 832, C <= 64, B <= 64 "
                "(F=%lld C=%lld B=%lld)", (long long)F, (long long)C, (long long)B);
  const int64_t d = C * F + C;
  ClientChainArgs a{};
  a.data = data; a.ldd = ldd; a.labels = labels; a.F = F; a.C = C; a.idx = idx;
  a.K = K; a.B = B; a.honest = honest; a.attack = attack; a.gamma = gamma; a.wd = weight_decay;
  a.W = W; a.b = b; a.X = X;
  if (layout == GM_LAYOUT_PANELS) {
    const int64_t Wp = gm_panel_width(K);
    if (Wp == 0 || ldx < K * Wp) return fail(GM_ERR_INVALID, "gm_client_chain_f32: panel stride");
    a.pstride = ldx;
    a.wshift = wshift_of(Wp);
  } else {
    if (ldx < d) return fail(GM_ERR_INVALID, "gm_client_chain_f32: ldx < C*F + C");
    a.ldx = ldx;
  }
  if (K == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_client_chain(a, reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_client_grads_f32(gm_ctx* c, const float* data, int64_t ldd, const int64_t* labels,
                        int64_t F, int64_t C, const int32_t* idx, int64_t K, int64_t B,
                        int64_t honest, int32_t attack, float beta, float weight_decay,
                        const float* W, const float* b, float* M, int64_t ldx, int32_t layout,
                        void* stream) {
  if (!c || !data || !labels || !idx || !W || !b || !M || K < 1 || K > INT32_MAX || B < 1 ||
      F < 1 || C < 1 || honest < 0 || honest > K || ldd < F || attack < 0 || attack > 2 ||
      (layout != GM_LAYOUT_ROWS && layout != GM_LAYOUT_PANELS) || !(beta >= 0.f && beta < 1.f))
    return fail(GM_ERR_INVALID, "gm_client_grads_f32: bad args");
  if (!client_grads_supported(F, C, B))
    return fail(GM_ERR_UNSUPPORTED, "gm_client_grads_f32: needs F <= 832, C <= 64, B <= 64 "
                "(F=%lld C=%lld B=%lld)", (long long)F, (long long)C, (long long)B);
  const int64_t d = C * F + C;
  ClientGradArgs a{};
  a.data = data; a.ldd = ldd; a.labels = labels; a.F = F; a.C = C; a.idx = idx;
  a.K = K; a.B = B; a.honest = honest; a.attack = attack; a.beta = beta; a.wd = weight_decay;
  a.W = W; a.b = b; a.M = M;
  if (layout == GM_LAYOUT_PANELS) {
    const int64_t Wp = gm_panel_width(K);
    if (Wp == 0)
      return fail(GM_ERR_UNSUPPORTED, "gm_client_grads_f32: K=%lld has no panel width",
                  (long long)K);
    if (ldx < K * Wp) return fail(GM_ERR_INVALID, "gm_client_grads_f32: panel stride");
    a.pstride = ldx;
    a.wshift = wshift_of(Wp);
  } else {
    if (ldx < d) return fail(GM_ERR_INVALID, "gm_client_grads_f32: ldx < C*F + C");
    a.ldx = ldx;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_client_grads(a, reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_oma_apply_f32(gm_ctx* c, float* X, int64_t K, int64_t d, int64_t ldx, const float* hr,
                     const float* hi, const float* nr, const float* ni, void* stream) {
  if (!c || !X || !hr || !hi || !nr || !ni || K < 0 || d < 0 || ldx < d)
    return fail(GM_ERR_INVALID, "gm_oma_apply_f32: bad args");
  if (K == 0 || d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_oma_apply(X, K, d, ldx, hr, hi, nr, ni, reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_fill_clients_f32(gm_ctx* c, float* X, int64_t K, int64_t d, int64_t ldx, int64_t B,
                        float mu_h, float sd_h, float mu_b, float sd_b, uint64_t seed,
                        void* stream) {
  if (!c || !X || K < 0 || d < 0 || ldx < d || B < 0 || B > K)
    return fail(GM_ERR_INVALID, "gm_fill_clients_f32: bad args");
  if (K == 0 || d == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  const int64_t d_total = c->d_total > 0 ? c->d_total : d;
  const int64_t col_off = c->d_total > 0 ? c->d_offset : 0;
  HIPCHK(launch_fill_clients(X, K, d, ldx, B, mu_h, sd_h, mu_b, sd_b, d_total, col_off, seed,
                             reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

int gm_fill_normal_f32(gm_ctx* c, float* v, int64_t n, float mu, float sd, uint64_t seed,
                       void* stream) {
  if (!c || !v || n < 0) return fail(GM_ERR_INVALID, "gm_fill_normal_f32: bad args");
  if (n == 0) return GM_OK;
  HIPCHK(hipSetDevice(c->device));
  const int64_t col_off = c->d_total > 0 ? c->d_offset : 0;
  HIPCHK(launch_fill_normal(v, n, mu, sd, col_off, seed, reinterpret_cast<hipStream_t>(stream)));
  return GM_OK;
}

}  // extern "C"
