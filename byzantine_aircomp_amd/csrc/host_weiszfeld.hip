// gm_weiszfeld_f32 (include/gmagg.h): one Weiszfeld problem per call.  The entry point
// validates and selects; the paths are run_gram, run_resident, run_resident_batched with
// P = 1 (host_batched.hip) and run_stream.  gm_weiszfeld_bf16 (client updates stored as
// bf16) validates and runs run_stream on a bf16 tile.  gm_cclip_f32 / gm_cclip_bf16 (centered
// clipping) run the same loop with the clipping rule in the K-space step.  What a call asks
// of run_stream is one StreamJob; the four entry points share one prologue (begin_call,
// check_panels, no_iteration).
//
// The host loop mirrors the reference's control flow (MNIST_Air_weight.py:145-160
// for gm, 173-184 for gm2) but keeps every decision on the device: the
// K-space kernel sets a `done` word that makes later launches no-ops, and the
// host only polls it every `check_every` iterations.
#include <cstring>

#include "host_ctx.h"

using namespace gmh;

namespace {

// What a call derives once from the context and the options.
// d-sharding: every decision that changes the sequence of collectives (Gram or
// streaming, the poll interval and with it the passes queued after the stop) is
// taken from GLOBAL quantities (K, d_total, options), so all ranks issue the same
// all-reduces even when the last shard is shorter or ragged.  Local properties
// (vector width, tile) only pick kernels.
struct CallTraits {
  bool sharded;
  int64_t d_total, col_off;
  bool host_noise;   // AirComp with the caller's draws (GM_NOISE_HOST)
  bool collective;   // sharded, or an all-reduce (RCCL, callback) is set: no resident path
};

CallTraits traits_of(const gm_ctx* c, int64_t d) {
  CallTraits tr{};
  tr.sharded = c->d_total > 0;
  tr.d_total = tr.sharded ? c->d_total : d;
  tr.col_off = tr.sharded ? c->d_offset : 0;
  tr.collective = tr.sharded || c->comm || c->ar_fn;
  return tr;
}

// The K-space step's rule: the reference's gm2 and gm (AirComp), or centered clipping.
enum class Rule { Gm2, Gm, Cclip };

// One call of the launch-per-pass loop (run_stream).
struct StreamJob {
  const void* X;         // fp32 elements, or bf16 where the tile says so (cfg.B16)
  int64_t K, d, ldx;
  bool panels;           // X in the panel layout, ldx its panel stride, cfg the panel tile
  PassCfg cfg;           // the STEP tile (two-pass: unused)
  int algo;              // GM_ALGO_STREAM (the fused pass) or GM_ALGO_TWOPASS
  const float* guess0;
  float* out;
  Rule rule;
  double tau;            // Rule::Cclip: the clipping radius
  int64_t maxiter;
  double tol, eps;
  int check_every;
  AirNoise air;          // Rule::Gm
  gm_noise_cb noise_cb;  // tr.host_noise: the caller's draws
  void* noise_user;
  CallTraits tr;
  PreOma oma;            // the pre-noise still to apply, if any
  hipStream_t s;
  bool guard_rejected;   // a Gram result was computed and refused before this loop
};

// The reference's draws of iteration `it` (OMA2, M:401-402, M:411): from the callback
// into the pinned staging, then to their device copies.
int upload_draws(gm_ctx* c, const StreamJob& j, const Workspace& w, int64_t it) {
  const int64_t K = j.K, d = j.d;
  hipStream_t s = j.s;
  float* h_hr = host_noise_stage(c);
  float* h_hi = h_hr + K;
  float* h_n = h_hi + K;   // d_total + 1
  if (j.noise_cb(j.noise_user, it, h_hr, h_hi, j.air.has_noise ? h_n : nullptr) != 0)
    return fail(GM_ERR_CALLBACK, "noise callback failed at iteration %lld", (long long)it);
  HIPCHK(hipMemcpyAsync(w.h_re, h_hr, sizeof(float) * K, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.h_im, h_hi, sizeof(float) * K, hipMemcpyHostToDevice, s));
  if (j.air.has_noise) {
    const float* n_cols = h_n + j.tr.col_off;   // this shard's columns, then the last element
    HIPCHK(hipMemcpyAsync(w.hnoise, n_cols, sizeof(float) * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.hnoise + d, h_n + j.tr.d_total, sizeof(float), hipMemcpyHostToDevice,
                          s));
  }
  return GM_OK;
}

// Small problems (resident.hip): one cooperative launch, X in VGPRs, every
// iteration on the device.
int run_resident(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                 const float* guess0, float* out, const gm_opts* o, gm_result* res,
                 const PassCfg& cfg, int cpb, int nb, hipStream_t s, bool* timed_out,
                 int64_t pstride = 0, int wshift = 0) {
  *timed_out = false;
  // granules [2][nb][2 values] in the slab region, + the timeout word in sums
  const size_t words = resident_gran_words(K, cfg, nb);
  const int64_t S = 2 * K + 2;
  Workspace w;
  int rc = ensure_ws(c, K, d, (int)((words + S - 1) / S), &w);
  if (rc) return rc;
  rc = ensure_host(c, sizeof(KState));
  if (rc) return rc;
  unsigned* bar = reinterpret_cast<unsigned*>(w.sums);  // reuse: timeout word, zeroed per call
  HIPCHK(hipMemsetAsync(w.st, 0, sizeof(KState), s));
  HIPCHK(hipMemsetAsync(bar, 0, 16, s));
  HIPCHK(hipMemsetAsync(w.slab, 0, align_up(words * 8, 16), s));   // every tag = 0
  ResArgs a{};
  a.X = X; a.K = K; a.d = d; a.ldx = ldx; a.guess0 = guess0; a.out = out;
  a.pstride = pstride; a.wshift = wshift;
  a.maxiter = o->maxiter; a.tol = (float)o->tol; a.eps = (float)o->eps;
  a.mode = o->mode; a.has_noise = aircomp_noise(o);
  a.P_max = o->P_max; a.noise_sd = noise_sd(o);
  a.seed = o->seed;
  a.gran = reinterpret_cast<unsigned long long*>(w.slab);
  a.checkin = a.gran + (size_t)2 * nb * S;      // (resident_gran_words: + nb + 1 slots)
  a.need = checkin_need((unsigned)nb);
  a.stride = res_xcd_stride(nb, c->num_cu);
  // beyond one XCD: the XCD-hierarchical gather (members -> group leader -> every block),
  // its member granules L2-kept where the check-in confirms a group on one XCD
  // (where it pays, measured: K = 50 × d = 48,670 (96 blocks of 512 columns) 8.45 -> 7.47 µs
  // per iteration, 50 × 60,000 (118 blocks) 8.78 -> 7.38; but 50 × 30,000 (59) 6.72 -> 7.32,
  // 50 × 20,000 (40) 5.99 -> 7.16 and K <= 32 slower at every size: the leader's extra hop
  // costs more than the polls it saves on smaller grids or fewer values;
  // profiles/r5s1_resident_hier_shapes_ab.jsonl, r5s1_resident_hier2_ab.jsonl)
  const int hm = res_hier_mode();
  a.hier = a.stride == 1 && nb > 8 && 2 * K + 2 <= cfg.NW * 64 &&
           (hm == 2 || (hm == 1 && nb >= 90 && K > 32)) && resident_has_exchange(cfg, cpb, 1);
  a.local = (a.stride == 8 || a.hier) && res_xcd_mode() == 2;
  a.lvl2 = a.checkin + nb + 1;
  // below the hierarchical gather's range: the split-scope exchange (one hop, as the flat
  // gather, but each reader polls its own XCD's blocks from L2-kept copies)
  a.split = a.stride == 1 && !a.hier && nb > 8 && res_xcd_mode() == 2 && res_split_mode() != 0 &&
            resident_has_exchange(cfg, cpb, 2);
  a.granL = a.lvl2 + (size_t)32 * (2 * K + 2);
  a.bar = bar; a.st = w.st;
  hipEvent_t e0, e1;
  rc = record_pass_begin(c, s, &e0, &e1);
  if (rc) return rc;
  HIPCHK(launch_resident(cfg, cpb, nb * (int)a.stride, a, s));
  rc = record_pass_end(c, s, e0, e1);
  if (rc) return rc;
  KState* hst = host_state(c);
  HIPCHK(hipMemcpyAsync(hst, w.st, sizeof(KState), hipMemcpyDeviceToHost, s));
  unsigned hbar[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(hbar, bar, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  static const bool verbose = getenv("GMAGG_RES_VERBOSE") != nullptr;
  if (verbose)
    fprintf(stderr, "gmagg resident: nb=%d stride=%u local=%d (requested %d) timed_out=%u\n", nb,
            a.stride, hbar[0] ? (int)hbar[0] - 1 : -1, a.local, hbar[2]);
  if (hbar[2]) {   // the grid was not co-resident long enough: caller reruns on streaming
    *timed_out = true;
    if (!hbar[3]) c->res_skip = kResSkipAfterCheckinFail;   // failed at the check-in
    drop_last_timing(c);
    return GM_OK;
  }
  gm_result r = result_from(*hst, GM_ALGO_RESIDENT);
  // The hierarchical gather ran whenever a.hier is set (its member granules are L2-kept
  // only where the check-in confirmed a group on one XCD; ADVICE r5: report the gather that
  // ran, as run_resident_batched does).  Otherwise bar[0] = 1 + local.
  r.exchange = a.hier ? GM_EXCHANGE_XCD_HIER
               : hbar[0] != 2 ? GM_EXCHANGE_AGENT
               : a.split ? GM_EXCHANGE_XCD_SPLIT : GM_EXCHANGE_XCD_LOCAL;
  if (res) *res = r;
  return GM_OK;
}

// Gram-space gm2 (gram.hip): G = X'X'^T once (MFMA), the Weiszfeld loop in K-space
// (one launch, fp64), one closing pass g = sum_k a_k x_k.  Two reads of X.
//
// AUTO guard (guarded = true).  The K-space loop is exact up to the error of G
// (fp32 accumulation; for the bf16 split also the bits of x' beyond h + m), and
// it has none of the reference's fp32 rounding of the iterate.  The closing pass
// is then a full streaming STEP pass at the returned weights, which also yields
// the exact distances ||x_k - g||^2; gram_verify compares the next weights from
// those with the K-space map's and measures the one-step error e = ||X'^T b||.
// The result is kept only if (1) e / (1 - rho) <= 1e-6 ||g|| (rho = the last
// K-space contraction ratio, clamped to [0.5, 0.95]), and (2) the reference's own
// fp32 movement noise floor, measured at 0.4-1.8 x 2^-24 ||g|| and
// taken as 2^-23 ||g||, is at most tol, so that the reference's loop does stop.
// Otherwise *rejected is set and the caller runs the streaming path.  With the floor
// below tol/3 the reference stops within +-1 iteration of the exact loop (guard
// ACCEPTED); between tol/3 and tol its count is decided by rounding — the streaming
// path's too — and the Gram's exact count lies in that window of legitimate stopping
// points (guard ACCEPTED_FLOOR; round 4: the whole C4 job, ||g|| = 74, is here).
int run_gram(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx, const float* guess0,
             float* out, const gm_opts* o, gm_result* res, const PassCfg& cfg, hipStream_t s,
             bool split, bool guarded, bool* rejected, int64_t pstride = 0) {
  *rejected = false;
  // panels (pstride > 0): X is [ceil(d/W)][K][W] with W = the STEP tile's chunk width
  // (cfg), a multiple of the Gram kernel's 64-column stage; the f16 kernel only
  int wshift = 0;
  if (pstride) {
    const int W = cfg.LPR * cfg.V;
    wshift = wshift_of(W);
    if ((1 << wshift) != W || W % 64 || !split) return fail(GM_ERR_UNSUPPORTED, "Gram on panels: W=%d", W);
  }
  const int KT = gram_kt(K), KP = 32 * KT;
  // split: the scaled f16 kernel (3 products), rerun as the bf16 split (4 products,
  // the full fp32 exponent range) if its G came out non-finite (GMAGG_GRAM_KIND=bf16
  // forces the bf16 kernel: A/B)
  const char* kind_env = getenv("GMAGG_GRAM_KIND");
  const bool force_bf16 = kind_env && strcmp(kind_env, "bf16") == 0;
  GramKind kind = !split ? GramKind::F32 : (force_bf16 && !pstride) ? GramKind::BF16 : GramKind::H16;
  GramGrid gg = gram_grid(d, kind, c->num_cu);
  const GramGrid gb = gram_grid(d, GramKind::BF16, c->num_cu);
  const size_t slab_n = std::max(gram_slab_floats(KT, gg),
                                 kind == GramKind::H16 ? gram_slab_floats(KT, gb) : 0);
  // closing pass: the STEP tile when it also yields the distances (guarded), else
  // the lighter sum-only tile
  const PassCfg ccfg = (guarded || pstride) ? cfg : light_cfg(K, cfg);
  const int J = ccfg.LPR * ccfg.V;
  const int nb_p = (int)std::max<int64_t>(
      1, std::min<int64_t>((d + J - 1) / J,
                           (int64_t)c->num_cu * pass_blocks_per_cu(ccfg, guarded ? 0 : 3)));
  Workspace w;
  int rc = ensure_ws(c, K, d, nb_p, &w, slab_n, KP);
  if (rc) return rc;
  rc = ensure_host(c, sizeof(KState) + 4 * sizeof(double));
  if (rc) return rc;
  KState* hst = host_state(c);
  double* hsums = host_after_states<double>(c);
  // centre p = guess0, staged to an aligned workspace copy (float4 loads)
  float* p = w.g[1];
  HIPCHK(hipMemcpyAsync(p, guess0, sizeof(float) * d, hipMemcpyDeviceToDevice, s));
again:
  HIPCHK(hipMemsetAsync(w.st, 0, sizeof(KState), s));
  hipEvent_t e0, e1;
  rc = record_pass_begin(c, s, &e0, &e1);
  if (rc) return rc;
  HIPCHK(launch_gram(X, K, d, ldx, p, kind, gg, w.gslab, w.G, w.st, s, pstride, wshift));
  rc = record_pass_end(c, s, e0, e1);
  if (rc) return rc;
  rc = allreduce(c, w.G, (int64_t)KP * KP, s);
  if (rc) return rc;
  // a non-finite G (f16 overflow on any rank, or a non-finite input) sets
  // gram_bad; checked after the all-reduce, so every rank takes the same branch
  HIPCHK(launch_gram_check(w.G, KP, w.st, s));
  HIPCHK(launch_gram_solve(w.G, KP, K, o->maxiter, (float)o->tol, (float)o->eps, w.alpha, w.u,
                           w.coef, w.st, s));
  // closing pass: g = sum_k a_k x_k (+ the exact distances to g when guarded)
  const int64_t S = guarded ? K + 2 : 2;
  PassArgs a{};
  a.X = X; a.K = K; a.d = d; a.ldx = pstride ? pstride : ldx;
  a.g_old = p; a.g_new = out; a.coef = w.coef; a.st = w.st;
  a.slab = w.slab; a.slab_stride = S;
  a.panel_stride = pstride;
  HIPCHK(launch_pass(ccfg, guarded ? 0 : 3, nb_p, a, s));
  HIPCHK(launch_slab_reduce(w.slab, nb_p, S, w.sums, w.st, s));   // [D (K)] [||p-g||^2, ||g||^2]
  rc = allreduce(c, w.sums, S, s);
  if (rc) return rc;
  if (guarded)
    HIPCHK(launch_gram_verify(w.G, KP, K, (float)o->eps, w.u, w.alpha, w.sums, w.r, w.st, s));
  HIPCHK(hipMemcpyAsync(hst, w.st, sizeof(KState), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hsums, w.sums + (S - 2), 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (hst->gram_bad && kind == GramKind::H16) {   // rare: the f16 range was exceeded
    if (pstride) {                                 // no bf16 panel kernel: streaming path
      *rejected = true;
      return GM_OK;
    }
    kind = GramKind::BF16;
    gg = gb;
    goto again;
  }
  bool floor_band = false;
  if (guarded) {
    const double u = std::ldexp(1.0, -24);
    const double gn = std::sqrt(std::max(0.0, hsums[1]));
    double rho = hst->guard_r;
    rho = rho != rho ? 0.5 : std::min(0.95, std::max(0.5, rho));
    const double pred = hst->guard_q / (1.0 - rho) / gn;
    const bool accurate = pred <= 1e-6;                     // NaN fails
    const double floor = kFloorUlps * u * gn;        // (oracle FLOOR_ULPS, the count window)
    const bool floor_ok = !hst->converged || floor <= o->tol;
    floor_band = hst->converged && floor > o->tol / 3.0;
    static const bool dbg = getenv("GMAGG_GUARD_DEBUG") != nullptr;
    if (dbg)
      fprintf(stderr, "[gram guard] K=%lld d=%lld q=%.3e rho=%.3f |g|=%.4e pred=%.3e converged=%d "
              "iters=%d floor_ok=%d band=%d accurate=%d\n", (long long)K, (long long)d, hst->guard_q,
              rho, gn, pred, (int)hst->converged, (int)hst->iters, (int)floor_ok, (int)floor_band,
              (int)accurate);
    if (!accurate || !floor_ok) {
      *rejected = true;
      return GM_OK;
    }
  }
  gm_result r = result_from(*hst, split ? GM_ALGO_GRAM : GM_ALGO_GRAM_F32);
  r.gram_kind = kind == GramKind::H16 ? 1 : kind == GramKind::BF16 ? 2 : 3;
  r.guard = !guarded ? GM_GUARD_NONE : floor_band ? GM_GUARD_ACCEPTED_FLOOR : GM_GUARD_ACCEPTED;
  if (res) *res = r;
  return GM_OK;
}

// Grids of the streaming loop's STEP and INIT passes (algo: GM_ALGO_STREAM or _TWOPASS).
void stream_grids(const gm_ctx* c, int64_t K, int64_t d, int algo, const PassCfg& cfg,
                  const PassCfg& cfg_i, int init_mode, int step_mode, int* nb_step, int* nb_init) {
  if (algo != GM_ALGO_STREAM) {
    *nb_step = *nb_init = twopass_blocks(K, d, c->num_cu);
    return;
  }
  const int J = cfg.LPR * cfg.V, Ji = cfg_i.LPR * cfg_i.V;
  const int64_t nch = (d + J - 1) / J, nchi = (d + Ji - 1) / Ji;
  const int64_t cap_s = (int64_t)c->num_cu * pass_blocks_per_cu(cfg, step_mode);
  const int64_t cap_i = (int64_t)c->num_cu * pass_blocks_per_cu(cfg_i, init_mode);
  *nb_step = (int)std::max<int64_t>(1, std::min(nch, cap_s));
  *nb_init = (int)std::max<int64_t>(1, std::min(nchi, cap_i));
}

// The launch-per-pass loop: an INIT pass, then per iteration one STEP pass over X (the
// fused streaming pass on tile cfg, or the two-pass kernels at K > 2048), the all-reduce
// of its partials and the K-space step.  panels: X in the panel layout, ldx its panel
// stride, cfg the panel tile (used for INIT too).  The job's pre-noise, if any is pending,
// is fused into INIT where the tile allows.
// Centered clipping is the same loop: the K-space step's third rule, and the STEP pass's
// column term is the old iterate.
// final_state: the KState the result was taken from (nullable).
int run_stream(gm_ctx* c, StreamJob& j, gm_result* res, KState* final_state = nullptr) {
  const int64_t K = j.K, d = j.d;
  hipStream_t s = j.s;
  const bool host_noise = j.tr.host_noise;
  const int64_t d_total = j.tr.d_total;
  const bool cclip = j.rule == Rule::Cclip, air = j.rule == Rule::Gm;
  // What the rule decides: the INIT pass (||x_k||^2 only for AirComp), the STEP pass and its
  // column term (PassArgs.noise; clipping's is the old iterate), the K-space step's mode.
  const int init_mode = air ? 2 : 1;
  const int step_mode = cclip ? kPassStepSelf : 0;
  const int noise_kind = cclip ? 3 : !j.air.has_noise ? 0 : (host_noise ? 2 : 1);
  const int kmode = cclip ? kModeCclip : air ? GM_MODE_AIRCOMP : GM_MODE_IDEAL;

  StreamPasses sp{c, s};
  sp.twopass = j.algo != GM_ALGO_STREAM;
  sp.cfg[0] = j.cfg;
  sp.cfg[1] = j.panels ? j.cfg : light_cfg(K, j.cfg);
  sp.mode[0] = step_mode;
  sp.mode[1] = init_mode;
  stream_grids(c, K, d, j.algo, sp.cfg[0], sp.cfg[1], init_mode, step_mode, &sp.nb[0], &sp.nb[1]);
  const int nb = std::max(sp.nb[0], sp.nb[1]);
  // gm2 on fp32 panels: late passes as corrections on a bf16 shadow.  Whether
  // the loop is armed follows from the job and GLOBAL sizes, so every rank of a sharded
  // context queues the same kernels and all-reduces the same K + 3 sums.
  PassCfg dcfg{};       // the correction pass's bf16 tile
  int64_t Wb = 0;
  bool delta = j.rule == Rule::Gm2 && j.panels && !j.cfg.B16 && !sp.twopass && !host_noise &&
               noise_kind == 0 && delta_knob() != 0 &&
               (delta_knob() == 1 || 4 * K * d_total >= kDeltaMinBytes) &&
               pass_kernel_delta(j.cfg, kPassStepExactD) != nullptr;
  int nb_d = 0;         // its grid
  if (delta) {
    // shadow panels of the fp32 chunk's width (32 columns): 4 lanes of 8 bf16 per row, 8 rows
    // per thread, two blocks per CU
    Wb = (int64_t)j.cfg.LPR * j.cfg.V;
    dcfg = PassCfg{8, 8, (int)(Wb / 8), 8, 2, true};
    delta = K <= 1024 && pass_kernel_delta(dcfg, kPassStepDelta) != nullptr;
    nb_d = (int)std::max<int64_t>(
        1, std::min<int64_t>((d + Wb - 1) / Wb,
                             (int64_t)c->num_cu * pass_blocks_per_cu(dcfg, kPassStepDelta)));
  }
  const int64_t slab_rows = std::max(sp.nb[0], nb_d);
  c->delta_info[0] = c->delta_info[1] = 0;
  c->delta_info[2] = GM_DELTA_OFF;
  Workspace w;
  int rc = ensure_ws(c, K, d, std::max(nb, nb_d), &w, 0, 0, delta);
  if (rc) return rc;
  if (delta) {
    bool have = ensure_shadow(c, sizeof(uint16_t) * (size_t)((d + Wb - 1) / Wb) * (size_t)(K * Wb));
    if (j.tr.collective) {
      // a rank without its buffer turns the path off on every rank: the kinds of pass, and with
      // them what the all-reduced sums mean, must be the same everywhere
      const double mine = have ? 0.0 : 1.0;
      double all = 0.0;
      HIPCHK(hipMemcpyAsync(w.sums, &mine, sizeof(double), hipMemcpyHostToDevice, s));
      rc = allreduce(c, w.sums, 1, s);
      if (rc) return rc;
      HIPCHK(hipMemcpyAsync(&all, w.sums, sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      have = all == 0.0;
    }
    c->delta_info[2] = have ? GM_DELTA_ARMED : GM_DELTA_NO_SHADOW;
    delta = have;
  }
  rc = ensure_host(c, kHostNoiseOff + sizeof(float) * (2 * K + d_total + 1) + 256);
  if (rc) return rc;
  KState* hst = host_state(c);
  KState* hslot = host_lagged(c);
  HIPCHK(hipMemsetAsync(w.st, 0, sizeof(KState), s));

  // (the kernels read a bf16 tile's elements behind the same pointer)
  sp.a.X = static_cast<const float*>(j.X);
  sp.a.K = K; sp.a.d = d; sp.a.ldx = j.ldx;
  sp.a.coef = w.coef; sp.a.st = w.st; sp.a.slab = w.slab;
  sp.a.noise = noise_kind; sp.a.hnoise = w.hnoise; sp.a.seed = j.air.seed;
  sp.a.col_off = j.tr.col_off;
  sp.a.panel_stride = j.panels ? j.ldx : 0;
  sp.problems = 1;
  sp.sums = w.sums;
  sp.pair = !j.panels;
  sp.oma = &j.oma;

  KspaceArgs ka = kspace_args(K, d_total, kmode, j.tol, j.eps, j.air);
  ka.tau = j.tau;
  ka.noise_src = host_noise ? 1 : 0;
  ka.sums = w.sums;
  ka.r = w.r;
  ka.h_re = w.h_re;
  ka.h_im = w.h_im;
  ka.n_last = w.hnoise + d;
  ka.coef = w.coef;
  ka.st = w.st;
  ka.delta = !delta ? 0 : delta_knob() == 1 ? 2 : 1;   // 2: the shadow is written in STEP 1
  ka.cb = w.cb;
  ka.Db = w.Db;
  ka.theta = delta ? delta_theta(j.cfg) : 0.0;   // (the two-pass loop has no tile: cfg is unset)
  const size_t timing_first = c->ev_used.size();

  // STEP t >= 1 of an armed loop: the exact pass and the correction pass are both queued, the
  // K-space step of t - 1 has chosen one and the other exits at once; each runs on its own grid,
  // writes slab rows of K + 3 sums and zeroes the rows only the other's larger grid would fill.
  auto delta_pair = [&](int64_t t) -> int {
    PassArgs a = sp.a;
    a.g_old = w.g[(t - 1) & 1];
    a.g_new = w.g[t & 1];
    a.slab_stride = K + 3;
    a.iter = t;
    a.shadow = c->shadow;
    a.shadow_stride = K * Wb;
    a.gbase = w.gbase;
    a.slab_rows = slab_rows;
    PassArgs b = a;
    b.X = reinterpret_cast<const float*>(c->shadow);
    b.ldx = b.panel_stride = K * Wb;
    const PassArgs* args[2] = {&a, &b};
    for (int kind = 0; kind < 2; ++kind) {
      hipEvent_t e0, e1;
      int rc2 = record_pass_begin(c, s, &e0, &e1);
      if (rc2) return rc2;
      HIPCHK(launch_pass(kind ? dcfg : j.cfg, kind ? kPassStepDelta : kPassStepExactD,
                         kind ? nb_d : sp.nb[0], *args[kind], s));
      rc2 = record_pass_end(c, s, e0, e1);
      if (rc2) return rc2;
    }
    HIPCHK(launch_slab_reduce(w.slab, (int)slab_rows, K + 3, w.sums, w.st, s));
    return allreduce(c, w.sums, K + 3, s);
  };

  auto poll = [&](KState* dst) -> int {
    HIPCHK(hipMemcpyAsync(dst, w.st, sizeof(KState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return GM_OK;
  };

  // Pass over X: INIT (t = -1) or STEP t; leaves the reduced partials in w.sums.
  auto do_pass = [&](int64_t t) -> int {
    if (delta && t >= 1) return delta_pair(t);
    const int rc2 = t <= 0 ? stream_pass(sp, t, j.guess0, 0, t < 0 ? nullptr : w.g[0])
                           : stream_pass(sp, t, w.g[(t - 1) & 1], 0, w.g[t & 1]);
    return rc2 ? rc2 : allreduce(c, w.sums, t < 0 ? 2 * K + 2 : K + 2, s);
  };

  // Initial distances (and ||x_k||^2, ||g0||^2), then iteration-0 coefficients.
  rc = do_pass(-1);
  if (rc) return rc;
  ka.t = -1;
  ka.do_check = 0;
  if (host_noise) { rc = upload_draws(c, j, w, 0); if (rc) return rc; }
  ka.do_coef = 1;
  HIPCHK(launch_kspace(ka, s));

  int check_every = j.check_every;
  if (check_every <= 0) check_every = (K * d_total >= (int64_t)1 << 24) ? 1 : 16;   // global
  if (host_noise) check_every = 1;
  // Polling every iteration (large passes): read iteration t-1's state while
  // iteration t is already queued, so the device never waits for the host.  If
  // t-1 stopped the loop, iteration t's launches see `done` and exit at once.
  static const bool no_lag = getenv("GMAGG_NO_LAG") != nullptr;   // A/B switch
  const bool lagged = check_every == 1 && !host_noise && !no_lag;
  if (lagged)
    for (auto& e : c->poll_ev)
      if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  int64_t pending = -1;   // iteration whose KState copy is in flight (lagged)

  int64_t t = 0, enqueued = 0;
  const KState* final_st = nullptr;   // set when a lagged poll already saw the stop
  for (; t < j.maxiter; ++t) {
    rc = do_pass(t);
    if (rc) return rc;
    enqueued = t + 1;
    const bool last = t + 1 == j.maxiter;
    ka.t = t;
    if (host_noise) {
      // tol test first; draw the next iteration only if the loop goes on (M:145-159)
      ka.do_check = 1;
      ka.do_coef = 0;
      HIPCHK(launch_kspace(ka, s));
      rc = poll(hst);
      if (rc) return rc;
      if (hst->done || last) break;
      rc = upload_draws(c, j, w, t + 1);
      if (rc) return rc;
      ka.do_check = 0;
      ka.do_coef = 1;
      HIPCHK(launch_kspace(ka, s));
      continue;
    }
    ka.do_check = 1;
    ka.do_coef = last ? 0 : 1;
    // lagged poll: the K-space step itself leaves its KState in the host-mapped slot
    ka.mirror = lagged && !last ? &hslot[t & 1] : nullptr;
    HIPCHK(launch_kspace(ka, s));
    ka.mirror = nullptr;
    if (lagged && !last) {
      HIPCHK(hipEventRecord(c->poll_ev[t & 1], s));
      if (pending >= 0) {
        HIPCHK(hipEventSynchronize(c->poll_ev[pending & 1]));
        if (hslot[pending & 1].done) {
          final_st = &hslot[pending & 1];
          break;
        }
      }
      pending = t;
      continue;
    }
    if (last || (t + 1) % check_every == 0) {
      rc = poll(hst);
      if (rc) return rc;
      if (hst->done) break;
    }
  }
  // The state the lagged poll saw is final (launches after the stop are no-ops and
  // leave it alone), so no second copy + sync: the host returns while the device
  // drains the queued no-op iteration, and the next call's work queues behind it.
  if (!final_st) {
    rc = poll(hst);
    if (rc) return rc;
    final_st = hst;
  }
  gm_result r = result_from(*final_st, j.algo);
  r.guard = j.guard_rejected ? GM_GUARD_REJECTED : GM_GUARD_NONE;
  if (r.iters < 1) return fail(GM_ERR_HIP, "Weiszfeld loop recorded no iteration");
  // passes queued after the stop (lagged poll) exited at once: not timed as passes
  if (!delta) {
    for (int64_t k = r.iters; k < enqueued; ++k) drop_last_timing(c);
  } else {
    // one record for STEP 0, then (exact, correction) per iteration: keep the kind that ran
    const uint32_t mask = final_st->kind_mask;
    std::vector<char> drop(1 + 2 * (size_t)std::max<int64_t>(0, enqueued - 1), 0);
    for (int64_t k = 1; k < enqueued; ++k) {
      const bool ran = k < r.iters;
      const bool corr = k < kDeltaMaxIter && ((mask >> k) & 1u) != 0;
      drop[1 + 2 * (k - 1)] = !ran || corr;
      drop[2 + 2 * (k - 1)] = !ran || !corr;
    }
    drop_timings(c, timing_first, drop);
    c->delta_info[0] = __builtin_popcount(mask);
    c->delta_info[1] = mask;
  }
  HIPCHK(hipMemcpyAsync(j.out, w.g[(r.iters - 1) & 1], sizeof(float) * d, hipMemcpyDeviceToDevice,
                        s));
  if (res) *res = r;
  if (final_state) *final_state = *final_st;
  return GM_OK;
}

// One validated gm_weiszfeld_f32 call and what the selection has decided so far.
struct Call {
  gm_ctx* c;
  const float* X;
  // The operand, traits and pending pre-noise every path reads, and the streaming loop's job
  // if the others decline; j.algo is o->algo, narrowed as paths decline
  StreamJob j;
  const gm_opts* o;
  gm_result* res;
  bool res_ok;           // the call's one turn of resident_allowed
};

// The Gram path on q's X (after the pending pre-noise); a result the guard refuses, or an
// f16 overflow on panels, declines with guard_rejected set.
int try_gram(Call& q, int64_t ldx, const PassCfg& cfg, bool split, bool guarded,
             int64_t pstride = 0) {
  bool rejected = false;
  int rc = q.j.oma.apply();
  if (rc) return rc;
  rc = run_gram(q.c, q.X, q.j.K, q.j.d, ldx, q.j.guess0, q.j.out, q.o, q.res, cfg, q.j.s, split,
                guarded, &rejected, pstride);
  if (rc || !rejected) return rc;
  q.j.guard_rejected = true;
  return kDeclined;
}

// The panel layout's streaming tile: pick_cfg's panel tile for K, whose chunk width is the
// panel width W (light_cfg's wider INIT tile is not used).
bool panel_cfg(int64_t K, int64_t W, PassCfg* cfg) {
  return W != 0 && pick_cfg(K, 4, W, cfg, true) && cfg->LPR * cfg->V == W;
}

// What the streaming tile asks of a panel layout [ceil(d/W)][K][W] of `elem`-byte elements:
// panels at least K*W elements apart, 16-byte aligned (bf16: the panel stride a multiple of
// 8 elements too), and 32-bit byte offsets within a panel.
int check_panels(const char* who, const void* X, int64_t K, int64_t W, int64_t ldx, int elem) {
  if (ldx < K * W || (reinterpret_cast<uintptr_t>(X) & 15) || (elem == 2 && ldx % 8) ||
      K * W * elem > 0x7fffffff)
    return fail(GM_ERR_INVALID, "%s: panel layout: need panel stride >= K*W (%lld)%s, 16-byte "
                "aligned X, K*W*%d < 2^31 (ldx=%lld)", who, (long long)(K * W),
                elem == 2 ? " and a multiple of 8" : "", elem, (long long)ldx);
  return GM_OK;
}

// The fp32 panel tile of a call, and whether its X is laid out for it.
int f32_panel_tile(const char* who, const float* X, int64_t K, int64_t ldx, PassCfg* cfg) {
  const int64_t W = gm_panel_width(K);
  if (!panel_cfg(K, W, cfg))
    return fail(GM_ERR_UNSUPPORTED, "%s: panel layout: no streaming tile of width %lld for "
                "K=%lld", who, (long long)W, (long long)K);
  return check_panels(who, X, K, W, ldx, 4);
}

// Panels [ceil(d/W)][K][W]: the guarded Gram, the one-XCD resident kernel, the batched
// resident kernel with P = 1; kDeclined leaves the streaming pass on *cfg.
int select_panels(Call& q, PassCfg* cfg) {
  gm_ctx* c = q.c;
  const gm_opts* o = q.o;
  const int64_t K = q.j.K, d = q.j.d, ldx = q.j.ldx;
  const int64_t W = gm_panel_width(K);
  const int rcp = f32_panel_tile("gm_weiszfeld_f32", q.X, K, ldx, cfg);
  if (rcp) return rcp;
  // gm2 at K <= 256: the scaled-f16 Gram reads panels too (AUTO on large d, as
  // for rows, guarded; explicit algo="gram" guarded likewise); streaming otherwise
  const bool gram_ok = o->mode == GM_MODE_IDEAL && gram_kt(K) > 0 && W % 64 == 0 &&
                       (W & (W - 1)) == 0;
  if ((q.j.algo == GM_ALGO_AUTO && gram_ok && q.j.tr.d_total >= (int64_t)1 << 18) ||
      (q.j.algo == GM_ALGO_GRAM && gram_ok)) {
    static const bool unguarded = getenv("GMAGG_GRAM_UNGUARDED") != nullptr;
    const int rc0 = try_gram(q, W, *cfg, true, q.j.algo == GM_ALGO_AUTO || !unguarded, ldx);
    if (rc0 != kDeclined) return rc0;
    q.j.algo = GM_ALGO_STREAM;
  }
  // One problem that fits on chip: the single-problem resident kernel (C2's, reading the
  // panels with its rows tile: V = 2 columns per lane, within one panel) when its grid
  // fits one XCD (the L2-kept exchange, §3.3: C2's shape 4.3 ms there against 6.7 ms on
  // the batched kernel's 4 blocks), else the batched kernel with P = 1 (K <= 52; gm at
  // K <= 50; the fused pre-noise included).  Either reads the panels once for all
  // iterations.
  auto wants_resident = [&] {
    return (q.j.algo == GM_ALGO_AUTO || q.j.algo == GM_ALGO_RESIDENT) && !q.j.tr.collective;
  };
  if (wants_resident() && !q.j.tr.host_noise && K <= 64 && q.res_ok) {
    PassCfg rcfg{};
    int cpb = 0, nbr = 0;
    if (pick_cfg(K, 2, W, &rcfg) && W % rcfg.V == 0 && (resident_tile(&rcfg, K), true) &&
        resident_plan(rcfg, (d + rcfg.LPR * rcfg.V - 1) / (rcfg.LPR * rcfg.V), c->num_cu, &cpb,
                      &nbr) &&
        res_xcd_stride(nbr, c->num_cu) == 8) {
      bool timed_out = false;
      int rco = q.j.oma.apply();
      if (rco) return rco;
      const int rc0 = run_resident(c, q.X, K, d, K * W, q.j.guess0, q.j.out, o, q.res, rcfg, cpb,
                                   nbr, q.j.s, &timed_out, ldx, wshift_of(W));
      if (rc0 || !timed_out) return rc0;
      q.j.algo = GM_ALGO_STREAM;   // the X noised above: stream (no second pre-noise)
    }
  }
  if (wants_resident()) {
    const int rc0 = run_resident_batched(c, q.X, 1, K, d, ldx, (d + W - 1) / W * ldx, true, W,
                                         q.j.guess0, d, q.j.out, d, o, q.res, q.j.s, q.res_ok);
    if (rc0 != kDeclined) return rc0;
  }
  if (q.j.algo == GM_ALGO_AUTO) q.j.algo = GM_ALGO_STREAM;
  if (q.j.algo != GM_ALGO_STREAM)
    return fail(GM_ERR_UNSUPPORTED, "panel layout: streaming, (gm2, K <= 256) Gram or (K <= 52 "
                "gm2 / K <= 50 gm, unsharded) resident only (algo %d)", q.j.algo);
  return kDeclined;
}

// AUTO: Gram-space (split bf16) for gm2 at K <= 256 on large d, kept if its
// accuracy guard passes (run_gram); streaming otherwise.  X is read twice
// instead of n+1 times (profiles/history/r01_cmp_algos.txt, r02_gram_split.txt).
// Sharded: the choice is made on d_total (every rank the same); each rank's
// shard must then meet the kernel's local needs, which shard_range-aligned,
// contiguous shards of a d_total % 4 == 0 update always do.
int rows_gram_auto(Call& q, int V) {
  const int64_t K = q.j.K, ldx = q.j.ldx, d_total = q.j.tr.d_total;
  PassCfg cfg{};
  const bool local_ok = gram_kt(K) > 0 && V == 4 && ldx < ((int64_t)1 << 26) &&
                        pick_cfg(K, V, ldx, &cfg);
  const bool take = q.j.algo == GM_ALGO_AUTO && q.o->mode == GM_MODE_IDEAL && gram_kt(K) > 0 &&
                    d_total >= (int64_t)1 << 18 && (q.j.tr.sharded ? d_total % 4 == 0 : local_ok);
  if (!take) return kDeclined;
  if (!local_ok)
    return fail(GM_ERR_INVALID, "sharded gm2 (AUTO -> Gram, d_total=%lld): this rank's shard "
                "must be 16-byte aligned with d_local %% 4 == 0 and ldx %% 4 == 0 like every "
                "other rank's (use sharded.shard_range + contiguous shards)",
                (long long)d_total);
  return try_gram(q, ldx, cfg, true, true);
}

// Small problems: the register-resident single launch when every chunk fits one
// co-resident block (unsharded, Philox or no noise).
int rows_resident(Call& q, int V) {
  gm_ctx* c = q.c;
  PassCfg cfg{};
  if (!((q.j.algo == GM_ALGO_AUTO || q.j.algo == GM_ALGO_RESIDENT) && !q.j.tr.host_noise &&
        !q.j.tr.collective && pick_cfg(q.j.K, V, q.j.ldx, &cfg)))
    return kDeclined;
  resident_tile(&cfg, q.j.K);
  const int J = cfg.LPR * cfg.V;
  const int64_t nch = (q.j.d + J - 1) / J;
  int cpb = 0, nbr = 0;
  if (!(q.res_ok && resident_plan(cfg, nch, c->num_cu, &cpb, &nbr))) return kDeclined;
  bool timed_out = false;
  int rco = q.j.oma.apply();
  if (rco) return rco;
  const int rc0 = run_resident(c, q.X, q.j.K, q.j.d, q.j.ldx, q.j.guess0, q.j.out, q.o, q.res, cfg,
                               cpb, nbr, q.j.s, &timed_out);
  if (rc0 || !timed_out) return rc0;
  // barrier timeout (e.g. a time-sliced GPU): the same problem, same draw keys,
  // on the launch-per-pass streaming path
  if (q.j.algo == GM_ALGO_RESIDENT) q.j.algo = GM_ALGO_AUTO;
  return kDeclined;
}

// Row-major AirComp gm over many passes (the reference's `gm`: 1000 iterations, never
// meeting tol; M:131-160) on a large client matrix: pack the panel layout once into a
// context-owned buffer (one read + one write of X) and stream every pass from it.  Rows
// stream at 79-80 % of HBM against 85-87 % on panels (C3 STEP 6.87-6.99 vs 6.35-6.47 ms),
// so the copy pays for itself after ~35 passes.  Results equal the row-major passes' bit
// for bit where both run the same tile (K outside 32 < K <= 64 and 128 < K <= 256, V = 4).
// If the buffer cannot be allocated the rows are streamed (ensure_stage).
// d-sharded calls too: the layout changes no collective (one all-reduce per pass either
// way), so a rank may decide it from its own shard.
int rows_staged(Call& q) {
  gm_ctx* c = q.c;
  const gm_opts* o = q.o;
  const int64_t K = q.j.K, d = q.j.d;
  if (!(q.j.algo == GM_ALGO_AUTO && aircomp_noise(o) && !q.j.tr.host_noise &&
        o->maxiter >= 64 && K * d >= ((int64_t)1 << 24)))
    return kDeclined;
  const int64_t W = gm_panel_width(K);
  PassCfg pcfg{};
  if (!stage_enabled() || W <= 0 || K * W * 4 > 0x7fffffff || !panel_cfg(K, W, &pcfg) ||
      !ensure_stage(c, sizeof(float) * (size_t)((d + W - 1) / W) * (size_t)(K * W)))
    return kDeclined;
  HIPCHK(launch_rows_to_panels(q.X, K, d, q.j.ldx, c->stage, W, K * W, q.j.s));
  // (pre_oma is gm2-only, so none is pending on this AirComp call)
  StreamJob staged = q.j;
  staged.X = c->stage;
  staged.ldx = K * W;
  staged.panels = true;
  staged.cfg = pcfg;
  staged.algo = GM_ALGO_STREAM;
  return run_stream(c, staged, q.res);
}

int rows_gram_explicit(Call& q, int V, PassCfg* cfg) {
  const gm_opts* o = q.o;
  const int64_t K = q.j.K, d = q.j.d, ldx = q.j.ldx;
  if (o->mode != GM_MODE_IDEAL)
    return fail(GM_ERR_UNSUPPORTED, "Gram variant is gm2 only (AirComp noise leaves span(X))");
  if (gram_kt(K) == 0 || V != 4 || !pick_cfg(K, V, ldx, cfg))
    return fail(GM_ERR_UNSUPPORTED, "Gram variant needs K <= 256, d and ldx multiples of 4, "
                "16-byte aligned X (K=%lld d=%lld ldx=%lld)", (long long)K, (long long)d,
                (long long)ldx);
  // the split kernel addresses a 16-row group with 32-bit lane offsets
  const bool split = q.j.algo == GM_ALGO_GRAM && ldx < ((int64_t)1 << 26);
  // Explicit Gram runs the same a-posteriori guard as AUTO: a result the guard
  // refuses is never returned; the call then runs the streaming path and
  // reports guard = GM_GUARD_REJECTED.  (GMAGG_GRAM_UNGUARDED=1: A/B timing of
  // the bare Gram path, whose closing pass is the lighter sum-only tile.)
  static const bool unguarded = getenv("GMAGG_GRAM_UNGUARDED") != nullptr;
  const int rc0 = try_gram(q, ldx, *cfg, split, !unguarded);
  if (rc0 == kDeclined) q.j.algo = GM_ALGO_STREAM;   // pick_cfg(K, V, ldx) succeeded above
  return rc0;
}

// Row-major [K][ldx]: try each path in turn and return unless it declined; kDeclined
// leaves q.j.algo = GM_ALGO_STREAM on *cfg, or GM_ALGO_TWOPASS (K > 2048).
int select_rows(Call& q, PassCfg* cfg) {
  const int V = pick_vec(q.X, q.j.d, q.j.ldx);
  int rc = rows_gram_auto(q, V);
  if (rc != kDeclined) return rc;
  rc = rows_resident(q, V);
  if (rc != kDeclined) return rc;
  if (q.j.algo == GM_ALGO_RESIDENT)
    return fail(GM_ERR_UNSUPPORTED, "resident kernel: problem too large, sharded or host noise");
  rc = rows_staged(q);
  if (rc != kDeclined) return rc;
  if (q.j.algo == GM_ALGO_AUTO || q.j.algo == GM_ALGO_STREAM) {
    if (pick_cfg(q.j.K, V, q.j.ldx, cfg)) q.j.algo = GM_ALGO_STREAM;
    else if (q.j.algo == GM_ALGO_STREAM)
      return fail(GM_ERR_UNSUPPORTED, "streaming pass supports K <= 2048 (K=%lld)",
                  (long long)q.j.K);
    else q.j.algo = GM_ALGO_TWOPASS;
  }
  if (q.j.algo == GM_ALGO_GRAM || q.j.algo == GM_ALGO_GRAM_F32) {
    rc = rows_gram_explicit(q, V, cfg);
    if (rc != kDeclined) return rc;
  }
  if (q.j.algo != GM_ALGO_STREAM && q.j.algo != GM_ALGO_TWOPASS)
    return fail(GM_ERR_INVALID, "unknown algo %d", q.o->algo);
  return kDeclined;
}

// ---- the entry points' prologue ----------------------------------------------------------

// What the four entry points check alike (gm_opts and gm_cclip_opts name the layout and the
// iteration bound alike), then the job's operand, loop controls, traits and stream.
template <class Opts>
int begin_call(const char* who, gm_ctx* c, const void* X, int64_t K, int64_t d, int64_t ldx,
               const float* guess0, float* out, const Opts* o, void* stream, StreamJob* j) {
  if (!c || !o || !out || !guess0 || !X) return fail(GM_ERR_INVALID, "%s: NULL argument", who);
  if (o->layout != GM_LAYOUT_ROWS && o->layout != GM_LAYOUT_PANELS)
    return fail(GM_ERR_INVALID, "%s: unknown layout %d", who, o->layout);
  if (K < 1 || d < 1 || (ldx < d && o->layout == GM_LAYOUT_ROWS))
    return fail(GM_ERR_INVALID, "%s: bad shape K=%lld d=%lld ldx=%lld", who, (long long)K,
                (long long)d, (long long)ldx);
  if (o->maxiter < 0) return fail(GM_ERR_INVALID, "%s: maxiter < 0", who);
  *j = StreamJob{};
  j->X = X; j->K = K; j->d = d; j->ldx = ldx;
  j->panels = o->layout == GM_LAYOUT_PANELS;
  j->algo = GM_ALGO_STREAM;
  j->guess0 = guess0;
  j->out = out;
  j->maxiter = o->maxiter;
  j->tol = o->tol;
  j->check_every = o->check_every;
  j->tr = traits_of(c, d);
  j->s = reinterpret_cast<hipStream_t>(stream);
  return GM_OK;
}

// gm2 / gm: the rule and the AirComp channel from the options.
int gm_rule(const char* who, const gm_opts* o, StreamJob* j) {
  if (o->mode != GM_MODE_IDEAL && o->mode != GM_MODE_AIRCOMP)
    return fail(GM_ERR_INVALID, "%s: unknown mode %d", who, o->mode);
  if (o->mode == GM_MODE_AIRCOMP && o->noise_source == GM_NOISE_HOST && !o->noise_cb)
    return fail(GM_ERR_INVALID, "%s: GM_NOISE_HOST needs noise_cb", who);
  j->rule = o->mode == GM_MODE_AIRCOMP ? Rule::Gm : Rule::Gm2;
  j->eps = o->eps;
  j->air = air_noise(o);
  j->noise_cb = o->noise_cb;
  j->noise_user = o->noise_user;
  j->tr.host_noise = o->mode == GM_MODE_AIRCOMP && o->noise_source == GM_NOISE_HOST;
  return GM_OK;
}

// Centered clipping: the K-space step's third rule (no AirComp draws, INIT without the row
// norms).
int cclip_rule(const char* who, const gm_cclip_opts* o, StreamJob* j) {
  if (!(o->tau > 0.0))   // NaN fails too
    return fail(GM_ERR_INVALID, "%s: tau must be > 0 (+inf allowed; got %g)", who, o->tau);
  j->rule = Rule::Cclip;
  j->tau = o->tau;
  return GM_OK;
}

// bf16 client updates run on one device's streaming pass only.
int bf16_refuse_collective(const gm_ctx* c, const char* who) {
  if (c->d_total > 0 || c->comm || c->ar_fn)
    return fail(GM_ERR_UNSUPPORTED, "%s: sharded / collective contexts are not supported", who);
  return GM_OK;
}

// The bf16 streaming tile of a job, and whether the kernel can read its X in place.
int bf16_tile(const char* who, StreamJob* j) {
  const int64_t K = j->K, d = j->d, ldx = j->ldx;
  if (!pick_cfg(K, 8, ldx, &j->cfg, j->panels, true))
    return fail(GM_ERR_UNSUPPORTED, "%s: no streaming tile for K=%lld (K <= 2048) at ldx=%lld",
                who, (long long)K, (long long)ldx);
  if (j->panels) return check_panels(who, j->X, K, (int64_t)j->cfg.LPR * j->cfg.V, ldx, 2);
  if ((reinterpret_cast<uintptr_t>(j->X) & 15) || ldx % 8 || d % 8)
    return fail(GM_ERR_UNSUPPORTED, "%s: row-major bf16 needs 16-byte aligned X with d and ldx "
                "multiples of 8 (d=%lld ldx=%lld); pack panels (gm_rows_to_panels_bf16)", who,
                (long long)d, (long long)ldx);
  return GM_OK;
}

// maxiter == 0: the loop body never runs and the guess is the result (after the pre-noise,
// which the reference applies whatever the aggregator then does).
template <class Res>
int no_iteration(StreamJob& j, Res* res) {
  const int rc = j.oma.apply();
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(j.out, j.guess0, sizeof(float) * j.d, hipMemcpyDeviceToDevice, j.s));
  if (res) {
    *res = Res{};
    res->last_movement = NAN;
  }
  return GM_OK;
}

// The clipping loop on a job whose tile is chosen.
int run_cclip(gm_ctx* c, StreamJob& j, gm_cclip_result* res) {
  gm_result r{};
  KState fin{};
  const int rc = run_stream(c, j, &r, &fin);
  if (rc || !res) return rc;
  res->iters = r.iters;
  res->last_movement = r.last_movement;
  res->converged = r.converged;
  res->clipped = fin.clipped;
  return GM_OK;
}

}  // namespace

// Centered clipping on fp32 client updates: run_stream's loop with the clipping rule in the
// K-space step, on the fused pass (K <= 2048; rows or panels) or the two-pass kernels
// (row-major, any K).  d-sharded contexts as gm2: the coefficients, a and the stop decision
// come from the all-reduced sums, the same on every rank.
extern "C" int gm_cclip_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                            const float* guess0, float* out, const gm_cclip_opts* o,
                            gm_cclip_result* res, void* stream) {
  static const char* const who = "gm_cclip_f32";
  StreamJob j;
  int rc = begin_call(who, c, X, K, d, ldx, guess0, out, o, stream, &j);
  if (!rc) rc = cclip_rule(who, o, &j);
  if (rc) return rc;
  WsOrder order(c, j.s);
  HIPCHK(order.err);
  if (j.maxiter == 0) return no_iteration(j, res);
  if (j.panels) {
    rc = f32_panel_tile(who, X, K, ldx, &j.cfg);
    if (rc) return rc;
  } else if (!pick_cfg(K, pick_vec(X, d, ldx), ldx, &j.cfg)) {
    j.algo = GM_ALGO_TWOPASS;   // K > 2048 (or rows too far apart for the tile's lane offsets)
  }
  return run_cclip(c, j, res);
}

// Centered clipping on bf16 client updates: the bf16 instantiation of the fused pass, under
// gm_weiszfeld_bf16's rules (one device, K <= 2048, rows readable in place or panels).
extern "C" int gm_cclip_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                             const float* guess0, float* out, const gm_cclip_opts* o,
                             gm_cclip_result* res, void* stream) {
  static const char* const who = "gm_cclip_bf16";
  StreamJob j;
  int rc = begin_call(who, c, X, K, d, ldx, guess0, out, o, stream, &j);
  if (!rc) rc = cclip_rule(who, o, &j);
  if (!rc) rc = bf16_refuse_collective(c, who);
  if (rc) return rc;
  WsOrder order(c, j.s);
  HIPCHK(order.err);
  if (j.maxiter == 0) return no_iteration(j, res);
  rc = bf16_tile(who, &j);
  if (rc) return rc;
  return run_cclip(c, j, res);
}

extern "C" int gm_weiszfeld_f32(gm_ctx* c, const float* X, int64_t K, int64_t d, int64_t ldx,
                                const float* guess0, float* out, const gm_opts* o,
                                gm_result* res, void* stream) {
  static const char* const who = "gm_weiszfeld_f32";
  Call q{c, X};
  StreamJob& j = q.j;
  int rc = begin_call(who, c, X, K, d, ldx, guess0, out, o, stream, &j);
  if (!rc) rc = gm_rule(who, o, &j);
  if (rc) return rc;
  if (o->pre_oma && (o->mode != GM_MODE_IDEAL || !(o->pre_oma_var >= 0)))
    return fail(GM_ERR_INVALID, "pre_oma: gm2 only (the reference applies OMA before non-gm "
                "aggregators, M:351), noise variance >= 0");
  WsOrder order(c, j.s);
  HIPCHK(order.err);
  q.o = o;
  q.res = res;
  j.algo = o->algo;
  j.oma = PreOma{o->pre_oma != 0, const_cast<float*>(X), K, d, ldx, j.tr.d_total, j.tr.col_off,
                 j.panels, pre_oma_sd(o), o->pre_oma_seed, j.s};
  if (j.maxiter == 0) return no_iteration(j, res);
  q.res_ok = o->algo == GM_ALGO_STREAM || resident_allowed(c);
  // Every path that runs returns from the selection; what it declines is left to the
  // launch-per-pass loop on the tile in j.cfg (panels keep their own: it sets the chunk
  // width the panel layout was built for).
  rc = j.panels ? select_panels(q, &j.cfg) : select_rows(q, &j.cfg);
  if (rc != kDeclined) return rc;
  return run_stream(c, j, res);
}

// bf16 client updates: the streaming loop only, on the bf16 instantiation of the fused pass
// (stream_pass_bf16.hip).  The element type travels in the tile (PassCfg.B16); the loop,
// the K-space step, the draws and the timing are run_stream's.
extern "C" int gm_weiszfeld_bf16(gm_ctx* c, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                                 const float* guess0, float* out, const gm_opts* o,
                                 gm_result* res, void* stream) {
  static const char* const who = "gm_weiszfeld_bf16";
  StreamJob j;
  int rc = begin_call(who, c, X, K, d, ldx, guess0, out, o, stream, &j);
  if (!rc) rc = gm_rule(who, o, &j);
  if (rc) return rc;
  if (o->algo != GM_ALGO_AUTO && o->algo != GM_ALGO_STREAM)
    return fail(GM_ERR_UNSUPPORTED, "%s: the streaming pass only (algo %d; the Gram, resident "
                "and two-pass paths read fp32)", who, o->algo);
  if (o->pre_oma)
    return fail(GM_ERR_UNSUPPORTED, "%s: pre_oma is not supported (the noised values would be "
                "rounded back to bf16)", who);
  rc = bf16_refuse_collective(c, who);
  if (rc) return rc;
  WsOrder order(c, j.s);
  HIPCHK(order.err);
  if (j.maxiter == 0) return no_iteration(j, res);
  rc = bf16_tile(who, &j);
  if (rc) return rc;
  return run_stream(c, j, res);
}

