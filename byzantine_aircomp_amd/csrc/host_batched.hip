// gm_weiszfeld_batched_f32 (include/gmagg.h): P independent problems per call (BASELINE
// C5).  The register-resident batched kernel where the problems fit on chip, else the
// streaming loop over all problems at once (blockIdx.y = problem).
#include "host_ctx.h"

using namespace gmh;

// Batched problems that fit on chip (resident_batched.hip, BASELINE C5): every problem's
// X is read once and held in VGPRs (+ LDS) for all its iterations, instead of once per
// pass.  Returns kDeclined when the shape is not eligible, or when the kernel timed out
// (blocks not co-resident) before touching X: the caller streams.  GMAGG_BATCH_RESIDENT=0
// turns it off (A/B).
int gmh::run_resident_batched(gm_ctx* c, const float* X, int64_t P, int64_t K, int64_t d,
                              int64_t ldx, int64_t ldp, bool panels, int64_t Wp,
                              const float* guess0, int64_t ldg, float* out, int64_t ldo,
                              const gm_opts* o, gm_result* results, hipStream_t s, bool res_ok) {
  static const bool on = env_int("GMAGG_BATCH_RESIDENT", 1) != 0;
  if (!on || c->d_total > 0) return kDeclined;
  if (o->mode == GM_MODE_AIRCOMP && o->noise_source != GM_NOISE_PHILOX) return kDeclined;
  if (!res_ok) return kDeclined;   // (resident_allowed, taken once by the caller)
  // float4 tile rows: 16-byte aligned problems, rows and panels
  if ((reinterpret_cast<uintptr_t>(X) & 15) || ldp % 4 || ldx % 4 || (panels && Wp % 4))
    return kDeclined;
  const int64_t pbytes = panels ? (d + Wp - 1) / Wp * ldx * 4 : K * ldx * 4;
  if (pbytes >= ((int64_t)1 << 31)) return kDeclined;
  RbPlan plan{};
  const int xcd = rb_xcd_major();
  if (!rb_plan(K, d, P, o->mode, c->num_cu, &plan, xcd == 2)) return kDeclined;

  const unsigned nblocks = (unsigned)(plan.ng * plan.nb);
  ResBArgs a{};
  auto lay = [&](char* base) {
    Carve cv{base};
    a.st = cv.take<KState>(P);
    a.flag = cv.take<unsigned>(4);
    a.gran = cv.take<unsigned long long>(rb_gran_words(K, plan));
    a.checkin = cv.take<unsigned long long>(nblocks + 1);
    return cv.off;
  };
  const size_t ws_bytes = lay(nullptr);
  int rc = grow_ws(c, ws_bytes);
  if (rc) return rc;
  lay(c->ws);
  rc = ensure_host(c, sizeof(KState) * P + 256);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(c->ws, 0, ws_bytes, s));   // states, the timeout word, every tag = 0

  a.X = X; a.P = P; a.K = K; a.d = d; a.ldx = ldx; a.x_ps = ldp;
  a.pstride = panels ? ldx : 0;
  a.wshift = panels ? wshift_of(Wp) : 0;
  a.prob_bytes = (int)pbytes;
  a.nb = plan.nb;
  a.guess0 = guess0; a.ldg = ldg; a.out = out; a.ldo = ldo;
  a.maxiter = o->maxiter; a.tol = (float)o->tol; a.eps = (float)o->eps;
  a.mode = o->mode; a.has_noise = aircomp_noise(o);
  a.P_max = o->P_max; a.noise_sd = noise_sd(o);
  a.seed = o->seed;
  a.pre_oma = o->pre_oma ? 1 : 0;
  a.oma_sd = pre_oma_sd(o);
  a.oma_seed = o->pre_oma_seed;
  a.need = checkin_need(nblocks);
  a.xcd_major = xcd != 0;
  // the hierarchical gather: sub-group granules L2-kept where the check-in confirms them
  a.hier = xcd != 0 && rb_hier_mode() == 1;
  a.local = xcd == 2 || a.hier != 0;
  a.lvl2 = a.gran + (size_t)plan.ng * 2 * plan.nb * (size_t)(2 * K + 2);
  hipEvent_t e0, e1;
  rc = record_pass_begin(c, s, &e0, &e1);
  if (rc) return rc;
  HIPCHK(launch_resident_batched(plan, a, res_coop_launch(), s));
  rc = record_pass_end(c, s, e0, e1);
  if (rc) return rc;
  KState* hst = host_state(c);
  unsigned* hflag = host_after_states<unsigned>(c, P);
  HIPCHK(hipMemcpyAsync(hst, a.st, sizeof(KState) * P, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hflag, a.flag, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  static const bool verbose = getenv("GMAGG_RES_VERBOSE") != nullptr;
  if (verbose)
    fprintf(stderr, "gmagg resident_batched: ng=%d nb=%d xcd=%d local_groups=%u timed_out=%u\n",
            plan.ng, plan.nb, xcd, hflag[1], hflag[0]);
  if (hflag[0]) {
    drop_last_timing(c);
    // The grid was not co-resident.  Failed at the check-in (hflag[2] == 0): no block
    // read or wrote X, the caller streams (the pre-noise fused into its INIT pass) and
    // the next calls skip the resident kernels for a while.  Timed out after the
    // check-in (a block descheduled for 2 s mid-call): with the fused pre-noise some
    // problems may already carry their noise, so that call cannot be streamed again.
    if (!hflag[2]) {
      c->res_skip = kResSkipAfterCheckinFail;
      return kDeclined;
    }
    if (o->pre_oma)
      return fail(GM_ERR_HIP, "batched resident kernel timed out after its check-in, with "
                  "the fused pre-noise begun (a block descheduled for 2 s?); X is partly noised");
    return kDeclined;
  }
  if (results)
    for (int64_t p = 0; p < P; ++p)
      results[p] = gm_result{hst[p].iters, hst[p].last_movement, hst[p].converged,
                             GM_ALGO_RESIDENT, GM_GUARD_NONE, 0,
                             a.hier == 1 ? GM_EXCHANGE_XCD_HIER
                             : hflag[1] == (unsigned)plan.ng ? GM_EXCHANGE_XCD_LOCAL
                                                             : GM_EXCHANGE_AGENT};
  return GM_OK;
}

namespace {

// One validated batched call, as the paths below see it (X / ldx / ldp / panels are the
// staged panel copy's when the rows were packed first).
struct BatchedCall {
  gm_ctx* c;
  const float* X;
  int64_t P, K, d, ldx, ldp;
  bool panels;
  int64_t Wp;   // panels: the panel width
  const float* guess0;
  int64_t ldg;
  float* out;
  int64_t ldo;
  const gm_opts* o;
  gm_result* results;
  hipStream_t s;
};

// The call's pre-noise (pre_oma: the reference's `--agg gm2 --var v`, M:351-352), for the
// paths that do not fuse it into the resident kernel.
PreOma pre_oma_of(const BatchedCall& q) {
  return PreOma{q.o->pre_oma != 0, const_cast<float*>(q.X), q.K, q.d, q.ldx, q.d, 0, q.panels,
                pre_oma_sd(q.o), q.o->pre_oma_seed, q.s, q.P, q.ldp};
}

// The streaming loop over all problems at once: one INIT pass, then per iteration one STEP
// pass + slab reduction + K-space step for every problem still active (the others exit at
// their `done` flag), the host polling the count of finished problems.
int run_stream_batched(const BatchedCall& q) {
  gm_ctx* c = q.c;
  const gm_opts* o = q.o;
  const int64_t P = q.P, K = q.K, d = q.d;
  hipStream_t s = q.s;
  PassCfg cfg{};
  int V = q.panels ? 4 : pick_vec(q.X, d, q.ldx);
  if (q.ldp % V) V = 1;
  if (!pick_cfg(K, V, q.ldx, &cfg, q.panels) || (q.panels && cfg.LPR * cfg.V != q.Wp))
    return fail(GM_ERR_UNSUPPORTED, "batched streaming pass supports K <= 2048");
  const int J = cfg.LPR * cfg.V;
  const int64_t nch = (d + J - 1) / J;
  // blocks per problem: the grid is OVERSUB rounds of co-resident blocks, so that the
  // iterations where only the slowest problems are still active (the others exit at
  // their `done` flag) still spread over the chip.  C5 on ProblemPanels: 8 rounds
  // 40.7-41.7k vs 2 rounds 39.7-39.9k problems/s (profiles/history/r2_c5_oversub.txt;
  // GMAGG_BATCH_OVERSUB: A/B)
  static const int oversub = env_pos("GMAGG_BATCH_OVERSUB", 8);
  const int64_t target = (int64_t)c->num_cu * pass_blocks_per_cu(cfg, 0) * oversub;
  const int nbp = (int)std::max<int64_t>(1, std::min<int64_t>(nch, (target + P - 1) / P));
  const int64_t S = 2 * K + 2;

  // workspace: per problem KState, sums, r, coef, slab[nbp][S], g[2][d]; + a done counter
  KState* st;
  int* cnt;
  double *sums, *rr, *slab;
  float *coef, *g[2];
  size_t zero_end = 0;
  auto lay = [&](char* base) {
    Carve cv{base};
    st = cv.take<KState>(P);
    cnt = cv.take<int>(4);
    zero_end = cv.off;   // KStates + counter
    sums = cv.take<double>(S * P);
    rr = cv.take<double>(K * P);
    coef = cv.take<float>(K * P);
    slab = cv.take<double>(S * nbp * P);
    g[0] = cv.take<float>(d * P);
    g[1] = cv.take<float>(d * P);
    return cv.off;
  };
  int rc = grow_ws(c, lay(nullptr));
  if (rc) return rc;
  lay(c->ws);
  rc = ensure_host(c, sizeof(KState) * P + 256);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(c->ws, 0, zero_end, s));

  KspaceArgs ka = kspace_args(K, d, o->mode, o->tol, o->eps, air_noise(o));
  ka.noise_src = 0;
  ka.sums = sums;
  ka.r = rr;
  ka.coef = coef;
  ka.st = st;
  ka.sums_ps = S;
  ka.n_done = cnt;

  PreOma oma = pre_oma_of(q);
  StreamPasses sp{c, s};
  sp.a.X = q.X; sp.a.K = K; sp.a.d = d; sp.a.ldx = q.ldx; sp.a.x_ps = q.ldp;
  sp.a.gnew_ps = d;
  sp.a.coef = coef; sp.a.st = st; sp.a.slab = slab;
  sp.a.noise = ka.has_noise ? 1 : 0; sp.a.seed = o->seed;
  sp.a.panel_stride = q.panels ? q.ldx : 0;
  sp.cfg[0] = sp.cfg[1] = cfg;
  sp.mode[0] = 0; sp.mode[1] = o->mode == GM_MODE_AIRCOMP ? 2 : 1;
  sp.nb[0] = sp.nb[1] = nbp;
  sp.problems = (int)P;
  sp.sums = sums; sp.sums_ps = S;
  sp.oma = &oma;
  auto do_pass = [&](int64_t t) -> int {
    if (t <= 0) return stream_pass(sp, t, q.guess0, q.ldg, t < 0 ? nullptr : g[0]);
    return stream_pass(sp, t, g[(t - 1) & 1], d, g[t & 1]);
  };
  int* hcnt = reinterpret_cast<int*>(host_state(c));   // (free until the final copy)
  auto poll_done = [&]() -> int {
    HIPCHK(hipMemcpyAsync(hcnt, cnt, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return *hcnt;
  };

  rc = do_pass(-1);
  if (rc) return rc;
  ka.t = -1;
  ka.do_check = 0;
  ka.do_coef = 1;
  HIPCHK(launch_kspace(ka, s, (int)P));
  static const int batch_check = env_pos("GMAGG_BATCH_CHECK", 16);
  int check_every = o->check_every > 0 ? o->check_every : batch_check;
  for (int64_t t = 0; t < o->maxiter; ++t) {
    rc = do_pass(t);
    if (rc) return rc;
    const bool last = t + 1 == o->maxiter;
    ka.t = t;
    ka.do_check = 1;
    ka.do_coef = last ? 0 : 1;
    HIPCHK(launch_kspace(ka, s, (int)P));
    if (!last && (t + 1) % check_every == 0) {
      const int nd = poll_done();
      if (nd < 0) return nd;
      if (nd >= P) break;
    }
  }
  HIPCHK(launch_batched_finalize(g[0], g[1], d, (int)P, st, q.out, q.ldo, s));
  KState* hst = host_state(c);
  HIPCHK(hipMemcpyAsync(hst, st, sizeof(KState) * P, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (q.results)
    for (int64_t p = 0; p < P; ++p)
      q.results[p] = gm_result{hst[p].iters, hst[p].last_movement, hst[p].converged,
                               GM_ALGO_STREAM, GM_GUARD_NONE, 0};
  return GM_OK;
}

// The paths of one validated call, in order: resident, the staged panel copy (which comes
// back here with the copy as X), maxiter == 0, streaming.  res_ok: the call's one turn of
// resident_allowed.
int batched_paths(const BatchedCall& q, bool res_ok) {
  gm_ctx* c = q.c;
  const gm_opts* o = q.o;
  const int64_t P = q.P, K = q.K, d = q.d;
  // Problems that fit on chip (K <= 52, d <= ~500k): the register-resident batched kernel
  // reads each problem's X once (resident_batched.hip); res_ok is set for AUTO or
  // GM_ALGO_RESIDENT only
  const int rcr = run_resident_batched(c, q.X, P, K, d, q.ldx, q.ldp, q.panels, q.Wp, q.guess0,
                                       q.ldg, q.out, q.ldo, o, q.results, q.s, res_ok);
  if (rcr != kDeclined) return rcr;
  if (o->algo == GM_ALGO_RESIDENT)
    return fail(GM_ERR_UNSUPPORTED, "batched resident kernel: K <= 52 (gm2) / K <= 50 (gm), "
                "d <= %lld, 16-byte aligned problems", (long long)c->num_cu * 2048);
  // Row-major AirComp problems over >= 64 passes: pack them once into the context's panel
  // buffer and stream every pass from it, as gm_weiszfeld_f32 does (C5 AirComp reading on
  // rows: every problem runs all 1000 iterations).
  if (!q.panels && o->mode == GM_MODE_AIRCOMP && o->maxiter >= 64 &&
      P * K * d >= ((int64_t)1 << 24)) {
    const int64_t W = gm_panel_width(K);
    if (stage_enabled() && W > 0 && K * W * 4 <= 0x7fffffff) {
      const int64_t pst = (d + W - 1) / W * K * W;   // problem stride (floats)
      if (ensure_stage(c, sizeof(float) * (size_t)(P * pst))) {
        for (int64_t p = 0; p < P; ++p)
          HIPCHK(launch_rows_to_panels(q.X + p * q.ldp, K, d, q.ldx, c->stage + p * pst, W, K * W,
                                       q.s));
        BatchedCall staged = q;
        staged.X = c->stage;
        staged.ldx = K * W;
        staged.ldp = pst;
        staged.panels = true;
        staged.Wp = W;
        // the copy is 16-byte aligned whatever X was, so the resident kernel gets its turn
        // on it, unless this call's own check-in has just failed
        return batched_paths(staged, res_ok && c->res_skip <= 0);
      }
    }
  }
  if (o->maxiter == 0) {
    const int rco = pre_oma_of(q).apply();
    if (rco) return rco;
    HIPCHK(hipMemcpy2DAsync(q.out, q.ldo * 4, q.guess0, q.ldg * 4, d * 4, P,
                            hipMemcpyDeviceToDevice, q.s));
    if (q.results)
      for (int64_t p = 0; p < P; ++p)
        q.results[p] = gm_result{0, NAN, 0, GM_ALGO_STREAM, GM_GUARD_NONE, 0};
    return GM_OK;
  }
  return run_stream_batched(q);
}

}  // namespace

extern "C" int gm_weiszfeld_batched_f32(gm_ctx* c, const float* X, int64_t P, int64_t K,
                                        int64_t d, int64_t ldx, int64_t ldp, const float* guess0,
                                        int64_t ldg, float* out, int64_t ldo, const gm_opts* o,
                                        gm_result* results, void* stream) {
  if (!c || !o || !X || !guess0 || !out)
    return fail(GM_ERR_INVALID, "gm_weiszfeld_batched_f32: NULL argument");
  // GM_LAYOUT_PANELS: problem p is [ceil(d/W)][K][W] at X + p*ldp, ldx = its panel stride
  const bool panels = o->layout == GM_LAYOUT_PANELS;
  if (o->layout != GM_LAYOUT_ROWS && !panels)
    return fail(GM_ERR_INVALID, "gm_weiszfeld_batched_f32: unknown layout %d", o->layout);
  const int64_t Wp = panels ? gm_panel_width(K) : 0;
  const int64_t rows_per_problem = panels ? (Wp > 0 ? (d + Wp - 1) / Wp : 0) : K;
  if (P < 1 || P > 65535 || K < 1 || d < 1 || ldx < (panels ? K * Wp : d) ||
      ldp < rows_per_problem * ldx || ldg < d || ldo < d || o->maxiter < 0 || (panels && Wp == 0))
    return fail(GM_ERR_INVALID, "gm_weiszfeld_batched_f32: bad shape P=%lld K=%lld d=%lld",
                (long long)P, (long long)K, (long long)d);
  if (panels && ((reinterpret_cast<uintptr_t>(X) & 15) || ldp % 4 || K * Wp * 4 > 0x7fffffff))
    return fail(GM_ERR_INVALID, "gm_weiszfeld_batched_f32 (panels): 16-byte aligned X and "
                "problem stride, K*W*4 < 2^31");
  if (o->mode == GM_MODE_AIRCOMP && o->noise_source != GM_NOISE_PHILOX)
    return fail(GM_ERR_UNSUPPORTED, "batched AirComp uses Philox noise only");
  if (c->d_total > 0) return fail(GM_ERR_UNSUPPORTED, "batched problems are not d-sharded");
  if (o->pre_oma && (o->mode != GM_MODE_IDEAL || !(o->pre_oma_var >= 0)))
    return fail(GM_ERR_INVALID, "pre_oma: gm2 only, noise variance >= 0");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WsOrder order(c, s);
  HIPCHK(order.err);
  const BatchedCall q{c, X, P, K, d, ldx, ldp, panels, Wp, guess0, ldg, out, ldo, o, results, s};
  // the turn of resident_allowed is taken only where a resident path is considered
  const bool wants_resident =
      o->maxiter > 0 && (o->algo == GM_ALGO_AUTO || o->algo == GM_ALGO_RESIDENT);
  return batched_paths(q, wants_resident && resident_allowed(c));
}
