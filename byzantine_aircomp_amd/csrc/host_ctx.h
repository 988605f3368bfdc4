// Host-only internals of the C-ABI layer, shared by api.hip (context API, thin wrappers,
// Krum), host_weiszfeld.hip (gm_weiszfeld_f32, gm_weiszfeld_bf16, gm_cclip_f32, gm_cclip_bf16)
// and host_batched.hip (gm_weiszfeld_batched_f32): the context, error reporting, workspace
// and pinned-buffer helpers, the all-reduce, pass timing, tile choices, the environment knobs
// and the one pass over X that both streaming loops run (stream_pass).
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gmagg.h"
#include "gmagg_internal.h"

struct gm_ctx {
  int device = 0;
  int num_cu = 256;
  int64_t d_total = -1;   // -1: unsharded
  int64_t d_offset = 0;
  gm_allreduce_cb ar_fn = nullptr;
  void* ar_user = nullptr;
  ncclComm_t comm = nullptr;
  char* ws = nullptr;
  size_t ws_bytes = 0;
  char* host = nullptr;   // pinned; what lives in it: "The pinned buffer" below
  size_t host_bytes = 0;
  bool timing = false;
  hipEvent_t poll_ev[2] = {nullptr, nullptr};   // lagged convergence polls
  std::vector<hipEvent_t> ev_free;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used;
  // Workspace ordering across streams: every call that touches ws / host records
  // ws_ev on its stream when it returns (work may still be queued: the lagged
  // poll returns before the no-op tail drains); a call on ANOTHER stream waits
  // for it before zeroing or overwriting the workspace.
  hipEvent_t ws_ev = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_pending = false;
  float* stage = nullptr;   // panel copy of a row-major client matrix (gm_weiszfeld_f32)
  size_t stage_bytes = 0;
  // bf16 shadow of an fp32 panel matrix (gm2's correction passes; run_stream), kept and reused
  // like `stage`; and what the last streaming gm2 call did with it (gm_delta_last_info)
  uint16_t* shadow = nullptr;
  size_t shadow_bytes = 0;
  int64_t delta_info[3] = {0, 0, GM_DELTA_OFF};
  // A register-resident grid that failed its co-residency check-in (device_util.h
  // grid_checkin: a shared GPU, CUs held by another stream) makes the next calls stream
  // straight away instead of paying the check-in's 100 ms again; retried after this many.
  int res_skip = 0;
  // the last Krum call (gm_krum_last_info): {algorithm, candidates, reason}
  int64_t krum_info[3] = {GM_KRUM_EXACT, 0, GM_KRUM_REASON_NOT_CHOSEN};
  // the last call of a bf16 distance entry (gm_dist_last_info): {tier, reason, slices, flush
  // width}.  After an MFMA-tier call dist_flag (pinned) receives the device's non-finite flag by
  // a copy queued on dist_stream; dist_pending until gm_dist_last_info has waited for it, and
  // dist_exact_slices is what info[2] becomes when the flag is up.
  int64_t dist_info[4] = {GM_DIST_EXACT, GM_DIST_REASON_REQUESTED_EXACT, 0, 0};
  int* dist_flag = nullptr;
  hipStream_t dist_stream = nullptr;
  bool dist_pending = false;
  int64_t dist_exact_slices = 0;
};

namespace gmh {

using namespace gmk;

inline thread_local std::string g_err;   // gm_last_error

inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(GM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                  __FILE__, __LINE__);                                                  \
  } while (0)

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// log2 of a panel width W (a power of two; 0 for W = 0, the row-major layout)
inline int wshift_of(int64_t W) {
  int ws = 0;
  while (((int64_t)1 << ws) < W) ++ws;
  return ws;
}

// A path that was not taken, or that declined after starting (a refused Gram result, a
// resident grid that was not co-resident): the caller goes on to the next path.
constexpr int kDeclined = 1;

// An integer environment knob, read at the call (callers that read once per process keep
// the value in a function-local static).
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
// A count knob: unset, zero or negative gives dflt.
inline int env_pos(const char* name, int dflt) {
  const int v = env_int(name, 0);
  return v > 0 ? v : dflt;
}

// ---- resident paths: the skip window and the environment knobs -------------------------

constexpr int kResSkipAfterCheckinFail = 64;

// Resident paths are tried unless a recent call's grid failed its check-in.  Called ONCE
// per public call (gm_weiszfeld_f32, gm_weiszfeld_batched_f32), so the skip window lasts
// kResSkipAfterCheckinFail calls however many resident paths a call considers.
inline bool resident_allowed(gm_ctx* c) {
  if (c->res_skip <= 0) return true;
  --c->res_skip;
  return false;
}

// GMAGG_RES_CHECKIN_FAIL=1: the check-in waits for one slot nobody writes, so it fails
// (tests of the fallback; read per call).
inline unsigned checkin_need(unsigned blocks) {
  return blocks + (env_int("GMAGG_RES_CHECKIN_FAIL", 0) != 0 ? 1u : 0u);
}

// XCD placement of the resident grids (read per call).  The single-problem kernel's blocks
// all on one XCD when they fit its CUs (stride 8: only blocks b % 8 == 0 work), its
// granules stored so that they stay in that XCD's L2 (GMAGG_RES_XCD=2, the default):
// C2 178.4 -> 227.3 aggregations/s (profiles/r4s2_xcd_local_ab.jsonl).  GMAGG_RES_XCD=1:
// the same placement with agent-scope (L2-dropping) stores, 172.9; 0: neither.  The batched
// kernel's groups are numbered XCD by XCD (GMAGG_RB_XCD=0 turns it off): a group of 49
// blocks spans 2-3 XCDs instead of 8, the AirComp exchange's traffic 259 -> 110 GB per
// 1024-problem launch, the prenoise sweep 70.5k -> 71.6k problems/s.
// (local stores only when the check-in confirms from XCC_ID that every block is on one XCD:
// resident.hip put_value; otherwise agent-scope stores, as for any placement)
inline int res_xcd_mode() { return env_int("GMAGG_RES_XCD", 2); }
// GMAGG_RB_HIER=1 (read per call): the batched resident kernel's groups gather by XCD
// (sub-group leaders, then the <= 3 sub-group sums) instead of flat over the group's 49
// blocks.  It cuts the C5 AirComp launch's HBM traffic 109.7 -> 33.8 GB (5.3x -> 1.65x the
// tile read) but measured slower — 818 -> 787 problems/s (AirComp), 70.3k -> 69.1k
// (prenoise): the exchange is latency-bound, not traffic-bound, and the leader's hop adds
// latency (profiles/r5s1_c5_rb_hier_ab.jsonl, r5s1_pmc_c5air_hier.txt).  Off by default.
inline int rb_hier_mode() { return env_int("GMAGG_RB_HIER", 0); }
// GMAGG_RES_SPLIT (read per call): 1 (default) the split-scope exchange for resident grids
// beyond one XCD that do not take the hierarchical gather (results bit-identical to the
// flat gather's; 50 x 20,000 6.03 -> 5.95 µs per iteration, 50 x 30,000 6.75 -> 6.62,
// 30 x 48,670 6.95 -> 6.77; profiles/r5s1_resident_split_ab.jsonl), 0 the flat gather
inline int res_split_mode() { return env_int("GMAGG_RES_SPLIT", 1); }
// GMAGG_RES_HIER (read per call): 1 (default) the XCD-hierarchical gather for resident grids
// beyond one XCD where it measured faster (>= 90 blocks, K > 32), 2 for every grid beyond
// one XCD, 0 never (the flat gather over every block)
inline int res_hier_mode() { return env_int("GMAGG_RES_HIER", 1); }
inline unsigned res_xcd_stride(int nb, int num_cu) {
  // GMAGG_RES_XCD_BPC=n (A/B): up to n blocks per CU of the one XCD
  static const int bpc = std::max(1, env_int("GMAGG_RES_XCD_BPC", 1));
  return (res_xcd_mode() != 0 && nb <= num_cu / 8 * bpc) ? 8u : 1u;
}
// The single-problem resident kernel's tile (round 4 session 2): at 32 < K <= 64, 8 waves
// of 8 rows per lane (512-thread blocks) instead of the streaming tile's 16 waves of 4 —
// half the waves in every cross-wave reduction and block barrier of the iteration, the
// same 256 columns per block: C2 238.0 -> 281.2 aggregations/s (profiles/r4s2_c2_tile_ab.jsonl).
// GMAGG_RES_CFG="NW,R" forces a tile (LPR 64; NW * R >= K), e.g. "16,4" the previous one.
inline void resident_tile(PassCfg* cfg, int64_t K) {
  if (cfg->LPR != 64) return;
  int nw = 0, r = 0;
  if (const char* e = getenv("GMAGG_RES_CFG")) {
    if (sscanf(e, "%d,%d", &nw, &r) != 2 || (int64_t)nw * r < K) nw = 0;
  } else if (K > 32 && K <= 64 && cfg->NW == 16 && cfg->R == 4) {
    nw = 8;
    r = 8;
  }
  if (nw > 0) {
    cfg->NW = nw;
    cfg->R = r;
  }
}
// GMAGG_RB_XCD: 0 round-robin numbering, 1 XCD-major (default), 2 XCD-major with whole
// groups per XCD whose granules stay in the XCD's L2 (resident_batched.hip rb_put)
inline int rb_xcd_major() {
  return env_int("GMAGG_RB_XCD", 1);      // 1 by default (round 4 A/B)
}

// ---- options -> kernel arguments -------------------------------------------------------

// OMA2's channel-noise std per real component (M:410)
inline double noise_sd(const gm_opts* o) { return std::sqrt(std::max(0.0, o->noise_var) / 2.0); }
// whether the AirComp passes add channel noise (options['noise_var'] is not None)
inline int aircomp_noise(const gm_opts* o) { return o->mode == GM_MODE_AIRCOMP && o->has_noise; }
// pre_oma's noise std (M:388)
inline float pre_oma_sd(const gm_opts* o) {
  return (float)std::sqrt(std::max(0.0, o->pre_oma_var));
}
// The AirComp channel fields of a streaming loop (all zero for centered clipping).
struct AirNoise {
  int has_noise;
  double noise_sd, P_max;
  uint64_t seed;
};
inline AirNoise air_noise(const gm_opts* o) {
  return {aircomp_noise(o), noise_sd(o), o->P_max, o->seed};
}
// The K-space step's arguments that come from the options (both streaming loops; the
// buffers and the per-iteration fields are the caller's).  mode: gm_mode, or kModeCclip.
inline KspaceArgs kspace_args(int64_t K, int64_t d_total, int mode, double tol, double eps,
                              const AirNoise& n) {
  KspaceArgs ka{};
  ka.K = K;
  ka.d_total = d_total;
  ka.mode = mode;
  ka.has_noise = n.has_noise;
  ka.tol = (float)tol;
  ka.eps = (float)eps;
  ka.P_max = n.P_max;
  ka.noise_sd = n.noise_sd;
  ka.seed = n.seed;
  return ka;
}

// What every path reports from the final device state.
inline gm_result result_from(const KState& st, int algo) {
  gm_result r{};
  r.iters = st.iters;
  r.last_movement = st.last_movement;
  r.converged = st.converged;
  r.algo_used = algo;
  return r;
}

// ---- workspace -------------------------------------------------------------------------

// Stream-orders the context's workspace between calls (see gm_ctx::ws_ev): the
// constructor selects the context's device and makes `s` wait for the previous call's
// tail when that call ran on another stream; the destructor marks the end of this call's
// work on `s`.
struct WsOrder {
  gm_ctx* c;
  hipStream_t s;
  hipError_t err;
  WsOrder(gm_ctx* c_, hipStream_t s_) : c(c_), s(s_), err(hipSetDevice(c_->device)) {
    if (err == hipSuccess && !c->ws_ev) err = hipEventCreateWithFlags(&c->ws_ev, hipEventDisableTiming);
    if (err == hipSuccess && c->ws_pending && c->ws_stream != s)
      err = hipStreamWaitEvent(s, c->ws_ev, 0);
  }
  ~WsOrder() {
    if (c->ws_ev && hipEventRecord(c->ws_ev, s) == hipSuccess) {
      c->ws_stream = s;
      c->ws_pending = true;
    }
  }
};

// The context's device workspace, at least `bytes` long (contents are not kept).
inline int grow_ws(gm_ctx* c, size_t bytes) {
  if (bytes <= c->ws_bytes) return GM_OK;
  if (c->ws) HIPCHK(hipFree(c->ws));
  c->ws = nullptr;
  c->ws_bytes = 0;
  HIPCHK(hipMalloc(&c->ws, bytes));
  c->ws_bytes = bytes;
  return GM_OK;
}

// Carves a buffer into 256-aligned, non-overlapping items in the order of the take()
// calls; `off` is the running total (the bytes needed once every item is taken, and the
// end of a prefix to zero after the last zeroed item).  A layout is written once as a
// function of the base and run twice: on a null base to size the buffer, then on the buffer.
struct Carve {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    const size_t o = off;
    off = align_up(off + sizeof(T) * count, 256);
    return base ? reinterpret_cast<T*>(base + o) : nullptr;
  }
};

// The single-problem paths' workspace (Weiszfeld streaming / resident / Gram, Krum, the
// honest variance).
struct Workspace {
  KState* st;
  double* sums;
  double* r;
  float* coef;
  double* slab;
  float* g[2];
  float* h_re;   // host-noise device copies
  float* h_im;
  float* hnoise; // d local + 1
  // Gram variant
  float* gslab;  // [blocks][tiles][1024] fp32 partial Grams
  double* G;     // [KP][KP]
  double* alpha;
  double* u;
  // gm2 with the bf16 shadow (delta): the base pass's iterate, coefficients and distances
  float* gbase;
  float* cb;
  double* Db;
};

inline int ensure_ws(gm_ctx* c, int64_t K, int64_t d, int nb, Workspace* w,
                     size_t gram_slab_n = 0, int KP = 0, bool delta = false) {
  const size_t S = 2 * K + 2;
  auto lay = [&](char* base) {
    Carve cv{base};
    w->st = cv.take<KState>(1);
    w->sums = cv.take<double>(S);
    w->r = cv.take<double>(K);
    w->coef = cv.take<float>(K);
    w->slab = cv.take<double>(S * (size_t)nb);
    w->g[0] = cv.take<float>(d);
    w->g[1] = cv.take<float>(d);
    w->h_re = cv.take<float>(K);
    w->h_im = cv.take<float>(K);
    w->hnoise = cv.take<float>(d + 1);
    w->gslab = cv.take<float>(gram_slab_n);
    w->G = cv.take<double>((size_t)KP * KP);
    w->alpha = cv.take<double>(K);
    w->u = cv.take<double>(K);
    w->gbase = cv.take<float>(delta ? d : 0);
    w->cb = cv.take<float>(delta ? K : 0);
    w->Db = cv.take<double>(delta ? K : 0);
    return cv.off;
  };
  const int rc = grow_ws(c, lay(nullptr));
  if (rc) return rc;
  lay(c->ws);
  return GM_OK;
}

// ---- the pinned buffer -----------------------------------------------------------------
//
// c->host is one pinned allocation that every path lays out from offset 0 for the length
// of its call (the ensure_host sizes at the call sites cover exactly these):
//   streaming        KState final | KState lagged[2] | pad to 256 | float h_re[K], h_im[K],
//                    noise[d_total + 1]   (the host-noise callback's staging)
//   resident         KState final
//   Gram             KState final | double {||p - g||^2, ||g||^2}
//   Krum (Gram)      KState final | int64 {candidate count, row of the smallest upper bound}
//   batched          KState final[P] | unsigned flag[4] (the resident kernel's; the streaming
//                    loop reads its done counter into the first int before the final copy)
// host_state / host_lagged / host_noise_stage / host_after_states name these.
inline KState* host_state(gm_ctx* c) { return reinterpret_cast<KState*>(c->host); }
inline KState* host_lagged(gm_ctx* c) { return host_state(c) + 1; }   // [2], by iteration parity
constexpr size_t kHostNoiseOff = align_up(3 * sizeof(KState), 256);
inline float* host_noise_stage(gm_ctx* c) { return reinterpret_cast<float*>(c->host + kHostNoiseOff); }
template <class T>
inline T* host_after_states(gm_ctx* c, int64_t P = 1) {
  return reinterpret_cast<T*>(c->host + sizeof(KState) * P);
}

inline int ensure_host(gm_ctx* c, size_t bytes) {
  if (bytes <= c->host_bytes) return GM_OK;
  if (c->host) HIPCHK(hipHostFree(c->host));
  c->host = nullptr;
  c->host_bytes = 0;
  // (a) Everything but the lagged slots arrives by hipMemcpyAsync + a stream synchronise.
  // The lagged slots are written by plain stores of the K-space kernel (KspaceArgs.mirror)
  // and read by the host only after hipEventSynchronize on the poll event recorded behind
  // that kernel.  The poll events are created without hipEventDisableSystemFence, so the
  // record carries a system-scope release of the kernel's stores, and the host never looks
  // at a slot while its kernel may still be running; no device-side fence and no host-
  // coherent polling is needed, so hipHostMallocDefault suffices whether or not the runtime
  // maps it fine-grained.
  // (b) Every entry point that touches c->host holds a WsOrder.  A lagged call returns while
  // its no-op tail is still queued, and that tail's K-space launch may still write its slot:
  // the next call's work (on the same stream by order, on another through ws_ev) queues
  // behind it, so no path reuses the buffer before the late slot write has landed.
  HIPCHK(hipHostMalloc(&c->host, bytes, hipHostMallocDefault));
  c->host_bytes = bytes;
  return GM_OK;
}

// ---- collectives and pass timing -------------------------------------------------------

inline int allreduce(gm_ctx* c, double* buf, int64_t n, hipStream_t s) {
  if (c->comm) {
    ncclResult_t r = ncclAllReduce(buf, buf, (size_t)n, ncclDouble, ncclSum, c->comm, s);
    if (r != ncclSuccess) return fail(GM_ERR_COMM, "ncclAllReduce: %s", ncclGetErrorString(r));
    return GM_OK;
  }
  if (c->ar_fn) {
    if (c->ar_fn(c->ar_user, buf, n, (void*)s) != 0)
      return fail(GM_ERR_CALLBACK, "all-reduce callback failed");
  }
  return GM_OK;
}

inline int record_pass_begin(gm_ctx* c, hipStream_t s, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!c->timing) return GM_OK;
  for (int i = 0; i < 2; ++i) {
    hipEvent_t e;
    if (!c->ev_free.empty()) {
      e = c->ev_free.back();
      c->ev_free.pop_back();
    } else {
      HIPCHK(hipEventCreate(&e));
    }
    (i == 0 ? *e0 : *e1) = e;
  }
  HIPCHK(hipEventRecord(*e0, s));
  return GM_OK;
}

inline int record_pass_end(gm_ctx* c, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  if (!c->timing) return GM_OK;
  HIPCHK(hipEventRecord(e1, s));
  c->ev_used.emplace_back(e0, e1);
  return GM_OK;
}

// Gives back the last recorded timing pair: a launch that did no pass's work (a resident
// grid that timed out, a streaming pass queued after the stop) is not counted.
inline void drop_last_timing(gm_ctx* c) {
  if (!c->timing || c->ev_used.empty()) return;
  c->ev_free.push_back(c->ev_used.back().first);
  c->ev_free.push_back(c->ev_used.back().second);
  c->ev_used.pop_back();
}

// Gives back the timing pairs first + i with drop[i] set, of the pairs recorded from position
// `first` on: of the two kernels gm2's shadow path queues per iteration, the one the device did
// not choose exited at once and is no pass, like every launch queued after the stop.
inline void drop_timings(gm_ctx* c, size_t first, const std::vector<char>& drop) {
  if (!c->timing) return;
  size_t keep = first;
  for (size_t i = first; i < c->ev_used.size(); ++i) {
    if (i - first < drop.size() && drop[i - first]) {
      c->ev_free.push_back(c->ev_used[i].first);
      c->ev_free.push_back(c->ev_used[i].second);
    } else {
      c->ev_used[keep++] = c->ev_used[i];
    }
  }
  c->ev_used.resize(keep);
}

// ---- tiles -----------------------------------------------------------------------------

// Streaming-pass tile for K rows.
// The tile is K_pad x J with J = LPR*V columns; NRG = 16*64/LPR row groups of
// R rows each cover K.  Bigger K -> narrower chunk, so a block's tile (and the
// bytes it has in flight) stays ~64-128 KiB.
// panel: the tile of a panel-layout call (its chunk width is the panel width W).
// b16: the same tile on bf16 elements (V = 8; PassCfg.B16).
inline bool pick_cfg(int64_t K, int V, int64_t ldx, PassCfg* cfg, bool panel = false,
                     bool b16 = false) {
  int nw = 16, lpr, r, occ = 1;
  if (K <= 16) { lpr = 64; r = 1; }
  else if (K <= 32) { lpr = 64; r = 2; }
  // 32 < K <= 64 on panels (C5's K = 50 batched problems): 512-thread blocks of 64 x 128
  // chunks, 5.41-5.49 vs 5.07-5.13 TB/s per C5 STEP pass (profiles/history/r2_c5_panels.txt); rows
  // keep (16,64,4), whose 256-column chunks let C1/C2 stay register-resident
  else if (K <= 64) { if (panel) { nw = 8; lpr = 32; r = 4; } else { lpr = 64; r = 4; } }
  else if (K <= 128) { lpr = 64; r = 8; }
  // 128 < K <= 256 on panels: 256 x 64 chunks (W = 64, each chunk 64 KB contiguous),
  // STEP 2.38 vs 2.54 ms and the C4-shard Gram closing pass 2.58 vs 2.80 ms against the
  // 256 x 128 tile (profiles/history/r2_k256_tiles.txt); rows keep the 512-B row segments
  else if (K <= 256) { if (panel) { lpr = 16; r = 4; } else { lpr = 32; r = 8; } }
  else if (K <= 512) { lpr = 16; r = 8; }
  // K <= 1024: two 512-thread blocks per CU, each with a 1024 x 32 tile (128 B row
  // segments): 6.29 vs 6.05 TB/s for one 1024-thread block (profiles/history/r01_occ_sweep.txt)
  else if (K <= 1024) { nw = 8; lpr = 8; r = 16; occ = 2; }
  else if (K <= 2048) { lpr = 4; r = 8; }
  else return false;
  // GMAGG_PASS_CFG="NW,LPR,R[,OCC]" forces a tile (tuning runs); it must cover K.
  if (const char* e = getenv("GMAGG_PASS_CFG")) {
    int a = 0, b = 0, c2 = 0, o = 1;
    const int n = sscanf(e, "%d,%d,%d,%d", &a, &b, &c2, &o);
    if (n >= 3 && b > 0 && (int64_t)a * (64 / b) * c2 >= K) {
      nw = a; lpr = b; r = c2; occ = n == 4 ? o : 1;
    }
  }
  // lane offsets are 32-bit: (rows per wave - 1) * ldx + ldx must fit in bytes
  if ((uint64_t)(64 / lpr) * (uint64_t)ldx * 4u >= (1ull << 31)) return false;   // buffer offsets
  *cfg = PassCfg{V, nw, lpr, r, occ, b16};
  return pass_cfg_supported(*cfg);
}

// Tile of the passes without phase A's weighted sum feeding phase B (INIT) or
// without phase B (the Gram closing pass): at 128 < K <= 256 the 1-KiB row
// segments of (16,64,16) beat the STEP tile (16,32,8): 2.81 / 2.76 vs 3.00 /
// 2.99 ms at K=256 x d=15.6M (profiles/history/r02_sweep_close.txt).
inline PassCfg light_cfg(int64_t K, const PassCfg& step) {
  if (getenv("GMAGG_PASS_CFG") || step.V != 4 || K <= 128 || K > 256) return step;
  const PassCfg c{4, 16, 64, 16, 1};
  return pass_cfg_supported(c) ? c : step;
}

inline int pick_vec(const float* X, int64_t d, int64_t ldx) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(X);
  if (d % 4 == 0 && ldx % 4 == 0 && p % 16 == 0) return 4;
  if (d % 2 == 0 && ldx % 2 == 0 && p % 8 == 0) return 2;
  return 1;
}

// PassArgs.chunk_pair for a row-major pass of `grid` blocks on tile `cfg`: the CU count when
// the grid is exactly two blocks per CU (GMAGG_CHUNK_PAIR=0: off, for A/B).  Only the 32-wave
// rows kernel reads it (the generic tile's chunk order, and so its sums, stay as they were)
inline int chunk_pair(const gm_ctx* c, const PassCfg& cfg, int64_t grid) {
  static const bool off = env_int("GMAGG_CHUNK_PAIR", 1) == 0;
  return !off && cfg.OCC == 2 && grid == 2 * (int64_t)c->num_cu ? c->num_cu : 0;
}

// ---- the staged panel copy -------------------------------------------------------------

// The context's panel copy of a row-major client matrix (gm_weiszfeld_f32 /
// gm_weiszfeld_batched_f32 stage row-major AirComp inputs into it).  GMAGG_STAGE_PANELS=0
// turns staging off.  Returns false (and streams the rows) when the buffer cannot be had.
inline bool stage_enabled() {
  static const bool on = env_int("GMAGG_STAGE_PANELS", 1) != 0;
  return on;
}

inline bool ensure_stage(gm_ctx* c, size_t bytes) {
  if (bytes <= c->stage_bytes) return true;
  if (c->stage) (void)hipFree(c->stage);   // (hipFree waits for queued work)
  c->stage = nullptr;
  c->stage_bytes = 0;
  if (hipMalloc(&c->stage, bytes) != hipSuccess) {
    (void)hipGetLastError();
    c->stage = nullptr;
    return false;
  }
  c->stage_bytes = bytes;
  return true;
}

// ---- the bf16 shadow (gm2's correction passes) -----------------------------------------

// GMAGG_DELTA, read once per process: 0 never, 1 at any size, unset (or anything else) the
// default: where 4 K d_total is at least kDeltaMinBytes.  The correction passes pay where X
// streams from HBM: eight times the 256 MiB Infinity Cache and more.
constexpr int64_t kDeltaMinBytes = (int64_t)1 << 31;
inline int delta_knob() {
  static const int v = [] {
    const char* e = getenv("GMAGG_DELTA");
    return !e ? -1 : e[0] == '0' && !e[1] ? 0 : e[0] == '1' && !e[1] ? 1 : -1;
  }();
  return v;
}

// The context's shadow buffer, at least `bytes` long; false when it cannot be had (the call
// then runs the exact passes only).
inline bool ensure_shadow(gm_ctx* c, size_t bytes) {
  if (bytes <= c->shadow_bytes) return true;
  if (c->shadow) (void)hipFree(c->shadow);   // (hipFree waits for queued work)
  c->shadow = nullptr;
  c->shadow_bytes = 0;
  if (hipMalloc(&c->shadow, bytes) != hipSuccess) {
    (void)hipGetLastError();
    c->shadow = nullptr;
    return false;
  }
  c->shadow_bytes = bytes;
  return true;
}

// ---- one pass of a streaming loop ------------------------------------------------------

// pre_oma: the reference's OMA(weight_f, var) before a non-gm aggregator (M:351-352),
// applied to X in place, exactly once on whichever path runs.  The streaming loops fuse it
// into their INIT pass (MODE 4: one read + write of X instead of OMA's read + write and
// INIT's read); every other path runs the standalone kernel first.  Draws as
// gm_oma_philox_f32 / _panels_f32; of P batched problems ldp elements apart, problem p is
// keyed seed + p * kSeedStride either way.
struct PreOma {
  bool pending;
  float* X;
  int64_t K, d, ldx, d_total, col_off;
  bool panels;
  float sd;
  uint64_t seed;
  hipStream_t s;
  int64_t P = 1, ldp = 0;
  int apply() {
    if (!pending) return GM_OK;
    pending = false;
    const int wshift = panels ? wshift_of(gm_panel_width(K)) : 0;
    HIPCHK(launch_oma_philox(X, K, d, ldx, d_total, col_off, sd, seed, s, wshift, P,
                             P > 1 ? ldp : 0));
    return GM_OK;
  }
};

// What the passes of one streaming loop have in common (run_stream, run_stream_batched).
// The tile, pass mode and grid are indexed by `init`: [0] STEP, [1] INIT.
struct StreamPasses {
  gm_ctx* c;
  hipStream_t s;
  PassArgs a;        // every field but the iterates, slab_stride, iter, chunk_pair and the OMA's
  bool twopass;      // the two-pass kernels (one row-major problem) instead of the fused pass
  PassCfg cfg[2];
  int mode[2], nb[2];
  int problems;
  double* sums;      // the reduced partials, sums_ps apart per problem
  int64_t sums_ps;
  bool pair;         // chunk_pair's block order (the single-problem loop on rows)
  PreOma* oma;
};

// Pass t over X (t < 0: INIT on the guess; else STEP t from g_old to g_new) and the reduction
// of its slab into p.sums.  INIT applies a pending pre-noise; STEP passes are the timed ones.
inline int stream_pass(const StreamPasses& p, int64_t t, const float* g_old, int64_t gold_ps,
                       float* g_new) {
  const bool init = t < 0;
  const PassCfg& cfg = p.cfg[init];
  const int nb = p.nb[init];
  int mode = p.mode[init];
  PassArgs a = p.a;
  a.g_old = g_old; a.gold_ps = gold_ps; a.g_new = g_new;
  a.slab_stride = init ? 2 * a.K + 2 : a.K + 2;
  a.iter = t;
  a.chunk_pair = p.pair ? chunk_pair(p.c, cfg, nb) : 0;
  if (init && p.oma->pending) {
    // the fused OMA needs float4 groups = Philox blocks: a V = 4 tile of the fused pass, the
    // INIT without the row norms (mode 1), a shard that starts on a multiple of 4 columns
    // (batched problems are unsharded: col_off = 0)
    if (!p.twopass && cfg.V == 4 && mode == 1 && a.col_off % 4 == 0) {
      mode = 4;
      a.oma_sd = p.oma->sd;
      a.oma_seed = p.oma->seed;
      p.oma->pending = false;
    } else {
      const int rco = p.oma->apply();
      if (rco) return rco;
    }
  }
  hipEvent_t e0, e1;
  int rc = init ? GM_OK : record_pass_begin(p.c, p.s, &e0, &e1);
  if (rc) return rc;
  if (p.twopass)   // (reduces its own partials)
    HIPCHK(launch_twopass(init, a.X, a.K, a.d, a.ldx, g_old, g_new, a.coef, a.st, a.noise,
                          a.hnoise, a.seed, t, a.col_off, a.slab, nb, p.sums, p.s));
  else
    HIPCHK(launch_pass(cfg, mode, nb, a, p.s, p.problems));
  if (!init) { rc = record_pass_end(p.c, p.s, e0, e1); if (rc) return rc; }
  if (!p.twopass)
    HIPCHK(launch_slab_reduce(a.slab, nb, a.slab_stride, p.sums, a.st, p.s, p.problems,
                              p.sums_ps));
  return GM_OK;
}

// Batched problems that fit on chip (host_batched.hip; gm_weiszfeld_f32 runs a panel-layout
// problem through it with P = 1).  kDeclined: not eligible, or the grid failed its check-in.
int run_resident_batched(gm_ctx* c, const float* X, int64_t P, int64_t K, int64_t d,
                         int64_t ldx, int64_t ldp, bool panels, int64_t Wp, const float* guess0,
                         int64_t ldg, float* out, int64_t ldo, const gm_opts* o,
                         gm_result* results, hipStream_t s, bool res_ok);

}  // namespace gmh
