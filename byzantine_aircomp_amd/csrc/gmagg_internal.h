// Internal interface between the C-ABI layer (api.hip, host_*.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmk {

constexpr int kTPB = 1024;           // threads per block of the streaming pass
constexpr int kWaves = kTPB / 64;

// Device-resident state of one Weiszfeld call (written by kspace_step, read by
// every kernel's early-exit test and by the host poll).
struct alignas(64) KState {
  int32_t done;          // 1 once the tol test fired (later launches are no-ops)
  int32_t converged;
  int64_t iters;         // loop bodies executed
  double last_movement;  // fp32 movement of the last body, widened
  float a_noise;         // scale of the next pass's column term: the per-column noise
                         // (AIRCOMP), or the old iterate's 1 - sum_k c_k (centered clipping)
  float s;               // scaler sqrt(mean(g^2)) of the current iterate (AIRCOMP)
  // Gram variant, written by gram_solve for the AUTO accuracy guard (host_weiszfeld.hip):
  double guard_q;        // ||X'^T b||: one-step error of the K-space map (gram_verify)
  double guard_r;        // last / previous K-space movement (contraction estimate)
  int32_t gram_bad;      // the reduced Gram has a non-finite entry (f16 overflow or input)
  int32_t clipped;       // centered clipping: clients with dist_k > tau at the last coefficients
  // gm2 on panels with the bf16 shadow (KspaceArgs.delta):
  uint32_t kind_mask;    // bit t: STEP t ran as a correction pass (t < kDeltaMaxIter)
  uint32_t flags;        // kFlag*: what the K-space step decided for the next STEP
};
static_assert(sizeof(KState) == 64, "KState: one 64-byte line, as the kernels index it");
constexpr uint32_t kFlagNextDelta = 1;     // the next STEP is a correction pass
constexpr uint32_t kFlagWriteShadow = 2;   // the next exact STEP stores its tile as bf16
constexpr uint32_t kFlagShadowDone = 4;    // the shadow is complete and a base pass is kept
constexpr int kDeltaMaxIter = 32;          // correction passes only at t < 32 (the mask's bits)

// Streaming pass configuration: V floats per lane per row, NW waves per
// block, LPR lanes per row segment (chunk width J = LPR*V columns), R rows
// per thread (the block covers NW*(64/LPR)*R rows).
struct PassCfg {
  int V, NW, LPR, R;
  int OCC = 1;   // blocks per CU the kernel's registers are capped for
  // X holds bf16 elements (gm_weiszfeld_bf16): V = 8 columns per lane, one 16-byte load as
  // the fp32 tile's V = 4, so the bytes per row segment, per chunk and per load and the
  // register tile are the fp32 tile's and the chunk is twice as wide (J = LPR * 8)
  bool B16 = false;
};

struct PassArgs {
  const float* X;         // bf16 tiles (PassCfg.B16): uint16_t elements behind the same pointer
  int64_t K, d, ldx;
  const float* g_old;     // iterate t (INIT: the initial guess)
  float* g_new;           // iterate t+1 (STEP)
  const float* coef;      // K normalised weights / AirComp coefficients (STEP)
  const KState* st;
  double* slab;           // [gridDim.x][slab_stride] per-block partial sums
  int64_t slab_stride;
  // column term of the STEP pass: g' = sum_k c_k x_k + a_noise * term (the AirComp variant's
  // additive noise, or centered clipping's old iterate)
  int noise;              // 0 none, 1 Philox, 2 host-supplied column draws, 3 g_old (cclip)
  const float* hnoise;    // noise == 2: local column draws (d floats)
  uint64_t seed;
  int64_t iter;           // Weiszfeld iteration index the pass computes
  int64_t col_off;        // global index of local column 0 (d-sharding)
  // Batched independent problems (BASELINE C5): blockIdx.y = problem p; X,
  // g_old, g_new advance by these element strides, coef by K, st by 1, slab by
  // gridDim.x * slab_stride, the Philox seed by p * kSeedStride.  0 / unused for P = 1.
  int64_t x_ps, gold_ps, gnew_ps;
  // > 0: X is in the panel layout [ceil(d/J)][K][J] with this many elements
  // between panels (J = the tile's chunk width); 0: row-major [K][ldx].
  int64_t panel_stride;
  // MODE 4 (INIT + OMA): the reference's OMA pre-noise (M:351-352, M:385-394) applied to
  // the tile in registers and written back before the INIT distances; Philox keyed by
  // oma_seed (+ p * kSeedStride for batched problem p), draws as gm_oma_philox_f32's
  float oma_sd;
  uint64_t oma_seed;
  // rows_pass only (the row-major gm2 STEP at two blocks per CU): P = the CU count when the
  // grid is two blocks per CU, else 0.  The hardware places block b and block b + P on one
  // CU, so they take adjacent chunks (first_chunk): the CU's two blocks read adjacent 128-B
  // segments of each row at about the same time (round 6: C3 rows STEP 6,844 -> 6,788 us,
  // with identical UTCL1 misses: DRAM / L2 locality; pairing b with b + 8 or b + 16 gains
  // nothing, and on panels the pairing measured 1.6 % slower:
  // profiles/r6s2_rows_chunk_pair_ab.jsonl, r6s2_utcl1_rows_chunk_pair.json)
  int chunk_pair;
  // The DELTA kernels only (kPassStepExactD / kPassStepDelta): the bf16 shadow of X in panels
  // of the fp32 chunk's width, shadow_stride elements between its panels (written by the exact pass when
  // kFlagWriteShadow is set, read by the correction pass through X / panel_stride), and the
  // base iterate G (written by every exact pass, read by the correction pass).
  uint16_t* shadow;
  int64_t shadow_stride;
  float* gbase;
  int64_t slab_rows;      // slab rows the reduction sums: the larger of the two kinds' grids
};

// The first chunk of block b in a grid-stride walk (chunks b', b' + grid, ...): b itself,
// or with the pairing above 2 (b mod P) + (b / P) for b < 2P (a permutation of [0, grid)
// when 2P divides the grid)
__host__ __device__ inline int64_t first_chunk(int P, int64_t b, int64_t grid) {
  if (P <= 0 || grid % (2 * P) != 0) return b;
  return 2 * ((b / (2 * P)) * P + b % P) + (b / P) % 2;
}

constexpr uint64_t kSeedStride = 0x9E3779B97F4A7C15ull;
// The reference's fp32 movement floor in ulps of ||g|| (M:180: an fp32 norm of a difference
// of fp32 iterates): the Gram guard accepts an exact-arithmetic count only where
// kFloorUlps * 2^-24 * ||g|| <= tol.  The SAME constant as oracle/aggregators.py FLOOR_ULPS
// (the count window the tests check counts against; measured: profiles/r5s1_movement_floor.txt)
constexpr double kFloorUlps = 2.0;

// KspaceArgs.mode beyond the public gm_mode values: centered clipping (gm_cclip_f32 / _bf16;
// Karimireddy, He & Jaggi 2021, Algorithm 2), c_k = min(1, tau / dist_k) / K and the old
// iterate weighted a = 1 - sum_k c_k.  The streaming loop only.
constexpr int kModeCclip = 2;

struct KspaceArgs {
  int64_t K, d_total, t;  // t = pass just completed, -1 after the initial pass
  int mode;               // gm_mode, or kModeCclip
  int has_noise, noise_src;
  float tol, eps;
  double P_max, noise_sd; // noise_sd = sqrt(noise_var / 2) (OMA2, M:410)
  uint64_t seed;
  int do_check, do_coef;
  const double* sums;     // reduced partials (all shards)
  double* r;              // ||x_k||^2, saved at init (AIRCOMP)
  const float* h_re;      // host-noise draws of iteration t+1 (device copies)
  const float* h_im;
  const float* n_last;    // the denominator's noise element
  float* coef;
  KState* st;
  // Batched: blockIdx.x = problem; sums advance by sums_ps, r / coef by K, st by 1.
  int64_t sums_ps;
  int* n_done;            // problems whose tol test has fired (nullable)
  KState* mirror;         // host-mapped copy of *st written at the end (nullable, one problem)
  double tau;             // kModeCclip: the clipping radius (> 0, +inf allowed)
  // gm2 with the bf16 shadow (mode 0 only; 0: the step as it always was).  From STEP 1 on the
  // step reads which kind of pass just ran from st->flags, forms the distances of a correction
  // pass as Db_k + sums[K + 2] - 2 sums[k], keeps c^b (cb) and D^b (Db) of every exact pass
  // from STEP 1 on, and chooses the next pass's kind and whether it writes the shadow.
  int delta;              // 1, or 2: the first exact pass that can (STEP 1) writes the shadow
  float* cb;             // [K] the base pass's coefficients, as that pass read them
  double* Db;             // [K] the base pass's exact squared distances
  double theta;           // correction iff max_k |c_k - cb_k| <= theta cb_k
};
// theta = 2^9 eps_tile / 4: the shadow's 2^-9 relative error on sum_k |c_k - cb_k| |x_kj| then
// stays within a quarter of the bar the exact tile is held to (eps_tile = (A + 32) 2^-24 with
// A = R + log2(64 / LPR) + NW of the STEP tile; tests/stream_cases.py).
inline double delta_theta(const PassCfg& cfg) {
  int lq = 0;
  if (cfg.LPR <= 0) return 0.0;   // no tile (the two-pass loop)
  while ((64 / cfg.LPR) >> (lq + 1)) ++lq;
  return (double)(cfg.R + lq + cfg.NW + 32) / (double)(1 << 17);
}
// The shadow is written by the pass after STEP t when the coefficients have begun to settle,
// r_t = max_k |c_k(t+1) - c_k(t)| / c_k(t) <= kDeltaArmRatio theta, and the movement is still
// at least kDeltaArmMove tol: the write costs 0.9 of a pass (measured at C3) and a correction
// saves half of one, so it pays from two corrections on, and with movement contracting by up to
// 64x per pass (C3: 60-200x) two more passes beyond the writing one run iff mv_t > 64^2 tol.
// A wrong guess costs that 0.9 of a pass, never a bit of the result.
constexpr double kDeltaArmRatio = 64.0;
constexpr double kDeltaArmMove = 4096.0;

// Streaming pass (stream_pass.hip).  mode: 0 step, 1 init, 2 init + ||x_k||^2, 3 Gram
// closing sum, 4 init after OMA pre-noise written back to X (V = 4 tiles), kPassStepSelf a
// STEP pass whose column term is the old iterate (centered clipping; PassArgs.noise = 3).
constexpr int kPassStepSelf = 5;
// The gm2 STEP's two kinds on fp32 panels with a bf16 shadow (DELTA = 1, 2 of the kernel
// template): the exact pass on the fp32 tile, and the correction pass, whose cfg is a bf16
// tile of the same chunk width and whose X / panel_stride are the shadow's.  Built for the
// 512 < K <= 1024 tile.
constexpr int kPassStepExactD = 6;
constexpr int kPassStepDelta = 7;
const void* pass_kernel_delta(const PassCfg& cfg, int mode);   // stream_pass_delta.hip
hipError_t launch_pass(const PassCfg& cfg, int mode, int grid, const PassArgs& a, hipStream_t s,
                       int problems = 1);
int pass_blocks_per_cu(const PassCfg& cfg, int mode);
// The row-major gm2 STEP / INIT at 512 < K <= 1024 on 32 waves per CU (rows_pass.hip).
bool rows_pass_eligible(const PassArgs& a, int mode);
hipError_t launch_rows_pass(int mode, int grid, const PassArgs& a, hipStream_t s);
bool pass_cfg_supported(const PassCfg& cfg);
int pass_variant();   // GMAGG_PASS_VARIANT (stream_pass.hip), -1 unset
// The bf16-input instantiations (stream_pass_bf16.hip): the tiles pick_cfg returns, modes
// 0-2, both layouts, the plain and the rolling schedule; nullptr for anything else.
const void* pass_kernel_bf16(const PassCfg& cfg, int mode, bool panel);
// The fp32 STEP instantiations with the old iterate as column term (stream_pass_cclip.hip):
// every tile and schedule launch_pass would pick for mode 0; nullptr for anything else.
const void* pass_kernel_self(const PassCfg& cfg, bool panel);

// Reduction, K-space step and the two-pass path (weiszfeld.hip).
hipError_t launch_slab_reduce(const double* slab, int nb, int64_t S, double* sums,
                              const KState* st, hipStream_t s, int problems = 1,
                              int64_t sums_ps = 0);
hipError_t launch_kspace(const KspaceArgs& a, hipStream_t s, int problems = 1);
hipError_t launch_twopass(bool init, const float* X, int64_t K, int64_t d, int64_t ldx,
                          const float* g_old, float* g_new, const float* coef, const KState* st,
                          int noise, const float* hnoise, uint64_t seed, int64_t iter,
                          int64_t col_off, double* slab, int nb, double* sums, hipStream_t s);
int twopass_blocks(int64_t K, int64_t d, int num_cu);
hipError_t launch_batched_finalize(const float* g0, const float* g1, int64_t d, int problems,
                                   const KState* st, float* out, int64_t ldo, hipStream_t s);

// Register-resident persistent kernel for small problems (resident.hip).
struct ResArgs {
  const float* X;
  int64_t K, d, ldx;
  // panels (pstride > 0): element (k, j) at X + (j >> wshift) * pstride + k * 2^wshift +
  // (j & (2^wshift - 1)); rows [K][ldx] otherwise
  int64_t pstride;
  int wshift;
  const float* guess0;
  float* out;
  int64_t maxiter;
  float tol, eps;
  int mode, has_noise;
  double P_max, noise_sd;
  uint64_t seed;
  unsigned long long* gran;  // [2][gridDim.x][2K + 2] {tag, fp32} granules (zeroed per call)
  unsigned* bar;         // [2] timeout flag, [3] check-in passed (zeroed per call)
  unsigned long long* checkin;   // [gridDim.x + 1] co-residency slots (zeroed per call)
  unsigned need;         // slots the check-in waits for (gridDim.x; + 1 forces a failure)
  // 1, or 8: the grid is 8x the working blocks and only blocks b % 8 == 0 work (logical
  // block b / 8), so that — workgroups being dispatched round-robin over the 8 XCDs — every
  // working block sits on ONE XCD and the exchange stays inside its L2 (A/B knob)
  unsigned stride;
  // 1: when the check-in finds every block on one XCD, the granules are stored so that
  // they stay in that XCD's L2 (resident.hip put_value); 0: agent-scope stores always
  int local;
  // XCD-hierarchical gather (grids beyond one XCD, stride 1): blocks b with b % 8 == x form
  // group x (the blocks dispatch places on XCD x); each block publishes to its group, the
  // group's first block (the leader) sums its members and publishes the group sum as an
  // fp32 {hi, lo} granule pair into lvl2 [2][8][2 (2K + 2)]; every block sums the 8 group
  // sums in group order.  0: the flat gather over every block.
  int hier;
  unsigned long long* lvl2;
  // split-scope exchange (stride 1, not hier): every granule also stored L2-kept into
  // granL [2][gridDim.x][2K + 2]; a reader polls its own XCD's blocks (b % 8 == its group)
  // there once the check-in confirms the group on one XCD
  int split;
  unsigned long long* granL;
  KState* st;
};
// Plan a resident launch over nch chunks: chunks per block and blocks (false: the
// grid cannot be co-resident / no kernel for the tile).
bool resident_plan(const PassCfg& cfg, int64_t nch, int num_cu, int* cpb, int* nb);
size_t resident_gran_words(int64_t K, const PassCfg& cfg, int nb);
// whether the resident kernel of this tile has exchange variant xg (1 hierarchical, 2 split)
bool resident_has_exchange(const PassCfg& cfg, int cpb, int xg);
hipError_t launch_resident(const PassCfg& cfg, int cpb, int grid, const ResArgs& a, hipStream_t s);
bool res_coop_launch();   // GMAGG_RES_COOP=1: cooperative launches (resident.hip)

// Register-resident batched kernel (resident_batched.hip, C5): NG groups of NB blocks,
// group g runs problems g, g + NG, ... each held in VGPRs for all its iterations.
struct ResBArgs {
  const float* X;         // problem p at X + p * x_ps; rows [K][ldx] or panels (pstride > 0)
  int64_t P, K, d, ldx, x_ps, pstride;
  int wshift;             // panels: W = 1 << wshift
  int prob_bytes;         // bytes of one problem's buffer (< 2^31; the loads' range)
  int nb;                 // blocks per group
  const float* guess0;
  int64_t ldg;
  float* out;
  int64_t ldo;
  int64_t maxiter;
  float tol, eps;
  int mode, has_noise;
  double P_max, noise_sd;
  uint64_t seed;          // AirComp Philox key (problem p: seed + p * kSeedStride)
  int pre_oma;            // gm2 --var: OMA pre-noise in registers, written back to X
  float oma_sd;
  uint64_t oma_seed;
  unsigned long long* gran;  // [NG][2][NB][2K + 2] {tag, fp32} granules (zeroed per call)
  unsigned* flag;         // [0] timeout flag, [2] check-in passed (zeroed per call)
  unsigned long long* checkin;   // [gridDim.x + 1] co-residency slots (zeroed per call)
  unsigned need;          // slots the check-in waits for (gridDim.x; + 1 forces a failure)
  // 1: logical block = blockIdx.x (a group's NB blocks round-robin over all 8 XCDs);
  // XCD-major: logical blocks numbered XCD by XCD (b % 8 first), so a group of NB blocks
  // spans ceil(NB / 32) + 1 XCDs instead of 8 (A/B knob)
  int xcd_major;
  // 1: groups whose blocks the check-in finds on one XCD store their granules into that
  // XCD's L2 (resident_batched.hip rb_put); the plan then gives each XCD whole groups
  int local;
  // 1 (with xcd_major): the XCD-hierarchical gather — a group's blocks gather by XCD
  // (sub-group leaders), then every block sums the <= 8 sub-group sums in lvl2
  // [NG][2][8][2 (2K + 2)] (resident_batched.hip)
  int hier;
  unsigned long long* lvl2;
  KState* st;             // [P]
};
struct RbPlan {
  int kr;                 // rows held per thread (K rounded up: 16, 32 or 52)
  int nb;                 // blocks per problem (2048 columns each)
  int ng;                 // problems in flight (groups)
  int mode;               // gm_mode (the kernel is built per mode)
};
// xcd_whole: whole groups per XCD (8 x floor(cap / 8 / nb) groups, when that is >= 8), so
// that each group's blocks share one L2 (GMAGG_RB_XCD=2)
bool rb_plan(int64_t K, int64_t d, int64_t P, int mode, int num_cu, RbPlan* plan,
             bool xcd_whole = false);
size_t rb_gran_words(int64_t K, const RbPlan& plan);
hipError_t launch_resident_batched(const RbPlan& plan, const ResBArgs& a, bool coop, hipStream_t s);

// Gram-space variant (gram.hip).  KT = K padded to 32-row tiles (0: unsupported).
// H16: scaled f16 h+m split, 3 products on v_mfma_f32_32x32x16_f16 (default);
// BF16: bf16 h+m split, 4 products on v_mfma_f32_32x32x16_bf16 (fallback when
// the f16 Gram is non-finite); F32: exact f32-input v_mfma_f32_32x32x2_f32.
enum class GramKind { F32, BF16, H16 };
struct GramGrid {
  int nb;          // blocks
  int64_t cpb;     // columns per block
  int nseg;        // fp32 partials per block
};
int gram_kt(int64_t K);
GramGrid gram_grid(int64_t d, GramKind kind, int num_cu);
size_t gram_slab_floats(int KT, const GramGrid& g);
// the f16 kernel's per-block scale exponents (written by every H16 launch_gram)
int* gram_block_exp(float* slab, int KT, const GramGrid& g);
// pstride > 0: X in the panel layout [ceil(d/W)][K][W], W = 1 << wshift (H16 only).
hipError_t launch_gram(const float* X, int64_t K, int64_t d, int64_t ldx, const float* p,
                       GramKind kind, const GramGrid& g, float* slab, double* G, KState* st,
                       hipStream_t s, int64_t pstride = 0, int wshift = 0);
hipError_t launch_gram_check(const double* G, int KP, KState* st, hipStream_t s);
hipError_t launch_gram_verify(const double* G, int KP, int64_t K, float eps, const double* u,
                              const double* alpha, const double* Dx, double* bvec, KState* st,
                              hipStream_t s);
hipError_t launch_gram_solve(const double* G, int KP, int64_t K, int64_t maxiter, float tol,
                             float eps, double* alpha, double* u, float* coef, KState* st,
                             hipStream_t s);

// Other aggregators (coordinate.hip).
// ws > 0: X in the panel layout [ceil(d/W)][K][W], W = 2^ws, ldx = the panel stride.
hipError_t launch_col_mean(const float* X, int64_t K, int64_t d, int64_t ldx, float* out,
                           hipStream_t s, int ws = 0);
hipError_t launch_col_select(const float* X, int64_t K, int64_t d, int64_t ldx, int mode,
                             int64_t b, float* out, hipStream_t s, int ws = 0);
// getVarience (M:127-129): one streaming pass, part[nb] fp64 block partials.
int honest_var_blocks(int64_t d, int num_cu);
hipError_t launch_honest_var(const float* X, int64_t H, int64_t d, int64_t ldx, int wshift,
                             int nb, double* part, float* out, hipStream_t s);
// Krum: D [K][K] fp64, part [krum_slices(K, d)][K][K] fp64, score [K] fp64.
int64_t krum_slices(int64_t K, int64_t d);
hipError_t launch_krum(const float* X, int64_t K, int64_t d, int64_t ldx, int64_t kk, double* D,
                       double* part, double* score, float* out, int64_t* index, hipStream_t s,
                       int ws = 0);
// launch_krum's first two steps on their own: D (pair_dist + pair_reduce), and every row's
// score (the sum of its kk smallest distances).
hipError_t launch_krum_dist(const float* X, int64_t K, int64_t d, int64_t ldx, int ws, double* D,
                            double* part, hipStream_t s);
hipError_t launch_krum_scores(const double* D, int64_t K, int64_t kk, double* score,
                              hipStream_t s);
// The exact tier on bf16 bit patterns (rows at any 2-byte alignment, or bf16 panels): the same
// kernels with the element widened at the load, so every result is the fp32 function's on the
// widened matrix, bit for bit.  gate (nullable, device): while *gate == 0 both distance
// launches are no-ops (the MFMA tier's fallback, pairdist_bf16.hip).
hipError_t launch_krum_dist(const uint16_t* X, int64_t K, int64_t d, int64_t ldx, int ws,
                            double* D, double* part, const int* gate, hipStream_t s);
// index = the first argmin of score [K]; out = that row of X, widened.
hipError_t launch_krum_argmin_row(const double* score, int64_t K, const uint16_t* X, int64_t d,
                                  int64_t ldx, int ws, int64_t* index, float* out, hipStream_t s);
hipError_t launch_copy_row_k(const uint16_t* X, int64_t d, int64_t ldx, int ws, int64_t k,
                             float* out, hipStream_t s);
hipError_t launch_multi_krum_pick(const double* score, int64_t K, int64_t m, const uint16_t* X,
                                  int64_t d, int64_t ldx, int ws, int32_t* flag, int32_t* list,
                                  float* out, hipStream_t s);
hipError_t launch_gather_mean(const uint16_t* X, int64_t d, int64_t ldx, int ws,
                              const int32_t* list, int64_t m, float* out, hipStream_t s);
hipError_t launch_nnm_mix(const uint16_t* X, int64_t K, int64_t d, int64_t ldx, int ws,
                          const uint32_t* mask, int64_t m, float* Y, int64_t ldy, int wsy,
                          hipStream_t s);
// The MFMA tier (pairdist_bf16.hip): D~ = max(0, G_ii + G_jj - 2 G_ij) from G = X X^T on the
// bf16 matrix cores, into D [K][K] (upper triangle), with the bound |D~ - D| <=
// pairdist_mfma_beta() (rho_i + rho_j).  X: bf16 rows (16-byte aligned, ldx % 8 == 0) or bf16
// panels.  part [pairdist_mfma_slices(K, d, num_cu)][K][K] fp64, rho [K] fp64 scratch; *flag
// (device, zeroed by the launcher) is raised when a G_ii is not finite.
constexpr int kMfmaFlush = 256;    // C: columns between two flushes of the fp32 accumulators
double pairdist_mfma_beta();
int64_t pairdist_mfma_slices(int64_t K, int64_t d, int num_cu);
hipError_t launch_pairdist_mfma(const uint16_t* X, int64_t K, int64_t d, int64_t ldx, int ws,
                                int num_cu, double* part, double* rho, double* D, int* flag,
                                hipStream_t s);
// D's lower triangle from its upper one (gm_pair_dist_bf16's full symmetric output).
hipError_t launch_mirror_upper(double* D, int64_t K, hipStream_t s);
// MeaMed, Multi-Krum and Bulyan (robust.hip).
// The mean of the `keep` values of each column nearest to its lower median, over rows
// rows[0 .. n-1] of X (device int32, strictly increasing; nullptr: rows 0 .. n-1); n <= 1024.
hipError_t launch_meamed(const float* X, int64_t d, int64_t ldx, int ws, const int32_t* rows,
                         int64_t n, int64_t keep, float* out, hipStream_t s);
// The m rows of smallest score (ties to the lower index) -> flag [K], their indices
// increasing -> list [m], their fp64 mean in that order -> out.
hipError_t launch_multi_krum_pick(const double* score, int64_t K, int64_t m, const float* X,
                                  int64_t d, int64_t ldx, int ws, int32_t* flag, int32_t* list,
                                  float* out, hipStream_t s);
// Its three steps, one launch each (the tail of DnC's rounds as well): flag[i] = 1 for the m rows
// first in the order of scores; the indices with flag[i] == want, increasing -> list; the fp64
// mean of rows list[0 .. m-1] in that order -> out.
hipError_t launch_score_top_m(const double* score, int64_t K, int64_t m, int32_t* flag,
                              hipStream_t s);
hipError_t launch_flags_to_list(const int32_t* flag, int64_t K, int32_t want, int32_t* list,
                                hipStream_t s);
hipError_t launch_gather_mean(const float* X, int64_t d, int64_t ldx, int ws, const int32_t* list,
                              int64_t m, float* out, hipStream_t s);
// Bulyan's theta selection rounds on D [K][K] (upper triangle): order [theta] in selection
// order, list [theta] the same rows increasing; score [K], ord [K][K] (each row's columns by
// stable rank) and alive [K] are scratch.
hipError_t launch_bulyan_select(const double* D, int64_t K, int64_t f, int64_t theta,
                                double* score, int32_t* ord, int32_t* alive, int32_t* order,
                                int32_t* list, hipStream_t s);
// Krum through the Gram (round 5): bounds + candidates from G [KP][KP] (lb, ub [K]; cand
// [2 + maxc] int64: count, -1 (a bound not finite) or -2 (more than maxc), the indices, then
// the row of the smallest upper bound), the candidates' exact rows (at most
// krum_refine_max() per launch; part [krum_slices][m][K], Dc [m][K], score [m]), the pick.
hipError_t launch_copy_row_k(const float* X, int64_t d, int64_t ldx, int ws, int64_t k, float* out,
                             hipStream_t s);
hipError_t launch_krum_gram_select(const double* G, int KP, int64_t K, int64_t kk, double epsg,
                                   const int* bexp, int nb, int64_t d, double* lb, double* ub,
                                   int64_t maxc, int64_t* cand, hipStream_t s);
int krum_refine_max();
hipError_t launch_krum_refine(const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                              const int64_t* cidx, int m, int64_t kk, double* part, double* Dc,
                              double* score, hipStream_t s);
hipError_t launch_krum_pick(const double* score, const int64_t* cidx, int64_t m, const float* X,
                            int64_t d, int64_t ldx, int ws, int64_t* index, float* out,
                            hipStream_t s);

// The clients' local SGD chain of one federated step (clients.hip).
struct ClientChainArgs {
  const float* data;      // training set [n][ldd] fp32 (row = one flattened sample)
  int64_t ldd;
  const int64_t* labels;  // [n]
  int64_t F, C;           // features, classes (the MLP's weight is [C][F])
  const int* idx;         // [K][B] dataset rows of each client's batch
  int64_t K, B, honest;
  int attack;             // 0 none / weightflip, 1 classflip, 2 dataflip
  float gamma, wd;
  float* W;               // [C][F], updated in place (the model's weight)
  float* b;               // [C]
  float* X;               // client matrix: rows [K][ldx] or panels
  int64_t ldx;            // rows: row stride
  int64_t pstride;        // > 0: panels, elements between panels (panel width 1 << wshift)
  int wshift;
  int stage;              // (set by launch_client_chain) the batch tile staged in LDS
};
bool client_chain_supported(int64_t F, int64_t C, int64_t B);
hipError_t launch_client_chain(const ClientChainArgs& a, hipStream_t s);

// The clients' gradients at one model, folded into their momenta (client_grads.hip): one
// workgroup per client.
struct ClientGradArgs {
  const float* data;      // training set [n][ldd] fp32 (row = one flattened sample)
  int64_t ldd;
  const int64_t* labels;  // [n]
  int64_t F, C;           // features, classes (the MLP's weight is [C][F])
  const int* idx;         // [K][B] dataset rows of each client's batch
  int64_t K, B, honest;
  int attack;             // 0 none, 1 classflip, 2 dataflip
  float beta, wd;
  const float* W;         // [C][F], read only
  const float* b;         // [C], read only
  float* M;               // momentum matrix: rows [K][ldx] or panels, updated in place
  int64_t ldx;            // rows: row stride
  int64_t pstride;        // > 0: panels, elements between panels (panel width 1 << wshift)
  int wshift;
  int stage;              // (set by launch_client_grads) the batch tile staged in LDS
};
bool client_grads_supported(int64_t F, int64_t C, int64_t B);
hipError_t launch_client_grads(const ClientGradArgs& a, hipStream_t s);

// OMA / synthetic fills (oma.hip).
hipError_t launch_oma_apply(float* X, int64_t K, int64_t d, int64_t ldx, const float* hr,
                            const float* hi, const float* nr, const float* ni, hipStream_t s);
hipError_t launch_rows_to_panels(const float* X, int64_t K, int64_t d, int64_t ldx, float* P,
                                 int64_t W, int64_t pstride, hipStream_t s);
// bf16 panels from row-major fp32 (round to nearest even, as torch's .to(bfloat16)) or
// bf16 rows (pack.hip)
hipError_t launch_rows_to_panels_bf16(const void* X, bool src_f32, int64_t K, int64_t d,
                                      int64_t ldx, uint16_t* P, int64_t W, int64_t pstride,
                                      hipStream_t s);
// s-bucketing (bucket.hip): Y[i] = the fp64 mean, rounded once, of rows perm[i s] ...
// perm[min(K, (i + 1) s) - 1] of X (perm == nullptr: the identity), i < ceil(K / s).  X fp32 or
// bf16 bit patterns, row-major [K][ldx] (Wi = 0) or panels of width Wi with panel stride
// ldx; Y fp32 rows [ceil(K/s)][ldy] (Wo = 0) or panels of width Wo with panel stride ldy.
// Any alignment (4-column vector items where both sides allow, else one column per item).
hipError_t launch_bucket_means(const void* X, bool bf16, int64_t K, int64_t d, int64_t ldx,
                               int64_t Wi, const int32_t* perm, int64_t s, float* Y, int64_t ldy,
                               int64_t Wo, hipStream_t stream);
// Nearest-neighbor mixing (nnm.hip).  From D [K][K] (launch_krum_dist) the membership of every
// row's m nearest rows, itself included, in the order of score_before: mask
// [nnm_mask_words(K)] = [K][2 ceil(K / 64)] words, bit j & 31 of word j >> 5 of row i set when
// j is in N(i); list (nullable, device) [K][m] the same members increasing.  K <= 4096.
int64_t nnm_mask_words(int64_t K);
hipError_t launch_nnm_neighbors(const double* D, int64_t K, int64_t m, uint32_t* mask,
                                int32_t* list, hipStream_t s);
// Y[i] = the fp64 sum of the rows of N(i) in increasing row index, divided by m, rounded once.
// X rows (ws = 0) or panels of width 2^ws, Y rows (wsy = 0, any ldy >= d) or panels of width
// 2^wsy; any alignment; columns >= d of Y are not written.
hipError_t launch_nnm_mix(const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                          const uint32_t* mask, int64_t m, float* Y, int64_t ldy, int wsy,
                          hipStream_t s);
// DnC's spectral part on the K x n sampled sub-matrix (dnc.hip; the definition is in
// include/gmagg.h).  The sub-matrix is kept as the gathered fp32 values G [K][n] and the column
// means mu [n]: a centred element is (double)G[k][j] - mu[j], formed where it is used.
struct DncState {
  int32_t done;         // the round's iteration has ended (later launches are no-ops)
  int32_t converged;
  int32_t iters;        // applications of C^T C
  int32_t degenerate;   // a zero or non-finite norm: every score is val
  int64_t kstar;        // the row the start vector is taken from
  double val;
  double movement;      // ||v_t - v_{t-1}|| of the last application
};
constexpr int kDncBlocks = 1024;      // most blocks of the n-space reductions (bn, bm entries)
struct DncWork {
  float* G;             // [K][n]
  double* mu;           // [n]
  double* v;            // [n] the unit iterate
  double* w;            // [n] C^T C v
  double* part;         // [slices][n] partial column sums of C^T p over row slices
  double* p;            // [K] row norms^2, then C v
  double* bn;           // [kDncBlocks] block partials of ||w||^2
  double* bm;           // [kDncBlocks] block partials of ||v_t - v_{t-1}||^2
  DncState* st;
  int64_t slices, slice_rows;
};
// Row slices of the C^T p pass for a K x n sub-matrix (a function of K and n alone, so the
// summation order, and with it every bit of the result, is too): slices = ceil(K / slice_rows).
void dnc_slices(int64_t K, int64_t n, int64_t* slices, int64_t* slice_rows);
// G[k][t] = X[k][cols[t]] (cols: device int64 [n], each in [0, d); not checked), then mu.
hipError_t launch_dnc_gather(const float* X, int64_t K, int64_t ldx, int ws, const int64_t* cols,
                             int64_t n, float* G, hipStream_t s);
hipError_t launch_dnc_center(const DncWork& w, int64_t K, int64_t n, hipStream_t s);
// The start vector (the centred row of largest norm, normalised) and the round's fresh state.
hipError_t launch_dnc_start(const DncWork& w, int64_t K, int64_t n, hipStream_t s);
// `count` applications v <- C^T C v / ||.|| with the movement test against tol; no-ops once
// the state is done.
hipError_t launch_dnc_iterate(const DncWork& w, int64_t K, int64_t n, double tol, int64_t count,
                              hipStream_t s);
// score[k] = (c_k . v)^2, or the state's val for every k after a degenerate norm.
hipError_t launch_dnc_scores(const DncWork& w, int64_t K, int64_t n, double* score, hipStream_t s);
// good[i] = flag[i] (first) or good[i] & flag[i].
hipError_t launch_dnc_and_flags(int32_t* good, const int32_t* flag, int64_t K, bool first,
                                hipStream_t s);
// The covariance filter's K-space solver and weighted mean (caf.hip; the definition is in
// include/gmagg.h).  Everything but the last pass works on D [K][K] (launch_krum_dist) and
// O(K) fp64 state; the host reads CafState once per round.
struct CafState {
  int32_t loop_done;    // no further round runs (every later launch is a no-op)
  int32_t it_done;      // the round's power iteration has ended (its launches are no-ops)
  int32_t iters;        // applications of M in this round
  int32_t converged;    // the movement test passed (or ||M e_r|| == 0)
  int32_t failed;       // a non-finite norm (a zero one inside the iteration): the loop ends
  int32_t degenerate;   // ||M e_r|| == 0: lambda = 0, no iteration
  int32_t rounds;       // rounds that reached step 3
  int32_t best_round;   // t*
  int32_t recorded;     // c* has been written
  int32_t round;        // t of the round in flight
  int32_t r;            // the start row
  int32_t pad;
  double S;             // sum c_k of the round in flight
  double best;          // lambda of round t* (+inf before the first)
  double Sbest;         // S*
  double lambda;        // the last round's
  double q, sz, rz;     // p.a / 2, 1.z and rho.z of the current iterate
  double nrm, movement; // of the last application
};
struct CafHead {
  double S;             // sum of the positive weights
  int32_t m;            // rows listed
  int32_t pad;
};
struct CafWork {
  double* D;            // [K][K], both triangles after launch_caf_begin
  CafState* st;
  CafHead* head;
  double *c, *cbest;    // [K] the weights in flight, and c*
  double *p, *sp;       // [K] c / S and its square root
  double *rho;          // [K] ||u_k||^2
  double *w, *z;        // [K] the unit iterate, and sqrt(p) o w
  double* y;            // [K] the last product with D
  double* coef;         // [K] c*_k / S* of the listed rows
  int32_t* list;        // [K] the rows with c*_k > 0, increasing
};
// Carves everything but D out of `base` (nullptr: sizes only); the bytes needed.
size_t caf_layout(char* base, int64_t K, CafWork* w);
// Mirrors D's upper triangle (w.D == nullptr: no D, only the weights are wanted) and sets c = 1,
// S = K and the fresh state (loop_done when f == 0).
hipError_t launch_caf_begin(const CafWork& w, int64_t K, int64_t f, hipStream_t s);
// One round: 2 power_iters + 4 launches, all no-ops once the loop has ended.
hipError_t launch_caf_round(const CafWork& w, int64_t K, int64_t f, int64_t power_iters,
                            double tol, hipStream_t s);
// out = float(sum over the rows with c_k > 0, increasing k, of (c_k / sum of those c) x_k), the
// sum of c in caf_sum's order; rows with c_k <= 0 or NaN are not read.  Writes w.coef, w.list
// and w.head.
hipError_t launch_caf_weighted_mean(const float* X, int64_t K, int64_t d, int64_t ldx, int ws,
                                    const double* c, const CafWork& w, float* out,
                                    hipStream_t s);
// The omniscient attacks (attack.hip), in place: rows H .. K-1 of X are overwritten from the
// statistics of rows 0 .. H-1; ws = log2 of the panel width (0: rows), ldx the row or panel
// stride.  Any alignment (4-column vector items where the base and stride allow).
// Affine: every Byzantine row becomes a mu + b sigma (b == 0: a mu), rounded once to fp32 or
// bf16 (X holds bf16 bit patterns).
hipError_t launch_attack_affine(void* X, bool bf16, int64_t K, int64_t H, int64_t d, int64_t ldx,
                                int ws, double a, double b, hipStream_t stream);
// Min-max (rule 0) / min-sum (rule 1) with deviation dev (0 std, 1 unit, 2 sign), fp32: D [H][H]
// the honest rows' squared distances (launch_krum_dist on H rows); workspace mu [d], p [d],
// slab [nb][2H + 1] with nb = attack_term_blocks(d), sums [2H + 1], rb [H], gam [2] (written:
// gamma for the kernels' p, then the definition's gamma).
int attack_term_blocks(int64_t d);
hipError_t launch_attack_minmax(float* X, int64_t K, int64_t H, int64_t d, int64_t ldx, int ws,
                                int rule, int dev, const double* D, double* mu, double* p,
                                double* slab, int nb, double* sums, double* rb, double* gam,
                                hipStream_t stream);
hipError_t launch_oma_philox(float* X, int64_t K, int64_t d, int64_t ldx, int64_t d_total,
                             int64_t col_off, float sd, uint64_t seed, hipStream_t s,
                             int wshift = 0, int64_t problems = 1, int64_t pstride = 0);
hipError_t launch_fill_clients(float* X, int64_t K, int64_t d, int64_t ldx, int64_t B,
                               float mu_h, float sd_h, float mu_b, float sd_b, int64_t d_total,
                               int64_t col_off, uint64_t seed, hipStream_t s);
hipError_t launch_fill_normal(float* v, int64_t n, float mu, float sd, int64_t off,
                              uint64_t seed, hipStream_t s);

}  // namespace gmk
