/*
 * gmagg.h — C ABI of the MI355X geometric-median aggregation library
 * (libgmagg.so, built from byzantine_aircomp_amd/csrc/ for gfx950).
 *
 * This is the drop-in boundary for the reference's aggregation call
 *     weight_vector = aggregate(weight_f, options)          MNIST_Air_weight.py:353
 * with aggregate resolved by eval(args.agg) (MNIST_Air_weight.py:580).  Each entry
 * point below names the reference function it replaces.  Plain pointers and
 * sizes only: no torch types cross this boundary.
 *
 * Conventions
 *   - Every call returns 0 (GM_OK) or a negative GM_ERR_* code; the message of
 *     the last failure on the calling thread is gm_last_error().  Nothing aborts
 *     or throws across the ABI.
 *   - Device pointers are HIP device pointers on the context's device; the
 *     caller owns X / guess / out, the library owns its workspace.
 *   - Work is stream-ordered on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream).  gm_weiszfeld_f32 blocks only to learn whether the
 *     iteration has converged; the OMA entry points never block.
 *   - A context is used by one host thread at a time.  Calls on one context may
 *     use different streams: each call makes its stream wait for the previous
 *     call's queued work on the context's workspace (an event), so they never
 *     race; for concurrent aggregations use one context per stream.
 *
 * Layout: X is row-major [K][ldx] fp32, row k = client k's flattened update
 * (model.parameters() order, MNIST_Air_weight.py:206-209), ldx >= d — the
 * reference's own torch.stack layout.  gm_weiszfeld_f32 also takes the panel
 * layout (gm_opts.layout = GM_LAYOUT_PANELS): X as [ceil(d/W)][K][W] with
 * W = gm_panel_width(K) and ldx = elements between panels (>= K*W); element
 * (k, j) at X[(j/W)*ldx + k*W + j%W].  Each streaming-pass chunk is then one
 * contiguous block of HBM.
 *
 * bf16 client updates: gm_weiszfeld_bf16 reads X stored as bfloat16 (uint16_t bit
 * patterns), half the bytes per pass.  Only X is 16-bit: a bf16 value widens to fp32
 * exactly (bits << 16), and the guess, the iterates, the output and every sum are what
 * gm_weiszfeld_f32 has, so the result is gm_weiszfeld_f32's on the widened matrix up to
 * the order of the column sums.  Its panel layout is [ceil(d/W)][K][W] bf16 with
 * W = gm_panel_width_bf16(K) (twice gm_panel_width(K): the same bytes per row segment).
 */
#ifndef GMAGG_H
#define GMAGG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMAGG_ABI_VERSION 5

enum gm_status {
    GM_OK = 0,
    GM_ERR_INVALID = -1,      /* bad argument (null pointer, negative size, ...) */
    GM_ERR_HIP = -2,          /* a HIP runtime call failed */
    GM_ERR_UNSUPPORTED = -3,  /* shape / mode this build does not handle */
    GM_ERR_CALLBACK = -4,     /* a user callback (noise, all-reduce) returned non-zero */
    GM_ERR_COMM = -5          /* RCCL failure */
};

enum gm_mode {
    GM_MODE_IDEAL = 0,        /* gm2: MNIST_Air_weight.py:162-184 */
    GM_MODE_AIRCOMP = 1       /* gm + OMA2 per iteration: MNIST_Air_weight.py:131-160, 396-414 */
};

enum gm_noise_source {
    GM_NOISE_PHILOX = 0,      /* on-device Philox4x32-10, keyed (seed, iteration, global index) */
    GM_NOISE_HOST = 1         /* caller supplies the reference's draws through noise_cb */
};

enum gm_layout {
    GM_LAYOUT_ROWS = 0,       /* [K][ldx] row-major (the reference's torch.stack of rows) */
    GM_LAYOUT_PANELS = 1      /* [ceil(d/W)][K][W], W = gm_panel_width(K), ldx = panel stride;
                                 streaming, (gm2, K <= 256, W % 64 == 0) the guarded Gram, or
                                 (K <= 52 gm2 / K <= 50 gm, unsharded) the resident kernel */
};

enum gm_algo {
    GM_ALGO_AUTO = 0,
    GM_ALGO_STREAM = 1,       /* fused one-read-per-iteration streaming Weiszfeld */
    GM_ALGO_TWOPASS = 2,      /* two reads per iteration; any K */
    GM_ALGO_GRAM = 3,         /* K x K Gram on MFMA, iterations in K-space (IDEAL only, K <= 256):
                                 scaled f16 hi/lo split, 3 v_mfma_f32_32x32x16_f16 products per
                                 off-diagonal tile (2 on the diagonal); an f16 range overflow
                                 reruns the bf16 h+m split (4 products, rows) or the streaming
                                 path (panels); the result is kept only if the a-posteriori
                                 guard passes (gm_result.guard / gram_kind) */
    GM_ALGO_RESIDENT = 4,     /* small problems: X held in VGPRs, all iterations in one launch */
    GM_ALGO_GRAM_F32 = 5      /* the Gram on the exact f32-input MFMA (4x the issue cycles) */
};

/* Host-noise callback for GM_NOISE_HOST: fill the draws of Weiszfeld iteration
 * `iter` (0-based), exactly as OMA2 draws them (MNIST_Air_weight.py:401-402, 411):
 * h_re[K], h_im[K] ~ N(0, 1/2) and, when the options ask for noise,
 * noise[d_total + 1] ~ N(0, noise_var / 2) (the last element is the
 * denominator's).  Buffers are host memory owned by the library.  Return 0. */
typedef int (*gm_noise_cb)(void* user, int64_t iter, float* h_re, float* h_im, float* noise);

/* Optional d-sharding hook: sum `count` doubles in place across all shards,
 * stream-ordered on `stream`.  Return 0.  (gm_ctx_init_rccl installs a native
 * RCCL all-reduce instead.) */
typedef int (*gm_allreduce_cb)(void* user, double* dev_buf, int64_t count, void* stream);

typedef struct gm_opts {
    int64_t maxiter;          /* options['maxiter'], reference default 200 (M:136, M:167) */
    double tol;               /* options['tol'], default 1e-5; compared as fp32 like the reference */
    double eps;               /* distance floor, 1e-4 in the reference (M:151, M:178) */
    int32_t mode;             /* gm_mode */
    int32_t has_noise;        /* AIRCOMP: options['noise_var'] is not None */
    double noise_var;         /* AIRCOMP: channel-noise variance (OMA2 std = sqrt(var/2), M:410) */
    double P_max;             /* AIRCOMP: options['P_max'], default 1 (M:136) */
    uint64_t seed;            /* GM_NOISE_PHILOX key */
    int32_t noise_source;     /* gm_noise_source */
    int32_t algo;             /* gm_algo */
    gm_noise_cb noise_cb;     /* GM_NOISE_HOST */
    void* noise_user;
    int32_t check_every;      /* host convergence poll interval in iterations; 0 = auto */
    int32_t layout;           /* gm_layout of X (gm_weiszfeld_f32 and gm_weiszfeld_batched_f32) */
    /* pre_oma = 1 (gm2 only): first apply OMA(X, pre_oma_var) IN PLACE, as the reference
     * does before every non-gm aggregator when --var is set (MNIST_Air_weight.py:351-352),
     * with the draws of gm_oma_philox_f32 (batched: problem p keyed pre_oma_seed + p *
     * 0x9E3779B97F4A7C15).  The streaming path fuses it into its first pass. */
    int32_t pre_oma;
    double pre_oma_var;
    uint64_t pre_oma_seed;
} gm_opts;

enum gm_guard {
    GM_GUARD_NONE = 0,        /* no Gram result was involved */
    GM_GUARD_ACCEPTED = 1,    /* Gram-space result, a-posteriori accuracy guard passed */
    GM_GUARD_REJECTED = 2,    /* a Gram result was refused; the streaming path produced out */
    GM_GUARD_ACCEPTED_FLOOR = 3 /* accepted, with tol inside the reference's fp32 movement
                                 floor band (tol/3 < 2^-23 ||g|| <= tol): any fp32 Weiszfeld's
                                 count is decided by rounding there; iters is the exact count */
};

enum gm_exchange {
    GM_EXCHANGE_NONE = 0,      /* launch-per-pass paths: partials reduced between launches */
    GM_EXCHANGE_AGENT = 1,     /* resident grid over several XCDs: agent-scope granule stores */
    GM_EXCHANGE_XCD_LOCAL = 2, /* resident grid on ONE XCD (confirmed from XCC_ID at the
                                  check-in): granules kept in that XCD's L2 */
    GM_EXCHANGE_XCD_HIER = 3,  /* resident grid over several XCDs, gathered per XCD: each
                                  block's granules kept in its XCD's L2 for the XCD's leader,
                                  the 8 per-XCD sums exchanged agent-scope */
    GM_EXCHANGE_XCD_SPLIT = 4  /* resident grid over several XCDs, one hop: each granule stored
                                  agent-scope and L2-kept, a reader polling its own XCD's
                                  blocks from the L2-kept copies */
};

typedef struct gm_result {
    int64_t iters;            /* Weiszfeld loop bodies executed (M:145 / M:173) */
    double last_movement;     /* ||guess_t - guess_{t+1}|| of the last body (M:156 / M:180) */
    int32_t converged;        /* 1 if the loop exited through the tol test */
    int32_t algo_used;        /* gm_algo actually run */
    int32_t guard;            /* gm_guard: what the Gram accuracy guard decided */
    int32_t gram_kind;        /* Gram runs: 1 scaled f16 split (3 MFMA products), 2 bf16 split
                                 (4 products, after an f16 range overflow), 3 f32-input; else 0 */
    int32_t exchange;         /* register-resident runs: how the blocks exchanged their
                                 per-iteration partials (gm_exchange); else GM_EXCHANGE_NONE */
} gm_result;

typedef struct gm_ctx gm_ctx;

/* Context: device binding, workspace, optional shard description. */
int gm_ctx_create(int device, gm_ctx** out);
int gm_ctx_destroy(gm_ctx* ctx);

/* d-sharding: this shard holds global columns [d_offset, d_offset + d_local) of
 * a d_total-long update; per-iteration partial sums go through the all-reduce.
 * Every rank must pass the same K, d_total and options; the library takes every
 * decision that changes the sequence of collectives (Gram or streaming, the poll
 * interval) from those global values, so a shorter or ragged last shard issues
 * exactly the all-reduces the others do.  For AUTO's Gram choice (gm2, K <= 256,
 * d_total >= 2^18, d_total % 4 == 0) each shard must also be 16-byte aligned with
 * d_local and ldx multiples of 4 — always true for contiguous shards cut at
 * 256-column boundaries (byzantine_aircomp_amd.sharded.shard_range). */
int gm_ctx_set_shard(gm_ctx* ctx, int64_t d_total, int64_t d_offset);
int gm_ctx_set_allreduce(gm_ctx* ctx, gm_allreduce_cb fn, void* user);
/* Native RCCL all-reduce over xGMI: `unique_id` is the 128-byte ncclUniqueId
 * made by rank 0 (gm_rccl_get_unique_id) and shared by the caller. */
int gm_rccl_get_unique_id(void* unique_id_128);
int gm_ctx_init_rccl(gm_ctx* ctx, const void* unique_id_128, int nranks, int rank);

/* gm2 / gm: Weiszfeld geometric median of the K rows of X.
 * Replaces gm2(wList, options) (MNIST_Air_weight.py:162-184) with
 * opts->mode = GM_MODE_IDEAL, and gm(wList, options) (MNIST_Air_weight.py:131-160,
 * calling OMA2 M:396-414 each iteration) with GM_MODE_AIRCOMP.
 * guess0 = options['guess'] (d floats); out receives the returned iterate
 * (d floats).  maxiter == 0 copies guess0 to out. */
int gm_weiszfeld_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx,
                     const float* guess0, float* out, const gm_opts* opts,
                     gm_result* result, void* stream);

/* gm2 on fp32 panels at 512 < K <= 1024 (the streaming path): once the Weiszfeld coefficients
 * have settled, a STEP pass may run as a CORRECTION on a bf16 copy of X (the shadow) that the
 * context owns: 2 K d more bytes of device memory, written by one of the exact passes; X itself
 * is never written.  With the most recent exact pass as base (coefficients c^b, output G, exact
 * distances D^b), g' = G + sum_k (c_k - c^b_k) bf16(x_k) and the distances follow in the same
 * read, so the pass moves half the bytes.  It runs only while |c_k - c^b_k| <= theta c^b_k for
 * every k (decided on the device from the all-reduced sums, the same on every rank of a
 * sharded context), theta = 2^9 eps / 4 with eps the tile's per-element bound (59 * 2^-24), so
 * the result agrees with the exact passes' to a quarter of that bound; otherwise the pass is
 * exact, as every pass is when the shadow cannot be allocated.
 * GMAGG_DELTA (environment, read once per process): 0 never; 1 at any size, the shadow written
 * by the second STEP whatever the cost rule says; by default the path is taken where
 * 4 K d_total >= 2 GiB and the shadow is written once the coefficients have begun to settle.
 * gm_delta_last_info: info[3] = {correction passes, bit t set when STEP t was one (t < 32),
 * gm_delta_status} of this context's last gm_weiszfeld_f32 call that ran the streaming loop. */
enum gm_delta_status {
  GM_DELTA_OFF = 0,          /* not eligible, below the size threshold or turned off */
  GM_DELTA_ARMED = 1,        /* the loop could take correction passes (info[0] says how many) */
  GM_DELTA_NO_SHADOW = 2     /* eligible, but the shadow could not be allocated: exact passes */
};
int gm_delta_last_info(gm_ctx* ctx, int64_t* info);

/* Panel width W of the GM_LAYOUT_PANELS layout for K clients (the streaming
 * tile's chunk width: 32 columns at 512 < K <= 1024); 0 if K is unsupported. */
int64_t gm_panel_width(int64_t K);

/* gm2 / gm on client updates stored as bf16: X holds bfloat16 bit patterns, row-major
 * [K][ldx] (opts->layout = GM_LAYOUT_ROWS) or panels [ceil(d/W)][K][W] with
 * W = gm_panel_width_bf16(K) and ldx = elements between panels (>= K*W, a multiple of 8).
 * guess0 and out are fp32; opts, the modes (gm2 and AirComp gm, Philox or host draws),
 * maxiter == 0 and gm_ctx_pass_timing are as for gm_weiszfeld_f32.  It runs the fused
 * streaming pass only: result->algo_used is GM_ALGO_STREAM.
 * GM_ERR_UNSUPPORTED (with a message) for: an algo other than GM_ALGO_AUTO / GM_ALGO_STREAM;
 * pre_oma; a sharded or collective context (gm_ctx_set_shard, gm_ctx_set_allreduce,
 * gm_ctx_init_rccl); K > 2048; a row-major X that is not 16-byte aligned with d and ldx
 * multiples of 8 (pack it: gm_rows_to_panels_bf16).  X is never written. */
int gm_weiszfeld_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                      const float* guess0, float* out, const gm_opts* opts,
                      gm_result* result, void* stream);

/* Panel width W of gm_weiszfeld_bf16's panel layout for K clients (the bf16 streaming
 * tile's chunk width: 64 columns at 512 < K <= 1024); 0 if K is unsupported. */
int64_t gm_panel_width_bf16(int64_t K);

/* Centered clipping (Karimireddy, He & Jaggi, "Learning from History for Byzantine Robust
 * Optimization", ICML 2021, Algorithm 2) — not one of the reference's aggregators.  From
 * v_0 = guess0, maxiter times
 *     v_{l+1} = v_l + (1/K) sum_k (x_k - v_l) min(1, tau / ||x_k - v_l||)
 * computed as sum_k c_k x_k + a v_l on the fused streaming pass: dist_k = sqrt(D_k) in fp64
 * with no distance floor (dist_k = 0 is unclipped), c_k = (float)(lambda_k / K),
 * a = (float)(1 - sum_k (double)c_k).  One read of X per iteration, maxiter + 1 in all. */
typedef struct gm_cclip_opts {
    double tau;               /* clipping radius, > 0; +inf gives the plain mean step */
    int64_t maxiter;          /* clipping iterations; 0 copies guess0 to out */
    double tol;               /* stop early once the fp32 movement ||v_l - v_{l+1}|| <= tol (the
                                 new iterate is returned); a negative tol never stops */
    int32_t layout;           /* gm_layout of X */
    int32_t check_every;      /* host poll interval in iterations; 0 = auto */
} gm_cclip_opts;

typedef struct gm_cclip_result {
    int64_t iters;            /* iterations executed */
    double last_movement;     /* ||v_l - v_{l+1}|| of the last one (NaN if none ran) */
    int32_t converged;        /* 1 if the loop exited through the tol test */
    int32_t clipped;          /* clients with dist_k > tau at the last iteration's coefficients */
} gm_cclip_result;

/* fp32 X, row-major [K][ldx] or panels (gm_panel_width(K), as gm_weiszfeld_f32); K > 2048
 * row-major runs the two-pass kernels.  Works on a d-sharded context (gm_ctx_set_shard + an
 * all-reduce) exactly as gm2: every rank derives the same c_k, a and stop decision from the
 * reduced sums.  gm_ctx_pass_timing counts one pass per iteration.
 * GM_ERR_INVALID: tau NaN or <= 0 (nothing is written). */
int gm_cclip_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx,
                 const float* guess0, float* out, const gm_cclip_opts* opts,
                 gm_cclip_result* result, void* stream);
/* bf16 X (bit patterns; layouts and panel width as gm_weiszfeld_bf16), fp32 guess0 / out.
 * GM_ERR_UNSUPPORTED (with a message) for a sharded or collective context, K > 2048, or a
 * row-major X that is not 16-byte aligned with d and ldx multiples of 8. */
int gm_cclip_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                  const float* guess0, float* out, const gm_cclip_opts* opts,
                  gm_cclip_result* result, void* stream);

/* Batched independent problems (BASELINE config C5, the draw.ipynb-style sweep
 * over many small aggregations): problem p aggregates the K rows at X + p*ldp
 * (row stride ldx) from guess0 + p*ldg into out + p*ldo.  One launch per pass
 * covers all P problems; each stops at its own tol test (gm2) or runs maxiter
 * (gm).  Options are shared; GM_MODE_AIRCOMP uses Philox only, problem p keyed
 * with seed + p * 0x9E3779B97F4A7C15.  results: P entries or NULL.  Not
 * combinable with d-sharding.  opts->layout = GM_LAYOUT_PANELS: problem p at X + p*ldp
 * is in the panel layout [ceil(d/W)][K][W] (W = gm_panel_width(K)) with panel stride
 * ldx >= K*W, ldp >= ceil(d/W)*ldx; the same results as the row-major call. */
int gm_weiszfeld_batched_f32(gm_ctx* ctx, const float* X, int64_t P, int64_t K, int64_t d,
                             int64_t ldx, int64_t ldp, const float* guess0, int64_t ldg,
                             float* out, int64_t ldo, const gm_opts* opts, gm_result* results,
                             void* stream);

/* The reference's other aggregators (MNIST_Air_weight.py:186-204), out[d]:
 *   gm_mean_f32          mean(wList, options)          M:186-187
 *   gm_median_f32        median(wList, options)        M:194-195 (lower median), K <= 2048
 *   gm_trimmed_mean_f32  trimmed_mean(wList, options)  M:189-192, trim = int(0.1 K) per end, K <= 2048
 *   gm_krum_f32          Krum(wList, options)          M:197-204, K <= 4096; *index = chosen row
 * Larger K returns GM_ERR_UNSUPPORTED. */
int gm_mean_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx, float* out,
                void* stream);
int gm_median_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx, float* out,
                  void* stream);
int gm_trimmed_mean_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx,
                        int64_t trim, float* out, void* stream);
int gm_krum_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx,
                int64_t honest_size, float* out, int64_t* index, void* stream);
/* The same four on client updates in the panel layout (GM_LAYOUT_PANELS: X as
 * [ceil(d/W)][K][W], W = gm_panel_width(K), panel_stride >= K*W): identical results. */
int gm_mean_panels_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t panel_stride,
                       float* out, void* stream);
int gm_median_panels_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t panel_stride,
                         float* out, void* stream);
int gm_trimmed_mean_panels_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d,
                               int64_t panel_stride, int64_t trim, float* out, void* stream);
int gm_krum_panels_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t panel_stride,
                       int64_t honest_size, float* out, int64_t* index, void* stream);
/* mean, median and trimmed mean of bf16 client updates (coordinate_bf16.hip): X holds bfloat16
 * bit patterns, layout GM_LAYOUT_ROWS ([K][ldx], ldx >= d, any 2-byte alignment; 16-byte loads
 * where the base is 16-byte aligned and ldx % 8 == 0) or GM_LAYOUT_PANELS ([ceil(d/W)][K][W],
 * W = gm_panel_width_bf16(K), ldx = panel stride >= K*W).  X is never written; out[d] is fp32.
 * The results are the fp32 functions' definitions on the widened values (exact): the median is
 * the widened element of rank (K-1)/2 (NaN for a column that holds a NaN), the mean and the
 * trimmed mean (0 <= 2 trim <= K-1) are fp64 sums rounded once, and both layouts and every
 * alignment return the same bits.  The selections work on 16-bit order keys: at most 16
 * counting steps per rank, or two 256-bin histograms.  GM_ERR_INVALID: a NULL argument, K < 1, d < 0, an unknown layout,
 * ldx < d on rows, a panel stride < K*W, trim out of range.  GM_ERR_UNSUPPORTED: K > 2048 for
 * the median and the trimmed mean (the mean has no limit on rows), or panels at a K without a
 * bf16 panel width.  A refused call writes nothing. */
int gm_mean_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                 int32_t layout, float* out, void* stream);
int gm_median_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                   int32_t layout, float* out, void* stream);
int gm_trimmed_mean_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                         int32_t layout, int64_t trim, float* out, void* stream);

/* Krum's algorithm (round 5).  K <= 256 on large inputs (AUTO: K >= 64 and K^2 d >= 2^29;
 * env GMAGG_KRUM=0 exact only, 1 Gram wherever eligible): the scaled-f16 Gram MFMA kernel
 * gives every pairwise distance within a stated bound, rows whose score bounds reach the
 * smallest upper bound are recomputed with the exact path's arithmetic, and the index equals
 * the exact path's.  gm_krum_last_info: info[3] = {algorithm, candidates recomputed,
 * reason} of this context's last Krum call. */
enum gm_krum_algo { GM_KRUM_EXACT = 0, GM_KRUM_GRAM = 1 };
enum gm_krum_reason {
  GM_KRUM_REASON_OK = 0,             /* the Gram path ran */
  GM_KRUM_REASON_NOT_CHOSEN = 1,     /* exact by choice (GMAGG_KRUM, AUTO's size rule) */
  GM_KRUM_REASON_NOT_ELIGIBLE = 2,   /* K > 256, misaligned rows, d or ldx % 4, panel width */
  GM_KRUM_REASON_GRAM_NONFINITE = 3, /* the f16 range was exceeded or the input is not finite */
  GM_KRUM_REASON_CANDIDATES = 4      /* more than 128 candidates, or a bound not finite */
};
int gm_krum_last_info(gm_ctx* ctx, int64_t* info);

/* Three more robust aggregators on the same machinery (fp32 only; one entry each, `layout`
 * GM_LAYOUT_ROWS: X as [K][ldx], ldx >= d, any alignment; GM_LAYOUT_PANELS: X as
 * [ceil(d/W)][K][W], W = gm_panel_width(K), ldx = panel stride >= K*W).  X is never written;
 * results are bit-identical for both layouts and every alignment.
 *
 * gm_meamed_f32: mean-around-median (Xie, Koyejo & Gupta 2018).  Per column, over the rows
 * used (rows[0 .. n_rows-1], or all K when rows is NULL, then n_rows == K):
 *   values are read as x + 0.0f (-0 becomes +0); med = their lower median (rank
 *   (n_rows - 1) / 2, gm_median_f32's); dev_k = |x_k - med| as one fp32 subtraction; the
 *   `keep` smallest dev are kept, ties at the threshold to the lower row index, a NaN dev
 *   (inf - inf) ranking after +inf; out = the fp64 sum of the kept values in a fixed order,
 *   divided by keep, rounded to fp32 once.  A NaN among the rows used gives NaN; infinities
 *   follow IEEE through the subtraction and the sum.
 *   rows   device int32[n_rows], strictly increasing indices into [0, K), or NULL.  It is NOT
 *          validated: an entry outside [0, K) reads out of bounds.
 * One stream-ordered kernel, one read of the rows used, no workspace, no host synchronisation.
 * K <= 1024.
 *
 * gm_multi_krum_f32: Multi-Krum (Blanchard et al. 2017).  score_i = gm_krum_f32's (the sum of
 * the honest - 1 smallest squared distances of row i, itself included), always on the exact
 * distance path (GMAGG_KRUM is ignored); the m rows of smallest score are selected, ties to
 * the lower row index; out = per column the fp64 sum of the selected rows in increasing row
 * index, divided by m, rounded once.  m == 1 is gm_krum_f32's exact-path row, bit for bit.
 * K <= 4096, 2 <= honest <= K + 1, 1 <= m <= K.
 *   selected   host int32[m], the selected rows increasing, or NULL.  Non-NULL blocks until
 *              the stream has run the call, like gm_krum_f32's index.
 *
 * gm_bulyan_f32: Bulyan (El Mhamdi, Guerraoui & Rouault 2018) with f = K - honest, K >= 4f + 3,
 * theta = K - 2f, beta = theta - 2f.  Stage 1, theta rounds on the set S of remaining rows
 * (all rows at first): the score of a row of S is the sum of its max(1, |S| - f - 1) smallest
 * squared distances to rows of S, itself included; the row of smallest score (ties to the
 * lower index) is selected and leaves S.  The distances are computed once (the exact path).
 * Stage 2: gm_meamed_f32 with keep = beta over the selected rows in increasing row index
 * (f == 0: the column mean).  K <= 1024.
 *   selected   host int32[theta], the selected rows in selection order, or NULL (blocks as
 *              above).
 *
 * GM_ERR_INVALID (nothing written): a NULL ctx, X or out, K < 1, d < 0, an unknown layout, ldx
 * too small for its layout, keep / n_rows / m / honest out of range, K < 4f + 3.
 * GM_ERR_UNSUPPORTED (with a message): K above the limit, panel input whose K has no panel
 * width.  d == 0 returns GM_OK.  Multi-Krum and Bulyan use the context's workspace
 * (stream-ordered with the other calls on it). */
int gm_meamed_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                  const int32_t* rows, int64_t n_rows, int64_t keep, float* out, void* stream);
int gm_multi_krum_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx,
                      int32_t layout, int64_t honest, int64_t m, float* out, int32_t* selected,
                      void* stream);
int gm_bulyan_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                  int64_t honest, float* out, int32_t* selected, void* stream);

/* getVarience(w_local, honestSize) (MNIST_Air_weight.py:127-129): the mean over the
 * first `honest` rows of ||x_k - mean||^2, written as ONE fp32 value to the device
 * pointer `out`; one streaming pass over the honest rows (fp64 sums). */
int gm_honest_variance_f32(gm_ctx* ctx, const float* X, int64_t honest, int64_t d, int64_t ldx,
                           float* out, void* stream);
/* The same on a client matrix of K rows in the panel layout (GM_LAYOUT_PANELS). */
int gm_honest_variance_panels_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t honest,
                                  int64_t d, int64_t panel_stride, float* out, void* stream);

/* OMA(message, noise_var): in-place per-client equalised AWGN
 * (MNIST_Air_weight.py:385-394), draws from on-device Philox keyed by `seed`. */
int gm_oma_philox_f32(gm_ctx* ctx, float* X, int64_t K, int64_t d, int64_t ldx,
                      double noise_var, uint64_t seed, void* stream);

/* OMA on P independent problems X[p] = X + p*pstride ([K][ldx] each; BASELINE C5,
 * the reference's `--agg gm2 --var v` pre-noise, MNIST_Air_weight.py:351-352):
 * problem p's draws are gm_oma_philox_f32's with seed + p * 0x9E3779B97F4A7C15. */
int gm_oma_philox_batched_f32(gm_ctx* ctx, float* X, int64_t P, int64_t K, int64_t d, int64_t ldx,
                              int64_t pstride, double noise_var, uint64_t seed, void* stream);

/* Batched OMA on P problems in the panel layout: problem p at X + p*pstride is
 * [ceil(d/W)][K][W] with panel_stride >= K*W; the same draws as
 * gm_oma_philox_batched_f32 on the row-major problems. */
int gm_oma_philox_batched_panels_f32(gm_ctx* ctx, float* X, int64_t P, int64_t K, int64_t d,
                                     int64_t panel_stride, int64_t pstride, double noise_var,
                                     uint64_t seed, void* stream);

/* The same OMA on client updates in the panel layout (GM_LAYOUT_PANELS: X as
 * [ceil(d/W)][K][W], W = gm_panel_width(K), panel_stride >= K*W): identical draws
 * and results to gm_oma_philox_f32 on the row-major matrix; padding untouched. */
int gm_oma_philox_panels_f32(gm_ctx* ctx, float* X, int64_t K, int64_t d, int64_t panel_stride,
                             double noise_var, uint64_t seed, void* stream);

/* Caller-side packing (row f2): copy the row-major client matrix X[K][ldx] (the
 * reference's flatten_list stack, MNIST_Air_weight.py:206-209) into the panel layout
 * P = [ceil(d/W)][K][W] with panel_stride >= K*W elements between panels
 * (GM_LAYOUT_PANELS).  Padding columns >= d are not written. */
int gm_rows_to_panels_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx,
                          float* P, int64_t W, int64_t panel_stride, void* stream);

/* The same packing into bf16 panels (gm_weiszfeld_bf16's layout, W = gm_panel_width_bf16(K)),
 * from row-major fp32 — rounded to nearest even, the bits of torch's .to(torch.bfloat16)
 * for finite values and infinities (NaN becomes 0x7FC0) — or from row-major bf16.
 * Padding columns >= d are not written. */
int gm_rows_to_panels_bf16_from_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d,
                                    int64_t ldx, uint16_t* P, int64_t W, int64_t panel_stride,
                                    void* stream);
int gm_rows_to_panels_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                           uint16_t* P, int64_t W, int64_t panel_stride, void* stream);

/* s-bucketing (Karimireddy, He & Jaggi, "Byzantine-Robust Learning on Heterogeneous Datasets
 * via Bucketing", ICLR 2022), the pre-step of every aggregator above on non-iid clients:
 *     Y[i] = mean of rows perm[i*s] .. perm[min(K, (i+1)*s) - 1] of X,   i < Kb = ceil(K / s)
 * (the last bucket is shorter when s does not divide K; s >= K gives one bucket).  Each
 * element is the fp64 sum of its bucket in that order, divided by the bucket's row count and
 * rounded to fp32 once; NaN and infinities propagate by IEEE rules.  The order is fixed, so the
 * result is bit-identical for every input layout, output layout and alignment.
 *   perm   device int32[K], or NULL for the identity.  It MUST be a permutation of 0..K-1:
 *          the kernel does not check it, and an entry outside [0, K) reads out of bounds.
 *   X      fp32 (gm_bucket_means_f32) or bfloat16 bit patterns (gm_bucket_means_bf16, widened
 *          exactly), layout_in GM_LAYOUT_ROWS ([K][ldx], ldx >= d, any alignment, K < 2^31)
 *          or GM_LAYOUT_PANELS ([ceil(d/W)][K][W], W = gm_panel_width(K) resp.
 *          gm_panel_width_bf16(K), ldx = panel stride >= K*W).  Never written.
 *   Y      fp32, layout_out GM_LAYOUT_ROWS ([Kb][ldy], ldy >= d) or GM_LAYOUT_PANELS
 *          ([ceil(d/Wo)][Kb][Wo], Wo = gm_panel_width(Kb), ldy = panel stride >= Kb*Wo;
 *          padding columns >= d of the last panel are not written).
 * One stream-ordered kernel that reads K*d elements and writes Kb*d floats: no workspace, no
 * host synchronisation.  GM_ERR_INVALID (nothing written): a NULL ctx, X or Y, K < 1, d < 0,
 * s < 1, an unknown layout, ldx or ldy too small for its layout.  GM_ERR_UNSUPPORTED (with a
 * message): panel input whose K, or panel output whose Kb, has no panel width.  d == 0
 * returns GM_OK.  Bucketing is column-local: on a d-sharded matrix every rank buckets its own
 * columns with the same perm. */
int gm_bucket_means_f32 (gm_ctx* ctx, const float*    X, int64_t K, int64_t d, int64_t ldx,
                         int32_t layout_in, const int32_t* perm, int64_t s, float* Y, int64_t ldy,
                         int32_t layout_out, void* stream);
int gm_bucket_means_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                         int32_t layout_in, const int32_t* perm, int64_t s, float* Y, int64_t ldy,
                         int32_t layout_out, void* stream);

/* Nearest-neighbor mixing, NNM (Allouah, Farhadkhani, Guerraoui, Gupta, Pinot & Stephan, "Fixing
 * by Mixing: A Recipe for Optimal Byzantine ML under Heterogeneity", AISTATS 2023, Algorithm 1),
 * the pre-step of every aggregator above under heterogeneity: every row is replaced by the mean
 * of its m = K - f nearest rows, itself included.  Y has K rows; X is fp32 [K, d], never written;
 * 0 <= f <= K - 1.
 *   1. Distances.  D[i][j] is the exact path's squared distance (gm_multi_krum_f32's: fp32
 *      differences, fp32 squares summed per 32-column stage, fp64 across stages), with
 *      D[i][i] = 0 whatever the row holds.
 *   2. Neighbours.  N(i) is the m rows j first in the order of (D[i][j], j): smaller distance
 *      first, NaN last, ties to the lower index.  i is in N(i) unless m or more rows of lower
 *      index lie at distance exactly 0 (copies of row i: the mean is the same whichever copy is
 *      taken).  A NaN or +-inf distance is ranked by the same rule.
 *   3. Mixing.  Y[i][j] = (sum over k in N(i) of X[k][j]) / m: the fp64 sum of exactly those m
 *      terms, divided in fp64, rounded to fp32 once.  A NaN term gives NaN, infinities follow
 *      IEEE; a row outside N(i) contributes nothing, whatever it holds.
 *   4. The terms are added in increasing k, so the result is a function of (K, d, N) only:
 *      bit-identical for rows, panels and every alignment of X and Y.  (The complement form,
 *      column sum minus the excluded rows, is not used: it cancels when the excluded rows are
 *      the huge Byzantine ones.)
 *   X          layout_in GM_LAYOUT_ROWS ([K][ldx], ldx >= d, any alignment) or GM_LAYOUT_PANELS
 *              ([ceil(d/W)][K][W], W = gm_panel_width(K), ldx = panel stride >= K*W).
 *   Y          layout_out likewise with ldy (rows: any ldy >= d); columns >= d are not written.
 *   neighbors  device int32 [K][K - f], each row's members increasing, or NULL.
 * Stream-ordered on the context's workspace like gm_multi_krum_f32; no host synchronisation.
 * GM_ERR_INVALID (nothing written): a NULL ctx, X or Y, K < 1, d < 0, f outside [0, K - 1], an
 * unknown layout, ldx or ldy too small for its layout.  GM_ERR_UNSUPPORTED (with a message):
 * K > 4096, a panel layout whose K has no panel width, a d-sharded or collective context (the
 * distances would need a K x K all-reduce).  d == 0 returns GM_OK before any device call. */
int gm_nnm_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout_in,
               int64_t f, float* Y, int64_t ldy, int32_t layout_out, int32_t* neighbors,
               void* stream);

/* Krum, Multi-Krum and NNM on bf16 client updates (pairdist_bf16.hip).  X holds bfloat16 bit
 * patterns, layout GM_LAYOUT_ROWS ([K][ldx], ldx >= d, any 2-byte alignment) or GM_LAYOUT_PANELS
 * ([ceil(d/W)][K][W], W = gm_panel_width_bf16(K), ldx = panel stride >= K*W); never written.
 * The outputs are fp32 as for the _f32 entries (gm_nnm_bf16's Y: rows, or fp32 panels of width
 * gm_panel_width(K)).  dist_mode chooses how the K x K squared distances are made:
 *
 *   GM_DIST_EXACT  the fp32 entries' kernels with each element widened at the load (exact).
 *     Every result (the selected rows, the index, the neighbour lists, out, Y) is the _f32
 *     entry's on the widened matrix, bit for bit, for both layouts and every alignment.
 *     (gm_krum_bf16 always takes the exact distance path, whose index the fp32 Gram path
 *     reproduces by construction.)
 *
 *   GM_DIST_MFMA   D~_ij = max(0, G_ii + G_jj - 2 G_ij), D~_ii = 0, from G = X X^T on the bf16
 *     matrix cores: exact products, fp32 accumulators added into fp64 every C = 256 columns,
 *     per-slice fp64 partials summed in a fixed order (no atomics: the same bits on every run).
 *     With D and rho_i = ||x_i||^2 in exact arithmetic on the widened values,
 *         |D~_ij - D_ij| <= beta (rho_i + rho_j),   beta = (17/8) C 2^-23 = 6.49e-5 <= 2^-13
 *     (derivation: pairdist_bf16.hip).  Every tile uses the same slices, flush boundaries and
 *     instruction order, so bit-identical rows get D~ = 0 between them and equal D~ towards
 *     every third row, and ties go to the lower index as on the exact tier.  The scores, the
 *     neighbour ranking and the closing passes are unchanged; out / Y are sums of the rows
 *     themselves, so only the SELECTION can differ from the exact tier, and only between rows
 *     whose scores or distances lie within the bound.
 *     Not eligible (rows not 16-byte aligned, or ldx % 8 != 0): the exact tier runs, reason
 *     GM_DIST_REASON_NOT_ELIGIBLE.  A G_ii that is not finite (a NaN, an infinity, or a square
 *     that overflows fp32) raises a device flag under which the exact tier's launches, always
 *     enqueued behind, run instead of returning at once: the result is the exact tier's, bit
 *     for bit, with no host synchronisation; reason GM_DIST_REASON_NONFINITE.
 *
 * gm_pair_dist_bf16 / gm_pair_dist_f32 write the distance matrix on its own: D device fp64
 * [K][K], full symmetric (fp32: the exact path).
 * gm_dist_last_info: info[4] = {tier that ran, reason, column slices S, flush width C in
 * columns (32: the exact tier's fp32 stage)} of this context's last call of one of the bf16
 * entries, *beta (nullable) the bound's constant.  It waits for the stream of that call.
 * Limits as the _f32 entries: K <= 4096; d-sharded and collective contexts are refused
 * (GM_ERR_UNSUPPORTED); d == 0 returns GM_OK (gm_krum_bf16: *index = 0). */
enum gm_dist_mode { GM_DIST_EXACT = 0, GM_DIST_MFMA = 1 };
enum gm_dist_reason {
  GM_DIST_REASON_OK = 0,              /* the tier asked for ran (MFMA) */
  GM_DIST_REASON_REQUESTED_EXACT = 1, /* exact by request */
  GM_DIST_REASON_NOT_ELIGIBLE = 2,    /* MFMA asked for on misaligned rows or ldx % 8 != 0 */
  GM_DIST_REASON_NONFINITE = 3        /* MFMA asked for, a G_ii not finite: the exact tier ran */
};
int gm_krum_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                 int32_t layout, int64_t honest_size, int32_t dist_mode, float* out,
                 int64_t* index, void* stream);
int gm_multi_krum_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                       int32_t layout, int64_t honest, int64_t m, int32_t dist_mode, float* out,
                       int32_t* selected, void* stream);
int gm_nnm_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                int32_t layout_in, int64_t f, int32_t dist_mode, float* Y, int64_t ldy,
                int32_t layout_out, int32_t* neighbors, void* stream);
int gm_pair_dist_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                      int32_t layout, int32_t dist_mode, double* D, void* stream);
int gm_pair_dist_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx,
                     int32_t layout, double* D, void* stream);
int gm_dist_last_info(gm_ctx* ctx, int64_t* info, double* beta);

/* Divide-and-Conquer, DnC (Shejwalkar & Houmansadr, "Manipulating the Byzantine: Optimizing Model
 * Poisoning Attacks and Defenses for Federated Learning", NDSS 2021, Algorithm 2): spectral
 * filtering on sampled coordinates, the defence the min-max / min-sum attacks above were
 * published with.
 *
 * Inputs:
 * - X, with K rows
 * - f = K - honestSize
 * - `iters` >= 1
 * - `remove` = q >= 0 rows per round
 * - per round t, a strictly increasing list J_t of n distinct columns, 1 <= n <= d
 *
 * Per round, all in fp64 on the fp32 values widened exactly:
 *
 * 1. mu_j = (sum_k x_kj) / K, summed in row order, for j in J_t.  c_kj = x_kj - mu_j.
 * 2. v is the top right singular vector of C = (c_kj), found by power iteration on C^T C or,
 *    equivalently, on C C^T.  Both are positive semidefinite, so the iterate never flips sign
 *    and no sign alignment is needed.
 *    - The start vector is yours to choose.  It must be deterministic and must not be the
 *      all-ones vector in K-space: the columns are centred, so that vector lies in the null
 *      space.  Document the choice.
 *    - Stop when the unit iterate moves by ||u_t - u_{t-1}||_2 <= `power_tol` (default 1e-10)
 *      or after `power_iters` (default 100) iterations.
 *    - A zero or non-finite norm ends the round at once, with every score equal to that value
 *      (0 or NaN).
 * 3. s_k = (sum_j c_kj v_j)^2.
 * 4. kept_t is the K - q rows first in the order (s ascending, NaN last, ties to the lower row
 *    index).  This is score_before's order in robust.hip.
 *
 * Then good = the intersection of the kept_t.  For each column, out is the fp64 sum of the good
 * rows in increasing row index, divided by |good| and rounded to fp32 once.  A single good row
 * is returned as itself.  This is exactly what gather_mean does.
 *
 * With q = 0 there is no spectral work and no column draw.  The result is the column mean of
 * all rows, bit for bit what `mean` returns.
 *
 * The result and every reported quantity are bit-identical for rows, panels and every
 * alignment.  The gathered values are the same in each case, so this is required, not hoped
 * for.
 *
 * The choices this implementation makes within that text:
 *   iteration  on C^T C, in the n-space of the sampled columns: v_t = C^T (C v_{t-1}) / ||.||, one
 *              "iteration" being one such application; the scores are (C v_t)^2 of the last
 *              iterate, converged or not.
 *   start      v_0 = c_r / ||c_r||, r the row of largest ||c_k||^2 (a NaN norm first, ties to
 *              the lower index): a vector of C's row space, which a row that stands out dominates.
 *              ||c_r|| zero or non-finite is the zero / non-finite norm of step 2 (all rows equal
 *              on J_t: every score 0; a NaN in a sampled column: every score NaN; an infinite
 *              norm scores +inf), with 0 iterations reported, converged = 1 for the zero norm
 *              only.
 *   sums       mu_j from 0.0 in row order; every other sum in a fixed order that depends on
 *              (K, n) alone.
 *
 *   X          fp32, layout GM_LAYOUT_ROWS ([K][ldx], ldx >= d, any alignment) or GM_LAYOUT_PANELS
 *              ([ceil(d/W)][K][W], W = gm_panel_width(K), ldx = panel stride >= K*W).  Never
 *              written; nothing at or past column d is read.
 *   columns    device int64 [iters][n], row t = J_t.  NOT validated: an entry outside [0, d)
 *              reads out of bounds.  Unused (may be NULL) when remove == 0.
 *   out        device fp32 [d].
 *   scores     device double [iters][K], round t's s_k (zeros when remove == 0).
 *   good       host int32 [K]: the good rows, increasing, in its first *n_good entries.
 *   niter, converged   host int32 [iters]: per round the iterations run and whether the movement
 *              test passed.
 * Uses the context's workspace (stream-ordered with the other calls on it): 4 K n bytes for the
 * sub-matrix plus O(n + K).  With remove > 0 the call blocks until the stream has run the
 * selection (the host reads the iteration's state and the good rows); the final mean is queued
 * behind it.
 * GM_ERR_INVALID (nothing written): a NULL pointer, K < 2, d < 0, an unknown layout, iters < 1,
 * remove < 0, remove * iters >= K, power_iters < 1, power_tol not >= 0, a rows layout with
 * ldx < d (a panel stride < K*W) and, with remove > 0, n < 1 or n > d.  GM_ERR_UNSUPPORTED (with a
 * message): K > 4096, K * n > 2^27 sampled elements, a panel layout whose K has no panel width, a
 * d-sharded or collective context. */
int gm_dnc_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
               const int64_t* columns, int64_t n, int64_t iters, int64_t remove,
               int64_t power_iters, double power_tol, float* out, double* scores, int32_t* good,
               int64_t* n_good, int32_t* niter, int32_t* converged, void* stream);

/* CAF, the covariance filter: the down-weighting spectral filter of robust mean estimation
 * (Diakonikolas, Kamath, Kane, Li, Moitra & Stewart, "Being Robust (in High Dimensions) Can Be
 * Practical", ICML 2017), which ByzFL ships as the Covariance-bound Agnostic Filter and attributes
 * to Allouah, Guerraoui & Stephan (2025).  It looks at the top eigen-direction of the weighted
 * covariance over all d coordinates (DnC looks at a sample of them) and needs only f, no bound on
 * the honest covariance.  Where ByzFL's code differs from this text, this text holds.
 *
 * Inputs: rows x_k, k < K, fp32 widened exactly; f = the number of Byzantine rows tolerated,
 * K >= 2 and 0 <= 2f < K; power_iters >= 1 (Python default 100) and power_tol >= 0 (1e-10).
 *
 * All arithmetic is fp64.  State: weights c_k = 1 and best = +inf.  Every sum over k runs in a
 * fixed order that depends on K alone.
 *
 * Round t = 0, 1, ..., run while S = sum_k c_k > K - 2f:
 * 1. p_k = c_k / S;  mu = sum_k p_k x_k;  u_k = x_k - mu;  M_ij = sqrt(p_i) sqrt(p_j) (u_i . u_j).
 *    M is K x K and positive semidefinite, with the nonzero spectrum of the weighted covariance
 *    sum_k p_k u_k u_k^T.
 * 2. The top eigenpair of M by power iteration.
 *    - Start: r = arg max_k M_kk (NaN first, ties to the lower index), w_0 = M e_r / ||M e_r||.
 *    - Step: w_i = M w_{i-1} / ||.||, one "application".
 *    - Stop when ||w_i - w_{i-1}||_2 <= power_tol, or after power_iters applications.
 *    - lambda = w^T M w of the last unit iterate, converged or not.
 *    - ||M e_r|| = 0 (all weighted rows equal): lambda = 0 with 0 applications, converged = 1;
 *      step 3 runs, then the loop ends.
 *    - A non-finite norm or lambda (and a zero norm inside the iteration, which cannot be
 *      normalised) ends the loop at once; if nothing has been recorded yet, the current c is.
 *      Such a round is not counted in `rounds`.
 * 3. If lambda < best (strict): best = lambda, c* = c, S* = S, t* = t.
 * 4. g_k = u_k . (sum_j sqrt(p_j) w_j u_j), tau_k = g_k^2, tau_max = the maximum over the rows
 *    with c_k > 0.  tau_max zero or non-finite ends the loop.  Otherwise
 *    c_k <- c_k (1 - tau_k / tau_max) for every row with c_k > 0: the arg-max row becomes exactly
 *    0 and a zero weight stays zero.  (The normalisation of the direction cancels in the ratio.)
 * Every completed round zeroes at least one positive weight, so the loop ends within K rounds;
 * the host caps it there.
 *
 * Result: out_j = float( sum_{k : c*_k > 0, increasing k} (c*_k / S*) x_kj ), fp64 sums rounded
 * once.  A row of weight 0 is skipped, not multiplied: whatever it holds contributes nothing and
 * the result pass does not read it.  f = 0 runs no round: the result is gm_mean_f32's, bit for
 * bit, with c* = 1, S* = K, rounds = 0 and a NaN eigenvalue.
 *
 * What is actually built (the K-space identities).  With D_ij = ||x_i - x_j||^2 (the exact
 * distance path of Krum, Multi-Krum and NNM: fp32 differences, fp32 squares summed per 32-column
 * stage, fp64 across stages), a = D p, q = p^T a / 2 and rho_k = ||u_k||^2 = a_k - q:
 *     u_i . u_j = (rho_i + rho_j - D_ij) / 2
 *     G z = (rho (1^T z) + 1 (rho^T z) - D z) / 2          for any z,  G = (u_i . u_j)
 *     M w = sqrt(p) o G (sqrt(p) o w),      g = G (sqrt(p) o w)
 * so one application of M is one product with the fixed matrix D plus two dot products, the
 * d x d covariance is never formed and X is read twice: once for D, once for the result.
 *
 * What the filter does not defend against: a non-finite entry makes D non-finite and ends the
 * filter in round 0 with c = 1; the result is then the plain weighted mean under IEEE rules
 * (NaN in the columns that hold it).  Compose with gm_clip_rows_f32 (clip / arc) for that.
 *
 * The result and every reported quantity are bit-identical for rows, panels and every alignment.
 *
 *   X          fp32, layout GM_LAYOUT_ROWS ([K][ldx], ldx >= d, any alignment: 16-byte loads where
 *              the base and ldx allow) or GM_LAYOUT_PANELS ([ceil(d/W)][K][W], W =
 *              gm_panel_width(K), ldx = panel stride >= K*W).  Never written.
 *   out        device fp32 [d].
 *   weights    device double [K], or NULL: c*.
 *   eigenvalue, weight   host, or NULL: lambda of round t* (NaN when no round was counted), S*.
 *   rounds, best_round   host, or NULL: the rounds that reached step 3, and t*.
 *   niter, converged     host int32 [K], or NULL: per counted round the applications run and
 *              whether the movement test passed; the first *rounds entries are written.
 * Uses the context's workspace (stream-ordered with the other calls on it): D (8 K^2 bytes), the
 * distance pass's partials and O(K) state.  The call blocks once per round (the host reads one
 * small state record to decide whether another round is queued), never per application; the
 * weighted mean is queued behind the last round and takes the rows and weights from device memory.
 * GM_ERR_INVALID (nothing written): a NULL ctx, X or out, K < 2, d < 0, f < 0, 2f >= K, an unknown
 * layout, a rows layout with ldx < d (a panel stride < K*W), power_iters < 1, power_tol not >= 0.
 * GM_ERR_UNSUPPORTED (with a message): K > 4096, a panel layout whose K has no panel width, a
 * d-sharded or collective context (the distances would need a K x K all-reduce).
 * d == 0 returns GM_OK, launches nothing and writes nothing. */
int gm_caf_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
               int64_t f, int64_t power_iters, double power_tol, float* out, double* weights,
               double* eigenvalue, double* weight, int32_t* rounds, int32_t* best_round,
               int32_t* niter, int32_t* converged, void* stream);

/* CAF's result pass on its own: out_j = float( sum_{k : w_k > 0, increasing k} (w_k / S) x_kj ),
 * S = the sum of the positive weights, fp64 sums rounded once.  A row whose weight is zero,
 * negative or NaN is skipped and not read.  With gm_caf_f32's `weights` on the same X this is that
 * call's out, bit for bit; no positive weight gives zeros.
 *   X, out     as gm_caf_f32's.   weights   device double [K].
 * No host synchronisation; works on a d-sharded context (columns are independent).
 * GM_ERR_INVALID (nothing written): a NULL pointer, K < 1, d < 0, an unknown layout, ldx too small.
 * GM_ERR_UNSUPPORTED: K > 4096, a panel layout whose K has no panel width.  d == 0: GM_OK. */
int gm_weighted_mean_f32(gm_ctx* ctx, const float* X, int64_t K, int64_t d, int64_t ldx,
                         int32_t layout, const double* weights, float* out, void* stream);

/* FLTrust (Cao, Fang, Liu & Gong, "FLTrust: Byzantine-robust Federated Learning via Trust
 * Bootstrapping", NDSS 2021): the only rule here that scores a client against a reference vector,
 * the server's own update, instead of against the other clients.
 *
 * Inputs:
 * - rows x_k, k < K
 * - the server vector s: `server` [d], or row `server_row` of X (exactly one of the two;
 *   server_row = -1 with a vector)
 * - a centre c [d]; NULL is zeros, and the rows are then the updates themselves
 *
 * All arithmetic is fp64 on the fp32 / bf16 values widened exactly:
 *
 *     u_k = x_k - c                      g = s - c
 *     a_k = sum_j u_kj g_j               n_k = sum_j u_kj^2        n_g = sum_j g_j^2
 *     counted_k = (k != server_row) and n_g finite and n_g > 0
 *                 and n_k finite and n_k > 0 and a_k finite
 *     cos_k = a_k / sqrt(n_k n_g)
 *     TS_k  = counted_k ? max(0, cos_k) : 0
 *     T     = sum_k TS_k                 (increasing k)
 *     coef_k = TS_k * sqrt(n_g / n_k) / T
 *     out_j = float( c_j + sum_{k : TS_k > 0, increasing k} coef_k u_kj )     (rounded once)
 *     T == 0:  out_j = c_j exactly  (zeros without a centre)
 *
 * The paper leaves T == 0 undefined; this build returns the centre.  A row with TS_k = 0 is
 * skipped, not multiplied by zero: whatever it holds (inf, NaN, 1e38) contributes nothing, and
 * the second pass does not read it.
 *
 * Two calls on the same input on the same device return the same bits.  Rows and panels agree to
 * rounding, not bit for bit (the order of the row sums differs); given equal coefficients the
 * sum over k is in increasing k in every layout.
 *
 *   X        fp32 (gm_fltrust_f32) or bfloat16 bit patterns (gm_fltrust_bf16); layout
 *            GM_LAYOUT_ROWS ([K][ldx], any ldx >= d, any alignment: 16-byte loads where the base
 *            and ldx allow, else one element at a time) or GM_LAYOUT_PANELS ([ceil(d/W)][K][W],
 *            W = gm_panel_width(K) resp. gm_panel_width_bf16(K), ldx = panel stride >= K*W).
 *            Never written; nothing at or past column d is read.
 *   server, centre, out   device fp32 [d]; out aliases nothing.
 *   stats    device double [3K + 2], or NULL: cos_k exactly as computed (IEEE NaN / inf where
 *            undefined; the server row's own is about 1), then n_k, then TS_k, then n_g and T.
 * Two passes over X on the context's workspace (stream-ordered with the other calls on it): one
 * read of all K rows for the sums, one of the rows with TS_k > 0 for the result.  On an
 * unsharded context the call makes no host synchronisation and no device-to-host copy: the
 * number of trusted rows and T == 0 are read on the device by the second pass.
 * On a d-sharded context (gm_ctx_set_shard plus an all-reduce) X, server, centre and out are this
 * rank's columns; the 2K + 1 fp64 sums go through the all-reduce once, between the first pass and
 * the K-space step, and every rank derives identical coefficients (identical stats bits).
 * GM_ERR_INVALID (nothing written): a NULL ctx, X or out, K < 1, d < 0, an unknown layout, ldx < d
 * (a panel stride < K*W), both or neither of server / server_row, server_row outside [0, K).
 * GM_ERR_UNSUPPORTED (with a message): K > 2048, a panel layout whose K has no panel width.
 * d == 0 returns GM_OK and launches nothing. */
int gm_fltrust_f32 (gm_ctx* ctx, const float*    X, int64_t K, int64_t d, int64_t ldx,
                    int32_t layout, const float* server, int64_t server_row, const float* centre,
                    float* out, double* stats, void* stream);
int gm_fltrust_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                    int32_t layout, const float* server, int64_t server_row, const float* centre,
                    float* out, double* stats, void* stream);

/* Norm clipping ahead of every aggregator above: static clipping (Sun, Kairouz, Suresh & McMahan,
 * "Can You Really Backdoor Federated Learning?", 2019) and its adaptive form ARC, Adaptive Robust
 * Clipping (Allouah, Guerraoui, Gupta, Jellouli, Rizk & Stephan, "Adaptive Gradient Clipping for
 * Robust Federated Learning", ICLR 2025): every row's update about a centre is scaled back to a
 * radius, a given one or the norm of the (k + 1)-th largest update.  Y has K rows.
 *
 * Inputs:
 * - rows x_k, k < K
 * - a centre c [d]; NULL is zeros, and the rows are then the updates themselves
 * - a rule: GM_CLIP_STATIC with tau > 0, or GM_CLIP_ARC with 0 <= f <= K - 1
 *
 * All arithmetic is fp64 on the fp32 / bf16 values widened exactly:
 *
 *     u_kj = x_kj - c_j                  n_k = sum_j u_kj^2
 *     ARC(f):      k = (2 f (K - f)) div K       (integer arithmetic; f <= K - 1, so k <= K/2)
 *                  T = the n at zero-based rank K - 1 - k in the order of score_before
 *                      (robust.hip: ascending, NaN last, ties to the lower index): the (k + 1)-th
 *                      largest n_k, with NaN ranked largest.  sqrt(T) is the paper's radius C.
 *     static(tau): T = (double)tau * (double)tau    (tau = +inf: nothing finite is clipped)
 *     s_k = 0                 if n_k is NaN or +inf
 *           1                 else if T is NaN or n_k <= T
 *           sqrt(T / n_k)     otherwise
 *     y_kj = x_kj widened, the same value (-0 stays -0)   if s_k == 1  (a copy, not an evaluation)
 *            c_j exactly (zeros without a centre)         if s_k == 0  (the row is not read again)
 *            float(c_j + s_k u_kj), rounded once          otherwise
 *
 * k is computed in integer arithmetic.  The floating-point evaluation int(2 * (f / K) * (K - f))
 * found elsewhere differs from it: of the pairs with K <= 4096 and f < K/2, 80 disagree, the
 * first at (K, f) = (242, 33), where the exact value is 57 and the float form gives 56.
 * The order of each n_k sum depends on (d, layout, load path) only and is the same for every
 * row, so rows that hold equal values have equal n_k bits, and a tie at the threshold leaves
 * both rows unclipped, deterministically.  A row whose norm is not finite maps to the centre (a
 * zero update; the paper leaves it undefined): like FLTrust's rows of zero trust it is skipped,
 * not multiplied by zero, and the second pass does not read it.
 *
 *   X        fp32 (gm_clip_rows_f32) or bfloat16 bit patterns (gm_clip_rows_bf16); layout_in
 *            GM_LAYOUT_ROWS ([K][ldx], any ldx >= d, any alignment: 16-byte loads where the base
 *            and ldx allow, else one element at a time) or GM_LAYOUT_PANELS ([ceil(d/W)][K][W],
 *            W = gm_panel_width(K) resp. gm_panel_width_bf16(K), ldx = panel stride >= K*W).
 *            Nothing at or past column d is read.
 *   Y        fp32, layout_out likewise with ldy and W = gm_panel_width(K); columns >= d are not
 *            written.  Out of place, Y overlaps no byte of X; X is not written, every row with
 *            s_k != 0 is read and all K rows are written.  In place, Y is X exactly (the same
 *            pointer, stride and layout; fp32 only): the rows with 0 < s_k < 1 are read, and only
 *            the rows with s_k != 1 are written.
 *   centre   device fp32 [d], or NULL.
 *   stats    device double [2K + 2], or NULL: n_k, then s_k, then T and the number of rows with
 *            s_k != 1.
 * Two passes over X on the context's workspace (stream-ordered with the other calls on it).  On
 * an unsharded context the call makes no host synchronisation and no device-to-host copy: the
 * second pass takes its row list and count from device memory.  Two calls on the same input on
 * the same device return the same bits; rows-out and panels-out hold the same bits for the same
 * input; input layouts agree to rounding (the order of the n_k sums differs).
 * On a d-sharded context (gm_ctx_set_shard plus an all-reduce) X, centre and Y are this rank's
 * columns; the K fp64 sums n_k go through the all-reduce once, between the first pass and the
 * K-space step, and every rank derives identical T and s_k (identical stats bits).
 * GM_ERR_INVALID (nothing written): a NULL ctx, X or Y, K < 1, d < 0, an unknown rule or layout,
 * ldx or ldy too small for its layout, f outside [0, K - 1] (ARC), tau not > 0 (static), Y
 * overlapping X other than as in place.  GM_ERR_UNSUPPORTED (with a message): K > 4096, a panel
 * layout whose K has no panel width, bf16 in place.  d == 0 returns GM_OK before any device call. */
typedef enum gm_clip_rule {
    GM_CLIP_STATIC = 0,       /* the radius tau */
    GM_CLIP_ARC = 1           /* the radius from the rows' own norms and f */
} gm_clip_rule;
int gm_clip_rows_f32 (gm_ctx* ctx, const float*    X, int64_t K, int64_t d, int64_t ldx,
                      int32_t layout_in, const float* centre, int32_t rule, int64_t f, double tau,
                      float* Y, int64_t ldy, int32_t layout_out, double* stats, void* stream);
int gm_clip_rows_bf16(gm_ctx* ctx, const uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                      int32_t layout_in, const float* centre, int32_t rule, int64_t f, double tau,
                      float* Y, int64_t ldy, int32_t layout_out, double* stats, void* stream);

/* Omniscient model-poisoning attacks, in place on the client matrix: rows 0 .. H-1 (H = K - byz
 * >= 2) are the honest clients, rows H .. K-1 the Byzantine ones (the reference's
 * messages[-byzantinesize:]), which are overwritten with ONE malicious row computed from the
 * honest rows' per-column statistics, in fp64 (bf16 inputs widened exactly):
 *     mu_j    = (sum_{k<H} x_kj) / H, summed in increasing k
 *     sigma_j = sqrt(sum_{k<H} (x_kj - mu_j)^2 / (H - 1))     (the unbiased estimate)
 * sigma comes from sums shifted by the column's first row, clamped at 0: a column whose honest
 * values are all equal has sigma_j == 0 and mu_j == that value exactly.
 *
 * gm_attack_affine_f32 / _bf16: every Byzantine row becomes y_j = a mu_j + b sigma_j, rounded
 * once to the storage type (bf16: to nearest even).  a = 1, b = -z is "A Little Is Enough"
 * (Baruch, Baruch & Goldberg 2019), a = -epsilon, b = 0 inner-product manipulation (Xie, Koyejo
 * & Gupta 2019).  b == 0 forms no sigma term (a column holding +inf gives a * inf, not NaN);
 * a NaN among a column's honest values gives NaN; infinities follow IEEE.
 *   X      fp32, or bfloat16 bit patterns; layout GM_LAYOUT_ROWS ([K][ldx], ldx >= d, any
 *          alignment) or GM_LAYOUT_PANELS ([ceil(d/W)][K][W], W = gm_panel_width(K) resp.
 *          gm_panel_width_bf16(K), ldx = panel stride >= K*W).  Only columns < d of rows >= H
 *          are written: the honest rows and the panels' padding columns keep their bits.
 * One stream-ordered kernel that reads H*d elements once and writes byz*d: no workspace, no host
 * synchronisation.  The result is bit-identical for every layout and alignment of one type,
 * and column-local: on a d-sharded matrix every rank attacks its own columns with the same a, b.
 *
 * gm_attack_minmax_f32 (fp32 only): the min-max (rule 0) and min-sum (rule 1) attacks of
 * Shejwalkar & Houmansadr 2021.  Every Byzantine row becomes m = mu - gamma p, rounded once, with
 * the deviation p = sigma (dev 0), mu / ||mu|| (dev 1) or sign(mu) (dev 2) and the largest gamma
 * that meets
 *     rule 0   max_i ||m - x_i||^2 <= max_ij ||x_i - x_j||^2 =: D*
 *              gamma = min_i (b_i + sqrt(b_i^2 + c (D* - a_i))) / c
 *     rule 1   sum_i ||m - x_i||^2 <= max_i sum_j ||x_i - x_j||^2 =: S*
 *              gamma = sqrt((S* - sum_i a_i) / (H c))
 * over the honest rows, where a_i = ||mu - x_i||^2, b_i = p . (mu - x_i), c = ||p||^2 (fp64 sums
 * in a fixed order); c == 0 gives gamma = 0, m = mu.  The pairwise distances are gm_krum_f32's
 * exact path on the H honest rows (fp32 squares summed per 32-column stage, fp64 across stages),
 * hence K <= 4096.  Not column-local.
 *   gamma   host double, or NULL.  Non-NULL receives gamma and blocks until the stream has run
 *           the call; the row is written from the device-side value either way.
 * Uses the context's workspace (stream-ordered with the other calls on it).
 *
 * GM_ERR_INVALID (nothing written): a NULL ctx or X, K < 1, d < 0, byz < 1, K - byz < 2, an
 * unknown layout, rule or dev, ldx too small for its layout.  GM_ERR_UNSUPPORTED (with a
 * message): panel input whose K has no panel width of its type, K > 4096 (min-max / min-sum).
 * d == 0 returns GM_OK. */
int gm_attack_affine_f32 (gm_ctx* ctx, float*    X, int64_t K, int64_t d, int64_t ldx,
                          int32_t layout, int64_t byz, double a, double b, void* stream);
int gm_attack_affine_bf16(gm_ctx* ctx, uint16_t* X, int64_t K, int64_t d, int64_t ldx,
                          int32_t layout, int64_t byz, double a, double b, void* stream);
int gm_attack_minmax_f32 (gm_ctx* ctx, float* X, int64_t K, int64_t d, int64_t ldx, int32_t layout,
                          int64_t byz, int32_t rule, int32_t dev, double* gamma, void* stream);

/* The K clients' local SGD steps of one federated step (the loop body M:291-343:
 * forward, CrossEntropyLoss (mean), backward, p -= gamma * (grad + weight_decay * p),
 * the client's parameters copied out as its row), as one stream-ordered kernel, for the
 * reference's linear model MLP(F, C) (M:53-61; F <= 832, C <= 64, batch B <= 64).
 * The clients run in sequence on ONE model, as the reference's aliasing state_dict
 * "snapshot" makes them (M:290, M:343): client k starts from client k-1's update, and
 * W / b end as the last client's parameters (the aggregator's guess, M:349).
 *   data     training samples [n][ldd] fp32 (device), labels [n] int64 (device)
 *   idx      [K][B] int32 dataset rows of each client's batch (device): the reference's
 *            RandomSampler draws (M:260-270), offset by the client's shard start
 *   honest   clients k >= honest are Byzantine: attack 1 = classflip (target C-1-y,
 *            M:320), 2 = dataflip (input 1-x, M:326), 0 = none (also weightflip,
 *            which rewrites the matrix afterwards, M:380-383)
 *   W, b     the model's weight [C][F] and bias [C] (device), updated in place
 *   X        the client matrix: row k = [W (C*F, row-major), b (C)], layout
 *            GM_LAYOUT_ROWS (ldx = row stride >= C*F + C) or GM_LAYOUT_PANELS
 *            (ldx = panel stride >= K*W, W = gm_panel_width(K)). */
int gm_client_chain_f32(gm_ctx* ctx, const float* data, int64_t ldd, const int64_t* labels,
                        int64_t F, int64_t C, const int32_t* idx, int64_t K, int64_t B,
                        int64_t honest, int32_t attack, float gamma, float weight_decay,
                        float* W, float* b, float* X, int64_t ldx, int32_t layout, void* stream);

/* The K clients' stochastic gradients at ONE model, folded into their momenta: the worker-
 * momentum loop in gradient space (Karimireddy, He & Jaggi, ICML 2021, Algorithm 1), as one
 * stream-ordered kernel with one workgroup per client, for the model gm_client_chain_f32
 * supports (MLP(F, C), CrossEntropyLoss mean, F <= 832, C <= 64, batch B <= 64).  For client k,
 * with theta = [W (C*F, row-major), b (C)]:
 *   g_k  = grad_theta meanCE(theta; batch k) + weight_decay * theta
 *   M_k <- beta * M_k + (1 - beta) * g_k      (fmaf(beta, m, (1 - beta) * (g + wd * p)))
 *   data, labels, idx, honest, attack   as gm_client_chain_f32's
 *   beta     in [0, 1).  beta == 0: M is write-only (row k = g_k; what M held, NaN included,
 *            does not reach the result)
 *   W, b     the model's weight [C][F] and bias [C] (device), read only
 *   M        the K x (C*F + C) momentum matrix, updated in place: GM_LAYOUT_ROWS (ldx = row
 *            stride >= C*F + C, any alignment) or GM_LAYOUT_PANELS (ldx = panel stride
 *            >= K*W, W = gm_panel_width(K)).  Nothing at or past column C*F + C of a row is
 *            read or written (panel padding columns are not written).
 * Row k depends only on (W, b, batch k, k >= honest, M_k): its bits are the same whatever K,
 * the grid's schedule or the layout.
 *
 * GM_ERR_INVALID (nothing written): NULL pointers, K < 1 or K >= 2^31 (the grid), B < 1, F < 1,
 * C < 1, ldd < F, honest outside [0, K], an unknown attack or layout, beta outside [0, 1) or
 * NaN, ldx or the panel stride too small.
 * GM_ERR_UNSUPPORTED (with a message): F, C or B beyond the limits, a panel layout whose K has
 * no panel width. */
int gm_client_grads_f32(gm_ctx*, const float* data, int64_t ldd, const int64_t* labels,
                        int64_t F, int64_t C, const int32_t* idx /*[K][B]*/, int64_t K, int64_t B,
                        int64_t honest, int32_t attack, float beta, float weight_decay,
                        const float* W, const float* b, float* M, int64_t ldx, int32_t layout,
                        void* stream);

/* OMA with the reference's own draws (device arrays): h_re[K], h_im[K],
 * n_re[K*d], n_im[K*d] (row-major, already scaled by sqrt(noise_var)).
 * Bit-exact with the reference's fp32 op order. */
int gm_oma_apply_f32(gm_ctx* ctx, float* X, int64_t K, int64_t d, int64_t ldx,
                     const float* h_re, const float* h_im, const float* n_re,
                     const float* n_im, void* stream);

/* Fill X[K][ldx] (first d columns) with seeded synthetic client updates on the
 * device: rows k < K - B ~ N(mu_h, sd_h^2), the last B rows ~ N(mu_b, sd_b^2)
 * (BASELINE.md §3 recipe), Philox-keyed so every shard generates its own
 * columns of the same global matrix (global column = d_offset + j). */
int gm_fill_clients_f32(gm_ctx* ctx, float* X, int64_t K, int64_t d, int64_t ldx, int64_t B,
                        float mu_h, float sd_h, float mu_b, float sd_b, uint64_t seed,
                        void* stream);
/* Fill v[n] ~ N(mu, sd^2) (global index = d_offset + i). */
int gm_fill_normal_f32(gm_ctx* ctx, float* v, int64_t n, float mu, float sd, uint64_t seed,
                       void* stream);

/* Timing hook for the dominant kernel: accumulated device time (ms, HIP
 * events on the launch stream) and launch count of the fused Weiszfeld pass
 * since the last reset. */
int gm_ctx_pass_timing(gm_ctx* ctx, int enable, double* total_ms, int64_t* launches);

const char* gm_last_error(void);
int gm_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* GMAGG_H */
