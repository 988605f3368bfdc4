// The fused streaming Weiszfeld pass for gfx950: ONE HBM read of X per
// iteration.
//
// Reference (MNIST_Air_weight.py): gm2's loop body M:174-181 computes
//   dist = max(1e-4, ||x_k - g||)          (a K x d read)
//   g'   = sum_k x_k/dist_k / sum 1/dist_k (another K x d read)
//   movement = ||g - g'||
// and the next body starts by re-reading X for the distances to g'.  Here a
// block owns a chunk of J columns x ALL K rows (in VGPRs) at a time:
//   phase A  g'_j = sum_k c_k x_kj          (c_k from the K-space step: 1/dist_k
//                                            normalised, or the AirComp gains)
//   phase B  D_k += sum_{j in chunk} (x_kj - g'_j)^2  -- the NEXT iteration's
//            distances, while the tile is still in registers
// plus ||g - g'||^2 and ||g'||^2.  INIT passes compute D_k to the initial
// guess (and ||x_k||^2 for the AirComp power control).
//
// Thread map (1024 threads = 16 waves): lane c of a row segment covers columns
// [c*V, c*V+V) of the chunk, QW = 64/LPR row groups per wave, NRG = 16*QW row
// groups per block, row group rg owns rows rg + NRG*i (i < R).  Every wave
// instruction reads LPR*V*4 contiguous bytes of QW rows: 1 KiB per
// instruction for V = 4.  Per-block partials go to a slab (fp64), summed by
// slab_reduce in a fixed order: deterministic, no atomics.
//
// The kernel template is in stream_pass_kernel.h; this file instantiates it for fp32
// elements (V = 1, 2, 4), stream_pass_bf16.hip for bf16 elements (V = 8), and
// stream_pass_cclip.hip the fp32 STEP pass of centered clipping (the old iterate as column term).
#include "stream_pass_kernel.h"

namespace gmk {

// ---------------------------------------------------------------------------
// Launch plumbing.  GMAGG_PASS_VARIANT: -1 auto (default), 0 plain, 1 pipelined
// (-DGMK_PIPE_VARIANT builds only), 2 rolling prefetch, 3 two tiles rolled two chunks
// ahead (panels).

int pass_variant() {
  static const int v = [] {
    const char* e = getenv("GMAGG_PASS_VARIANT");
    return e ? atoi(e) : -1;
  }();
  return v;
}

template <int V, int NW, int LPR, int R, int MODE, int OCC>
static const void* pass_fn(bool panel) {
  // Measured on MI355X (profiles/history/r01_ab_pass.txt, r01_pipe_sweep.txt): the plain
  // pass is as fast or faster than the two-tile PIPE variant at every K, so that
  // one is only built with -DGMK_PIPE_VARIANT for A/B runs.
  // Panels: the rolling-prefetch STEP pass (6.44-6.56 vs 6.63 ms at C3), and since round 6
  // the INIT pass too (mode 1 / 2; the fused-OMA INIT, mode 4, stays plain): the plain INIT
  // ran 117-128 us above the STEP pass at C3 in three of four interleaved pairs (12 in the
  // first), the rolling one 32-48 us (profiles/r6s3_init_roll_ab.jsonl; round 2 had measured no
  // gain, profiles/history/r2_init_ab.txt).  The schedule moves loads, not arithmetic: the
  // results are the same bits.
  constexpr bool kRollDefault = MODE == 0;
  constexpr bool kRollPanel = kRollDefault || MODE == 1 || MODE == 2;
  if constexpr (V == 4) {
    if (panel) {
      const int pv = pass_variant();
      if (pv == 3)
        return reinterpret_cast<const void*>(&weiszfeld_pass<V, NW, LPR, R, MODE, 3, OCC, true>);
      if (pv == 2 || (pv < 0 && kRollPanel))
        return reinterpret_cast<const void*>(&weiszfeld_pass<V, NW, LPR, R, MODE, 2, OCC, true>);
      return reinterpret_cast<const void*>(&weiszfeld_pass<V, NW, LPR, R, MODE, 0, OCC, true>);
    }
  } else if (panel) {
    return nullptr;
  }
#ifdef GMK_PIPE_VARIANT
  if (pass_variant() == 1)
    return reinterpret_cast<const void*>(&weiszfeld_pass<V, NW, LPR, R, MODE, 1, OCC>);
#endif
  // Row-major STEP passes with float4 rows also take the rolling prefetch: C5's
  // batched K=50 tile streams 4.64 vs 4.43 TB/s (profiles/history/r04_c5_roll_ab.txt).
  if (pass_variant() == 2 || (pass_variant() < 0 && kRollDefault && V == 4))
    return reinterpret_cast<const void*>(&weiszfeld_pass<V, NW, LPR, R, MODE, 2, OCC>);
  return reinterpret_cast<const void*>(&weiszfeld_pass<V, NW, LPR, R, MODE, 0, OCC>);
}

template <int V, int NW, int LPR, int R, int OCC>
static const void* pass_fn_mode(int mode, bool panel) {
  switch (mode) {
    case 0: return pass_fn<V, NW, LPR, R, 0, OCC>(panel);
    case 1: return pass_fn<V, NW, LPR, R, 1, OCC>(panel);
    case 2: return pass_fn<V, NW, LPR, R, 2, OCC>(panel);
    case 4:
      if constexpr (V == 4) return pass_fn<V, NW, LPR, R, 4, OCC>(panel);
      else return nullptr;
    default: return pass_fn<V, NW, LPR, R, 3, OCC>(panel);
  }
}

static const void* pass_kernel(const PassCfg& cfg, int mode, bool panel = false) {
  if (mode == kPassStepExactD || mode == kPassStepDelta)   // stream_pass_delta.hip
    return panel ? pass_kernel_delta(cfg, mode) : nullptr;
  if (cfg.B16) return pass_kernel_bf16(cfg, mode, panel);
  if (mode == kPassStepSelf) return pass_kernel_self(cfg, panel);   // stream_pass_cclip.hip
#define GMK_CASE(V_, W_, L_, R_, O_)                                                 \
  if (cfg.V == V_ && cfg.NW == W_ && cfg.LPR == L_ && cfg.R == R_ && cfg.OCC == O_) \
    return pass_fn_mode<V_, W_, L_, R_, O_>(mode, panel);
  GMK_FOR_EACH_CFG(GMK_CASE, 4)
  GMK_FOR_EACH_CFG(GMK_CASE, 2)
  GMK_FOR_EACH_CFG(GMK_CASE, 1)
#undef GMK_CASE
  return nullptr;
}

bool pass_cfg_supported(const PassCfg& cfg) { return pass_kernel(cfg, 0) != nullptr; }

hipError_t launch_pass(const PassCfg& cfg, int mode, int grid, const PassArgs& a, hipStream_t s,
                       int problems) {
  // the K <= 1024 row-major tile's passes without a column term (gm2, noiseless gm): the
  // 32-wave rows kernel (rows_pass.hip), the same two blocks per CU, so the same grid and slab
  if (problems == 1 && cfg.V == 4 && cfg.NW == 8 && cfg.LPR == 8 && cfg.R == 16 && cfg.OCC == 2 &&
      rows_pass_eligible(a, mode))
    return launch_rows_pass(mode, grid, a, s);
  const void* fn = pass_kernel(cfg, mode, a.panel_stride > 0);
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<PassArgs*>(&a)};
  return hipLaunchKernel(fn, dim3(grid, problems), dim3(cfg.NW * 64), args, 0, s);
}

int pass_blocks_per_cu(const PassCfg& cfg, int mode) {
  const void* fn = pass_kernel(cfg, mode, mode == kPassStepExactD || mode == kPassStepDelta);
  int n = 0;
  if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, cfg.NW * 64, 0) != hipSuccess ||
      n < 1)
    return 1;
  return n;
}

}  // namespace gmk
