// The fused streaming Weiszfeld pass on bf16 client updates (gm_weiszfeld_bf16): the
// kernel template of stream_pass_kernel.h with B16 set.  X is stored as bf16, half the
// bytes of the fp32 matrix per pass; everything that is not X (the iterate, the weights,
// the sums) is what the fp32 pass has.  A lane owns V = 8 columns, one 16-byte load as the
// fp32 tile's four floats, so each pick_cfg tile keeps its (NW, LPR, R, OCC), its bytes per
// row segment, per chunk and per load instruction and its register tile; the chunk is
// twice as wide (J = LPR * 8), and with it s_red, s_g and the finisher threads.
//
// Built: the tiles pick_cfg can return (rows and panels), modes 0 (STEP), 1 (INIT) and
// 2 (INIT + ||x_k||^2) and the STEP pass of centered clipping (SELF: the old iterate as column
// term), both layouts, the plain schedule and the rolling prefetch.  Not
// built: the Gram closing sum (mode 3) and the fused OMA write-back (mode 4), which would
// round the noised values back to bf16.  The 32-wave rows kernel (rows_pass.hip) is never
// taken: launch_pass selects it for V = 4 tiles only.
#include "stream_pass_kernel.h"

namespace gmk {

// The schedule follows the fp32 choice (stream_pass.hip pass_fn) — panels roll every mode,
// rows roll the STEP pass — except where the rolled kernel spills and the plain one does not
// (compiler resource report, DESIGN.md §3.1, bytes of scratch per lane rolled / plain):
//   the two-blocks-per-CU tile of 512 < K <= 1024   STEP 92 / 0, INIT 28 / 0, AirComp INIT
//                                                   564 / 100; measured at K=1000 x d=11M:
//                                                   STEP 3,656 us rolled, 3,372-3,392 plain
//   the AirComp INIT (mode 2) of tiles with R >= 8  132-184 / 0
//   the STEP pass of the 256 < K <= 512 tile        20 / 0
// GMAGG_PASS_VARIANT=0 / 2 forces one schedule.
// SELF: the STEP pass with the old iterate as column term (centered clipping, gm_cclip_bf16;
// launch mode kPassStepSelf), on the schedule of the plain STEP pass.
template <int NW, int LPR, int R, int OCC, int MODE, bool SELF = false>
static const void* pass_fn_bf16(bool panel) {
  const int pv = pass_variant();
  constexpr bool kRollSpills = OCC > 1 || (MODE == 2 && R >= 8) ||
                               (MODE == 0 && LPR == 16 && R == 8);
  const bool roll = pv == 2 || (pv != 0 && (panel || MODE == 0) && !kRollSpills);
  if (panel)
    return roll ? reinterpret_cast<const void*>(&weiszfeld_pass<8, NW, LPR, R, MODE, 2, OCC, true, true, SELF>)
                : reinterpret_cast<const void*>(&weiszfeld_pass<8, NW, LPR, R, MODE, 0, OCC, true, true, SELF>);
  return roll ? reinterpret_cast<const void*>(&weiszfeld_pass<8, NW, LPR, R, MODE, 2, OCC, false, true, SELF>)
              : reinterpret_cast<const void*>(&weiszfeld_pass<8, NW, LPR, R, MODE, 0, OCC, false, true, SELF>);
}

// pick_cfg's tiles (host_ctx.h): (waves per block, lanes per row segment, rows per thread,
// blocks per CU).
#define GMK_FOR_EACH_BF16_CFG(X_)                                                         \
  X_(16, 64, 1, 1) X_(16, 64, 2, 1) X_(16, 64, 4, 1) X_(8, 32, 4, 1) X_(16, 64, 8, 1)     \
  X_(16, 32, 8, 1) X_(16, 16, 4, 1) X_(16, 16, 8, 1) X_(8, 8, 16, 2) X_(16, 4, 8, 1)

const void* pass_kernel_bf16(const PassCfg& cfg, int mode, bool panel) {
  if (!cfg.B16 || cfg.V != 8) return nullptr;
#define GMK_CASE(W_, L_, R_, O_)                                                     \
  if (cfg.NW == W_ && cfg.LPR == L_ && cfg.R == R_ && cfg.OCC == O_) {               \
    switch (mode) {                                                                  \
      case 0: return pass_fn_bf16<W_, L_, R_, O_, 0>(panel);                         \
      case 1: return pass_fn_bf16<W_, L_, R_, O_, 1>(panel);                         \
      case 2: return pass_fn_bf16<W_, L_, R_, O_, 2>(panel);                         \
      case kPassStepSelf: return pass_fn_bf16<W_, L_, R_, O_, 0, true>(panel);       \
      default: return nullptr;                                                       \
    }                                                                                \
  }
  GMK_FOR_EACH_BF16_CFG(GMK_CASE)
#undef GMK_CASE
  return nullptr;
}

// The correction pass of gm2 on a bf16 shadow of fp32 panels (DELTA = 2; stream_pass_delta.hip
// dispatches).  The shadow's panels are as wide as the fp32 chunk that writes them (32 columns at
// 512 < K <= 1024), so the tile is 1024 rows x 32 columns: 4 lanes per 64-byte row, 8 rows per
// thread, 64 KiB per chunk, on the plain schedule, two blocks per CU (87 VGPRs, no scratch).
// Three blocks per CU (80 VGPRs, 28 bytes of scratch) measured slower at C3: 3.48 against
// 3.28 ms per pass, three interleaved rounds.
const void* pass_kernel_bf16_delta(const PassCfg& cfg) {
  if (!(cfg.B16 && cfg.V == 8 && cfg.NW == 8 && cfg.LPR == 4 && cfg.R == 8 && cfg.OCC == 2))
    return nullptr;
  return reinterpret_cast<const void*>(&weiszfeld_pass<8, 8, 4, 8, 0, 0, 2, true, true, false, 2>);
}

}  // namespace gmk
