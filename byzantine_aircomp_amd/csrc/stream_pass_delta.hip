// The gm2 STEP on fp32 panels once late iterations run as corrections on a bf16 shadow of X
// (DESIGN.md §3.1): the exact pass that can also write the shadow and always writes the base
// iterate (DELTA = 1, here), and the correction pass on the shadow (DELTA = 2, built with the
// other bf16 tiles in stream_pass_bf16.hip).  Both are variants of the template in
// stream_pass_kernel.h; the kernels of every other path are the instantiations they were.
//
// Built for the two-blocks-per-CU tile of 512 < K <= 1024 (C3's): fp32 chunks of 32 columns
// writing into 64-column bf16 panels.
#include "stream_pass_kernel.h"

namespace gmk {

const void* pass_kernel_bf16_delta(const PassCfg& cfg);   // stream_pass_bf16.hip

const void* pass_kernel_delta(const PassCfg& cfg, int mode) {
  if (mode == kPassStepDelta) return cfg.B16 && cfg.V == 8 ? pass_kernel_bf16_delta(cfg) : nullptr;
  if (mode != kPassStepExactD || cfg.B16 || cfg.V != 4 || cfg.NW != 8 || cfg.LPR != 8 ||
      cfg.R != 16 || cfg.OCC != 2)
    return nullptr;
  // the schedule of the fp32 panel STEP (stream_pass.hip pass_fn): rolling unless forced plain
  if (pass_variant() == 0)
    return reinterpret_cast<const void*>(
        &weiszfeld_pass<4, 8, 8, 16, 0, 0, 2, true, false, false, 1>);
  return reinterpret_cast<const void*>(&weiszfeld_pass<4, 8, 8, 16, 0, 2, 2, true, false, false, 1>);
}

}  // namespace gmk
