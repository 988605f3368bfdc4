// The fused streaming STEP pass with the old iterate as column term (centered clipping,
// gm_cclip_f32): the kernel template of stream_pass_kernel.h with SELF set, for fp32
// elements.  v' = sum_k c_k x_k + a v is the STEP pass's g' = sum_k c_k x_k (+ a n_j) with
// the finisher thread's own g_old in place of a noise draw: no extra load.  SELF kernels sum
// c_k x_k in fp64, so that identical rows are a fixed point to the last bit.  These are
// separate instantiations, in a file of their own, so that the gm2 / gm kernels of
// stream_pass.hip are the code they were (and the library's longest compile gets no longer);
// the bf16 ones are in stream_pass_bf16.hip with that file's build flags.
#include "stream_pass_kernel.h"

namespace gmk {

// The schedule is pass_fn's choice for a STEP pass (stream_pass.hip): panels and float4
// rows roll the prefetch; GMAGG_PASS_VARIANT = 0 / 2 / 3 forces one.
template <int V, int NW, int LPR, int R, int OCC>
static const void* self_fn(bool panel) {
  const int pv = pass_variant();
  if constexpr (V == 4) {
    if (panel) {
      if (pv == 3)
        return reinterpret_cast<const void*>(
            &weiszfeld_pass<V, NW, LPR, R, 0, 3, OCC, true, false, true>);
      if (pv == 2 || pv < 0)
        return reinterpret_cast<const void*>(
            &weiszfeld_pass<V, NW, LPR, R, 0, 2, OCC, true, false, true>);
      return reinterpret_cast<const void*>(
          &weiszfeld_pass<V, NW, LPR, R, 0, 0, OCC, true, false, true>);
    }
  } else if (panel) {
    return nullptr;
  }
  if (pv == 2 || (pv < 0 && V == 4))
    return reinterpret_cast<const void*>(
        &weiszfeld_pass<V, NW, LPR, R, 0, 2, OCC, false, false, true>);
  return reinterpret_cast<const void*>(
      &weiszfeld_pass<V, NW, LPR, R, 0, 0, OCC, false, false, true>);
}

const void* pass_kernel_self(const PassCfg& cfg, bool panel) {
  if (cfg.B16) return nullptr;
#define GMK_CASE(V_, W_, L_, R_, O_)                                                 \
  if (cfg.V == V_ && cfg.NW == W_ && cfg.LPR == L_ && cfg.R == R_ && cfg.OCC == O_) \
    return self_fn<V_, W_, L_, R_, O_>(panel);
  GMK_FOR_EACH_CFG(GMK_CASE, 4)
  GMK_FOR_EACH_CFG(GMK_CASE, 2)
  GMK_FOR_EACH_CFG(GMK_CASE, 1)
#undef GMK_CASE
  return nullptr;
}

}  // namespace gmk
