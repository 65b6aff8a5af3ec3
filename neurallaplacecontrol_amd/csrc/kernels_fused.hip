// One-launch planner body (nlc_fused_kernel.h), hidden width 128 (the harness's hidden_units, train_utils.py:29-54), and the
// width dispatch of the launcher.
#include "nlc_fused_kernel.h"

namespace nlc {

template hipError_t launch_nl_plan_fused_ht<8>(const FusedArgs&, unsigned, int, hipStream_t);
template hipError_t fused_max_resident_blocks_ht<8>(int, int*);

hipError_t fused_max_resident_blocks(int h, int bpc_built, int* blocks_per_cu) {
  return with_width(h, [&](auto ht) { return fused_max_resident_blocks_ht<ht>(bpc_built, blocks_per_cu); });
}

hipError_t launch_nl_plan_fused(const FusedArgs& a, int g, unsigned grid, int bpc_built, hipStream_t s) {
  if (a.r.K <= 0) return hipSuccess;
  if (2 * g != a.r.net.h) return hipErrorInvalidValue;
  return with_width(a.r.net.h, [&](auto ht) { return launch_nl_plan_fused_ht<ht>(a, grid, bpc_built, s); });
}

}  // namespace nlc

// tools/split_phase_clocks.py (a -DNLC_PHASE_CLOCKS=1 build of this unit): phase sums of the latency-split bodies launched from here
namespace nlc {
NLC_DEFINE_SPLIT_CLK_READER(nlc_debug_split_clocks_fused)
}
