// One-launch planner body (nlc_fused_kernel.h) for hidden_units = 256 (GRU hidden 128): 64 KB of cooperative hidden-state
// images / 68 KB of rollout exchange per workgroup -> two workgroups per CU (256 VGPRs), the fused body's minimum.
#include "nlc_fused_kernel.h"

namespace nlc {

template hipError_t launch_nl_plan_fused_ht<16>(const FusedArgs&, unsigned, int, hipStream_t);
template hipError_t fused_max_resident_blocks_ht<16>(int, int*);

}  // namespace nlc
