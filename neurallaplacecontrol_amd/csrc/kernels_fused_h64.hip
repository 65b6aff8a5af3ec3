// One-launch planner body (nlc_fused_kernel.h) for hidden_units = 64, the class default (w_nl.py:72; GRU hidden 32).
#include "nlc_fused_kernel.h"

namespace nlc {

template hipError_t launch_nl_plan_fused_ht<4>(const FusedArgs&, unsigned, int, hipStream_t);
template hipError_t fused_max_resident_blocks_ht<4>(int, int*);

}  // namespace nlc
