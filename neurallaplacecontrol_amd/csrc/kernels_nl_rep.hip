// The representation function alone (nl_repfunc_kernel, nl_repfunc_split_kernel) for hidden_units = 128 (see kernels_nl.hip).
#include "nlc_nl_launch.h"

namespace nlc {

template hipError_t launch_nl_repfunc_ht<8, false>(const RepFuncArgs&, hipStream_t);
template hipError_t launch_nl_repfunc_ht<8, true>(const RepFuncArgs&, hipStream_t);

}  // namespace nlc

// tools/split_phase_clocks.py (a -DNLC_PHASE_CLOCKS=1 build of this unit): phase sums of the latency-split bodies launched from here
namespace nlc {
NLC_DEFINE_SPLIT_CLK_READER(nlc_debug_split_clocks_rep)
}
