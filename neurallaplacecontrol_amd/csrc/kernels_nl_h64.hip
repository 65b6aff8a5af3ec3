// Representation MLP + ILT + rollout kernels for hidden_units = 64 (the class default, w_nl.py:72): see kernels_nl.hip.
#include "nlc_nl_launch.h"

namespace nlc {

template hipError_t launch_nl_rollout_ht<4, false>(const RolloutArgs&, hipStream_t, bool);
template hipError_t launch_nl_forward_ht<4, false>(const ForwardArgs&, hipStream_t);
template hipError_t launch_nl_forward_ht<4, true>(const ForwardArgs&, hipStream_t);
template hipError_t launch_nl_repfunc_ht<4, false>(const RepFuncArgs&, hipStream_t);
template hipError_t launch_nl_repfunc_ht<4, true>(const RepFuncArgs&, hipStream_t);

}  // namespace nlc
