// Representation MLP + ILT + rollout kernels for hidden_units = 256: see kernels_nl.hip.
#include "nlc_nl_launch.h"

namespace nlc {

template hipError_t launch_nl_rollout_ht<16, false>(const RolloutArgs&, hipStream_t, bool);

}  // namespace nlc
