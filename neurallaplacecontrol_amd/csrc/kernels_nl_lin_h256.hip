// LIN instances of the rollout kernels (kernels_nl_lin.hip), hidden width 256.
#include "nlc_nl_launch.h"

namespace nlc {

template hipError_t launch_nl_rollout_ht<16, true>(const RolloutArgs&, hipStream_t, bool);

}  // namespace nlc
