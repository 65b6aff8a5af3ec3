// Single model forward (nl_forward_kernel) for hidden_units = 256, per-row query times (see kernels_nl.hip; a
// translation unit of its own: the build is as long as its longest unit).
#include "nlc_nl_launch.h"

namespace nlc {

template hipError_t launch_nl_forward_ht<16, true>(const ForwardArgs&, hipStream_t);

}  // namespace nlc
