// Representation function alone (nl_repfunc_kernel) for hidden_units = 256 (see kernels_nl.hip; a translation unit of its own: the width-256 instances are the
// longest compiles of the library, and the build is as long as its longest unit).
#include "nlc_nl_launch.h"

namespace nlc {

template hipError_t launch_nl_repfunc_ht<16, false>(const RepFuncArgs&, hipStream_t);
template hipError_t launch_nl_repfunc_ht<16, true>(const RepFuncArgs&, hipStream_t);

}  // namespace nlc
