// Launchers of the representation MLP + ILT + rollout kernels (nlc_nl_kernels.h) for one hidden width h = 16 HT, declared in
// nlc_kernels.h.  Included by the units that instantiate them (the list in nlc_kernels.h).
#pragma once
#include "nlc_nl_kernels.h"

namespace nlc {

// LIN: fixed Talbot / Stehfest models (kernels_nl_lin.hip), which need the second coefficient matrix Cp2
template <int HT, bool LIN>
hipError_t launch_nl_rollout_ht(const RolloutArgs& a, hipStream_t s, bool split) {
  if constexpr (LIN) {
    if (a.net.Cp2 == nullptr || a.net.lin != 1) return hipErrorInvalidValue;
  }
  if (split) {
    if (a.cost_variant != 0)  // the cost variant's instance of the body
      return launch_nt3(a.net.nt3, [&](auto nt3) {
        hipLaunchKernelGGL((nl_rollout_split_kernel<HT, nt3, LIN, true>), dim3((unsigned)((a.K + 15) / 16)), dim3(256), 0, s, a);
      });
    return launch_nt3(a.net.nt3, [&](auto nt3) {
      hipLaunchKernelGGL((nl_rollout_split_kernel<HT, nt3, LIN>), dim3((unsigned)((a.K + 15) / 16)), dim3(256), 0, s, a);
    });
  }
  if (a.cost_variant != 0) return hipErrorInvalidValue;  // (the wave-per-tile body has no such instance: the host's post-pass)
  return launch_nt3(a.net.nt3, [&](auto nt3) {
    hipLaunchKernelGGL((nl_rollout_kernel<HT, nt3, LIN>), dim3((unsigned)((a.K + 63) / 64)), dim3(256), 0, s, a);
  });
}

template <int HT, bool GENERAL_T>
hipError_t launch_nl_forward_ht(const ForwardArgs& a, hipStream_t s) {
  return launch_nt3(a.net.nt3, [&](auto nt3) {
    hipLaunchKernelGGL((nl_forward_kernel<HT, nt3, GENERAL_T>), dim3((unsigned)((a.N + 63) / 64)), dim3(256), 0, s, a);
  });
}

template <int HT, bool GENERAL_T>
hipError_t launch_nl_repfunc_ht(const RepFuncArgs& a, hipStream_t s) {
  // the latency-split form is built for the planner path at h = 128 only (abi_planner_nl.hip sets split there)
  if constexpr (HT == 8 && !GENERAL_T) {
    if (a.slot_major && !a.write_angles && a.split) {
      return launch_nt3(a.net.nt3, [&](auto nt3) {
        hipLaunchKernelGGL((nl_repfunc_split_kernel<HT, nt3>), dim3((unsigned)((a.N + 15) / 16)), dim3(256), 0, s, a);
      });
    }
  }
  return launch_nt3(a.net.nt3, [&](auto nt3) {
    hipLaunchKernelGGL((nl_repfunc_kernel<HT, nt3, GENERAL_T>), dim3((unsigned)((a.N + 63) / 64)), dim3(256), 0, s, a);
  });
}

}  // namespace nlc
