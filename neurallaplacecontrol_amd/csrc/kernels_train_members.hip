// Per-member settings and patience of a trainer group (nlc_*_train_group_step_members, nlc_train_patience; abi_train.hip):
//
//   train_adam_members_kernel  train_adam_kernel's grid (the ChunkTable's cstart[kTensors] chunks on x, the member on y, the
//                              same GroupStrides) and its body, clip_adam (nlc_train_dev.h), with lr, weight decay, clip
//                              norm and the active flag read from four device arrays [M].  Betas, eps and the step count
//                              stay the group's: the host passes omb1, beta2, omb2, eps, bc1 and bc2_sqrt, and the kernel
//                              forms step_size = -(lr[m] / bc1) with one FP64 division (correctly rounded: v_div_scale /
//                              v_div_fmas / v_div_fixup, no reciprocal).  A member with active[m] == 0 gets gradnorm[m] from
//                              workgroup 0 and nothing else: its workgroups return before any access to params, m or v, so
//                              its three rows are not even rewritten.
//   train_patience_kernel      one thread per member, after train_commit_best_kernel in stream order: patience_step
//                              (nlc_train_members.h), the reference's waiting / patience counter (train_utils.py:439-448).
//
// The norm, the coefficient, the chunk walk and the element loop are train_adam_kernel's own code, so an active member's
// bits are those of train_adam_kernel with that member's scalars.  No atomics; LDS is the one coefficient word.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage): docs/training.md, "The back end of a step, written once".
#include "nlc_train_dev.h"  // first: brings the HIP runtime in before nlc_train.h's __host__ __device__ math
#include "nlc_train_members.h"

namespace nlc {
namespace train {

__global__ __launch_bounds__(kThreads) void train_adam_members_kernel(const MembersAdamArgs a) {
  const int64_t mi = blockIdx.y;  // member of the group: its own settings
  const bool active = a.active[mi] != 0;
  if (!active && blockIdx.x != 0) return;  // (uniform over the workgroup) a frozen member: workgroup 0 stays for the norm
  const AdamScalars k{a.wd[mi], a.omb1, a.beta2, a.omb2, member_step_size(a.lr[mi], a.bc1), a.bc2_sqrt, a.eps};
  clip_adam(a.params, a.m, a.v, a.grad, a.sq, a.gradnorm, a.ct, a.gs, a.max_norm[mi], k, active);
}

__global__ __launch_bounds__(kPatienceThreads) void train_patience_kernel(const PatienceArgs a) {
  const int64_t m = (int64_t)blockIdx.x * kPatienceThreads + threadIdx.x;
  if (m >= a.M) return;
  int64_t waiting = a.waiting[m], stopped_at = a.stopped_at[m];
  int32_t active = a.active[m];
  if (active == 0) return;
  patience_step(a.improved[m] != 0, a.patience, a.tag, &waiting, &active, &stopped_at);
  a.waiting[m] = waiting;
  a.active[m] = active;
  a.stopped_at[m] = stopped_at;
}

hipError_t launch_train_adam_members(const MembersAdamArgs& a, int M, hipStream_t s) {
  hipLaunchKernelGGL(train_adam_members_kernel, dim3(a.ct.cstart[kTensors], M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_train_patience(const PatienceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(train_patience_kernel, dim3((a.M + kPatienceThreads - 1) / kPatienceThreads), dim3(kPatienceThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace train
}  // namespace nlc
