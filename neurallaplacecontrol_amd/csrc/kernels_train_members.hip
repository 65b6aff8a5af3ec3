// Per-member settings and patience of a trainer group (nlc_*_train_group_step_members, nlc_train_patience; abi_train.hip):
//
//   train_adam_members_kernel  train_adam_kernel's grid and chunk walk (kernels_train.hip: cstart[kTensors] chunks on x, the
//                              member on y, the same GroupStrides), with lr, weight decay, clip norm and the active flag read
//                              from four device arrays [M].  Betas, eps and the step count stay the group's: the host passes
//                              omb1, beta2, omb2, eps, bc1 and bc2_sqrt, and the kernel forms step_size = -(lr[m] / bc1) with
//                              one FP64 division (correctly rounded: v_div_scale / v_div_fmas / v_div_fixup, no reciprocal).
//                              A member with active[m] == 0 gets gradnorm[m] from workgroup 0 and nothing else: its workgroups
//                              return before any access to params, m or v, so its three rows are not even rewritten.
//   train_patience_kernel      one thread per member, after train_commit_best_kernel in stream order: patience_step
//                              (nlc_train_members.h), the reference's waiting / patience counter (train_utils.py:439-448).
//
// The element math is nlc_train.h's adam_element and clip_coef, the norm is summed in train_adam_kernel's order: an active
// member's bits are those of train_adam_kernel with that member's scalars.  No atomics; LDS is the one coefficient word.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage): docs/training.md, "Per-member settings and patience".
#include <hip/hip_runtime.h>

#include "nlc_train_members.h"

namespace nlc {
namespace train {

__global__ __launch_bounds__(kThreads) void train_adam_members_kernel(const MembersAdamArgs a) {
  __shared__ double coef_s;
  const int b = blockIdx.x;
  const int64_t mi = blockIdx.y;  // member of the group: its own settings, chunk sums, clip coefficient and slices of params / m / v
  const bool active = a.active[mi] != 0;
  if (!active && b != 0) return;  // (uniform over the workgroup)
  const double max_norm = a.max_norm[mi];
  const double* sq = a.sq + mi * a.gs.ws;
  if (threadIdx.x == 0) {
    // clip_grad_norm_: total = || (||g_0||, ..., ||g_15||) ||, every workgroup from the same sums in the same order
    double tot2 = 0.0;
    for (int i = 0; i < kTensors; ++i) {
      double s = 0.0;
      for (int c = a.cstart[i]; c < a.cstart[i + 1]; ++c) s += sq[c];
      const double n = sqrt(s);
      tot2 += n * n;
    }
    const double total = sqrt(tot2);
    coef_s = max_norm > 0.0 ? clip_coef(max_norm, total) : 1.0;
    if (b == 0 && a.gradnorm) a.gradnorm[mi] = total;
  }
  if (!active) return;  // a frozen member: the norm is reported, params / m / v are not touched
  __syncthreads();
  const double coef = coef_s;
  AdamScalars k;
  k.wd = a.wd[mi];
  k.omb1 = a.omb1;
  k.beta2 = a.beta2;
  k.omb2 = a.omb2;
  k.step_size = member_step_size(a.lr[mi], a.bc1);
  k.bc2_sqrt = a.bc2_sqrt;
  k.eps = a.eps;
  const double* grad = a.grad + mi * a.gs.grad;
  double* params = a.params + mi * a.gs.params;
  double* mom = a.m + mi * a.gs.params;
  double* var = a.v + mi * a.gs.params;
  int t = 0;
  while (t + 1 < kTensors && a.cstart[t + 1] <= b) ++t;
  const int64_t e0 = a.off[t] + (int64_t)(b - a.cstart[t]) * kChunk;
  const int64_t e1 = e0 + kChunk < a.off[t + 1] ? e0 + kChunk : a.off[t + 1];
  for (int64_t e = e0 + threadIdx.x; e < e1; e += kThreads) {
    double gv = grad[e];
    if (max_norm > 0.0) gv = gv * coef;
    double p = params[e], mm = mom[e], vv = var[e];
    adam_element(&p, &mm, &vv, gv, k);
    params[e] = p;
    mom[e] = mm;
    var[e] = vv;
  }
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
  hipLaunchKernelGGL(train_adam_members_kernel, dim3(a.cstart[kTensors], M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_train_patience(const PatienceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(train_patience_kernel, dim3((a.M + kPatienceThreads - 1) / kPatienceThreads), dim3(kPatienceThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace train
}  // namespace nlc
