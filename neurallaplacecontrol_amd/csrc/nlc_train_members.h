// Per-member hyper-parameters and patience of a trainer group (kernels_train_members.hip, abi_train.hip): the clip + Adam
// launch of a group step with lr, weight decay, clip norm and an "active" flag read per member from device arrays, and the
// reference's early-stopping counter (train_utils.py:315-317, :439-448) per member on the device.  Plain C++:
// tests/helpers/train_members_host.cpp compiles the rule and the step-size expression with g++.
//
// A header of its own: the training, evaluation and selection kernels do not include it.  The element math is nlc_train.h's
// adam_element and clip_coef, called unchanged.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nlc_train.h"

namespace nlc {
namespace train {

constexpr int kPatienceThreads = 256;

// torch.optim.Adam's step_size of one member, -(lr / bc1) with bc1 = 1 - beta1 ** step: one correctly rounded FP64 division
// and a sign flip, which is Python's (lr / bc1) * -1 of the single trainer bit for bit.  No reciprocal, no fast-math form.
NLC_HD double member_step_size(double lr, double bc1) { return -(lr / bc1); }

// The reference's rule at one check (train_utils.py:439-448), for a member that is still active:
//   if cum_loss < best_loss: waiting = 0        (improved: nlc_train_keep_best's flag of this check)
//   elif waiting > patience: break              (the member stops: active = 0, stopped_at = tag)
//   else: waiting += 1
// patience is a double so that the reference's default, inf, never stops a member; the comparison is strict, so patience 0
// stops at the second check in a row without improvement.  A member with active == 0 is left alone.
NLC_HD void patience_step(bool improved, double patience, int64_t tag, int64_t* waiting, int32_t* active, int64_t* stopped_at) {
  if (*active == 0) return;
  if (improved) {
    *waiting = 0;
  } else if ((double)*waiting > patience) {
    *active = 0;
    *stopped_at = tag;
  } else {
    *waiting = *waiting + 1;
  }
}

// AdamArgs with the three per-member settings and the flag in device arrays [gridDim.y]; betas, eps and the step count (bc1,
// bc2_sqrt) stay one per group
struct MembersAdamArgs {
  double *params, *m, *v;
  const double* grad;
  const double* sq;
  const double* lr;        // [M]
  const double* wd;        // [M]; 0: no decay term
  const double* max_norm;  // [M]; <= 0: no clipping
  const int32_t* active;   // [M]; 0: the member's rows of params / m / v are neither read nor written
  double omb1, beta2, omb2, eps, bc1, bc2_sqrt;
  double* gradnorm;  // [M]; may be NULL; written for frozen members too
  ChunkTable ct;
  GroupStrides gs;  // params / m / v by params, grad by grad, sq by ws
};
static_assert(sizeof(MembersAdamArgs) == 376 && offsetof(MembersAdamArgs, ct) == 128 && offsetof(MembersAdamArgs, gs) == 336,
              "MembersAdamArgs: the table sits where off[] and cstart[] sat");

struct PatienceArgs {
  const int32_t* improved;  // [M]
  int64_t* waiting;         // [M]
  int32_t* active;          // [M]
  int64_t* stopped_at;      // [M]
  double patience;
  int64_t tag;
  int M;
};

}  // namespace train
}  // namespace nlc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace nlc {
namespace train {
// the grid of launch_train_adam: cstart[kTensors] chunks on x, the M members on y
hipError_t launch_train_adam_members(const MembersAdamArgs& a, int M, hipStream_t s);
// one thread per member
hipError_t launch_train_patience(const PatienceArgs& a, hipStream_t s);
}  // namespace train
}  // namespace nlc
#endif
