// Cartpole state reward of the harness running_cost's three branches (mppi_with_model.py:145-171 -> ctcartpole.py:311-339):
// the error pair (e0, e1) of the pole tip against the goal, and the variant bits, to the reward.  __host__ __device__, so that
// tests/helpers/cost_host.cpp compiles the same functions with g++ and tests/test_cost_variant_host.py checks them on the CPU
// against oracle.envs.cartpole_cost_variant.  Contraction is off here whatever the unit is built with: the torch-CPU op order.
#pragma once
#include <math.h>

#include "../../include/nlc.h"
#include "nlc_math.h"

namespace nlc {
namespace cost {

// goal x of the pole tip: 0, or -2 / +2 on the change_goal branch (ctcartpole.py:313-319).  The closure's `if state_constraint
// / elif change_goal` (mppi_with_model.py:146-152) never passes change_goal on the constraint branch.
NLC_HD double cartpole_goal_x(int variant) {
  if ((variant & NLC_COST_STATE_CONSTRAINT) || !(variant & NLC_COST_CHANGE_GOAL)) return 0.0;
  return (variant & NLC_COST_GOAL_FLIPPED) ? 2.0 : -2.0;
}

// state_reward of ctcartpole.py:320-334.  The wall term is about 1 100 at e0 = 0 and +inf from e0 = 70.3: the accurate double
// exp (the rational gate exponentials of nlc_math.h cover a bounded range only); a +inf cost weighs exactly 0 (nlc.h).
NLC_HD double cartpole_state_reward(double e0, double e1, int variant) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (variant & NLC_COST_STATE_CONSTRAINT) return -((e0 * e0 + exp(e0 * 10.0 + 7.0)) + e1 * e1);
  return -(e0 * e0 + e1 * e1);
}

}  // namespace cost
}  // namespace nlc
