// Host build of the cartpole state reward of the running cost's three branches (neurallaplacecontrol_amd/csrc/nlc_cost.h) for
// tests/test_cost_variant_host.py (g++, no GPU).
#include "../../neurallaplacecontrol_amd/csrc/nlc_cost.h"
using namespace nlc::cost;
extern "C" {
// rows (e0, e1) -> state reward of the variant
void nlc_c_cartpole_state_reward(const double* e, int variant, double* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = cartpole_state_reward(e[2 * i], e[2 * i + 1], variant);
}
double nlc_c_cartpole_goal_x(int variant) { return cartpole_goal_x(variant); }
}
