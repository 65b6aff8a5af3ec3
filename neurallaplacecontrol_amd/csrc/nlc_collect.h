// Per-element math of the expert-data collector's control step (kernels_collect.hip: collect_step_kernel), the device form of
// loop() / step_env() in mppi_dataset_collector.py:192-268.  Everything here is __host__ __device__ so that
// tests/helpers/collect_host.cpp compiles the same functions with g++ and tests/test_collect_host.py checks them on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/nlc.h"
#include "nlc_math.h"

namespace nlc {
namespace collect {

// Philox streams of a control step: counter = (global episode lo, hi, step, stream), key = the collector's seed
constexpr uint32_t kStreamInterval = 0, kStreamActionNoise = 1, kStreamObsNoise = 2 /* and 3: states 2, 3 */,
                   kStreamRandomPolicy = 4;

// ---- integration interval tsn of one step from u in (0, 1)  (build_time_grid(only_one_step), base_env.py:103-120)
//   fixed    dt
//   uniform  rand * 2 * dt
//   exp      Exponential(rate 1/dt) by inversion: -dt log(u)  (u is never 0, so tsn is finite and > 0)
NLC_HD double interval(int ts_grid, double dt, double u) {
  if (ts_grid == NLC_TS_GRID_UNIFORM) return (2.0 * dt) * u;
  if (ts_grid == NLC_TS_GRID_EXP) return -dt * log(u);
  return dt;
}

// ---- the expert's command plus uniform noise, clipped  (mppi_dataset_collector.py:250-254):
//   action += ((rand - 0.5) * 2 * action_high) * random_action_noise;  action.clip(low, high)
// scale < 0 stands for `random_action_noise is None`: neither the noise nor the clip
NLC_HD double noisy_action(double a, double u, double low, double high, double scale) {
  if (scale < 0.0) return a;
  const double v = a + ((2.0 * u - 1.0) * high) * scale;
  return fmin(fmax(v, low), high);
}
// model_name == "random" (:255-256): action_space.sample(), uniform in [low, high]
NLC_HD double random_action(double u, double low, double high) { return low + (high - low) * u; }

// ---- observation-time channel: column nu of an action buffer of B rows of W = nu + 1 doubles
// get_action_with_encode_obs_time (:20-24): the column rolls with the buffer, the new row's entry is 0
NLC_HD void time_channel_roll(double* ab, int B, int W, int nu) {
  for (int r = 0; r + 1 < B; ++r) ab[r * W + nu] = ab[(r + 1) * W + nu];
  ab[(B - 1) * W + nu] = 0.0;
}
// step_env (:206-208): every entry ages by the step's interval, the newest is 0
NLC_HD void time_channel_advance(double* ab, int B, int W, int nu, double tsn) {
  for (int r = 0; r < B; ++r) ab[r * W + nu] = ab[r * W + nu] + tsn;
  ab[(B - 1) * W + nu] = 0.0;
}

// ---- dataset row of env e of the batch that starts at global episode episode_base, control step it: episode-major, as
// the reference's torch.cat over episodes lays the rows out (:426-439)
NLC_HD int64_t row_index(int64_t episode_base, int64_t e, int steps_per_episode, int it) {
  return (episode_base + e) * (int64_t)steps_per_episode + it;
}

}  // namespace collect
}  // namespace nlc
