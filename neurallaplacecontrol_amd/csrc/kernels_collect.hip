// Expert-data collection: one control step of the collector's loop() / step_env() for E envs, recorded as dataset rows.
//   loop()      mppi_dataset_collector.py:224-309   (s0, action noise + clip, a0 / sn / ts rows, episode return)
//   step_env()  :192-222                            (get_action, integrate_system(2, g), time channel, observation noise)
// One lane per env; every lane touches only its own env's state, buffer, return and dataset row, so there is no
// communication, no atomics and no LDS.  The dynamics, observation, reward and buffer roll are the device bodies
// env_step_kernel runs (nlc_env_dev.h); the element math of the collector itself is nlc_collect.h (host-testable).
// Memory-bound on the row stores: (2 d + B W + 1) doubles per env and step.  Built with -ffp-contract=off (csrc/Makefile), as
// nlc_env_dev.h requires.
#include "nlc_device.h"

#include "nlc_collect.h"
#include "nlc_env_dev.h"
#include "nlc_kernels.h"

namespace nlc {

// one Philox block of (global episode, step, stream): a draw depends on nothing else (not on E, the lane or the batching)
__device__ __forceinline__ u4 collect_block(uint64_t seed, int64_t episode, int it, uint32_t stream) {
  return philox4x32_10(u4{(uint32_t)episode, (uint32_t)((uint64_t)episode >> 32), (uint32_t)it, stream}, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}
// two standard normals of one block (Box-Muller, as mppi_draw)
__device__ __forceinline__ void collect_normal_pair(const u4 r, double* z0, double* z1) {
  const double u1 = u53(r.x, r.y), u2 = u53(r.z, r.w);
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  m::sincos_bounded(2.0 * kPi * u2 - kPi, &sn, &cs);  // angle in (-pi, pi)
  *z0 = rad * cs;
  *z1 = rad * sn;
}

__global__ __launch_bounds__(256) void collect_step_kernel(const CollectStepArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  const int n = env_state_dim(a.env), d = env_obs_dim(a.env);
  const int W = a.nu + a.time_channel;
  const int64_t episode = a.episode_base + e;
  const int64_t row = collect::row_index(a.episode_base, e, a.steps_per_episode, a.it);
  double s[4], o[6];
  for (int i = 0; i < n; ++i) s[i] = a.state[e * n + i];
  // 1. s0: the observation the planner was given
  env_observe(a.env, s, o);
  for (int i = 0; i < d; ++i) a.s0[row * d + i] = o[i];
  // 2. the action
  double act[NLC_MAX_NU];
  {
    const bool random = a.policy == NLC_POLICY_RANDOM;
    double u[2] = {0.5, 0.5};
    if (random || a.action_noise >= 0.0) {
      const u4 r = collect_block(a.seed, episode, a.it, random ? collect::kStreamRandomPolicy : collect::kStreamActionNoise);
      u[0] = u53(r.x, r.y);
      u[1] = u53(r.z, r.w);
    }
    static_assert(NLC_MAX_NU <= 2, "one Philox block yields two uniforms");
#pragma unroll
    for (int j = 0; j < NLC_MAX_NU; ++j) {
      act[j] = 0.0;
      if (j < a.nu)
        act[j] = random ? collect::random_action(u[j], a.action_low, a.action_high)
                        : collect::noisy_action(a.action[e * a.nu + j], u[j], a.action_low, a.action_high, a.action_noise);
    }
  }
  // 3. the action buffer
  double* ab = a.abuf + e * a.B * W;
  double at[NLC_MAX_NU];
  env_roll_buffer(ab, a.B, W, a.nu, a.delay, act, at);
  if (a.time_channel) collect::time_channel_roll(ab, a.B, W, a.nu);
  // 4. the interval
  double tsn = a.dt;
  if (a.ts_grid != NLC_TS_GRID_FIXED) {
    const u4 r = collect_block(a.seed, episode, a.it, collect::kStreamInterval);
    tsn = collect::interval(a.ts_grid, a.dt, u53(r.x, r.y));
  }
  // 5. one Euler step of size tsn; the reward sees the state before the observation noise
  env_euler_step(a.env, s, at, a.friction, tsn);
  a.ret[e] = a.ret[e] + env_reward(a.env, s, at, a.nu);
  // 6. time channel, observation noise on the reduced state (it persists: the noisy state is stored)
  if (a.time_channel) collect::time_channel_advance(ab, a.B, W, a.nu, tsn);
  if (a.obs_noise != 0.0) {
    double z[4];
    collect_normal_pair(collect_block(a.seed, episode, a.it, collect::kStreamObsNoise), &z[0], &z[1]);
    z[2] = z[3] = 0.0;
    if (n > 2) collect_normal_pair(collect_block(a.seed, episode, a.it, collect::kStreamObsNoise + 1), &z[2], &z[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) s[i] = s[i] + z[i] * a.obs_noise;
  }
  for (int i = 0; i < n; ++i) a.state[e * n + i] = s[i];
  // 7. the rest of the row
  env_observe(a.env, s, o);
  for (int i = 0; i < d; ++i) a.sn[row * d + i] = o[i];
  const int bw = a.B * W;
  for (int i = 0; i < bw; ++i) a.a0[row * bw + i] = ab[i];
  a.ts[row] = tsn;
}

hipError_t launch_collect_step(const CollectStepArgs& a, hipStream_t s) {
  if (a.E <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(collect_step_kernel, dim3((unsigned)((a.E + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace nlc
