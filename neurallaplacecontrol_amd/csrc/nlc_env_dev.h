// Device bodies of one env control step, shared by env_step_kernel (kernels_mppi.hip) and collect_step_kernel
// (kernels_collect.hip): the reduced-state rhs, the Euler update, the trig observation, the reward and the delay-buffer roll.
// The two kernels must produce the SAME bits for the same step (tests/test_gpu_collector.py pins them with torch.equal): every
// unit that includes this header is built with -ffp-contract=off (csrc/Makefile, EXTRA_<unit>), as env_step_kernel's unit
// always was, so that a*b+c is a multiply and an add in both.
#pragma once
#include "nlc_device.h"
#include "nlc_kernels.h"

namespace nlc {

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

__device__ __forceinline__ int env_state_dim(int env) { return (env == NLC_ENV_PENDULUM) ? 2 : 4; }
__device__ __forceinline__ int env_obs_dim(int env) {
  return (env == NLC_ENV_CARTPOLE) ? 5 : ((env == NLC_ENV_PENDULUM) ? 3 : 6);
}

// Reduced-state rhs of the three envs (ctcartpole.py:185-237, ctpendulum.py:111-125, ctacrobot.py:168-228; the 4-D /
// 2-D branches: explicit angles).  Only cartpole clamps the action inside its rhs.
__device__ __forceinline__ void env_rhs(int env, const double* s, const double* a, int friction, double* ds) {
  if (env == NLC_ENV_CARTPOLE) {
    const double xd = s[1], th = s[2], thd = s[3];
    const double c = cos(th), sn = sin(th);
    const double g = 9.8, fmag = 3.0, mc = 1.0, mp = 0.1, len = 1.0;
    const double mt = mp + mc, pml = mp * len;
    const double force = clampd(a[0], -fmag, fmag) * fmag;
    double temp, thacc;
    if (friction) {
      const double sg = (xd > 0.0) ? 1.0 : ((xd < 0.0) ? -1.0 : 0.0);
      temp = (force + pml * thd * thd * sn - 5e-4 * sg) / mt;
      thacc = (g * sn - c * temp - 2e-6 * thd / pml) / (len * (4.0 / 3.0 - mp * c * c / mt));
    } else {
      temp = (force + pml * thd * thd * sn) / mt;
      thacc = (g * sn - c * temp) / (len * (4.0 / 3.0 - mp * c * c / mt));
    }
    ds[0] = xd;
    ds[1] = temp - pml * thacc * c / mt;
    ds[2] = thd;
    ds[3] = thacc;
  } else if (env == NLC_ENV_PENDULUM) {
    ds[0] = s[1];
    ds[1] = -15.0 * sin(s[0] + kPi) + 3.0 * a[0];  // -3g/(2l), 3/(m l^2)
  } else {
    const double th1 = s[0], th2 = s[1], d1v = s[2], d2v = s[3];
    const double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8;
    const double c2 = cos(th2), s2 = sin(th2);
    const double D1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2 * l1 * lc2 * c2) + I1 + I2;
    const double D2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2;
    const double phi2 = m2 * lc2 * g * cos(th1 + th2 - kPi / 2.0);
    const double phi1 = -m2 * l1 * lc2 * (d2v * d2v) * s2 - 2 * m2 * l1 * lc2 * d2v * d1v * s2 +
                        (m1 * lc1 + m2 * l1) * g * cos(th1 - kPi / 2) + phi2;
    const double dd2 = (a[0] + D2 / D1 * phi1 - m2 * l1 * lc2 * (d1v * d1v) * s2 - phi2) /
                       (m2 * (lc2 * lc2) + I2 - (D2 * D2) / D1);
    ds[0] = d1v;
    ds[1] = d2v;
    ds[2] = -(a[1] + D2 * dd2 + phi1) / D1;
    ds[3] = dd2;
  }
}
// torch_transform_states: reduced state -> trig observation
__device__ __forceinline__ void env_observe(int env, const double* s, double* o) {
  if (env == NLC_ENV_CARTPOLE) {
    o[0] = s[0];
    o[1] = s[1];
    o[2] = 1.0 * cos(s[2]);
    o[3] = 1.0 * sin(s[2]);
    o[4] = s[3];
  } else if (env == NLC_ENV_PENDULUM) {
    o[0] = cos(s[0]);
    o[1] = sin(s[0]);
    o[2] = s[1];
  } else {
    o[0] = cos(s[0]);
    o[1] = sin(s[0]);
    o[2] = cos(s[1]);
    o[3] = sin(s[1]);
    o[4] = s[2];
    o[5] = s[3];
  }
}
// diff_reward(s, a) on the reduced state, as integrate_system evaluates it (base_env.py:164)
__device__ __forceinline__ double env_reward(int env, const double* s, const double* a, int nu) {
  double uu = 0.0;
  for (int j = 0; j < nu; ++j) uu += a[j] * a[j];
  if (env == NLC_ENV_CARTPOLE) {
    const double e0 = s[0] + 1.0 * sin(s[2]) - 0.0, e1 = 1.0 * cos(s[2]) - 1.0;
    return (-(e0 * e0 + e1 * e1) + 0.01 * (-(s[1] * s[1]) - s[3] * s[3])) + (-0.01 * uu);
  } else if (env == NLC_ENV_PENDULUM) {
    const double c = cos(s[0]), sn = sin(s[0]);
    const double om = 1.0 - c;
    return (-1.0 * (om * om + sn * sn) + 0.01 * (-(s[1] * s[1]))) + (-0.01 * uu);
  }
  const double p1x = -1.0 * cos(s[0]), p1y = 1.0 * sin(s[0]);
  const double p2x = p1x - 1.0 * cos(s[0] + s[1]), p2y = p1y + 1.0 * sin(s[0] + s[1]);
  const double ex = p2x - 1.0 - 1.0;
  return ((-(ex * ex) - p2y * p2y) + 1e-1 * (-(s[2] * s[2]) - s[3] * s[3])) + (-1e-4 * uu);
}
// get_action (mppi_with_model.py:25-28) on the action columns of one env's buffer: rows of W doubles (W = nu, or nu + 1 with
// the collector's time channel, whose column nlc_collect.h handles), rolled by one row, the new action in the last row;
// `at` = the applied action, row B - 1 - delay
__device__ __forceinline__ void env_roll_buffer(double* ab, int B, int W, int nu, int delay, const double* action, double* at) {
  for (int r = 0; r + 1 < B; ++r)
    for (int j = 0; j < nu; ++j) ab[r * W + j] = ab[(r + 1) * W + j];
  for (int j = 0; j < nu; ++j) ab[(B - 1) * W + j] = action[j];
  for (int j = 0; j < nu; ++j) at[j] = ab[(B - 1 - delay) * W + j];
}
// odeint(method="euler") over ts = [0, h]: one explicit Euler step of the rhs on the reduced state
__device__ __forceinline__ void env_euler_step(int env, double* s, const double* at, int friction, double h) {
  const int n = env_state_dim(env);
  double ds[4];
  env_rhs(env, s, at, friction, ds);
  for (int i = 0; i < n; ++i) s[i] = s[i] + h * ds[i];
}

}  // namespace nlc
