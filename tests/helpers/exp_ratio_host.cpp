// Host build of the rational exponential of neurallaplacecontrol_amd/csrc/nlc_math.h (exp_ratio_parts) and of the gate forms
// built on it, for tests/test_exp_ratio_host.py (g++, no GPU).  What the device build computes -- the shipped sigmoid_pair2 / tanh2
// themselves, the two-wide instantiation, v_rcp_f64 + refinement, the v_min_f64 clamps -- is measured by
// tests/test_gpu_math_device.py, which runs the same tests on tools/math_dev_check.hip's build of these symbols.
#include "../../neurallaplacecontrol_amd/csrc/nlc_math.h"
using namespace nlc::m;
extern "C" {
// e^y = 2^n num / den: m[i] = 2^n num, d[i] = den (HALF = 0), or from the half argument y / 2 (HALF = 1, tanh's form)
int nlc_t_exp_ratio(const double* y, double* m, double* d, long n, int half) {
  for (long i = 0; i < n; ++i) {
    double num, den, sh;
    if (half)
      exp_ratio_parts<true>(0.5 * y[i], &num, &den, &sh);
    else
      exp_ratio_parts<false>(y[i], &num, &den, &sh);
    m[i] = ldexp(num, exp_shift_int(sh));
    d[i] = den;
  }
  return 0;
}
// sigmoid_pair2 of nlc_gru_tile.h on (x[i], x[i + 1]) as (a, b) of one hidden unit and (x[i + 2], x[i + 3]) as the other's
int nlc_t_sigmoid_ratio(const double* x, double* y, long n) {
  for (long i = 0; i + 3 < n; i += 4) {
    double D[4], Q[4];
    for (int k = 0; k < 4; ++k) {
      double num, sh;
      exp_ratio_parts<false>(fmin(-x[i + k], 170.0), &num, &D[k], &sh);
      Q[k] = D[k] + ldexp(num, exp_shift_int(sh));
    }
    const double P0 = Q[0] * Q[1], P1 = Q[2] * Q[3];
    const double R = 1.0 / (P0 * P1);
    const double inv0 = P1 * R, inv1 = P0 * R;
    y[i] = (D[0] * Q[1]) * inv0;
    y[i + 1] = (D[1] * Q[0]) * inv0;
    y[i + 2] = (D[2] * Q[3]) * inv1;
    y[i + 3] = (D[3] * Q[2]) * inv1;
  }
  return 0;
}
// tanh_pair_fast (the rollout's hidden activation; tanh2 of nlc_gru_tile.h is the same arithmetic two-wide)
int nlc_t_tanh_ratio(const double* x, double* y, long n) {
  for (long i = 0; i + 1 < n; i += 2) tanh_pair_fast(x[i], x[i + 1], &y[i], &y[i + 1]);
  return 0;
}
}
