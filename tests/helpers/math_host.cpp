// Host build of neurallaplacecontrol_amd/csrc/nlc_math.h for tests/test_math_host.py (g++, no GPU).  tools/math_dev_check.hip
// exports the same symbols from the device build (tests/test_gpu_math_device.py); every entry returns 0 (the device build's
// report a failed HIP call).
#include "../../neurallaplacecontrol_amd/csrc/nlc_math.h"
#include "../../tools/nlc_math_table.h"  // the measured-and-dropped table-driven alternative (not in the product)
extern "C" {
int nlc_t_tanh(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::tanh_d(x[i]); return 0; }
int nlc_t_sigmoid(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::sigmoid_d(x[i]); return 0; }
int nlc_t_exp(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::exp_d(x[i]); return 0; }
int nlc_t_sin(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) { double s, c; nlc::m::sincos_bounded(x[i], &s, &c); y[i] = s; } return 0; }
int nlc_t_cos(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) { double s, c; nlc::m::sincos_bounded(x[i], &s, &c); y[i] = c; } return 0; }
int nlc_t_tan(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::tan_0_halfpi(x[i]); return 0; }
}
extern "C" {
int nlc_t_tan_pi4(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::tan_pi4_plus(x[i]); return 0; }
int nlc_t_cosq(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::cos_quadrant(x[i], (int)(i % 7) - 3); return 0; }
}
static const double kTab[64] = {NLC_EXP_TABLE_VALUES};
extern "C" {
int nlc_t_tanh_t(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::tanh_t(x[i], kTab); return 0; }
int nlc_t_sigmoid_t(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::sigmoid_t(x[i], kTab); return 0; }
}
extern "C" {
// short forms of the Fourier ILT kernel: cos(x + m pi/2) with m = i & 1, tan(x) on [0, pi/2] as num/den
int nlc_t_cos_mpio2(const double* x, double* y, long n) {
  for (long i = 0; i < n; ++i) {
    const double dm = (double)(i & 1);
    y[i] = nlc::m::cos_plus_mpio2(nlc::m::ilt_trig_k(), x[i], 0.5 * dm, dm);
  }
  return 0;
}
int nlc_t_tan_short(const double* x, double* y, long n) {
  for (long i = 0; i < n; ++i) {
    double num, den;
    nlc::m::tan_parts_short(nlc::m::ilt_trig_k(), x[i], &num, &den);
    y[i] = num / den;
  }
  return 0;
}
int nlc_t_sin_mpio2(const double* x, double* y, long n) {
  for (long i = 0; i < n; ++i) {
    const double dm = (double)(i & 1);
    double sn, cs;
    nlc::m::sincos_plus_mpio2(nlc::m::ilt_trig_k(), x[i], 0.5 * dm, dm, &sn, &cs);
    y[i] = sn;
  }
  return 0;
}
}
extern "C" {
// round 3: the rollout kernels' hidden-layer activation (instruction count over ulps): pairs (x[i], x[i + 1])
int nlc_t_tanh_pair_fast(const double* x, double* y, long n) {
  for (long i = 0; i + 1 < n; i += 2) nlc::m::tanh_pair_fast(x[i], x[i + 1], &y[i], &y[i + 1]);
  if (n & 1) { double t; nlc::m::tanh_pair_fast(x[n - 1], 0.0, &y[n - 1], &t); }
  return 0;
}
}
extern "C" {
// round 6: the row-per-lane Fourier ILT kernel's forms -- tan(pi/4 + a) as num/den (Cephes rational), cos(x + m pi/2) with m = i & 1
int nlc_t_tan_rat(const double* a, double* y, long n) {
  for (long i = 0; i < n; ++i) {
    double num, den;
    nlc::m::tan_parts_rat(nlc::m::ilt_row_k(), a[i], &num, &den);
    y[i] = num / den;
  }
  return 0;
}
int nlc_t_cos_kpio2(const double* x, double* y, long n) {
  for (long i = 0; i < n; ++i)
    y[i] = (i & 1) ? -nlc::m::cos_or_sin_reduced<1>(nlc::m::ilt_row_k(), x[i]) : nlc::m::cos_or_sin_reduced<0>(nlc::m::ilt_row_k(), x[i]);
  return 0;
}
}
extern "C" {
int nlc_t_sincos_reduced(const double* x, double* sn, double* cs, long n) {
  for (long i = 0; i < n; ++i) nlc::m::sincos_reduced(nlc::m::ilt_row_k(), x[i], &sn[i], &cs[i]);
  return 0;
}
}
extern "C" {
// the functions every other one here is built from (pairs (x[i], x[i + 1]) as in nlc_t_tanh_pair_fast)
int nlc_t_tanh_pair_d(const double* x, double* y, long n) {
  for (long i = 0; i + 1 < n; i += 2) nlc::m::tanh_pair_d(x[i], x[i + 1], &y[i], &y[i + 1]);
  if (n & 1) { double t; nlc::m::tanh_pair_d(x[n - 1], 0.0, &y[n - 1], &t); }
  return 0;
}
int nlc_t_exp_neg(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::exp_neg(x[i]); return 0; }
int nlc_t_expm1_neg(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::expm1_neg(x[i]); return 0; }
int nlc_t_rcp_refined(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::rcp_refined(x[i]); return 0; }
int nlc_t_div_fast(const double* num, const double* den, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::div_fast(num[i], den[i]); return 0; }
int nlc_t_min_abs(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = nlc::m::min_abs(x[i], 372.5); return 0; }
}
