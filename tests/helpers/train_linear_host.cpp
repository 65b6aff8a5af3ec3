// Host build of the linear-ILT (fixed Talbot / Stehfest) element math of the fused training step
// (neurallaplacecontrol_amd/csrc/nlc_train.h) for tests/test_train_linear_host.py (g++, no GPU).  With a main() of its own
// (-DNLC_T_MAIN) it is a stand-alone program for sanitizer builds.
#include "../../neurallaplacecontrol_amd/csrc/nlc_train.h"
using namespace nlc::train;
extern "C" {
// n rows of S terms.  y (n, 2, S): the tanh outputs behind [theta | phi]; t (n); wr, wi (S).  Out:
//   x (n)          the prediction linear_row_sum / t, as the kernel forms it
//   val (n, S)     the terms R c of linear_phase
//   dth, dph (n, S) d x / d theta_k, d x / d phi_k: ilt_term_bwd with w = 1 and g = 1 / t
//   dpre (n, 2, S) d x / d pre-activation (y = tanh(pre)): linear_row_bwd with g = 1 / t
void nlc_t_linear_rows(const double* y, const double* t, const double* wr, const double* wi, long n, int S, double* x,
                       double* val, double* dth, double* dph, double* dpre) {
  for (long i = 0; i < n; ++i) {
    const double* yt = y + 2 * i * S;
    const double* yp = yt + S;
    x[i] = linear_row_sum(yt, yp, wr, wi, S) / t[i];
    const double g = 1.0 / t[i];
    for (int k = 0; k < S; ++k) {
      double c, cp;
      linear_phase(sphere_theta(yt[k]), wr[k], wi[k], &c, &cp);
      const double R = sphere_radius(sphere_phi(yp[k]));
      val[i * S + k] = R * c;
      ilt_term_bwd(g, 1.0, R, c, cp, &dth[i * S + k], &dph[i * S + k]);
    }
    linear_row_bwd(g, yt, yp, wr, wi, S, dpre + 2 * i * S, dpre + 2 * i * S + S);
  }
}
// query points: node_re, node_im (S), t (n) -> theta_s, phi_s (n, S)
void nlc_t_linear_query(const double* node_re, const double* node_im, const double* t, long n, int S, double* th, double* ph) {
  for (long i = 0; i < n; ++i)
    for (int k = 0; k < S; ++k) linear_query_point(node_re[k], node_im[k], t[i], &th[i * S + k], &ph[i * S + k]);
}
}

#ifdef NLC_T_MAIN
#include <cstdio>
#include <vector>
// every entry once at S = 1 .. 33 on in-range inputs; a sanitizer reports what the loops touch out of bounds
int main() {
  double sum = 0.0;
  for (int S = 1; S <= 33; ++S) {
    const long n = 5;
    std::vector<double> y(n * 2 * S), t(n), wr(S), wi(S), x(n), val(n * S), dth(n * S), dph(n * S), dpre(n * 2 * S), th(n * S),
        ph(n * S);
    for (size_t i = 0; i < y.size(); ++i) y[i] = -0.9 + 1.8 * (double)((i * 37) % 101) / 100.0;
    for (long i = 0; i < n; ++i) t[i] = 0.02 + 0.2 * (double)i;
    for (int k = 0; k < S; ++k) {
      wr[k] = 1.0 + k;
      wi[k] = 0.5 * k;
    }
    nlc_t_linear_rows(y.data(), t.data(), wr.data(), wi.data(), n, S, x.data(), val.data(), dth.data(), dph.data(), dpre.data());
    nlc_t_linear_query(wr.data(), wi.data(), t.data(), n, S, th.data(), ph.data());
    for (long i = 0; i < n; ++i) sum += x[i] + th[i * S] + ph[i * S + S - 1] + dpre[2 * i * S + 2 * S - 1];
  }
  std::printf("ok %.17g\n", sum);
  return 0;
}
#endif
