// Host build of the NODE training step's element math (neurallaplacecontrol_amd/csrc/nlc_train_node.h: the fixed Euler grid
// and the backward of one sub-step) for tests/test_train_node_host.py (g++, no GPU).  With a main() of its own (-DNLC_T_MAIN)
// it is a stand-alone program for sanitizer builds.
#include "../../neurallaplacecontrol_amd/csrc/nlc_train_node.h"
using namespace nlc::train;
extern "C" {
int nlc_t_node_max_sub(void) { return kNodeTrainMaxSub; }
// n end times -> nsub (n), bad (n), widths (n, kNodeTrainMaxSub; entries past nsub untouched)
void nlc_t_node_grid(const double* t_end, double step, long n, int* nsub, int* bad, double* h) {
  for (long i = 0; i < n; ++i) nsub[i] = node_euler_grid(t_end[i], step, h + i * kNodeTrainMaxSub, &bad[i]);
}
// one row, one sub-step x' = x + h f(cat(x, u)): blob [W0 | b0 | W2 | b2 | W4 | b4]; out: f (dy), a1, a2 (H), then for
// xbar_next = dL/dx': d3 (dy), d2, d1 (H), xbar (dy)
void nlc_t_node_substep(const double* blob, int H, int dy, int nu, const double* x, const double* u, double h,
                        const double* xbar_next, double* f, double* a1, double* a2, double* d3, double* d2, double* d1,
                        double* xbar) {
  const int in = dy + nu;
  const double* W0 = blob;
  const double* b0 = W0 + (long)H * in;
  const double* W2 = b0 + H;
  const double* b2 = W2 + (long)H * H;
  const double* W4 = b2 + H;
  const double* b4 = W4 + (long)dy * H;
  node_func_row(W0, b0, W2, b2, W4, b4, H, dy, nu, x, u, a1, a2, f);
  node_substep_bwd_row(W0, W2, W4, H, dy, nu, h, xbar_next, a1, a2, d3, d2, d1, xbar);
}
}

#ifdef NLC_T_MAIN
#include <cstdio>
#include <limits>
#include <vector>
// the grid at in-range, bad and over-long times and the sub-step at every width the tests use; a sanitizer reports what the
// loops touch out of bounds
int main() {
  double sum = 0.0;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double ts[] = {0.05, 0.1, 0.125, 0.15, 0.4, 1e-9, 0.399999, 12.8, 0.0, -1.0, nan, 12.85, 1e300, inf};
  const long n = sizeof(ts) / sizeof(ts[0]);
  std::vector<int> nsub(n), bad(n);
  std::vector<double> h(n * kNodeTrainMaxSub, 0.0);
  nlc_t_node_grid(ts, 0.05, n, nsub.data(), bad.data(), h.data());
  for (long i = 0; i < n; ++i) {
    if (nsub[i] < 0 || nsub[i] > kNodeTrainMaxSub) return 1;
    for (int k = 0; k < nsub[i]; ++k) sum += bad[i] ? 0.0 : h[i * kNodeTrainMaxSub + k];
  }
  const int Hs[] = {1, 5, 15, 16, 17, 33, 270, 272};
  for (int H : Hs)
    for (int dy = 1; dy <= 8; dy += 7)
      for (int nu = 1; nu <= 2; ++nu) {
        const int in = dy + nu;
        std::vector<double> blob((size_t)H * in + H + (size_t)H * H + H + (size_t)dy * H + dy), x(dy), u(nu), xb(dy), f(dy), a1(H),
            a2(H), d3(dy), d2(H), d1(H), xbar(dy);
        for (size_t i = 0; i < blob.size(); ++i) blob[i] = -0.3 + 0.6 * (double)((i * 37) % 101) / 100.0;
        for (int i = 0; i < dy; ++i) x[i] = 0.1 * i - 0.2, xb[i] = 0.5 - 0.1 * i;
        for (int i = 0; i < nu; ++i) u[i] = 1.0 - i;
        nlc_t_node_substep(blob.data(), H, dy, nu, x.data(), u.data(), 0.05, xb.data(), f.data(), a1.data(), a2.data(), d3.data(),
                           d2.data(), d1.data(), xbar.data());
        sum += f[dy - 1] + d1[H - 1] + xbar[0];
      }
  std::printf("ok %.17g\n", sum);
  return 0;
}
#endif
