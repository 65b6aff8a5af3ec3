// Host build of the NODE's fixed-grid solvers (neurallaplacecontrol_amd/csrc/nlc_node_rk.h: the tableaus; nlc_train_node.h: the
// grid under a method's cap and one sub-step with its backward) for tests/test_node_rk_host.py (g++, no GPU).  With a main() of
// its own (-DNLC_T_MAIN) it is a stand-alone program for sanitizer builds.
#include <vector>

#include "../../neurallaplacecontrol_amd/csrc/nlc_train_node.h"
using namespace nlc;
using namespace nlc::train;
namespace {
NodeRk tableau(int method) { return method == 1 ? NodeRkOf<1>::T : method == 2 ? NodeRkOf<2>::T : NodeRkOf<0>::T; }
}  // namespace
extern "C" {
int nlc_t_rk_ok(int method) { return node_method_ok(method) ? 1 : 0; }
int nlc_t_rk_max_sub(int method) { return node_train_max_sub(method); }
// s, a [4][4], b [4]
int nlc_t_rk_tableau(int method, double* a, double* b) {
  const NodeRk T = tableau(method);
  for (int i = 0; i < kNodeMaxStages; ++i) {
    b[i] = T.b[i];
    for (int j = 0; j < kNodeMaxStages; ++j) a[i * kNodeMaxStages + j] = T.a[i][j];
  }
  return T.s;
}
// y' = lam y, y(0) = 1 over n equal sub-steps to t_end, through the stage and combine functions the kernels call
double nlc_t_rk_linear(int method, double lam, double t_end, int n) {
  const NodeRk T = tableau(method);
  const double h = t_end / n;
  double y = 1.0, k[kNodeMaxStages];
  for (int s = 0; s < n; ++s) {
    for (int i = 0; i < T.s; ++i) k[i] = lam * node_rk_stage_input(T, i, y, h, k);
    y = node_rk_combine(T, y, h, k);
  }
  return y;
}
// the grid of a row under the method's cap: count, bad flag, widths (h: node_train_max_sub(method) doubles)
int nlc_t_rk_grid(int method, double t_end, double step, int* bad, double* h) {
  const int n = node_rk_count(t_end, step, node_train_max_sub(method), bad);
  for (int k = 0; k < n; ++k) h[k] = node_euler_width(t_end, step, n, k);
  return n;
}
// one sub-step and its backward: blob [W0 | b0 | W2 | b2 | W4 | b4]; grad (the blob's size) is overwritten
void nlc_t_rk_substep(int method, const double* blob, int H, int dy, int nu, const double* y, const double* u, double h,
                      const double* ybar_next, double* y_next, double* ybar, double* grad) {
  const int in = dy + nu;
  const double* W0 = blob;
  const double* b0 = W0 + (long)H * in;
  const double* W2 = b0 + H;
  const double* b2 = W2 + (long)H * H;
  const double* W4 = b2 + H;
  const double* b4 = W4 + (long)dy * H;
  const long P = (b4 + dy) - blob;
  for (long i = 0; i < P; ++i) grad[i] = 0.0;
  std::vector<double> work((size_t)kNodeMaxStages * (kNodeMaxDy * 3 + 2 * H) + 2 * H, 0.0);
  node_rk_substep_row(tableau(method), W0, b0, W2, b2, W4, b4, H, dy, nu, y, u, h, ybar_next, y_next, ybar, grad, work.data());
}
}

#ifdef NLC_T_MAIN
#include <cstdio>
// every method at the shapes' corners; a sanitizer reports what the loops touch out of bounds
int main() {
  double sum = 0.0;
  for (int method = 0; method < kNodeMethods; ++method) {
    sum += nlc_t_rk_linear(method, -1.0, 1.0, 16);
    const int cap = nlc_t_rk_max_sub(method);
    std::vector<double> hw(cap);
    const double ts[] = {0.05, 0.125, 0.05 * cap, 0.05 * cap + 0.01, 0.0, -1.0, 1e300};
    for (double t : ts) {
      int bad = 0;
      const int n = nlc_t_rk_grid(method, t, 0.05, &bad, hw.data());
      if (n < 0 || n > cap) return 1;
      for (int k = 0; k < n; ++k) sum += bad ? 0.0 : hw[k];
    }
    const int Hs[] = {1, 17, 272};
    for (int H : Hs)
      for (int dy = 1; dy <= 8; dy += 7)
        for (int nu = 1; nu <= 2; ++nu) {
          const int in = dy + nu;
          const size_t P = (size_t)H * in + H + (size_t)H * H + H + (size_t)dy * H + dy;
          std::vector<double> blob(P), grad(P), y(dy), u(nu), yb(dy), yn(dy), ybar(dy);
          for (size_t i = 0; i < P; ++i) blob[i] = -0.3 + 0.6 * (double)((i * 37) % 101) / 100.0;
          for (int i = 0; i < dy; ++i) y[i] = 0.1 * i - 0.2, yb[i] = 0.5 - 0.1 * i;
          for (int i = 0; i < nu; ++i) u[i] = 1.0 - i;
          nlc_t_rk_substep(method, blob.data(), H, dy, nu, y.data(), u.data(), 0.05, yb.data(), yn.data(), ybar.data(), grad.data());
          sum += yn[dy - 1] + ybar[0] + grad[P - 1];
        }
  }
  std::printf("ok %.17g\n", sum);
  return 0;
}
#endif
