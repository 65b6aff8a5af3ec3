// The fixed-grid solvers of the NODE baseline (train_utils.py:717-723: odeint(..., method=self.method, options={"step_size":
// 0.05})), written once as explicit Runge-Kutta tableaus for the inference kernels (kernels_node.hip), the training kernels
// (kernels_train_node.hip), the host checks and tests/helpers/node_rk_host.cpp (g++).  Plain C++, no other header.
//
// torchdiffeq is absent offline: the three methods are restated from the published algorithm (fixed_grid.py Euler / Midpoint
// / RK4, rk_common.py rk4_alt_step_func) -- parity unpinned vs upstream, like the grid itself (nlc_train_node.h).  All three
// share that grid; the ODE function ignores t, so a tableau needs no c_i.  One sub-step of width h from y:
//   Y_i = y + h sum_{j<i} a_ij k_j,  k_i = f(Y_i)  (i = 1 .. s),   y' = y + h sum_i b_i k_i
//   euler     s = 1: y' = y + h f(y)
//   midpoint  s = 2: k2 = f(y + (h/2) k1), y' = y + h k2
//   rk4       s = 4: torchdiffeq's fixed-grid rk4 is the 3/8 rule, not the classic tableau:
//                    k2 = f(y + h k1/3), k3 = f(y + h (k2 - k1/3)), k4 = f(y + h (k1 - k2 + k3)),
//                    y' = y + (k1 + 3 (k2 + k3) + k4) h / 8
// Backward of one sub-step given ybar' = dL/dy': kbar_i = h b_i ybar'; for i = s .. 1: Ybar_i = J_f(Y_i)^T kbar_i (the
// three-layer backward, whose deltas at Y_i are the weight-gradient samples) and kbar_j += h a_ij Ybar_i for j < i; finally
// ybar = ybar' + sum_i Ybar_i.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLC_RK_HD __host__ __device__ inline
#else
#define NLC_RK_HD inline
#endif

namespace nlc {

constexpr int kNodeMethods = 3;    // nlc_set_option "node_method": 0 euler, 1 midpoint, 2 rk4
constexpr int kNodeMaxStages = 4;  // s of the widest tableau

struct NodeRk {
  int s;
  double a[kNodeMaxStages][kNodeMaxStages];  // a[i][j], j < i (strictly lower triangle)
  double b[kNodeMaxStages];
};

constexpr NodeRk node_rk_tableau(int method) {
  return method == 1   ? NodeRk{2, {{0, 0, 0, 0}, {0.5, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, {0.0, 1.0, 0.0, 0.0}}
         : method == 2 ? NodeRk{4,
                                {{0, 0, 0, 0}, {1.0 / 3.0, 0, 0, 0}, {-1.0 / 3.0, 1.0, 0, 0}, {1.0, -1.0, 1.0, 0}},
                                {0.125, 0.375, 0.375, 0.125}}
                       : NodeRk{1, {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, {1.0, 0.0, 0.0, 0.0}};
}
// the tableau of a method as one constant object (the kernels index it with run-time stage numbers: a constant in memory, never a
// per-lane copy)
template <int METHOD>
struct NodeRkOf {
  static constexpr NodeRk T = node_rk_tableau(METHOD);
};
constexpr bool node_method_ok(int method) { return method >= 0 && method < kNodeMethods; }
constexpr int node_rk_stages(int method) { return node_rk_tableau(method).s; }

// stage input i of a sub-step of width h: y + h sum_{j<i} a_ij k_j for one component (k[j * stride]: that component's slopes
// so far)
NLC_RK_HD double node_rk_stage_input(const NodeRk& T, int i, double y, double h, const double* k, int stride = 1) {
  double acc = 0.0;
  for (int j = 0; j < i; ++j) acc += T.a[i][j] * k[j * stride];
  return i == 0 ? y : y + h * acc;
}
// the sub-step's end value for one component
NLC_RK_HD double node_rk_combine(const NodeRk& T, double y, double h, const double* k, int stride = 1) {
  double acc = 0.0;
  for (int i = 0; i < T.s; ++i) acc += T.b[i] * k[i * stride];
  return y + h * acc;
}
// backward, one component: kbar_i at the start, and what stage i's Ybar_i adds to kbar_j (j < i)
NLC_RK_HD double node_rk_kbar_init(const NodeRk& T, int i, double h, double ybar_next) { return (h * T.b[i]) * ybar_next; }
NLC_RK_HD double node_rk_kbar_add(const NodeRk& T, int i, int j, double h, double Ybar_i) { return (h * T.a[i][j]) * Ybar_i; }

}  // namespace nlc
