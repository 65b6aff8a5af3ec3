// Fused training step of the NODE baseline (kernels_train_node.hip, abi_train.hip): the reference's iteration
// (train_utils.py:388-408) over NODE.forward (:696-724) -- x = cat((obs - mean) / std, zeros(aug)), u = window[:, -1, :] raw,
// f = Linear -> tanh -> Linear -> tanh -> Linear on cat(x, u), forward Euler on torchdiffeq's fixed grid, MSE of the first d
// columns against target.  Plain C++ (__host__ __device__ where the kernels call it): tests/helpers/train_node_host.cpp compiles
// the grid and the sub-step backward with g++ and tests/test_train_node_host.py checks them against oracle/node_model.py.
//
// nlc_train.h is included, not changed: the reduce / Adam launches, the workspace partition, Norm, Batch and GroupStrides are
// the other families'.
#pragma once
#include <math.h>
#include <stdint.h>

#include "nlc_node_rk.h"
#include "nlc_train.h"

namespace nlc {
namespace train {

constexpr int kNodeTrainMaxSub = 256;  // most Euler sub-steps of a row: t <= 5.1 s at dt = 0.05 with normalize_time
constexpr int kNodeMaxH = 272;         // hidden_units nlc_set_node_model takes
constexpr int kNodeMaxDy = 8;          // d + augment_dim
constexpr int kNodeMaxIn = kNodeMaxDy + NLC_MAX_NU;
constexpr int kNodeChunk = 4;          // ODE-function evaluations whose samples one weight-gradient pass sums (Euler: sub-steps)
// A multi-stage method (nlc_node_rk.h) tapes its stage inputs in the tape the Euler states have, so the cap is on a row's taped
// ODE-function evaluations: kNodeTrainMaxSub / s sub-steps (midpoint 128, rk4 64), and the slab has one size for every method.
constexpr int node_train_max_sub(int method) { return kNodeTrainMaxSub / node_rk_stages(method); }
static_assert(kNodeChunk % kNodeMaxStages == 0, "a weight-gradient chunk holds whole sub-steps of every method");
constexpr int kNodeTensors = 6;        // 0.weight, 0.bias, 2.weight, 2.bias, 4.weight, 4.bias (nlc_set_node_model's order)

// ---- torchdiffeq's fixed grid over [0, t_end] (fixed_grid.py / solvers.py, restated by oracle.node_model.euler_substeps):
// niters = ceil(t_end / step_size + 1) points k * step_size, the last one replaced by t_end; h_k = grid[k + 1] - grid[k].
// The count of sub-steps, niters - 1: 0 for !(t_end > 0) (NaN included), at most kNodeTrainMaxSub.  *bad is set when the row
// cannot be integrated as asked (no positive time, or past the cap): the kernels give such a row a NaN squared error.  The
// division is a true IEEE one on the device too (a reciprocal multiply moves the ceil at grid points).
NLC_HD int node_euler_count(double t_end, double step_size, int* bad) {
  *bad = 1;
  if (!(t_end > 0.0)) return 0;
  const double niters = ceil(t_end / step_size + 1.0);  // '/' is the correctly rounded division (no fast-math here)
  if (!(niters <= (double)(kNodeTrainMaxSub + 1))) return kNodeTrainMaxSub;  // past the cap (inf and NaN included)
  *bad = 0;
  const int n = (int)niters - 1;
  return n < 0 ? 0 : n;
}
// the same count under a method's cap of max_sub sub-steps (node_train_max_sub)
NLC_HD int node_rk_count(double t_end, double step_size, int max_sub, int* bad) {
  *bad = 1;
  if (!(t_end > 0.0)) return 0;
  const double niters = ceil(t_end / step_size + 1.0);
  if (!(niters <= (double)(max_sub + 1))) return max_sub;
  *bad = 0;
  const int n = (int)niters - 1;
  return n < 0 ? 0 : n;
}
// width of sub-step k < nsub
NLC_HD double node_euler_width(double t_end, double step_size, int nsub, int k) {
  const double lo = (double)k * step_size;
  const double hi = k == nsub - 1 ? t_end : (double)(k + 1) * step_size;
  return hi - lo;
}
// count and widths (h holds kNodeTrainMaxSub doubles)
NLC_HD int node_euler_grid(double t_end, double step_size, double* h, int* bad) {
  const int nsub = node_euler_count(t_end, step_size, bad);
  for (int k = 0; k < nsub; ++k) h[k] = node_euler_width(t_end, step_size, nsub, k);
  return nsub;
}

// ---- one Euler sub-step x' = x + h f(cat(x, u)) and its backward.  aten's tanh_backward: g * (1 - y * y)
NLC_HD double node_tanh_bwd(double g, double y) { return g * (1.0 - y * y); }
// dL/df of the sub-step from dL/dx'
NLC_HD double node_out_delta(double h, double xbar_next) { return h * xbar_next; }

// one row, serially: the activations a1, a2 [H] and f [dy] of cat(x [dy], u [nu]); blob-order weights
inline void node_func_row(const double* W0, const double* b0, const double* W2, const double* b2, const double* W4,
                          const double* b4, int H, int dy, int nu, const double* x, const double* u, double* a1, double* a2,
                          double* f) {
  const int in = dy + nu;
  for (int j = 0; j < H; ++j) {
    double acc = 0.0;
    for (int c = 0; c < in; ++c) acc += W0[(int64_t)j * in + c] * (c < dy ? x[c] : u[c - dy]);
    a1[j] = m::tanh_d(acc + b0[j]);
  }
  for (int j = 0; j < H; ++j) {
    double acc = 0.0;
    for (int l = 0; l < H; ++l) acc += W2[(int64_t)j * H + l] * a1[l];
    a2[j] = m::tanh_d(acc + b2[j]);
  }
  for (int i = 0; i < dy; ++i) {
    double acc = 0.0;
    for (int j = 0; j < H; ++j) acc += W4[(int64_t)i * H + j] * a2[j];
    f[i] = acc + b4[i];
  }
}
// its backward: xbar_next [dy] = dL/dx' -> d3 [dy], d2 [H], d1 [H] (dL/d pre-activation of layers 4, 2, 0: the bias gradients,
// and times a2 / a1 / cat(x, u) the weight gradients) and xbar [dy] = dL/dx = xbar_next + W0[:, :dy]^T d1
inline void node_substep_bwd_row(const double* W0, const double* W2, const double* W4, int H, int dy, int nu, double h,
                                 const double* xbar_next, const double* a1, const double* a2, double* d3, double* d2, double* d1,
                                 double* xbar) {
  const int in = dy + nu;
  for (int i = 0; i < dy; ++i) d3[i] = node_out_delta(h, xbar_next[i]);
  for (int j = 0; j < H; ++j) {
    double g = 0.0;
    for (int i = 0; i < dy; ++i) g += W4[(int64_t)i * H + j] * d3[i];
    d2[j] = node_tanh_bwd(g, a2[j]);
  }
  for (int l = 0; l < H; ++l) {
    double g = 0.0;
    for (int j = 0; j < H; ++j) g += W2[(int64_t)j * H + l] * d2[j];
    d1[l] = node_tanh_bwd(g, a1[l]);
  }
  for (int i = 0; i < dy; ++i) {
    double g = 0.0;
    for (int l = 0; l < H; ++l) g += W0[(int64_t)l * in + i] * d1[l];
    xbar[i] = xbar_next[i] + g;
  }
}

// ---- one sub-step of a multi-stage method (nlc_node_rk.h) for one row, serially, and its backward: the host statement of what
// the kernels do, checked against float64 autograd by tests/test_node_rk_host.py.  Stage i's backward from kbar_i = dL/dk_i:
// d3 = kbar_i, d2, d1 as above, Ybar_i = W0[:, :dy]^T d1
inline void node_stage_bwd_row(const double* W0, const double* W2, const double* W4, int H, int dy, int nu, const double* kbar,
                               const double* a1, const double* a2, double* d2, double* d1, double* Ybar) {
  const int in = dy + nu;
  for (int j = 0; j < H; ++j) {
    double g = 0.0;
    for (int i = 0; i < dy; ++i) g += W4[(int64_t)i * H + j] * kbar[i];
    d2[j] = node_tanh_bwd(g, a2[j]);
  }
  for (int l = 0; l < H; ++l) {
    double g = 0.0;
    for (int j = 0; j < H; ++j) g += W2[(int64_t)j * H + l] * d2[j];
    d1[l] = node_tanh_bwd(g, a1[l]);
  }
  for (int i = 0; i < dy; ++i) {
    double g = 0.0;
    for (int l = 0; l < H; ++l) g += W0[(int64_t)l * in + i] * d1[l];
    Ybar[i] = g;
  }
}
// y [dy] -> y_next [dy] over width h, then ybar_next [dy] -> ybar [dy] and the sub-step's gradient of the blob-order weights
// added to grad (node_blob_offsets' layout: W0 | b0 | W2 | b2 | W4 | b4).  work: kNodeMaxStages * (kNodeMaxDy * 3 + 2 * H) +
// 2 * H doubles
inline void node_rk_substep_row(const NodeRk& T, const double* W0, const double* b0, const double* W2, const double* b2,
                                const double* W4, const double* b4, int H, int dy, int nu, const double* y, const double* u,
                                double h, const double* ybar_next, double* y_next, double* ybar, double* grad, double* work) {
  const int in = dy + nu, S = T.s;
  double* Y = work;                               // [S][8] stage inputs
  double* k = Y + kNodeMaxStages * kNodeMaxDy;    // [8][S] slopes, component-major
  double* kb = k + kNodeMaxStages * kNodeMaxDy;   // [8][S] their adjoints
  double* a1 = kb + kNodeMaxStages * kNodeMaxDy;  // [S][H]
  double* a2 = a1 + (int64_t)kNodeMaxStages * H;  // [S][H]
  double* d2 = a2 + (int64_t)kNodeMaxStages * H;
  double* d1 = d2 + H;
  double f[kNodeMaxDy], Yb[kNodeMaxDy], d3[kNodeMaxDy];
  for (int i = 0; i < S; ++i) {
    for (int c = 0; c < dy; ++c) Y[i * kNodeMaxDy + c] = node_rk_stage_input(T, i, y[c], h, k + c * S);
    node_func_row(W0, b0, W2, b2, W4, b4, H, dy, nu, Y + i * kNodeMaxDy, u, a1 + (int64_t)i * H, a2 + (int64_t)i * H, f);
    for (int c = 0; c < dy; ++c) k[c * S + i] = f[c];
  }
  for (int c = 0; c < dy; ++c) {
    y_next[c] = node_rk_combine(T, y[c], h, k + c * S);
    ybar[c] = ybar_next[c];
    for (int i = 0; i < S; ++i) kb[c * S + i] = node_rk_kbar_init(T, i, h, ybar_next[c]);
  }
  double* gW0 = grad;
  double* gb0 = gW0 + (int64_t)H * in;
  double* gW2 = gb0 + H;
  double* gb2 = gW2 + (int64_t)H * H;
  double* gW4 = gb2 + H;
  double* gb4 = gW4 + (int64_t)dy * H;
  for (int i = S - 1; i >= 0; --i) {
    for (int c = 0; c < dy; ++c) d3[c] = kb[c * S + i];
    node_stage_bwd_row(W0, W2, W4, H, dy, nu, d3, a1 + (int64_t)i * H, a2 + (int64_t)i * H, d2, d1, Yb);
    for (int c = 0; c < dy; ++c) {
      ybar[c] += Yb[c];
      for (int j = 0; j < i; ++j) kb[c * S + j] += node_rk_kbar_add(T, i, j, h, Yb[c]);
      gb4[c] += d3[c];
      for (int l = 0; l < H; ++l) gW4[(int64_t)c * H + l] += d3[c] * a2[(int64_t)i * H + l];
    }
    for (int j = 0; j < H; ++j) {
      gb2[j] += d2[j];
      gb0[j] += d1[j];
      for (int l = 0; l < H; ++l) gW2[(int64_t)j * H + l] += d2[j] * a1[(int64_t)i * H + l];
      for (int c = 0; c < in; ++c) gW0[(int64_t)j * in + c] += d1[j] * (c < dy ? Y[i * kNodeMaxDy + c] : u[c - dy]);
    }
  }
}

// ---- blob offsets, padded to kTensors with empty tensors as rnn_blob_offsets pads its six
inline void node_blob_offsets(int d, int aug, int nu, int H, int64_t off[kTensors + 1]) {
  const int64_t dy = d + aug, in = dy + nu;
  const int64_t n[kNodeTensors] = {H * in, H, (int64_t)H * H, H, dy * H, dy};
  off[0] = 0;
  for (int i = 0; i < kTensors; ++i) off[i + 1] = off[i] + (i < kNodeTensors ? n[i] : 0);
}

// ---- one workgroup's slab, a function of the shape alone (the sub-step counts live on the device) and the same for every
// method: the tape of the ODE function's inputs (Euler: the states x_k; s stages: Y_i of sub-step k at entry k s + i) up to
// the cap, and the samples (evaluation, row) of one weight-gradient chunk
struct NodeActLayout {
  int64_t Xt, A1, A2, D1, D2, D3, Z, total;
};
NLC_HD NodeActLayout node_act_layout(int H, int in) {
  const int64_t S = (int64_t)kNodeChunk * kRows;
  NodeActLayout L;
  int64_t o = 0;
  L.Xt = act_take(&o, (int64_t)kNodeTrainMaxSub * kRows * kNodeMaxDy);  // x_k: [k][r][8]
  L.A1 = act_take(&o, S * H);                                           // tanh of layer 0: [s][H]
  L.A2 = act_take(&o, S * H);
  L.D1 = act_take(&o, S * H);  // dL/d pre-activation of layer 0
  L.D2 = act_take(&o, S * H);
  L.D3 = act_take(&o, S * kNodeMaxDy);
  L.Z = act_take(&o, S * in);  // cat(x_k, u)
  L.total = o;
  return L;
}

// training (partial, act set) and evaluation (both NULL; tile_loss per tile, idx may be NULL) share the argument block
struct NodeTrainArgs {
  int d, nin, B;  // nin: unused (the ODE function takes the raw action); B: window length, the newest action is read
  int aug, nu, H, row_times;
  double time_div, step_size;
  Norm norm;
  Batch batch;
  int64_t ntiles;
  int64_t P, A;
  NodeActLayout L;
  double* partial;
  double* tile_loss;
  double* act;
  int64_t off[kNodeTensors + 1];
  GroupStrides gs;
};

// static LDS of the two kernels, in doubles (two activation tiles; the training kernel adds the four waves' addends of W2^T d2)
constexpr int kNodeLdH = kNodeMaxH + 2;
constexpr int kNodeBwdRows = 4;
// (a method of s > 1 stages adds y and the slopes k_i, and in training their adjoints: node_rk_lds_doubles)
constexpr int64_t node_rk_lds_doubles(bool train, int stages) {
  return stages > 1 ? (int64_t)(1 + stages * (train ? 2 : 1)) * kRows * kNodeMaxDy : 0;
}
constexpr int64_t node_lds_doubles(bool train, int stages = 1) {
  return 2 * (int64_t)kRows * kNodeLdH + (train ? 4 * (int64_t)kNodeBwdRows * kNodeLdH : 0) + 8 * (int64_t)kRows * kNodeMaxDy +
         node_rk_lds_doubles(train, stages);
}

}  // namespace train
}  // namespace nlc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace nlc {
namespace train {
// method: nlc_node_rk.h (the ctx option "node_method"); the stage count is a template parameter of the kernels
hipError_t launch_node_train_fwd_bwd(const NodeTrainArgs& a, int method, int nblk, int M, hipStream_t s);
hipError_t launch_node_eval(const NodeTrainArgs& a, int method, int G, int M, hipStream_t s);
}  // namespace train
}  // namespace nlc
#endif
