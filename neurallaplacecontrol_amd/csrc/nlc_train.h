// Per-element math of the fused training step (kernels_train.hip): NeuralLaplaceModel's loss / gradient / clip / Adam
// iteration of the reference's training loop (train_utils.py:388-408).  Everything here is __host__ __device__ so that
// tests/helpers/train_host.cpp compiles the same functions with g++ and tests/test_train_host.py checks them against
// torch's autograd / clip_grad_norm_ / Adam on the CPU.
//
// Operation order follows the torch kernels the reference runs, so the host build agrees with them to a few ulp:
//   tanh backward        g * (1 - y*y)                                     (aten tanh_backward)
//   sigmoid backward     g * ((1 - y) * y)                                 (aten sigmoid_backward)
//   clip_grad_norm_      coef = max_norm / (total + 1e-6), clamped to 1, always multiplied (torch/nn/utils/clip_grad.py)
//   Adam (foreach)       g += wd p;  m.lerp_(g, 1 - b1);  v = v*b2 + (1 - b2)*(g*g);  p += -(lr/bc1) * (m / (sqrt(v)/sqrt(bc2) + eps))
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/nlc.h"  // NLC_MAX_D, NLC_MAX_NIN
#include "nlc_math.h"

namespace nlc {
namespace train {

constexpr double kPiT = 3.14159265358979323846;

// ---- GRU cell backward (torch.nn.GRU gate order [r; z; n]):
//   r = sig(gi_r + gh_r), z = sig(gi_z + gh_z), n = tanh(gi_n + r * hn), hn = W_hn h + b_hn, h' = (1 - z) n + z h.
// Given the saved r, z, n, hn and the previous hidden state, dh' -> the gradients of the input-side pre-activations
// (gi_r, gi_z, gi_n: also those of b_ih and, times x, of W_ih), of the hidden-side n pre-activation gh_n = dn_pre * r (the
// hidden side's r / z gradients equal the input side's) and the direct part z * dh' of dh (the rest is W_hh^T (gh)).
NLC_HD void gru_cell_bwd(double dh, double r, double z, double n, double hn, double h_prev, double* gi_r, double* gi_z,
                         double* gi_n, double* gh_n, double* dh_direct) {
  const double dn = dh * (1.0 - z);
  const double dz = dh * (h_prev - n);
  const double dn_pre = dn * (1.0 - n * n);
  const double dr = dn_pre * hn;
  *gi_r = dr * ((1.0 - r) * r);
  *gi_z = dz * ((1.0 - z) * z);
  *gi_n = dn_pre;
  *gh_n = dn_pre * r;
  *dh_direct = dh * z;
}

// ---- sphere map of LaplaceRepresentationFunc.forward (w_nl.py:59-62), y = tanh(out):
//   theta = y * pi                      -> d out = (g * pi) * (1 - y^2)
//   phi = y * pi / 2 - pi/2 + pi/2      -> d out = ((g / 2) * pi) * (1 - y^2)
NLC_HD double sphere_theta_bwd(double g, double y) { return (g * kPiT) * (1.0 - y * y); }
NLC_HD double sphere_phi_bwd(double g, double y) { return ((g / 2.0) * kPiT) * (1.0 - y * y); }
// forward values, in the reference's operation order
NLC_HD double sphere_theta(double y) { return y * kPiT; }
NLC_HD double sphere_phi(double y) { return y * kPiT / 2.0 - kPiT / 2.0 + kPiT / 2.0; }

// ---- one term of the Fourier line integral, x = s(t) sum_k w_k R_k c_k with R = tan(phi/2 + pi/4), c_k = cos(theta + k pi/2)
// (scale 2), c'_k = d c_k / d theta:  dx/dtheta_k = w_k R_k c'_k,  dx/dphi_k = w_k c_k (1 + R_k^2) / 2.  g = dL/dx * s(t).
NLC_HD void ilt_term_bwd(double g, double wk, double R, double c, double c_prime, double* d_theta, double* d_phi) {
  *d_theta = (g * wk) * R * c_prime;
  *d_phi = (g * wk) * c * (0.5 * (1.0 + R * R));
}

// ---- the linear algorithms (fixed Talbot, Stehfest: fixed nodes delta_k and weights W_k, s_k = delta_k / t):
// x = (1/t) sum_k Re(W_k F_k) with F_k = R_k e^{i theta_k}, so a term is R_k c_k with
// c_k = W_re cos(theta) - W_im sin(theta) in place of the Fourier series' quarter turn, and c'_k = d c_k / d theta.
// ilt_term_bwd with w_k = 1 and g = dL/dx / t gives the term's gradients.
NLC_HD void linear_phase(double th, double wr, double wi, double* c, double* c_prime) {
  double sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
  sincos(th, &sn, &cs);
#else
  sn = sin(th);
  cs = cos(th);
#endif
  *c = wr * cs - wi * sn;
  *c_prime = -wr * sn - wi * cs;
}
// R = |F| of the sphere point at latitude phi (both ILT families)
NLC_HD double sphere_radius(double phi) { return tan(phi / 2.0 + kPiT / 4.0); }
// a row's line integral sum_k R_k c_k over the S terms of one state dim (yt / yp: the tanh outputs behind theta / phi;
// wr / wi: the weight tables); the prediction is this over t
NLC_HD double linear_row_sum(const double* yt, const double* yp, const double* wr, const double* wi, int S) {
  double acc = 0.0;
  for (int k = 0; k < S; ++k) {
    double cv, cp;
    linear_phase(sphere_theta(yt[k]), wr[k], wi[k], &cv, &cp);
    acc += sphere_radius(sphere_phi(yp[k])) * cv;
  }
  return acc;
}
// its backward down to the last layer's pre-activations: g = dL/dx / t -> dt[k], dp[k]
NLC_HD void linear_row_bwd(double g, const double* yt, const double* yp, const double* wr, const double* wi, int S, double* dt,
                           double* dp) {
  for (int k = 0; k < S; ++k) {
    double cv, cp, gth, gph;
    linear_phase(sphere_theta(yt[k]), wr[k], wi[k], &cv, &cp);
    ilt_term_bwd(g, 1.0, sphere_radius(sphere_phi(yp[k])), cv, cp, &gth, &gph);
    dt[k] = sphere_theta_bwd(gth, yt[k]);
    dp[k] = sphere_phi_bwd(gph, yp[k]);
  }
}
// the query point s = delta / t of a linear algorithm on the Riemann sphere (as rep_inputs_kernel's linear branch)
NLC_HD void linear_query_point(double node_re, double node_im, double t, double* theta_s, double* phi_s) {
  const double sr = node_re / t, si = node_im / t;
  const double a2v = sr * sr + si * si;
  *theta_s = atan2(si, sr);
  *phi_s = asin((a2v - 1.0) / (a2v + 1.0));
}
// the Fourier series at ILT scale 2, T = scale t: gamma = alpha - log_tol / (scale T), the real part of every query point
constexpr double kFourierScale = 2.0;
NLC_HD double fourier_gamma(double alpha, double log_tol, double Tt) { return alpha - log_tol / (kFourierScale * Tt); }
// its query point s_k = gamma + i pi k / T on the Riemann sphere (as rep_inputs_kernel's Fourier branch)
NLC_HD void fourier_query_point(double alpha, double log_tol, double t, int k, double* theta_s, double* phi_s) {
  const double Tt = kFourierScale * t;
  const double gamma = fourier_gamma(alpha, log_tol, Tt);
  const double im = kPiT * (double)k / Tt;
  const double a2v = gamma * gamma + im * im;
  *theta_s = atan2(im, gamma);
  *phi_s = asin((a2v - 1.0) / (a2v + 1.0));
}
// and the factor e^{gamma t} / T of its prediction
NLC_HD double fourier_pred_factor(double alpha, double log_tol, double t) {
  const double Tt = kFourierScale * t;
  return exp(fourier_gamma(alpha, log_tol, Tt) * t) / Tt;
}

// ---- clip_grad_norm_: coefficient the gradients are multiplied by (NaN total -> NaN, as torch.clamp propagates it)
NLC_HD double clip_coef(double max_norm, double total_norm) {
  const double c = max_norm / (total_norm + 1e-6);
  return c > 1.0 ? 1.0 : c;
}

// ---- torch.optim.Adam (foreach, non-capturable, amsgrad off), one element; g is the (clipped) gradient.
// Host-side scalars of the step: omb1 = 1 - beta1 (lerp weight), omb2 = 1 - beta2, step_size = -(lr / bc1),
// bc2_sqrt = bc2 ** 0.5 with bc_i = 1 - beta_i ** step.
struct AdamScalars {
  double wd, omb1, beta2, omb2, step_size, bc2_sqrt, eps;
};
NLC_HD void adam_element(double* p, double* m, double* v, double g, const AdamScalars& k) {
  if (k.wd != 0.0) g = g + k.wd * *p;  // torch._foreach_add(grads, params, alpha=weight_decay)
  // torch.lerp: weight < 0.5 -> self + w (end - self), else end - (end - self)(1 - w)
  const double diff = g - *m;
  *m = fabs(k.omb1) < 0.5 ? *m + k.omb1 * diff : g - diff * (1.0 - k.omb1);
  *v = *v * k.beta2;
  *v = *v + k.omb2 * (g * g);
  const double denom = sqrt(*v) / k.bc2_sqrt + k.eps;
  *p = *p + k.step_size * (*m / denom);
}

}  // namespace train
}  // namespace nlc

// ---- shapes and buffers of the fused training step (shared by kernels_train.hip and abi_train.hip; plain C++ so the host
// test can include this header too)
namespace nlc {
namespace train {

constexpr int kRows = 16;      // rows per tile: one workgroup, and the k = 4 x 4 sample steps of the MFMA weight gradients
constexpr int kThreads = 256;  // threads per training workgroup
constexpr int kMaxB = 16;      // longest action window (action_buffer_size, config.py:58: 4)
constexpr int kMaxBlocks = 128;
constexpr int kChunk = 1024;   // parameters per reduce / Adam workgroup (never straddles two tensors)
constexpr int kTensors = 16;   // blob tensors (include/nlc.h, nlc_set_model)
constexpr int kMaxD = NLC_MAX_D;      // largest state_dim
constexpr int kMaxNin = NLC_MAX_NIN;  // largest GRU input dim

// per-tile activations, tapes and deltas in one workgroup's slab (doubles, each array 64-byte aligned)
struct ActLayout {
  int64_t X0, H0, G0, H1, G1, a0, a1, a2, u, d3, d2, d1, denc, tn, tgt, sq, DI0, DH0, DI1, DH1, DX1, dhA, dD, total;
};
NLC_HD int64_t act_take(int64_t* o, int64_t n) {
  const int64_t r = *o;
  *o += (n + 7) & ~(int64_t)7;
  return r;
}
NLC_HD ActLayout act_layout(int d, int nin, int g, int h, int S, int B) {
  const int64_t R = kRows, K0 = 2 * S + d + 2, O = 2 * d * S;
  ActLayout L;
  int64_t o = 0;
  L.X0 = act_take(&o, B * R * nin);         // layer-0 inputs, flipped window, normalised: [s][r][nin]
  L.H0 = act_take(&o, (B + 1) * R * g);     // layer-0 hidden states h_0 = 0 .. h_B: [s][r][g]
  L.G0 = act_take(&o, B * R * 4 * g);       // layer-0 tape [r | z | n | W_hn h + b_hn]: [s][r][4g]
  L.H1 = act_take(&o, (B + 1) * R * g);
  L.G1 = act_take(&o, B * R * 4 * g);
  L.a0 = act_take(&o, R * K0);              // MLP input [theta_s | phi_s | obs_n | enc]
  L.a1 = act_take(&o, R * h);
  L.a2 = act_take(&o, R * h);
  L.u = act_take(&o, R * O);                // tanh of the last layer (sphere map input)
  L.d3 = act_take(&o, R * O);
  L.d2 = act_take(&o, R * h);
  L.d1 = act_take(&o, R * h);
  L.denc = act_take(&o, R * 2);
  L.tn = act_take(&o, R);
  L.tgt = act_take(&o, R * d);
  L.sq = act_take(&o, R * d);
  L.DI0 = act_take(&o, B * R * 3 * g);      // input-side gate gradients [s][r][3g]
  L.DH0 = act_take(&o, B * R * 3 * g);      // hidden-side gate gradients [s][r][3g]
  L.DI1 = act_take(&o, B * R * 3 * g);
  L.DH1 = act_take(&o, B * R * 3 * g);
  L.DX1 = act_take(&o, B * R * g);          // gradient reaching layer 0's outputs through layer 1's inputs
  L.dhA = act_take(&o, R * g);
  L.dD = act_take(&o, R * g);
  L.total = o;
  return L;
}

// blob offsets (nlc_set_model's state_dict order): off[i] .. off[i + 1] is tensor i
inline void blob_offsets(int d, int nin, int g, int h, int S, int64_t off[kTensors + 1]) {
  const int64_t g3 = 3 * g, K0 = 2 * S + d + 2, O = 2 * d * S;
  const int64_t n[kTensors] = {g3 * nin, g3 * g, g3, g3, g3 * g, g3 * g, g3, g3, 2 * g, 2, h * K0, h, (int64_t)h * h, h, O * h, O};
  off[0] = 0;
  for (int i = 0; i < kTensors; ++i) off[i + 1] = off[i] + n[i];
}

// first reduce / Adam chunk of each tensor (cstart[kTensors] = number of chunks): chunks are cut per tensor, so none straddles
// two, and an empty tensor owns none
inline int chunk_starts(const int64_t off[kTensors + 1], int cstart[kTensors + 1]) {
  cstart[0] = 0;
  for (int t = 0; t < kTensors; ++t) cstart[t + 1] = cstart[t] + (int)((off[t + 1] - off[t] + kChunk - 1) / kChunk);
  return cstart[kTensors];
}

// the blob's tensors and their chunks, as the plan and the reduce / Adam launches carry them: the one place the pair is
// declared, and chunk_range / clip_total_norm the one place it is walked
struct ChunkTable {
  int64_t off[kTensors + 1];
  int cstart[kTensors + 1];  // first chunk of each tensor
};
inline int chunk_starts(ChunkTable& c) { return chunk_starts(c.off, c.cstart); }

// chunk b of the grid's x axis: its tensor t and its elements [e0, e1) of the blob
struct ChunkRange {
  int t;
  int64_t e0, e1;
};
NLC_HD ChunkRange chunk_range(const ChunkTable& c, int b) {
  int t = 0;
  while (t + 1 < kTensors && c.cstart[t + 1] <= b) ++t;
  const int64_t e0 = c.off[t] + (int64_t)(b - c.cstart[t]) * kChunk;
  const int64_t e1 = e0 + kChunk < c.off[t + 1] ? e0 + kChunk : c.off[t + 1];
  return ChunkRange{t, e0, e1};
}

// clip_grad_norm_'s total = || (||g_0||, ..., ||g_15||) || from the chunk sums of squares sq[0 .. cstart[kTensors]): tensor
// i's chunks summed in order, its norm squared again as torch does.  An empty tensor adds sqrt(0)^2 = +0, which changes no
// bit of the sum: a table padded with empty tensors gives the total of the table without them
NLC_HD double clip_total_norm(const double* sq, const ChunkTable& c) {
  double tot2 = 0.0;
  for (int i = 0; i < kTensors; ++i) {
    double s = 0.0;
    for (int k = c.cstart[i]; k < c.cstart[i + 1]; ++k) s += sq[k];
    const double n = sqrt(s);
    tot2 += n * n;
  }
  return sqrt(tot2);
}

// ---- DeltaTRNN / RNN (kernels_train_rnn.hip): one GRU layer of width H and linear_out over [h_B | obs_n | ts_n]
constexpr int kRnnTensors = 6;  // W_ih, W_hh, b_ih, b_hh, linear_out.weight, linear_out.bias (nlc_set_rnn_model's order)

// blob offsets of the six tensors; the table is padded to kTensors with empty tensors (off[6..] = P), which own no reduce /
// Adam chunk and add 0 to the gradient norm, so train_reduce_kernel / train_adam_kernel serve both models unchanged
inline void rnn_blob_offsets(int d, int nin, int H, int time_input, int64_t off[kTensors + 1]) {
  const int64_t H3 = 3 * (int64_t)H, F = H + d + (time_input ? 1 : 0);
  const int64_t n[kRnnTensors] = {H3 * nin, H3 * H, H3, H3, d * F, d};
  off[0] = 0;
  for (int i = 0; i < kTensors; ++i) off[i + 1] = off[i] + (i < kRnnTensors ? n[i] : 0);
}

// one workgroup's slab: the tapes and gate gradients of a tile, [s][r][...] (the current step's state lives in LDS)
struct RnnActLayout {
  int64_t X, Hs, G, DI, DH, total;
};
NLC_HD RnnActLayout rnn_act_layout(int nin, int H, int B) {
  const int64_t R = kRows;
  RnnActLayout L;
  int64_t o = 0;
  L.X = act_take(&o, B * R * nin);       // normalised window, forward order: [s][r][nin]
  L.Hs = act_take(&o, (B + 1) * R * H);  // hidden states h_0 = 0 .. h_B: [s][r][H]
  L.G = act_take(&o, B * R * 4 * H);     // tape [r | z | n | W_hn h + b_hn]: [s][r][4H]
  L.DI = act_take(&o, B * R * 3 * H);    // input-side gate gradients [s][r][3H]
  L.DH = act_take(&o, B * R * 3 * H);    // hidden-side gate gradients [s][r][3H]
  L.total = o;
  return L;
}

// ---- a group of M same-shaped models trained by the same launches (run_exp_multi.py:105-110 fans (env, delay, model_name)
// out; the members of a group share the descriptor and differ in weights and data): blockIdx.y is the member, and a kernel
// moves its base pointers by these strides, in doubles / int64 / rows from member m to member m + 1.  A single model is the
// M = 1 case (blockIdx.y = 0: every stride multiplies 0).
struct GroupStrides {
  int64_t params;  // parameter blob (and Adam moments): P
  int64_t ws;      // the member's workspace region (partials, tile losses, slabs, summed gradient, chunk sums): TrainWsLayout::total
  int64_t grad;    // summed gradient: ws when it lives in the workspace (a step), P when the caller supplies [M][P]
  int64_t idx;     // index array: N
  int64_t rows;    // dataset rows (obs, window, ts, target): 0 = every member reads the same dataset
};

// one member's workspace, in doubles: [partials nblk * P | tile losses | slabs nblk * A | summed gradient P | chunk sums of
// squares], every array and the total a multiple of 32 doubles, so M regions back to back stay 256-byte aligned
struct TrainWsLayout {
  int64_t partial, tile_loss, act, grad, sq, total;
};
inline TrainWsLayout train_ws_layout(int nblk, int64_t P, int64_t A, int chunks) {
  auto al = [](int64_t n) { return (n + 31) / 32 * 32; };
  TrainWsLayout w;
  int64_t o = 0;
  w.partial = o;
  o += al((int64_t)nblk * P);
  w.tile_loss = o;
  o += al(nblk);
  w.act = o;
  o += al((int64_t)nblk * A);
  w.grad = o;
  o += al(P);
  w.sq = o;
  o += al(chunks);
  w.total = o;
  return w;
}
constexpr int kMaxGroup = 65535;  // members of a group: the grid's y limit

// ---- what the four forward launches (training and evaluation, both families) are given alike
// normalisation constants of the model descriptor: state mean / std, action mean / std
struct Norm {
  double sm[kMaxD], ss[kMaxD], am[kMaxNin], as[kMaxNin];
};
// member 0's blob and dataset, and the N rows of the call: idx [N] into obs (rows, d), window (rows, B, nin), ts (rows),
// target (rows, d).  ts is not read by an RNN without time input; evaluation takes idx == NULL for rows 0 .. N - 1
struct Batch {
  const double* params;
  const double *obs, *window, *ts, *target;
  const int64_t* idx;
  int64_t N;
};

struct RnnTrainArgs {
  int d, nin, B, time_input;
  double time_div;
  Norm norm;
  Batch batch;
  int ntiles;
  int64_t P, A;
  RnnActLayout L;
  double* partial;
  double* tile_loss;
  double* act;
  int64_t off[kRnnTensors + 1];
  GroupStrides gs;
};

struct TrainArgs {
  int d, nin, g, h, S, B;
  double time_div, alpha, log_tol;
  Norm norm;
  Batch batch;
  int ntiles;
  int64_t P, A;
  ActLayout L;        // offsets into a workgroup's slab for this call's B
  double* partial;    // [gridDim.x][P] per-workgroup gradient sums
  double* tile_loss;  // [gridDim.x] per-workgroup sums of squared errors
  double* act;        // [gridDim.x][A]
  int64_t off[kTensors + 1];
  GroupStrides gs;    // batch, partial / tile_loss / act are member 0's
  // fixed Talbot / Stehfest: the device tables [node_re | node_im | W_re | W_im], S doubles each, shared by every member;
  // NULL: the Fourier series (alpha, log_tol).  Selects the kernel instance
  const double* lin_tab;
};

struct ReduceArgs {
  const double* partial;
  const double* tile_loss;
  int nblk, d;
  int64_t P, N;
  double* grad;  // (P) summed gradient
  double* sq;    // (chunks) sum of squares of each chunk
  double* loss;  // 0-dim
  ChunkTable ct;
  GroupStrides gs;  // partial / tile_loss / sq by ws, grad by grad; loss is [gridDim.y]
};

struct AdamArgs {
  double *params, *m, *v;
  const double* grad;
  const double* sq;
  double max_norm;  // <= 0: no clipping
  AdamScalars k;
  double* gradnorm;  // [gridDim.y]; may be NULL
  ChunkTable ct;
  GroupStrides gs;  // params / m / v by params, grad by grad, sq by ws
};

// the table sits where off[] and cstart[] sat: no byte of a kernel argument moved
static_assert(sizeof(ChunkTable) == 208, "ChunkTable");
static_assert(sizeof(ReduceArgs) == 312 && offsetof(ReduceArgs, ct) == 64 && offsetof(ReduceArgs, gs) == 272, "ReduceArgs");
static_assert(sizeof(AdamArgs) == 360 && offsetof(AdamArgs, ct) == 112 && offsetof(AdamArgs, gs) == 320, "AdamArgs");

}  // namespace train
}  // namespace nlc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace nlc {
namespace train {
// M: members of the group = the grid's y dimension (1: a single model)
hipError_t launch_train_fwd_bwd(const TrainArgs& a, int nblk, int M, hipStream_t s);
hipError_t launch_train_reduce(const ReduceArgs& a, int M, hipStream_t s);
hipError_t launch_train_adam(const AdamArgs& a, int M, hipStream_t s);
hipError_t launch_rnn_train_fwd_bwd(const RnnTrainArgs& a, int H, int nblk, int M, hipStream_t s);  // H: 64, 128 or 160
}  // namespace train
}  // namespace nlc
#endif
