// Shapes and buffers of the forward-only evaluation of the fused trainers (kernels_train_eval.hip, abi_train.hip): the held-out
// loss of the reference's get_val_loss_delay_precomputed (overlay.py:112-115: model(s0, a0, ts), then an MSE) on the tiles,
// blobs and index arrays of the training step (nlc_train.h).  Plain C++: tests/helpers/train_eval_host.cpp compiles the
// layout functions with g++.
//
// Nothing is taped, so a tile's activations live in LDS and the workspace holds the tile losses only.
#pragma once
#include <stdint.h>

#include "nlc_train.h"

namespace nlc {
namespace train {

constexpr int64_t kLdsBytes = 160 * 1024;  // LDS of a gfx950 compute unit, and the most one workgroup may take
constexpr int kEvalPerCu = 2;              // evaluation workgroups a compute unit is given at most (256 threads each)

// ---- the evaluation workspace, in doubles: one member's region is its tile losses [ntiles], rounded up to 32 doubles, so M
// regions back to back stay 256-byte aligned (GroupStrides::ws = total)
struct EvalWsLayout {
  int64_t ntiles, tile_loss, total;
};
inline EvalWsLayout eval_ws_layout(int64_t N) {
  EvalWsLayout w;
  w.ntiles = (N + kRows - 1) / kRows;
  w.tile_loss = 0;
  w.total = (w.ntiles + 31) / 32 * 32;
  return w;
}

// workgroups on the grid's x axis: every tile its own until the chip is full (per_cu workgroups on each of the cus compute
// units, shared by the M members on y); beyond that a workgroup walks tiles b, b + G, ...  The losses do not depend on G: a
// tile's sum goes to tile_loss[tile]
inline int eval_grid(int64_t ntiles, int cus, int per_cu, int M) {
  int64_t cap = (int64_t)cus * per_cu / M;
  if (cap < 1) cap = 1;
  return (int)(ntiles < cap ? ntiles : cap);
}

// row stride of a [16][n] LDS array of doubles: the smallest >= n that is 2 mod 4, an odd multiple of four banks, so the 16
// rows of an MFMA's A operand start on 16 different bank quads
NLC_HD int eval_ld(int n) { return ((n + 1) & ~3) + 2; }

// ---- NeuralLaplaceModel: one workgroup's LDS, in doubles.  The encoder's state (h0, h1, the gate tile G [16][4g]) and the
// MLP's activations (a1, a2 and the last layer's chunk u) are never live together and share one region.  The last layer
// and the line integral go dc state dims at a time (u holds [theta | phi] of dc dims, S terms each): dc = d unless that
// does not fit (S = 129 at h = 256)
struct EvalLdsLayout {
  int64_t X, a0, tn, tgt, sq, h0, h1, G, a1, a2, u, total;
  int ldg, ldG, ldK, ldh, ldu, dc;
};
NLC_HD EvalLdsLayout eval_lds_layout(int d, int nin, int g, int h, int S, int B) {
  const int64_t R = kRows;
  EvalLdsLayout L;
  L.ldg = eval_ld(g);
  L.ldG = eval_ld(4 * g);
  L.ldK = eval_ld(2 * S + d + 2);
  L.ldh = eval_ld(h);
  int64_t o = 0;
  L.X = act_take(&o, (int64_t)B * R * nin);  // layer-0 inputs, flipped window, normalised: [s][r][nin]
  L.a0 = act_take(&o, R * L.ldK);            // MLP input [theta_s | phi_s | obs_n | enc]
  L.tn = act_take(&o, R);
  L.tgt = act_take(&o, R * d);
  L.sq = act_take(&o, R * d);
  const int64_t shared = o;
  L.h0 = act_take(&o, R * L.ldg);
  L.h1 = act_take(&o, R * L.ldg);
  L.G = act_take(&o, R * L.ldG);  // layer 0: [r | z | hn] of h W_hh^T; layer 1: [r | z | in | hn]
  const int64_t gru_end = o;
  o = shared;
  L.a1 = act_take(&o, R * L.ldh);
  L.a2 = act_take(&o, R * L.ldh);
  L.u = o;
  const int64_t cap = kLdsBytes / (int64_t)sizeof(double);
  L.dc = d;
  while (L.dc > 1 && L.u + R * eval_ld(2 * L.dc * S) > cap) --L.dc;
  L.ldu = eval_ld(2 * L.dc * S);
  const int64_t mlp_end = L.u + ((R * L.ldu + 7) & ~(int64_t)7);
  L.total = gru_end > mlp_end ? gru_end : mlp_end;
  return L;
}

// ---- DeltaTRNN / RNN: the static LDS of rnn_eval_kernel<H>, in doubles (hidden state, gate tile, window, [obs_n | ts_n],
// target, squared errors)
constexpr int64_t rnn_eval_lds_doubles(int H) {
  return (int64_t)kRows * (H + 2) + (int64_t)kRows * (3 * H + 2) + (int64_t)kMaxB * kRows * kMaxNin +
         (int64_t)kRows * (kMaxD + 1) + 2 * (int64_t)kRows * kMaxD;
}

// workgroups of this LDS size a compute unit runs side by side, at most kEvalPerCu
inline int eval_per_cu(int64_t lds_bytes) {
  const int64_t n = lds_bytes > 0 ? kLdsBytes / lds_bytes : kEvalPerCu;
  return (int)(n < 1 ? 1 : n > kEvalPerCu ? kEvalPerCu : n);
}

struct EvalArgs {
  int d, nin, g, h, S, B;
  double time_div, alpha, log_tol;
  Norm norm;
  Batch batch;
  int64_t ntiles;
  EvalLdsLayout L;
  double* tile_loss;  // [ntiles] per member
  int64_t off[kTensors + 1];
  GroupStrides gs;        // params, ws (= EvalWsLayout::total), idx, rows; grad unused
  const double* lin_tab;  // as TrainArgs::lin_tab: NULL selects the Fourier instance
};

struct RnnEvalArgs {
  int d, nin, B, time_input;
  double time_div;
  Norm norm;
  Batch batch;
  int64_t ntiles;
  double* tile_loss;
  int64_t off[kRnnTensors + 1];
  GroupStrides gs;
};

struct EvalReduceArgs {
  const double* tile_loss;
  int64_t ntiles, N, ws;  // ws: doubles from a member's tile losses to the next member's
  int d;
  double* loss;  // [gridDim.y]
};

}  // namespace train
}  // namespace nlc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace nlc {
namespace train {
// G workgroups on x, the M members on y
hipError_t launch_train_eval(const EvalArgs& a, int G, int M, hipStream_t s);
hipError_t launch_rnn_eval(const RnnEvalArgs& a, int H, int G, int M, hipStream_t s);  // H: 64, 128 or 160
hipError_t launch_eval_reduce(const EvalReduceArgs& a, int M, hipStream_t s);
}  // namespace train
}  // namespace nlc
#endif
