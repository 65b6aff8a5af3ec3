// Shapes and buffers of the fused training step of a de Hoog NeuralLaplaceModel (kernels_train_dehoog.hip, abi_train.hip;
// ctx option "train_dehoog").  The quotient-difference table does not fit beside the rest of train_fwd_bwd_kernel, so the
// step is cut at the interface between the representation MLP and the line integral -- the (rows, d, S) sphere angles the
// stand-alone ILT kernels take -- and the existing de Hoog launches run in the gap:
//
//   1 train_dehoog_fwd_kernel    gather, normalisation, query points, reverse GRU (taped), linear_out, MLP -> theta, phi, t
//   2 launch_ilt_dehoog          pred (rows, d)
//   3 train_dehoog_loss_kernel   squared error -> tile_loss, gx = (2 / (N d)) (pred - target), 0 past N
//   4 launch_ilt_dehoog_bwd      gtheta, gphi (its tape: the scratch region below)
//   5 train_dehoog_bwd_kernel    sphere-map backward, then MLP, linear_out and GRU backward into the workgroup's partial
//   6, 7 train_reduce_kernel, train_adam_kernel / train_adam_members_kernel
//
// A tile's slab must survive from launch 1 to launch 5, so every tile has a workgroup (and a slab) of its own: at most
// kMaxBlocks tiles, N <= kDehoogMaxRows.  Plain C++: tests/helpers/train_dehoog_host.cpp compiles the layout with g++.
#pragma once
#include <stdint.h>

#include "nlc_dehoog_tape.h"
#include "nlc_train.h"

namespace nlc {
namespace train {

constexpr int64_t kDehoogMaxRows = (int64_t)kMaxBlocks * kRows;  // 2048: one tile per workgroup, the existing step's grid

// The workspace of a de Hoog call, in doubles: the M member regions of the other NL models (TrainWsLayout, member_total
// doubles each: partials, tile losses, slabs, summed gradient, chunk sums), then what the ILT launches read and write.  Those
// arrays hold the members back to back -- member m's rows are rows m * rows .. (m + 1) * rows - 1 of one (M rows, d, S) array
// -- because launches 2 and 4 take the group as one batch of M * rows points.  rows = 16 x the tiles of a member: rows past N
// of a ragged tile are there, with finite stand-ins.  Every array starts on a multiple of 32 doubles (256 bytes).
struct DehoogWsLayout {
  int64_t rows;  // per member
  int64_t theta, phi, gtheta, gphi;  // (M rows, d, S)
  int64_t pred, gx;                  // (M rows, d)
  int64_t t;                         // (M rows) normalised times
  int64_t scratch, scratch_bytes;    // the QD tape of launch 4: what its launcher asks for (nlc_dehoog_tape.h), M rows d table rows
  int64_t total;
};
inline DehoogWsLayout dehoog_ws_layout(int M, int64_t N, int d, int S, int64_t member_total) {
  auto al = [](int64_t n) { return (n + 31) / 32 * 32; };
  int64_t ntiles = (N + kRows - 1) / kRows;
  if (ntiles > kMaxBlocks) ntiles = kMaxBlocks;  // (a larger N is refused by the entries; the size stays defined)
  DehoogWsLayout w;
  w.rows = ntiles * kRows;
  const int64_t R = (int64_t)M * w.rows;
  int64_t o = al((int64_t)M * member_total);
  auto take = [&](int64_t n) {
    const int64_t r = o;
    o += al(n);
    return r;
  };
  w.theta = take(R * d * S);
  w.phi = take(R * d * S);
  w.gtheta = take(R * d * S);
  w.gphi = take(R * d * S);
  w.pred = take(R * d);
  w.gx = take(R * d);
  w.t = take(R);
  w.scratch_bytes = dehoog_bwd_tape_bytes(R * d, S);
  w.scratch = take((w.scratch_bytes + 7) / 8);
  w.total = o;
  return w;
}

// the de Hoog contour's query point s_k = gamma + i pi k / T on the Riemann sphere, T = scale t, gamma = alpha - log_tol /
// (scale T) (as rep_inputs_kernel's Fourier / de Hoog branch, at the model's ILT scale)
NLC_HD void dehoog_query_point(double alpha, double log_tol, double scale, double t, int k, double* theta_s, double* phi_s) {
  const double Tt = scale * t;
  const double gamma = alpha - log_tol / (scale * Tt);
  const double im = kPiT * (double)k / Tt;
  const double a2v = gamma * gamma + im * im;
  *theta_s = atan2(im, gamma);
  *phi_s = asin((a2v - 1.0) / (a2v + 1.0));
}

// launches 1 and 5: the step's arguments (lin_tab unused) and member 0's slices of the ILT arrays; member m's are m * rows
// rows further on
struct DehoogTrainArgs {
  TrainArgs t;
  double scale;  // the model's ILT scale
  int64_t rows;
  double *theta, *phi, *tq;       // launch 1 writes
  const double *gtheta, *gphi;    // launch 5 reads
};

// launch 3: one workgroup per tile, the member on y
struct DehoogLossArgs {
  const double* pred;  // (M rows, d)
  const double* act;   // the slabs (targets of the tile: ActLayout::tgt)
  double* gx;          // (M rows, d)
  double* tile_loss;
  int64_t rows, N, A, tgt, ws;  // A: slab size, tgt: offset of the targets in a slab, ws: member stride of act / tile_loss
  int d;
};

}  // namespace train
}  // namespace nlc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace nlc {
namespace train {
// nblk tiles on x (one workgroup each), the M members on y
hipError_t launch_train_dehoog_fwd(const DehoogTrainArgs& a, int nblk, int M, hipStream_t s);
hipError_t launch_train_dehoog_loss(const DehoogLossArgs& a, int nblk, int M, hipStream_t s);
hipError_t launch_train_dehoog_bwd(const DehoogTrainArgs& a, int nblk, int M, hipStream_t s);
}  // namespace train
}  // namespace nlc
#endif
