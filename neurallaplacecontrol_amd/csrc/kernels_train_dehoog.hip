// Fused training step of a de Hoog NeuralLaplaceModel (ctx option "train_dehoog"; nlc_train_dehoog.h has the launch sequence):
// the forward and backward halves of train_fwd_bwd_kernel (kernels_train.hip), cut at the (rows, d, S) sphere angles, and the
// loss kernel between the two de Hoog ILT launches (kernels_dehoog.hip, kernels_dehoog_bwd.hip, both unchanged).  The
// quotient-difference table stays in those kernels: ilt_dehoog_bwd_kernel<16> alone takes up to 360 registers.
//
// One 256-thread workgroup per 16-row tile, the member of a group on blockIdx.y, as in train_fwd_bwd_kernel; a workgroup does
// not walk tiles, because the tile's slab (tapes, activations, targets) is read again by launches 3 and 5.  No atomics, no read
// of another member's memory: a member's bits do not depend on M.  The layers are nlc_train_nl_dev.h's, the weight / bias
// gradients nlc_train_dev.h's, in train_fwd_bwd_kernel's order.  Two things differ from the Fourier step: the line integral,
// and the last dense layer's tanh, which is the device library's here (dense_tanh_out below says why), so that layer's
// outputs u -- and through 1 - u^2 its backward -- are not tanh_d's bits.
//
// Rows past N of a ragged tile are zeros at t = 1 (finite inputs to every layer, as in train_fwd_bwd_kernel).  The table may
// still turn them into non-finite angles' gradients, so launch 5 SELECTS 0 for their last-layer deltas instead of relying on
// gx = 0 times whatever came back.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage) are in docs/training.md, section "de Hoog".
#include "nlc_train_nl_dev.h"  // first: brings the HIP runtime in before nlc_train.h's __host__ __device__ math

#include "nlc_train_dehoog.h"

namespace nlc {
namespace train {

namespace {

// dense_tanh (nlc_train_nl_dev.h) with the device library's tanh: the last layer only.  A de Hoog model's |F_k| is small where
// its transform decays (1e-3 on the tamed test weights), which puts the phi outputs within 1e-3 of -1: R = tan((1 + y) pi / 4)
// then carries an absolute error of y 1 / (1 + y) times over, and the table another order of magnitude.  tanh_d's 4 ulp gave
// 1e-11 relative on the loss where the grad-mode path (torch.tanh, this same library function) is at 1e-15; measured on
// the MI355X, docs/training.md
__device__ void dense_tanh_out(const double* __restrict__ W, const double* __restrict__ b, const double* in, int K, int M,
                               double* out) {
  for (int p = threadIdx.x; p < kRows * M; p += kThreads) {
    const int r = p & (kRows - 1), j = p >> 4;
    const double* x = in + (int64_t)r * K;
    const double* w = W + (int64_t)j * K;
    double acc = 0.0;
#pragma unroll 8
    for (int i = 0; i < K; ++i) acc += w[i] * x[i];
    out[(int64_t)r * M + j] = tanh(acc + b[j]);
  }
}

}  // namespace

// launch 1
__global__ __launch_bounds__(kThreads) void train_dehoog_fwd_kernel(const DehoogTrainArgs da) {
  const TrainArgs& a = da.t;
  const int d = a.d, nin = a.nin, g = a.g, h = a.h, S = a.S, B = a.B;
  const int K0 = 2 * S + d + 2, O = 2 * d * S;
  const ActLayout& L = a.L;
  const int64_t mi = blockIdx.y;
  double* ws = a.act + mi * a.gs.ws + (int64_t)blockIdx.x * a.A;
  double* X0 = ws + L.X0;
  double* H0 = ws + L.H0;
  double* G0 = ws + L.G0;
  double* H1 = ws + L.H1;
  double* G1 = ws + L.G1;
  double* a0 = ws + L.a0;
  double* a1 = ws + L.a1;
  double* a2 = ws + L.a2;
  double* u = ws + L.u;
  double* tn = ws + L.tn;
  double* tgt = ws + L.tgt;
  const double* prm = a.batch.params + mi * a.gs.params;
  const int64_t* off = a.off;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  // ---- inputs: gathered rows, normalised as nlc_model_forward (w_nl.py:120-131); rows past N are zeros at t = 1
  for (int p = threadIdx.x; p < kRows * (B * nin + d + 1); p += kThreads) {
    const int r = p & (kRows - 1), e = p >> 4;
    const bool valid = row0 + r < a.batch.N;
    // (evaluation may pass no index array: rows 0 .. N - 1)
    const int64_t pick = !valid ? 0 : a.batch.idx ? a.batch.idx[mi * a.gs.idx + row0 + r] : row0 + r;
    const int64_t src = pick + mi * a.gs.rows;
    if (e < B * nin) {
      const int s = e / nin, c = e - s * nin;  // step s of the reversed window = window row B - 1 - s
      X0[((int64_t)s * kRows + r) * nin + c] =
          valid ? (a.batch.window[(src * B + (B - 1 - s)) * nin + c] - a.norm.am[c]) / a.norm.as[c] : 0.0;
    } else if (e < B * nin + d) {
      const int c = e - B * nin;
      a0[(int64_t)r * K0 + 2 * S + c] = valid ? (a.batch.obs[src * d + c] - a.norm.sm[c]) / a.norm.ss[c] : 0.0;
      tgt[r * d + c] = valid ? a.batch.target[src * d + c] : 0.0;
    } else {
      tn[r] = valid ? a.batch.ts[src] / a.time_div : 1.0;
    }
  }
  for (int p = threadIdx.x; p < kRows * g; p += kThreads) {
    H0[p] = 0.0;
    H1[p] = 0.0;
  }
  __syncthreads();
  // ---- query points of the row's t on the Riemann sphere, at the model's ILT scale
  for (int p = threadIdx.x; p < kRows * S; p += kThreads) {
    const int r = p & (kRows - 1), k = p >> 4;
    dehoog_query_point(a.alpha, a.log_tol, da.scale, tn[r], k, &a0[(int64_t)r * K0 + k], &a0[(int64_t)r * K0 + S + k]);
  }
  // ---- reverse GRU encoder (w_nl.py:25-29), two layers
  gru_layer_fwd(a, prm + off[0], X0, nin, H0, G0);
  gru_layer_fwd(a, prm + off[4], H0 + (int64_t)kRows * g, g, H1, G1);
  // ---- linear_out -> enc, the last two latent columns
  {
    const double* Wlo = prm + off[8];
    const double* blo = prm + off[9];
    const double* hB = H1 + (int64_t)B * kRows * g;
    if (threadIdx.x < 2 * kRows) {
      const int r = threadIdx.x & (kRows - 1), c = threadIdx.x >> 4;
      double acc = 0.0;
      for (int i = 0; i < g; ++i) acc += Wlo[c * g + i] * hB[(int64_t)r * g + i];
      a0[(int64_t)r * K0 + 2 * S + d + c] = acc + blo[c];
    }
  }
  __syncthreads();
  // ---- representation MLP (w_nl.py:55-58)
  dense_tanh(prm + off[10], prm + off[11], a0, K0, h, a1);
  __syncthreads();
  dense_tanh(prm + off[12], prm + off[13], a1, h, h, a2);
  __syncthreads();
  dense_tanh_out(prm + off[14], prm + off[15], a2, h, O, u);
  __syncthreads();
  // ---- sphere map (w_nl.py:59-62) -> the ILT launches' (rows, d, S) angles and (rows) times, whole lines per row
  const int dS = d * S;
  const int64_t out0 = mi * da.rows + row0;
  for (int p = threadIdx.x; p < kRows * dS; p += kThreads) {
    const int r = p / dS, j = p - r * dS;
    da.theta[(out0 + r) * dS + j] = sphere_theta(u[(int64_t)r * O + j]);
    da.phi[(out0 + r) * dS + j] = sphere_phi(u[(int64_t)r * O + dS + j]);
  }
  if (threadIdx.x < kRows) da.tq[out0 + threadIdx.x] = tn[threadIdx.x];
}

// launch 3: a tile's squared errors, summed in the slab order train_fwd_bwd_kernel sums them in, and the loss gradient
__global__ __launch_bounds__(kThreads) void train_dehoog_loss_kernel(const DehoogLossArgs a) {
  __shared__ double sq[kRows * kMaxD];
  const int64_t mi = blockIdx.y;
  const int d = a.d;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const double* tgt = a.act + mi * a.ws + (int64_t)blockIdx.x * a.A + a.tgt;
  const double loss_norm = 2.0 / ((double)a.N * (double)d);  // MSELoss backward: 2 / numel * (input - target)
  if ((int)threadIdx.x < kRows * d) {
    const int r = threadIdx.x & (kRows - 1), c = threadIdx.x >> 4;
    const int64_t o = (mi * a.rows + row0 + r) * d + c;
    const bool valid = row0 + r < a.N;
    const double diff = a.pred[o] - tgt[r * d + c];
    sq[r * d + c] = valid ? diff * diff : 0.0;
    a.gx[o] = valid ? loss_norm * diff : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < kRows * d; ++i) s += sq[i];
    a.tile_loss[mi * a.ws + blockIdx.x] = s;
  }
}

// launch 5
__global__ __launch_bounds__(kThreads) void train_dehoog_bwd_kernel(const DehoogTrainArgs da) {
  const TrainArgs& a = da.t;
  const int d = a.d, nin = a.nin, g = a.g, h = a.h, S = a.S, B = a.B;
  const int K0 = 2 * S + d + 2, O = 2 * d * S;
  const ActLayout& L = a.L;
  const int64_t mi = blockIdx.y;
  double* ws = a.act + mi * a.gs.ws + (int64_t)blockIdx.x * a.A;
  double* X0 = ws + L.X0;
  double* H0 = ws + L.H0;
  double* G0 = ws + L.G0;
  double* H1 = ws + L.H1;
  double* G1 = ws + L.G1;
  double* a0 = ws + L.a0;
  double* a1 = ws + L.a1;
  double* a2 = ws + L.a2;
  double* u = ws + L.u;
  double* d3 = ws + L.d3;
  double* d2 = ws + L.d2;
  double* d1 = ws + L.d1;
  double* denc = ws + L.denc;
  double* DI0 = ws + L.DI0;
  double* DH0 = ws + L.DH0;
  double* DI1 = ws + L.DI1;
  double* DH1 = ws + L.DH1;
  double* DX1 = ws + L.DX1;
  double* dhA = ws + L.dhA;
  double* dD = ws + L.dD;
  const double* prm = a.batch.params + mi * a.gs.params;
  const int64_t* off = a.off;
  double* part = a.partial + mi * a.gs.ws + (int64_t)blockIdx.x * a.P;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const bool first = true;  // one tile per workgroup: every sum starts at 0
  // ---- sphere map backward: the ILT's angle gradients -> the last layer's pre-activation deltas; exactly 0 past N
  const int dS = d * S;
  const int64_t in0 = mi * da.rows + row0;
  for (int p = threadIdx.x; p < kRows * dS; p += kThreads) {
    const int r = p / dS, j = p - r * dS;
    const bool valid = row0 + r < a.batch.N;
    const double gth = da.gtheta[(in0 + r) * dS + j], gph = da.gphi[(in0 + r) * dS + j];
    d3[(int64_t)r * O + j] = valid ? sphere_theta_bwd(gth, u[(int64_t)r * O + j]) : 0.0;
    d3[(int64_t)r * O + dS + j] = valid ? sphere_phi_bwd(gph, u[(int64_t)r * O + dS + j]) : 0.0;
  }
  __syncthreads();
  // ---- MLP backward
  dense_tanh_bwd(prm + off[14], d3, h, O, a2, d2);
  __syncthreads();
  dense_tanh_bwd(prm + off[12], d2, h, h, a1, d1);
  __syncthreads();
  // the latent enc columns of layer 0's input: the only input gradient that flows on (into the encoder)
  if (threadIdx.x < 2 * kRows) {
    const int r = threadIdx.x & (kRows - 1), c = threadIdx.x >> 4;
    const double* W0 = prm + off[10];
    double acc = 0.0;
    for (int j = 0; j < h; ++j) acc += W0[(int64_t)j * K0 + 2 * S + d + c] * d1[(int64_t)r * h + j];
    denc[r * 2 + c] = acc;
  }
  // MLP weight / bias gradients (independent of the encoder's backward)
  wgrad_mfma(part + off[14], O, h, kRows, d3, O, a2, h, first);
  wgrad_mfma(part + off[12], h, h, kRows, d2, h, a1, h, first);
  wgrad_mfma(part + off[10], h, K0, kRows, d1, h, a0, K0, first);
  bgrad(part + off[15], O, kRows, d3, O, first);
  bgrad(part + off[13], h, kRows, d2, h, first);
  bgrad(part + off[11], h, kRows, d1, h, first);
  __syncthreads();
  // ---- linear_out backward
  {
    const double* Wlo = prm + off[8];
    const double* hB = H1 + (int64_t)B * kRows * g;
    for (int p = threadIdx.x; p < 2 * g; p += kThreads) {
      const int c = p / g, i = p - c * g;
      double acc = 0.0;
      for (int r = 0; r < kRows; ++r) acc += denc[r * 2 + c] * hB[(int64_t)r * g + i];
      part[off[8] + p] = acc;
    }
    if (threadIdx.x < 2) {
      const int c = threadIdx.x;
      double acc = 0.0;
      for (int r = 0; r < kRows; ++r) acc += denc[r * 2 + c];
      part[off[9] + c] = acc;
    }
    for (int p = threadIdx.x; p < kRows * g; p += kThreads) {
      const int r = p & (kRows - 1), i = p >> 4;
      dhA[r * g + i] = Wlo[i] * denc[r * 2] + Wlo[g + i] * denc[r * 2 + 1];
    }
  }
  __syncthreads();
  // ---- GRU backprop through time: layer 1 (its input gradient -> DX1), then layer 0
  gru_layer_bwd(a, prm + off[4], g, H1, G1, DI1, DH1, nullptr, DX1, dhA, dD);
  for (int p = threadIdx.x; p < kRows * g; p += kThreads) dhA[p] = 0.0;
  __syncthreads();
  gru_layer_bwd(a, prm + off[0], nin, H0, G0, DI0, DH0, DX1, nullptr, dhA, dD);
  // ---- GRU weight / bias gradients: sums over the B * 16 (step, row) samples
  const int ns = B * kRows, g3 = 3 * g;
  wgrad_mfma(part + off[0], g3, nin, ns, DI0, g3, X0, nin, first);
  wgrad_mfma(part + off[1], g3, g, ns, DH0, g3, H0, g, first);
  wgrad_mfma(part + off[4], g3, g, ns, DI1, g3, H0 + (int64_t)kRows * g, g, first);
  wgrad_mfma(part + off[5], g3, g, ns, DH1, g3, H1, g, first);
  bgrad(part + off[2], g3, ns, DI0, g3, first);
  bgrad(part + off[3], g3, ns, DH0, g3, first);
  bgrad(part + off[6], g3, ns, DI1, g3, first);
  bgrad(part + off[7], g3, ns, DH1, g3, first);
}

hipError_t launch_train_dehoog_fwd(const DehoogTrainArgs& a, int nblk, int M, hipStream_t s) {
  hipLaunchKernelGGL(train_dehoog_fwd_kernel, dim3(nblk, M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_train_dehoog_loss(const DehoogLossArgs& a, int nblk, int M, hipStream_t s) {
  hipLaunchKernelGGL(train_dehoog_loss_kernel, dim3(nblk, M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_train_dehoog_bwd(const DehoogTrainArgs& a, int nblk, int M, hipStream_t s) {
  hipLaunchKernelGGL(train_dehoog_bwd_kernel, dim3(nblk, M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace train
}  // namespace nlc
