// The NeuralLaplaceModel training step's layers on a 16-row tile, shared by the kernels that run them (kernels_train.hip: the
// whole step in one launch; kernels_train_dehoog.hip: its forward and backward halves around the de Hoog ILT launches): the
// reverse GRU's two layers forward (taped) and backward through time, and the representation MLP's dense + tanh layers.
// All tapes are global-memory arrays of the workgroup's slab (nlc_train.h ActLayout).
#pragma once
#include "nlc_train_dev.h"

namespace nlc {
namespace train {

namespace {

// one GRU layer forward over the B window steps of the tile: X [s][r][din] inputs, H [s][r][g] states (H[0] = 0 on entry),
// G [s][r][4g] tape
__device__ void gru_layer_fwd(const TrainArgs& a, const double* __restrict__ W, const double* X, int din, double* H, double* G) {
  const int g = a.g;
  const double* Wih = W;
  const double* Whh = W + (int64_t)3 * g * din;
  const double* bih = Whh + (int64_t)3 * g * g;
  const double* bhh = bih + 3 * g;
  for (int s = 0; s < a.B; ++s) {
    for (int p = threadIdx.x; p < kRows * g; p += kThreads) {
      const int r = p & (kRows - 1), j = p >> 4;
      const double* x = X + ((int64_t)s * kRows + r) * din;
      const double* hp = H + ((int64_t)s * kRows + r) * g;
      double ir = 0.0, iz = 0.0, in_ = 0.0, hr = 0.0, hz = 0.0, hn = 0.0;
      for (int c = 0; c < din; ++c) {
        const double xc = x[c];
        ir += Wih[(int64_t)j * din + c] * xc;
        iz += Wih[(int64_t)(g + j) * din + c] * xc;
        in_ += Wih[(int64_t)(2 * g + j) * din + c] * xc;
      }
#pragma unroll 8
      for (int c = 0; c < g; ++c) {
        const double hc = hp[c];
        hr += Whh[(int64_t)j * g + c] * hc;
        hz += Whh[(int64_t)(g + j) * g + c] * hc;
        hn += Whh[(int64_t)(2 * g + j) * g + c] * hc;
      }
      ir += bih[j];
      iz += bih[g + j];
      in_ += bih[2 * g + j];
      hr += bhh[j];
      hz += bhh[g + j];
      hn += bhh[2 * g + j];
      const double rr = m::sigmoid_d(ir + hr);
      const double zz = m::sigmoid_d(iz + hz);
      const double nn = m::tanh_d(in_ + rr * hn);
      const double hnew = (1.0 - zz) * nn + zz * hp[j];
      double* tape = G + ((int64_t)s * kRows + r) * 4 * g;
      tape[j] = rr;
      tape[g + j] = zz;
      tape[2 * g + j] = nn;
      tape[3 * g + j] = hn;
      H[((int64_t)(s + 1) * kRows + r) * g + j] = hnew;
    }
    __syncthreads();
  }
}

// backprop through time of one GRU layer: dhA [r][g] holds dL/dh_B on entry (layer 1; 0 for layer 0), DXin [s][r][g] the
// gradient reaching the layer's OUTPUT at step s from above (layer 0: layer 1's input gradient; NULL for layer 1).
// Writes the gate gradients DI / DH [s][r][3g] and, if DXout != NULL, the gradient of the layer's INPUT at every step.
__device__ void gru_layer_bwd(const TrainArgs& a, const double* __restrict__ W, int din, const double* H, const double* G,
                              double* DI, double* DH, const double* DXin, double* DXout, double* dhA, double* dD) {
  const int g = a.g, g3 = 3 * g;
  const double* Wih = W;
  const double* Whh = W + (int64_t)3 * g * din;
  for (int s = a.B - 1; s >= 0; --s) {
    for (int p = threadIdx.x; p < kRows * g; p += kThreads) {
      const int r = p & (kRows - 1), j = p >> 4;
      const int64_t sr = (int64_t)s * kRows + r;
      double dh = dhA[r * g + j];
      if (DXin) dh += DXin[sr * g + j];
      const double* tape = G + sr * 4 * g;
      double gr, gz, gn, ghn, dd;
      gru_cell_bwd(dh, tape[j], tape[g + j], tape[2 * g + j], tape[3 * g + j], H[sr * g + j], &gr, &gz, &gn, &ghn, &dd);
      DI[sr * g3 + j] = gr;
      DI[sr * g3 + g + j] = gz;
      DI[sr * g3 + 2 * g + j] = gn;
      DH[sr * g3 + j] = gr;
      DH[sr * g3 + g + j] = gz;
      DH[sr * g3 + 2 * g + j] = ghn;
      dD[r * g + j] = dd;
    }
    __syncthreads();
    if (s > 0) {
      for (int p = threadIdx.x; p < kRows * g; p += kThreads) {
        const int r = p & (kRows - 1), i = p >> 4;
        const double* dgh = DH + ((int64_t)s * kRows + r) * g3;
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < g3; ++j) acc += Whh[(int64_t)j * g + i] * dgh[j];
        dhA[r * g + i] = dD[r * g + i] + acc;
      }
    }
    if (DXout) {
      for (int p = threadIdx.x; p < kRows * din; p += kThreads) {
        const int r = p & (kRows - 1), i = p >> 4;
        const double* dgi = DI + ((int64_t)s * kRows + r) * g3;
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < g3; ++j) acc += Wih[(int64_t)j * din + i] * dgi[j];
        DXout[((int64_t)s * kRows + r) * din + i] = acc;
      }
    }
    __syncthreads();
  }
}

// out[r][j] = tanh(sum_i W[j][i] in[r][i] + b[j])  (j < M, i < K)
__device__ void dense_tanh(const double* __restrict__ W, const double* __restrict__ b, const double* in, int K, int M, double* out) {
  for (int p = threadIdx.x; p < kRows * M; p += kThreads) {
    const int r = p & (kRows - 1), j = p >> 4;
    const double* x = in + (int64_t)r * K;
    const double* w = W + (int64_t)j * K;
    double acc = 0.0;
#pragma unroll 8
    for (int i = 0; i < K; ++i) acc += w[i] * x[i];
    out[(int64_t)r * M + j] = m::tanh_d(acc + b[j]);
  }
}

// delta[r][i] = (sum_j W[j][i] dout[r][j]) * (1 - y[r][i]^2)  (W is M x K, i < K)
__device__ void dense_tanh_bwd(const double* __restrict__ W, const double* dout, int K, int M, const double* y, double* delta) {
  for (int p = threadIdx.x; p < kRows * K; p += kThreads) {
    const int r = p & (kRows - 1), i = p >> 4;
    const double* dz = dout + (int64_t)r * M;
    double acc = 0.0;
#pragma unroll 8
    for (int j = 0; j < M; ++j) acc += W[(int64_t)j * K + i] * dz[j];
    const double yy = y[(int64_t)r * K + i];
    delta[(int64_t)r * K + i] = acc * (1.0 - yy * yy);
  }
}

}  // namespace

}  // namespace train
}  // namespace nlc
