// Device-side pieces the training kernels share (kernels_train.hip, kernels_train_rnn.hip): weight / bias gradients as sums
// over a tile's samples.
#pragma once
#include "nlc_device.h"
#include "nlc_train.h"

namespace nlc {
namespace train {
namespace {

constexpr int kWaves = kThreads / 64;

// out[m][k] (+)= sum_s D[s * ldD + m] * X[s * ldX + k]  (m < M, k < K, s < ns) on v_mfma_f64_16x16x4_f64: samples are the
// k dimension of the MFMA (4 per instruction), 16 x 16 output tiles dealt round-robin to the workgroup's waves.  first: the
// accumulator starts at 0, else at the values already in out (the workgroup's earlier tiles).
__device__ void wgrad_mfma(double* __restrict__ out, int M, int K, int ns, const double* __restrict__ D, int ldD,
                           const double* __restrict__ X, int ldX, bool first) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, c = lane & 15;
  const int mt = (M + 15) >> 4, kt = (K + 15) >> 4;
  for (int tile = wave; tile < mt * kt; tile += kWaves) {
    const int m0 = (tile / kt) << 4, k0 = (tile % kt) << 4;
    v4d acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + q + 4 * r, col = k0 + c;
      acc[r] = (!first && row < M && col < K) ? out[(int64_t)row * K + col] : 0.0;
    }
    const bool am = m0 + c < M, bk = k0 + c < K;
#pragma unroll 4
    for (int s0 = 0; s0 < ns; s0 += 4) {
      const int s = s0 + q;
      const double a = (s < ns && am) ? D[(int64_t)s * ldD + m0 + c] : 0.0;
      const double b = (s < ns && bk) ? X[(int64_t)s * ldX + k0 + c] : 0.0;
      acc = mfma(a, b, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + q + 4 * r, col = k0 + c;
      if (row < M && col < K) out[(int64_t)row * K + col] = acc[r];
    }
  }
}

// out[m] (+)= sum_s D[s * ldD + m], samples in order
__device__ void bgrad(double* __restrict__ out, int M, int ns, const double* __restrict__ D, int ldD, bool first) {
  for (int m = threadIdx.x; m < M; m += kThreads) {
    double acc = first ? 0.0 : out[m];
#pragma unroll 8
    for (int s = 0; s < ns; ++s) acc += D[(int64_t)s * ldD + m];
    out[m] = acc;
  }
}

}  // namespace
}  // namespace train
}  // namespace nlc
