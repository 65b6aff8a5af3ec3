// Device-side pieces the training and evaluation kernels share (kernels_train.hip, kernels_train_rnn.hip,
// kernels_train_eval.hip): weight / bias gradients as sums over a tile's samples, the layer-0 GRU gate element of the
// evaluation kernels, the Fourier series' quarter turn, the fixed-order block sum of the two reduce kernels, the clip + Adam
// body of the two Adam kernels (kernels_train.hip, kernels_train_members.hip), and the launch dispatch over the RNN widths.
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

// element j of a width-H GRU's first layer: r, z, n and hn = W_hn h + b_hn (torch.nn.GRU gate order [r; z; n]) from the
// row's normalised input x [nin] (nin <= 3: plain FMAs) and its hidden products gh = [r | z | n] of h W_hh^T (NULL at the
// first step: h_0 = 0).  The caller blends h' = (1 - z) n + z h with its own previous state and keeps what it tapes
struct Gate {
  double r, z, n, hn;
};
__device__ __forceinline__ Gate gru_gate0(const double* x, int nin, const double* __restrict__ Wih,
                                          const double* __restrict__ bih, const double* __restrict__ bhh, const double* gh,
                                          int H, int j) {
  double ir = 0.0, iz = 0.0, in_ = 0.0;
  for (int c = 0; c < nin; ++c) {
    const double xc = x[c];
    ir += Wih[j * nin + c] * xc;
    iz += Wih[(H + j) * nin + c] * xc;
    in_ += Wih[(2 * H + j) * nin + c] * xc;
  }
  ir += bih[j];
  iz += bih[H + j];
  in_ += bih[2 * H + j];
  const double hr = (gh ? gh[j] : 0.0) + bhh[j];
  const double hz = (gh ? gh[H + j] : 0.0) + bhh[H + j];
  Gate g;
  g.hn = (gh ? gh[2 * H + j] : 0.0) + bhh[2 * H + j];
  g.r = m::sigmoid_d(ir + hr);
  g.z = m::sigmoid_d(iz + hz);
  g.n = m::tanh_d(in_ + g.r * g.hn);
  return g;
}

// c_k = cos(theta + k pi/2) and its theta derivative, from one sincos (exact quarter turns: ILT scale 2)
__device__ __forceinline__ void quarter(double th, int k, double* c, double* cp) {
  double sn, cs;
  sincos(th, &sn, &cs);
  switch (k & 3) {
    case 0: *c = cs; *cp = -sn; break;
    case 1: *c = -sn; *cp = -cs; break;
    case 2: *c = -cs; *cp = sn; break;
    default: *c = sn; *cp = cs; break;
  }
}

// the sum of s over the workgroup's kThreads threads in a fixed tree (pairs i, i + w for w = 128 .. 1), on every thread
__device__ __forceinline__ double block_sum(double s) {
  __shared__ double red[kThreads];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// clip_grad_norm_ + Adam.step() of chunk blockIdx.x of member blockIdx.y: what train_adam_kernel and
// train_adam_members_kernel do once they have the member's settings (params / m / v / grad / sq / gradnorm are member 0's).
// Every workgroup forms the total norm from the same chunk sums in the same order (clip_total_norm); workgroup 0 reports it.
// active == false (uniform over the workgroup): the norm is reported, params / m / v are neither read nor written
__device__ __forceinline__ void clip_adam(double* params, double* m, double* v, const double* grad, const double* sq,
                                          double* gradnorm, const ChunkTable& ct, const GroupStrides& gs, double max_norm,
                                          const AdamScalars& k, bool active) {
  __shared__ double coef_s;
  const int b = blockIdx.x;
  const int64_t mi = blockIdx.y;  // member of the group: its own chunk sums, clip coefficient and slices of params / m / v
  if (threadIdx.x == 0) {
    const double total = clip_total_norm(sq + mi * gs.ws, ct);
    coef_s = max_norm > 0.0 ? clip_coef(max_norm, total) : 1.0;
    if (b == 0 && gradnorm) gradnorm[mi] = total;
  }
  if (!active) return;
  __syncthreads();
  const double coef = coef_s;
  grad += mi * gs.grad;
  params += mi * gs.params;
  m += mi * gs.params;
  v += mi * gs.params;
  const ChunkRange r = chunk_range(ct, b);
  for (int64_t e = r.e0 + threadIdx.x; e < r.e1; e += kThreads) {
    double gv = grad[e];
    if (max_norm > 0.0) gv = gv * coef;
    double p = params[e], mm = m[e], vv = v[e];
    adam_element(&p, &mm, &vv, gv, k);
    params[e] = p;
    m[e] = mm;
    v[e] = vv;
  }
}

// host: f(std::integral_constant<int, H>{}) at the H among the widths nlc_set_rnn_model takes (a kernel instance each);
// false when H is none of them
template <class F, int... Ws>
bool for_width(int H, F f, std::integer_sequence<int, Ws...>) {
  return ((H == Ws && (f(std::integral_constant<int, Ws>{}), true)) || ...);
}
template <class F>
bool for_rnn_width(int H, F f) {
  return for_width(H, f, std::integer_sequence<int, 64, 128, 160>{});
}

}  // namespace
}  // namespace train
}  // namespace nlc
