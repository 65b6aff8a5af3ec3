// Fused training step of the DeltaTRNN / RNN baselines (train_utils.py:550-631 trained by the loop :388-408): forward,
// squared error and backward of one 16-row tile per workgroup, float64.  train_reduce_kernel and train_adam_kernel
// (kernels_train.hip) finish the iteration from the workgroups' partials, as for the NL model.
//
//   rnn_train_fwd_bwd_kernel<H>   rows gathered through the int64 index array and normalised with nlc_rnn_desc's constants;
//                                 a forward-order GRU (h_0 = 0, gate order [r; z; n]) with its gates taped; linear_out over
//                                 [h_B | obs_n | ts_n] (ts_n only with time_input); squared error; then linear_out's backward and
//                                 backprop through time (nlc_train.h gru_cell_bwd).  Weight gradients are sums over the tile's
//                                 samples, accumulated onto the workgroup's partial in blob order.
//
// The three products with the hidden state run on v_mfma_f64_16x16x4_f64 with the tile's 16 rows as the MFMA's M:
//   forward    h W_hh^T          [16 x H] [H x 3H]    3H / 16 column tiles dealt round-robin to the four waves
//   backward   dgh W_hh          [16 x 3H] [3H x H]   H / 16 column tiles (4, 8 or 10) x two halves of k: a wave takes one half
//                                                     of every second tile, so the four waves carry the same 3H H / 64 MFMAs
//                                                     at every width; the halves meet in the next step's element phase
//   gradient   sum_s dgh_s^T h_{s-1}                  wgrad_mfma: k = 16 rows x (B - 1) steps (h_0 = 0 adds nothing)
// An MFMA's four k lanes take four contiguous quarters of the k range, so a lane walks its operands with unit stride.
// The current hidden state, the gate tile and dL/dh stay in LDS ([row][feature], 16 (5 H + 6) doubles: 101 KB at H = 160);
// the tapes go to the workgroup's slab.  The nin <= 3 input projection and the d <= 8 output layer are plain FMAs.
// No atomics: a workgroup sums its tiles in order and the reduce kernel the workgroups in order (bit-reproducible).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage): docs/training.md.
#include "nlc_train_dev.h"

namespace nlc {
namespace train {

namespace {

constexpr int kLdPad = 2;  // doubles of padding per LDS row: rows of an MFMA's A operand start on different banks

// gS[r][n] = sum_k hS[r][k] W_hh[n][k]  (n < 3H, k < H)
template <int H>
__device__ __forceinline__ void hidden_fwd_mfma(const double* hS, const double* __restrict__ Whh, double* gS) {
  constexpr int LH = H + kLdPad, LG = 3 * H + kLdPad, KQ = H / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, c = lane & 15;
  const double* arow = hS + c * LH + q * KQ;
  for (int tile = wave; tile < 3 * H / 16; tile += kWaves) {
    const double* wrow = Whh + (int64_t)(tile * 16 + c) * H + q * KQ;
    v4d acc = splat(0.0);
#pragma unroll 8
    for (int t = 0; t < KQ; ++t) acc = mfma(arow[t], wrow[t], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) gS[(q + 4 * r) * LG + tile * 16 + c] = acc[r];
  }
}

// dL/dh_{s-1}[r][i] = dS[r][i] (the direct part, on entry) + sum_j gS[r][j] W_hh[j][i]  (j < 3H, i < H), left as two
// addends: dS takes the first half of j on top of what it held, pS the second half
template <int H>
__device__ __forceinline__ void hidden_bwd_mfma(const double* gS, const double* __restrict__ Whh, double* dS, double* pS) {
  constexpr int LH = H + kLdPad, LG = 3 * H + kLdPad, KQ = 3 * H / 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, c = lane & 15;
  const int half = wave & 1;
  const int j0 = half * (3 * H / 2) + q * KQ;
  const double* arow = gS + c * LG + j0;
  double* out = half ? pS : dS;
  for (int tile = wave >> 1; tile < H / 16; tile += kWaves / 2) {
    const double* wcol = Whh + (int64_t)j0 * H + tile * 16 + c;
    v4d acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = half ? 0.0 : dS[(q + 4 * r) * LH + tile * 16 + c];
#pragma unroll 8
    for (int t = 0; t < KQ; ++t) acc = mfma(arow[t], wcol[(int64_t)t * H], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(q + 4 * r) * LH + tile * 16 + c] = acc[r];
  }
}

}  // namespace

template <int H>
__global__ __launch_bounds__(kThreads) void rnn_train_fwd_bwd_kernel(const RnnTrainArgs a) {
  static_assert(H % 32 == 0 && (3 * H) % 16 == 0, "k quarters of both products must be whole");
  constexpr int H3 = 3 * H, LH = H + kLdPad, LG = H3 + kLdPad, LF = kMaxD + 1;
  __shared__ double hS[kRows * LH];      // forward: the current hidden state; backward: second addend of dL/dh
  __shared__ double gS[kRows * LG];      // forward: h W_hh^T; backward: the hidden-side gate gradients
  __shared__ double dS[kRows * LH];      // backward: dL/dh
  __shared__ double fS[kRows * LF];      // [obs_n | ts_n]
  __shared__ double tS[kRows * kMaxD];   // target
  __shared__ double eS[kRows * kMaxD];   // dL/dpred
  __shared__ double sqS[kRows * kMaxD];  // squared errors
  const int d = a.d, nin = a.nin, B = a.B, ti = a.time_input ? 1 : 0;
  const int F = H + d + ti;
  const RnnActLayout& L = a.L;
  const int64_t mi = blockIdx.y;  // member of the group (nlc_train.h GroupStrides; a single model is M = 1)
  double* ws = a.act + mi * a.gs.ws + (int64_t)blockIdx.x * a.A;
  double* X = ws + L.X;
  double* Hs = ws + L.Hs;
  double* G = ws + L.G;
  double* DI = ws + L.DI;
  double* DH = ws + L.DH;
  const double* prm = a.batch.params + mi * a.gs.params;
  const double* Wih = prm + a.off[0];
  const double* Whh = prm + a.off[1];
  const double* bih = prm + a.off[2];
  const double* bhh = prm + a.off[3];
  const double* Wo = prm + a.off[4];
  const double* bo = prm + a.off[5];
  double* part = a.partial + mi * a.gs.ws + (int64_t)blockIdx.x * a.P;
  double* tile_loss = a.tile_loss + mi * a.gs.ws;
  // the member's slice of the index array and its rows of a stacked dataset (gs.rows = 0: the shared one)
  const int64_t* idx = a.batch.idx + mi * a.gs.idx;
  const int64_t drow = mi * a.gs.rows;
  const double* obs = a.batch.obs + drow * d;
  const double* window = a.batch.window + drow * B * nin;
  const double* tsp = ti ? a.batch.ts + drow : nullptr;  // a model without time input has no ts (batch.ts may be NULL)
  const double* target = a.batch.target + drow * d;
  const double loss_norm = 2.0 / ((double)a.batch.N * (double)d);  // MSELoss backward: 2 / numel * (input - target)

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const bool first = tile == (int)blockIdx.x;
    const int64_t row0 = (int64_t)tile * kRows;
    // ---- inputs: gathered rows, normalised (train_utils.py:618-626 / :577-582, the branch resolved in the descriptor); rows
    // past N are zeros, and their loss gradient is 0
    for (int p = threadIdx.x; p < kRows * (B * nin + d + 1); p += kThreads) {
      const int r = p & (kRows - 1), e = p >> 4;
      const bool valid = row0 + r < a.batch.N;
      const int64_t src = valid ? idx[row0 + r] : 0;
      if (e < B * nin) {
        const int s = e / nin, c = e - s * nin;
        X[((int64_t)s * kRows + r) * nin + c] = valid ? (window[(src * B + s) * nin + c] - a.norm.am[c]) / a.norm.as[c] : 0.0;
      } else if (e < B * nin + d) {
        const int c = e - B * nin;
        fS[r * LF + c] = valid ? (obs[src * d + c] - a.norm.sm[c]) / a.norm.ss[c] : 0.0;
        tS[r * kMaxD + c] = valid ? target[src * d + c] : 0.0;
      } else {
        fS[r * LF + d] = (valid && ti) ? tsp[src] / a.time_div : 0.0;
      }
    }
    for (int p = threadIdx.x; p < kRows * H; p += kThreads) {
      const int r = p / H, j = p - r * H;
      hS[r * LH + j] = 0.0;
      Hs[p] = 0.0;
    }
    __syncthreads();
    // ---- GRU forward (h_0 = 0: the first step has no hidden product)
    for (int s = 0; s < B; ++s) {
      if (s > 0) {
        hidden_fwd_mfma<H>(hS, Whh, gS);
        __syncthreads();
      }
      for (int p = threadIdx.x; p < kRows * H; p += kThreads) {
        const int r = p / H, j = p - r * H;
        const int64_t sr = (int64_t)s * kRows + r;
        const double* x = X + sr * nin;
        double ir = 0.0, iz = 0.0, in_ = 0.0;
        for (int c = 0; c < nin; ++c) {
          const double xc = x[c];
          ir += Wih[(int64_t)j * nin + c] * xc;
          iz += Wih[(int64_t)(H + j) * nin + c] * xc;
          in_ += Wih[(int64_t)(2 * H + j) * nin + c] * xc;
        }
        ir += bih[j];
        iz += bih[H + j];
        in_ += bih[2 * H + j];
        const double* gh = gS + r * LG;
        const double hr = (s > 0 ? gh[j] : 0.0) + bhh[j];
        const double hz = (s > 0 ? gh[H + j] : 0.0) + bhh[H + j];
        const double hn = (s > 0 ? gh[2 * H + j] : 0.0) + bhh[2 * H + j];
        const double rr = m::sigmoid_d(ir + hr);
        const double zz = m::sigmoid_d(iz + hz);
        const double nn = m::tanh_d(in_ + rr * hn);
        const double hnew = (1.0 - zz) * nn + zz * hS[r * LH + j];
        double* tape = G + sr * 4 * H;
        tape[j] = rr;
        tape[H + j] = zz;
        tape[2 * H + j] = nn;
        tape[3 * H + j] = hn;
        Hs[(sr + kRows) * H + j] = hnew;
        hS[r * LH + j] = hnew;
      }
      __syncthreads();
    }
    // ---- linear_out over [h_B | obs_n | ts_n], squared error, dL/dpred
    for (int p = threadIdx.x; p < kRows * d; p += kThreads) {
      const int r = p & (kRows - 1), c = p >> 4;
      const double* w = Wo + (int64_t)c * F;
      const double* hB = hS + r * LH;
      double acc = 0.0;
#pragma unroll 8
      for (int i = 0; i < H; ++i) acc += w[i] * hB[i];
      for (int i = 0; i < d + ti; ++i) acc += w[H + i] * fS[r * LF + i];
      const double diff = (acc + bo[c]) - tS[r * kMaxD + c];
      const bool valid = row0 + r < a.batch.N;
      sqS[r * d + c] = valid ? diff * diff : 0.0;
      eS[r * kMaxD + c] = valid ? loss_norm * diff : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = first ? 0.0 : tile_loss[blockIdx.x];
      for (int i = 0; i < kRows * d; ++i) s += sqS[i];
      tile_loss[blockIdx.x] = s;
    }
    // ---- linear_out backward: its weight / bias gradients and dL/dh_B
    for (int p = threadIdx.x; p < d * F; p += kThreads) {
      const int c = p / F, i = p - c * F;
      double acc = first ? 0.0 : part[a.off[4] + p];
      for (int r = 0; r < kRows; ++r) acc += eS[r * kMaxD + c] * (i < H ? hS[r * LH + i] : fS[r * LF + i - H]);
      part[a.off[4] + p] = acc;
    }
    if ((int)threadIdx.x < d) {
      const int c = threadIdx.x;
      double acc = first ? 0.0 : part[a.off[5] + c];
      for (int r = 0; r < kRows; ++r) acc += eS[r * kMaxD + c];
      part[a.off[5] + c] = acc;
    }
    for (int p = threadIdx.x; p < kRows * H; p += kThreads) {
      const int r = p / H, j = p - r * H;
      double acc = 0.0;
      for (int c = 0; c < d; ++c) acc += Wo[(int64_t)c * F + j] * eS[r * kMaxD + c];
      dS[r * LH + j] = acc;
    }
    __syncthreads();
    // ---- backprop through time
    for (int s = B - 1; s >= 0; --s) {
      for (int p = threadIdx.x; p < kRows * H; p += kThreads) {
        const int r = p / H, j = p - r * H;
        const int64_t sr = (int64_t)s * kRows + r;
        const double dh = s < B - 1 ? dS[r * LH + j] + hS[r * LH + j] : dS[r * LH + j];
        const double* tape = G + sr * 4 * H;
        double gr, gz, gn, ghn, dd;
        gru_cell_bwd(dh, tape[j], tape[H + j], tape[2 * H + j], tape[3 * H + j], Hs[sr * H + j], &gr, &gz, &gn, &ghn, &dd);
        DI[sr * H3 + j] = gr;
        DI[sr * H3 + H + j] = gz;
        DI[sr * H3 + 2 * H + j] = gn;
        DH[sr * H3 + j] = gr;
        DH[sr * H3 + H + j] = gz;
        DH[sr * H3 + 2 * H + j] = ghn;
        gS[r * LG + j] = gr;
        gS[r * LG + H + j] = gz;
        gS[r * LG + 2 * H + j] = ghn;
        dS[r * LH + j] = dd;
      }
      __syncthreads();
      if (s > 0) {
        hidden_bwd_mfma<H>(gS, Whh, dS, hS);
        __syncthreads();
      }
    }
    // ---- GRU weight / bias gradients: sums over the (step, row) samples; W_hh pairs dgh_s with h_{s-1}, and h_0 = 0
    const int ns = B * kRows;
    wgrad_mfma(part + a.off[0], H3, nin, ns, DI, H3, X, nin, first);
    wgrad_mfma(part + a.off[1], H3, H, ns - kRows, DH + (int64_t)kRows * H3, H3, Hs + (int64_t)kRows * H, H, first);
    bgrad(part + a.off[2], H3, ns, DI, H3, first);
    bgrad(part + a.off[3], H3, ns, DH, H3, first);
    __syncthreads();
  }
}

hipError_t launch_rnn_train_fwd_bwd(const RnnTrainArgs& a, int H, int nblk, int M, hipStream_t s) {
  const bool found = for_rnn_width(H, [&](auto w) {
    hipLaunchKernelGGL((rnn_train_fwd_bwd_kernel<decltype(w)::value>), dim3(nblk, M), dim3(kThreads), 0, s, a);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace train
}  // namespace nlc
