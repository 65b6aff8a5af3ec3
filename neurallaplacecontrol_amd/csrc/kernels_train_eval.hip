// Held-out loss of the fused trainers: the forward-only siblings of train_fwd_bwd_kernel / rnn_train_fwd_bwd_kernel.  The
// reference's validation loss (overlay.py:112-115, :175-177) is model(s0, a0, ts) followed by an MSE; here that is two
// launches on the training step's data conventions (rows gathered through an int64 index array, the flat parameter blob,
// blockIdx.y the member of a group with nlc_train.h's GroupStrides), with no backward, no tape and no Adam:
//
//   train_eval_kernel<kLinear>   NeuralLaplaceModel, one 16-row tile at a time: normalisation as nlc_model_forward, the 2-layer
//                                reverse GRU, linear_out, the per-row query points (Fourier, or node / t of fixed Talbot /
//                                Stehfest), the representation MLP, the sphere map and the line integral at the row's own t,
//                                squared error against target.  The tile's sum goes to tile_loss[tile].
//   rnn_eval_kernel<H>           DeltaTRNN / RNN: forward-order GRU, linear_out over [h_B | obs_n | ts_n], squared error.
//   eval_reduce_kernel           one workgroup per member: loss[m] = sum(tile_loss) / (N d), in a fixed order.
//
// Nothing outlives a tile, so every activation is in LDS (nlc_train_eval.h EvalLdsLayout; [row][feature] doubles with a row
// stride that is an odd multiple of four banks) and the workspace is the tile losses.  All products with 16 or more
// input features run on v_mfma_f64_16x16x4_f64 with the tile's rows as the MFMA's M and 16 output features as its N
// (dense_mfma); an MFMA's four k lanes take k = 4 t + q, so the four read 32 contiguous bytes of a weight row and four
// neighbouring banks of an activation row.  The element math is nlc_train.h's and nlc_math.h's, the expressions those of the
// training kernels' forward; the order of the products' sums differs, so the loss agrees with loss_and_grad's to rounding
// (tests/test_gpu_train_eval.py: 1e-12 relative), not bit for bit.
//
// No atomics: a tile's squared errors are summed in order by one thread, and the tiles by eval_reduce_kernel in an order
// that depends on the tile count alone -- not on the grid, on M or on a member's neighbours.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage): docs/training.md, "Held-out loss".
#include <atomic>

#include "nlc_train_dev.h"
#include "nlc_train_eval.h"

namespace nlc {
namespace train {

namespace {

// acc += in[c][k] W[n][k] over k < K for the lane's row c of the tile and output feature n (x, w: the two rows)
__device__ __forceinline__ v4d mfma_row(const double* x, const double* __restrict__ w, int K, int q, v4d acc) {
  const int K4 = K >> 2;
  x += q;
  w += q;
  int t = 0;
  for (; t + 4 <= K4; t += 4) {  // four k steps' operands in flight
    double xa[4], wa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xa[i] = x[4 * (t + i)];
      wa[i] = w[4 * (t + i)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = mfma(xa[i], wa[i], acc);
  }
  for (; t < K4; ++t) acc = mfma(x[4 * t], w[4 * t], acc);
  x -= q;
  w -= q;
  if (K & 3) {
    const int k = 4 * K4 + q;
    const bool ok = k < K;
    acc = mfma(ok ? x[k] : 0.0, ok ? w[k] : 0.0, acc);
  }
  return acc;
}

// epi(r, n, sum_k in[r][k] W[n][k] + sum_k in2[r][k] W2[n][k])  for the 16 rows r and n < Nout; in / in2 are LDS arrays
// [16][ldi / ldi2], W / W2 row-major [Nout][K / K2] in global memory (in2 == NULL: one product).  The 16-feature output
// tiles are dealt round-robin to the four waves, starting at wave rot
template <class Epi>
__device__ __forceinline__ void dense_mfma(const double* in, int ldi, const double* __restrict__ W, int K, const double* in2,
                                           int ldi2, const double* __restrict__ W2, int K2, int Nout, int rot, Epi epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, c = lane & 15;
  const int nt = (Nout + 15) >> 4;
  for (int tile = (wave - rot) & (kWaves - 1); tile < nt; tile += kWaves) {
    const int n = tile * 16 + c;
    const int nc = n < Nout ? n : Nout - 1;  // a ragged tile's spare lanes read the last row and store nothing
    v4d acc = splat(0.0);
    acc = mfma_row(in + c * ldi, W + (int64_t)nc * K, K, q, acc);
    if (in2) acc = mfma_row(in2 + c * ldi2, W2 + (int64_t)nc * K2, K2, q, acc);
    if (n < Nout) {
#pragma unroll
      for (int r = 0; r < 4; ++r) epi(q + 4 * r, n, acc[r]);
    }
  }
}
template <class Epi>
__device__ __forceinline__ void dense_mfma(const double* in, int ldi, const double* __restrict__ W, int K, int Nout, int rot,
                                           Epi epi) {
  dense_mfma(in, ldi, W, K, nullptr, 0, nullptr, 0, Nout, rot, epi);
}

// out[r][n] = tanh(sum_k in[r][k] W[n][k] + b[n])
__device__ __forceinline__ void dense_tanh_lds(const double* in, int ldi, const double* __restrict__ W,
                                               const double* __restrict__ b, int K, int Nout, double* out, int ldo) {
  dense_mfma(in, ldi, W, K, Nout, 0, [=](int r, int n, double v) { out[r * ldo + n] = m::tanh_d(v + b[n]); });
}

}  // namespace

template <bool kLinear>
__global__ __launch_bounds__(kThreads) void train_eval_kernel(const EvalArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int d = a.d, nin = a.nin, g = a.g, h = a.h, S = a.S, B = a.B;
  const int K0 = 2 * S + d + 2;
  const int lg = 31 - __clz(g);  // g = h / 2 is 32, 64 or 128
  const EvalLdsLayout& L = a.L;
  const int ldg = L.ldg, ldG = L.ldG, ldK = L.ldK, ldh = L.ldh, ldu = L.ldu;
  double* X0 = lds + L.X;
  double* a0 = lds + L.a0;
  double* tn = lds + L.tn;
  double* tgt = lds + L.tgt;
  double* sq = lds + L.sq;
  double* h0 = lds + L.h0;
  double* h1 = lds + L.h1;
  double* G = lds + L.G;
  double* a1 = lds + L.a1;
  double* a2 = lds + L.a2;
  double* u = lds + L.u;
  const int64_t mi = blockIdx.y;  // member of the group: its own blob, tile losses, index array and dataset rows
  const Batch& b = a.batch;
  const double* prm = b.params + mi * a.gs.params;
  const int64_t* off = a.off;
  double* tile_loss = a.tile_loss + mi * a.gs.ws;
  const int64_t* idx = b.idx ? b.idx + mi * a.gs.idx : nullptr;
  const int64_t drow = mi * a.gs.rows;
  // the encoder's tensors (blob order: W_ih, W_hh, b_ih, b_hh of layer 0, then of layer 1)
  const double* Wih0 = prm + off[0];
  const double* Whh0 = prm + off[1];
  const double* bih0 = prm + off[2];
  const double* bhh0 = prm + off[3];
  const double* Wih1 = prm + off[4];
  const double* Whh1 = prm + off[5];
  const double* bih1 = prm + off[6];
  const double* bhh1 = prm + off[7];

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRows;
    // ---- inputs: gathered rows, normalised as nlc_model_forward (w_nl.py:120-131); rows past N are zeros at t = 1 (finite
    // everywhere) and add nothing to the loss
    for (int p = threadIdx.x; p < kRows * (B * nin + d + 1); p += kThreads) {
      const int r = p & (kRows - 1), e = p >> 4;
      const bool valid = row0 + r < b.N;
      const int64_t src = (valid ? (idx ? idx[row0 + r] : row0 + r) : 0) + drow;
      if (e < B * nin) {
        const int s = e / nin, c = e - s * nin;  // step s of the reversed window = window row B - 1 - s
        X0[(s * kRows + r) * nin + c] =
            valid ? (b.window[(src * B + (B - 1 - s)) * nin + c] - a.norm.am[c]) / a.norm.as[c] : 0.0;
      } else if (e < B * nin + d) {
        const int c = e - B * nin;
        a0[r * ldK + 2 * S + c] = valid ? (b.obs[src * d + c] - a.norm.sm[c]) / a.norm.ss[c] : 0.0;
        tgt[r * d + c] = valid ? b.target[src * d + c] : 0.0;
      } else {
        tn[r] = valid ? b.ts[src] / a.time_div : 1.0;
      }
    }
    for (int p = threadIdx.x; p < kRows * ldg; p += kThreads) {
      h0[p] = 0.0;
      h1[p] = 0.0;
    }
    __syncthreads();
    // ---- query points s_k = gamma + i pi k / T (linear algorithms: node_k / t) of the row's t on the Riemann sphere
    for (int p = threadIdx.x; p < kRows * S; p += kThreads) {
      const int r = p & (kRows - 1), k = p >> 4;
      if constexpr (kLinear) {
        linear_query_point(a.lin_tab[k], a.lin_tab[S + k], tn[r], &a0[r * ldK + k], &a0[r * ldK + S + k]);
      } else {
        fourier_query_point(a.alpha, a.log_tol, tn[r], k, &a0[r * ldK + k], &a0[r * ldK + S + k]);
      }
    }
    // ---- reverse GRU encoder (w_nl.py:25-29): both layers step by step, h_0 = 0 (the first step has no hidden products)
    for (int s = 0; s < B; ++s) {
      if (s > 0) {
        dense_mfma(h0, ldg, Whh0, g, 3 * g, 0, [=](int r, int n, double v) { G[r * ldG + n] = v; });
        __syncthreads();
      }
      for (int p = threadIdx.x; p < kRows * g; p += kThreads) {
        const int r = p >> lg, j = p & (g - 1);
        const Gate gt = gru_gate0(X0 + (s * kRows + r) * nin, nin, Wih0, bih0, bhh0, s > 0 ? G + r * ldG : nullptr, g, j);
        h0[r * ldg + j] = (1.0 - gt.z) * gt.n + gt.z * h0[r * ldg + j];
      }
      __syncthreads();
      // layer 1: the r and z gates take both products in one accumulator; the n gate keeps its two halves apart
      // G = [r | z | W_in x | W_hn h]
      {
        const int rot1 = (2 * g / 16) & (kWaves - 1), rot2 = (3 * g / 16) & (kWaves - 1);
        const auto store = [=](int col0) { return [=](int r, int n, double v) { G[r * ldG + col0 + n] = v; }; };
        dense_mfma(h0, ldg, Wih1, g, s > 0 ? h1 : nullptr, ldg, Whh1, g, 2 * g, 0, store(0));
        dense_mfma(h0, ldg, Wih1 + (int64_t)2 * g * g, g, g, rot1, store(2 * g));
        if (s > 0) dense_mfma(h1, ldg, Whh1 + (int64_t)2 * g * g, g, g, rot2, store(3 * g));
      }
      __syncthreads();
      for (int p = threadIdx.x; p < kRows * g; p += kThreads) {
        const int r = p >> lg, j = p & (g - 1);
        const double* gg = G + r * ldG;
        const double pr = gg[j] + bih1[j] + bhh1[j];
        const double pz = gg[g + j] + bih1[g + j] + bhh1[g + j];
        const double in_ = gg[2 * g + j] + bih1[2 * g + j];
        const double hn = (s > 0 ? gg[3 * g + j] : 0.0) + bhh1[2 * g + j];
        const double rr = m::sigmoid_d(pr);
        const double zz = m::sigmoid_d(pz);
        const double nn = m::tanh_d(in_ + rr * hn);
        h1[r * ldg + j] = (1.0 - zz) * nn + zz * h1[r * ldg + j];
      }
      __syncthreads();
    }
    // ---- linear_out -> enc, the last two latent columns
    if (threadIdx.x < 2 * kRows) {
      const double* Wlo = prm + off[8];
      const double* blo = prm + off[9];
      const int r = threadIdx.x & (kRows - 1), c = threadIdx.x >> 4;
      double acc = 0.0;
      for (int i = 0; i < g; ++i) acc += Wlo[c * g + i] * h1[r * ldg + i];
      a0[r * ldK + 2 * S + d + c] = acc + blo[c];
    }
    __syncthreads();
    // ---- representation MLP (w_nl.py:55-58); a1 / a2 / u take over the encoder's LDS
    dense_tanh_lds(a0, ldK, prm + off[10], prm + off[11], K0, h, a1, ldh);
    __syncthreads();
    dense_tanh_lds(a1, ldh, prm + off[12], prm + off[13], h, h, a2, ldh);
    __syncthreads();
    // ---- last layer, sphere map and line integral, L.dc state dims at a time: u = [tanh behind theta | behind phi], each
    // [dims][S].  x = e^{gamma t} / T * sum_k w_k R_k c_k; the linear algorithms: x = (1/t) sum_k R_k Re(W_k e^{i theta_k})
    for (int c0 = 0; c0 < d; c0 += L.dc) {
      const int dcc = d - c0 < L.dc ? d - c0 : L.dc;
      const int nq = dcc * S;
      const double* W3 = prm + off[14];
      const double* b3 = prm + off[15];
      dense_tanh_lds(a2, ldh, W3 + (int64_t)c0 * S * h, b3 + c0 * S, h, nq, u, ldu);
      dense_tanh_lds(a2, ldh, W3 + (int64_t)(d + c0) * S * h, b3 + (d + c0) * S, h, nq, u + nq, ldu);
      __syncthreads();
      // every term of the sums, in place of its theta entry
      for (int p = threadIdx.x; p < kRows * nq; p += kThreads) {
        const int r = p & (kRows - 1), e = p >> 4;
        const int k = e % S;
        double* yt = u + r * ldu + e;
        const double yp = yt[nq];
        if constexpr (kLinear) {
          double cv, cp;
          linear_phase(sphere_theta(*yt), a.lin_tab[2 * S + k], a.lin_tab[3 * S + k], &cv, &cp);
          *yt = sphere_radius(sphere_phi(yp)) * cv;
        } else {
          double cv, cp;
          quarter(sphere_theta(*yt), k, &cv, &cp);
          const double R = tan(sphere_phi(yp) / 2.0 + kPi / 4.0);
          *yt = (k == 0 ? 0.5 : 1.0) * R * cv;
        }
      }
      __syncthreads();
      for (int p = threadIdx.x; p < kRows * dcc; p += kThreads) {
        const int r = p & (kRows - 1), cc = p >> 4;
        const double* term = u + r * ldu + cc * S;
        double acc = 0.0;
        for (int k = 0; k < S; ++k) acc += term[k];
        const double t = tn[r];
        const double pred = kLinear ? acc / t : fourier_pred_factor(a.alpha, a.log_tol, t) * acc;
        const int c = c0 + cc;
        const double diff = pred - tgt[r * d + c];
        sq[r * d + c] = row0 + r < b.N ? diff * diff : 0.0;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int i = 0; i < kRows * d; ++i) s += sq[i];
      tile_loss[tile] = s;
    }
    // the next tile's first barrier orders this read of sq before its rewrite
  }
}

template <int H>
__global__ __launch_bounds__(kThreads) void rnn_eval_kernel(const RnnEvalArgs a) {
  static_assert(H % 16 == 0, "whole 16-feature output tiles and k quads");
  constexpr int H3 = 3 * H, LH = H + 2, LG = H3 + 2, LF = kMaxD + 1;
  __shared__ double hS[kRows * LH];               // the current hidden state
  __shared__ double gS[kRows * LG];               // h W_hh^T
  __shared__ double xS[kMaxB * kRows * kMaxNin];  // normalised window, forward order: [s][r][nin]
  __shared__ double fS[kRows * LF];               // [obs_n | ts_n]
  __shared__ double tS[kRows * kMaxD];            // target
  __shared__ double sqS[kRows * kMaxD];           // squared errors
  static_assert(kRows * LH + kRows * LG + kMaxB * kRows * kMaxNin + kRows * LF + 2 * kRows * kMaxD == rnn_eval_lds_doubles(H),
                "rnn_eval_lds_doubles is what the host sizes the grid with");
  const int d = a.d, nin = a.nin, B = a.B, ti = a.time_input ? 1 : 0;
  const int F = H + d + ti;
  const int64_t mi = blockIdx.y;  // member of the group (nlc_train.h GroupStrides; a single model is M = 1)
  const double* prm = a.batch.params + mi * a.gs.params;
  const double* Wih = prm + a.off[0];
  const double* Whh = prm + a.off[1];
  const double* bih = prm + a.off[2];
  const double* bhh = prm + a.off[3];
  const double* Wo = prm + a.off[4];
  const double* bo = prm + a.off[5];
  double* tile_loss = a.tile_loss + mi * a.gs.ws;
  const int64_t* idx = a.batch.idx ? a.batch.idx + mi * a.gs.idx : nullptr;
  const int64_t drow = mi * a.gs.rows;  // the member's rows of a stacked dataset (gs.rows = 0: the shared one)
  const double* obs = a.batch.obs + drow * d;
  const double* window = a.batch.window + drow * B * nin;
  const double* tsp = ti ? a.batch.ts + drow : nullptr;  // a model without time input has no ts (batch.ts may be NULL)
  const double* target = a.batch.target + drow * d;

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRows;
    // ---- inputs: gathered rows, normalised (train_utils.py:618-626 / :577-582, the branch resolved in the descriptor); rows
    // past N are zeros and add nothing to the loss
    for (int p = threadIdx.x; p < kRows * (B * nin + d + 1); p += kThreads) {
      const int r = p & (kRows - 1), e = p >> 4;
      const bool valid = row0 + r < a.batch.N;
      const int64_t src = valid ? (idx ? idx[row0 + r] : row0 + r) : 0;
      if (e < B * nin) {
        const int s = e / nin, c = e - s * nin;
        xS[(s * kRows + r) * nin + c] = valid ? (window[(src * B + s) * nin + c] - a.norm.am[c]) / a.norm.as[c] : 0.0;
      } else if (e < B * nin + d) {
        const int c = e - B * nin;
        fS[r * LF + c] = valid ? (obs[src * d + c] - a.norm.sm[c]) / a.norm.ss[c] : 0.0;
        tS[r * kMaxD + c] = valid ? target[src * d + c] : 0.0;
      } else {
        fS[r * LF + d] = (valid && ti) ? tsp[src] / a.time_div : 0.0;
      }
    }
    for (int p = threadIdx.x; p < kRows * LH; p += kThreads) hS[p] = 0.0;
    __syncthreads();
    // ---- GRU forward (h_0 = 0: the first step has no hidden product)
    for (int s = 0; s < B; ++s) {
      if (s > 0) {
        dense_mfma(hS, LH, Whh, H, H3, 0, [&](int r, int n, double v) { gS[r * LG + n] = v; });
        __syncthreads();
      }
      for (int p = threadIdx.x; p < kRows * H; p += kThreads) {
        const int r = p / H, j = p - r * H;
        const Gate gt = gru_gate0(xS + (s * kRows + r) * nin, nin, Wih, bih, bhh, s > 0 ? gS + r * LG : nullptr, H, j);
        hS[r * LH + j] = (1.0 - gt.z) * gt.n + gt.z * hS[r * LH + j];
      }
      __syncthreads();
    }
    // ---- linear_out over [h_B | obs_n | ts_n], squared error
    for (int p = threadIdx.x; p < kRows * d; p += kThreads) {
      const int r = p & (kRows - 1), c = p >> 4;
      const double* w = Wo + c * F;
      const double* hB = hS + r * LH;
      double acc = 0.0;
#pragma unroll 8
      for (int i = 0; i < H; ++i) acc += w[i] * hB[i];
      for (int i = 0; i < d + ti; ++i) acc += w[H + i] * fS[r * LF + i];
      const double diff = (acc + bo[c]) - tS[r * kMaxD + c];
      sqS[r * d + c] = row0 + r < a.batch.N ? diff * diff : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int i = 0; i < kRows * d; ++i) s += sqS[i];
      tile_loss[tile] = s;
    }
    // the next tile's first barrier orders this read of sqS before its rewrite
  }
}

// loss[m] = sum of the member's tile losses / (N d): thread i sums tiles i, i + 256, ... in order, then the 256 sums meet in
// a fixed tree (block_sum, nlc_train_dev.h) -- an order the tile count alone decides
__global__ __launch_bounds__(kThreads) void eval_reduce_kernel(const EvalReduceArgs a) {
  const double* tile_loss = a.tile_loss + (int64_t)blockIdx.y * a.ws;
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < a.ntiles; k += kThreads) s += tile_loss[k];
  s = block_sum(s);
  if (threadIdx.x == 0) a.loss[blockIdx.y] = s / ((double)a.N * (double)a.d);
}

// more than 64 KB of dynamic LDS per workgroup needs hipFuncAttributeMaxDynamicSharedMemorySize, per function and per device
template <class F>
static hipError_t lds_attr_once(F* fn, std::atomic<unsigned long long>& done) {
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev)) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  const unsigned long long bit = 1ull << dev;
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  if (hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes)) return e;
  done.fetch_or(bit, std::memory_order_release);
  return hipSuccess;
}

hipError_t launch_train_eval(const EvalArgs& a, int G, int M, hipStream_t s) {
  static std::atomic<unsigned long long> done[2];
  const bool lin = a.lin_tab != nullptr;
  const auto kernel = lin ? train_eval_kernel<true> : train_eval_kernel<false>;
  const size_t lds = (size_t)a.L.total * sizeof(double);
  if (lds > (size_t)kLdsBytes) return hipErrorInvalidValue;
  if (hipError_t e = lds_attr_once(kernel, done[lin])) return e;
  hipLaunchKernelGGL(kernel, dim3(G, M), dim3(kThreads), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_rnn_eval(const RnnEvalArgs& a, int H, int G, int M, hipStream_t s) {
  const bool found = for_rnn_width(H, [&](auto w) {
    hipLaunchKernelGGL((rnn_eval_kernel<decltype(w)::value>), dim3(G, M), dim3(kThreads), 0, s, a);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_eval_reduce(const EvalReduceArgs& a, int M, hipStream_t s) {
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(1, M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace train
}  // namespace nlc
