// Fused training step and held-out loss of the NODE baseline (train_utils.py:637-724 trained by the loop :388-408): forward
// Euler through Linear -> tanh -> Linear -> tanh -> Linear on cat(x, u), squared error, and the backward through the sub-steps
// in reverse, one 16-row tile per workgroup, float64.  train_reduce_kernel / train_adam_kernel (kernels_train.hip) finish the
// iteration from the workgroups' partials and eval_reduce_kernel (kernels_train_eval.hip) the held-out loss, unchanged.
//
//   node_train_fwd_bwd_kernel   rows gathered through the int64 index array, the state normalised with nlc_node_desc's
//                               constants, the augmented columns zero, u the window's newest action, raw.  Every row carries
//                               its own sub-step count and widths (nlc_train_node.h node_euler_count / node_euler_width from
//                               ts on the device): the batch's first row's time by default (train_utils.py:719), the row's own
//                               with row_times.  The loops run to the tile's largest count with per-row predication; no barrier
//                               depends on a row's count.  Forward: the states x_k are taped (8 doubles per row and sub-step).
//                               Backward: a sub-step's two hidden layers are rebuilt from x_k; its deltas and activations go to
//                               the slab, and every kNodeChunk sub-steps one pass adds their outer products to the workgroup's
//                               partial in blob order (wgrad_mfma: the samples are the MFMA's k).
//   node_train_fwd_bwd_rk_kernel<METHOD>, node_eval_rk_kernel<METHOD>
//                               the same template for the midpoint and rk4 tableaus of nlc_node_rk.h (ctx option "node_method"):
//                               the stage inputs Y_i are taped where Euler tapes x_k, and the backward walks a sub-step's stages
//                               last to first (kbar_i = h b_i ybar', Ybar_i = J_f(Y_i)^T kbar_i, kbar_j += h a_ij Ybar_i).
//   node_eval_kernel            the forward half: nothing taped, no slab; the tile's sum of squared errors to tile_loss[tile].
//
// Few live rows (the reference trains NODE at batch 1): the 2.weight products put the lanes along the contiguous input index of
// a weight row, which streams coalesced from L2 with 8-byte accesses (rows of the unpadded blob are only 8-byte aligned), and
// every loaded weight serves all live rows of the tile; only live rows are computed and sampled.
// Memory safety does not depend on the data: a count is at most kNodeTrainMaxSub, the slab is sized for that, and a row whose
// time is not positive or past the cap gets a NaN squared error.  No atomics (bit-reproducible; a member's bits do not depend
// on M).  Resources (hipcc -Rpass-analysis=kernel-resource-usage): docs/training.md.
#include "nlc_train_dev.h"
#include "nlc_train_node.h"

namespace nlc {
namespace train {

namespace {

constexpr int LH = kNodeLdH;   // LDS row stride of an activation tile
constexpr int LX = kNodeMaxDy; // row stride of the small per-row arrays
constexpr int kFwdRows = 8;    // rows one stream of 2.weight serves in the forward product
constexpr int kBwdRows = kNodeBwdRows;
constexpr int kSlots = (kNodeMaxH + 63) / 64;  // columns a lane owns in the backward product
static_assert(kRows % kFwdRows == 0 && kRows % kBwdRows == 0, "row blocks tile the 16 rows");

struct NodeW {
  const double *W0, *b0, *W2, *b2, *W4, *b4;
  int H, dy, nu, in;
};

// a1S[r][j] = tanh(W0[j] . cat(x_r, u_r) + b0[j]), live rows
__device__ __forceinline__ void layer0(const NodeW& w, const double* xS, const double* uS, double* a1S, int nlive) {
  for (int p = threadIdx.x; p < nlive * w.H; p += kThreads) {
    const int r = p / w.H, j = p - r * w.H;
    const double* wr = w.W0 + (int64_t)j * w.in;
    double acc = 0.0;
    for (int c = 0; c < w.dy; ++c) acc += wr[c] * xS[r * LX + c];
    for (int c = 0; c < w.nu; ++c) acc += wr[w.dy + c] * uS[r * NLC_MAX_NU + c];
    a1S[r * LH + j] = m::tanh_d(acc + w.b0[j]);
  }
}

// a2S[r][j] = W2[j] . a1S[r] + b2[j] (pre-activation), live rows.  A wave takes the weight rows j = wave, wave + 4, ...; its
// lanes walk the row (l = lane, lane + 64, ...), each loaded weight multiplies up to eight rows, and the eight lane sums meet
// in ten exchanges: three halving steps leave value 4 b5 + 2 b4 + b3 on a lane, three more sum its eight lanes
__device__ __forceinline__ void layer2_pre(const NodeW& w, const double* a1S, double* a2S, int nlive) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = w.H;
  const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
  const int mine = (b5 ? 4 : 0) + (b4 ? 2 : 0) + (b3 ? 1 : 0);
  for (int rb = 0; rb < nlive; rb += kFwdRows) {
    const int nr = nlive - rb < kFwdRows ? nlive - rb : kFwdRows;
    for (int j = wave; j < H; j += kWaves) {
      const double* wrow = w.W2 + (int64_t)j * H;
      double acc[kFwdRows];
#pragma unroll
      for (int rr = 0; rr < kFwdRows; ++rr) acc[rr] = 0.0;
      for (int l = lane; l < H; l += 64) {
        const double wv = wrow[l];
#pragma unroll
        for (int rr = 0; rr < kFwdRows; ++rr)
          if (rr < nr) acc[rr] = fma(wv, a1S[(rb + rr) * LH + l], acc[rr]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double send = b5 ? acc[q] : acc[q + 4], keep = b5 ? acc[q + 4] : acc[q];
        acc[q] = keep + __shfl_xor(send, 32);
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const double send = b4 ? acc[q] : acc[q + 2], keep = b4 ? acc[q + 2] : acc[q];
        acc[q] = keep + __shfl_xor(send, 16);
      }
      {
        const double send = b3 ? acc[0] : acc[1], keep = b3 ? acc[1] : acc[0];
        acc[0] = keep + __shfl_xor(send, 8);
      }
      acc[0] += __shfl_xor(acc[0], 4);
      acc[0] += __shfl_xor(acc[0], 2);
      acc[0] += __shfl_xor(acc[0], 1);
      if ((lane & 7) == 0 && mine < nr) a2S[(rb + mine) * LH + j] = acc[0] + w.b2[j];
    }
  }
}

// sum over j < n of wv[j * stride] * act[j] for the thread's row, by its 16 lanes (q = threadIdx.x & 15): every lane gets it
__device__ __forceinline__ double dot16(const double* __restrict__ wv, int stride, const double* act, int n) {
  const int q = threadIdx.x & 15;
  double acc = 0.0;
  for (int j = q; j < n; j += 16) acc = fma(wv[(int64_t)j * stride], act[j], acc);
  acc += __shfl_xor(acc, 8);
  acc += __shfl_xor(acc, 4);
  acc += __shfl_xor(acc, 2);
  acc += __shfl_xor(acc, 1);
  return acc;
}

// the hidden activations of cat(xS, uS): a1S, a2S (live rows); ends on a barrier
__device__ __forceinline__ void hidden_fwd(const NodeW& w, const double* xS, const double* uS, double* a1S, double* a2S,
                                           int nlive) {
  layer0(w, xS, uS, a1S, nlive);
  __syncthreads();
  layer2_pre(w, a1S, a2S, nlive);
  __syncthreads();
  for (int p = threadIdx.x; p < nlive * w.H; p += kThreads) {
    const int r = p / w.H, j = p - r * w.H;
    a2S[r * LH + j] = m::tanh_d(a2S[r * LH + j]);
  }
  __syncthreads();
}

// METHOD: the tableau of nlc_node_rk.h, its stage count S a compile-time constant; the Euler instances (S = 1) are the code
// they have always been.  S > 1: rkS (LDS of the kernel's own) holds y, the slopes k_i and, in training, their adjoints
// kbar_i, kRows * LX doubles each; the tape holds the stage inputs Y_i (entry k S + i) and a weight-gradient chunk kNodeChunk / S
// sub-steps.
template <bool kTrain, int METHOD>
__device__ __forceinline__ void node_tiles(const NodeTrainArgs& a, double* rkS) {
  constexpr const NodeRk& T = NodeRkOf<METHOD>::T;
  constexpr int S = T.s;
  constexpr int RK = kRows * LX;              // one small per-row array
  constexpr int kMaxSub = kNodeTrainMaxSub / S;  // node_train_max_sub(METHOD)
  static_assert(kSlots * 64 >= kNodeMaxH, "a lane's column slots cover the widest layer");
  __shared__ double a1S[kRows * LH];  // tanh of layer 0; backward: its delta, in place
  __shared__ double a2S[kRows * LH];  // tanh of layer 2; backward: its delta, in place
  __shared__ double pS[kTrain ? kWaves * kBwdRows * LH : 1];  // backward: the four waves' addends of W2^T d2
  __shared__ double xS[kRows * LX];   // x_k
  __shared__ double uS[kRows * NLC_MAX_NU];
  __shared__ double tgS[kRows * LX];  // target
  __shared__ double xbS[kRows * LX];  // dL/dx_k
  __shared__ double d3S[kRows * LX];  // dL/df of the sub-step
  __shared__ double sqS[kRows * LX];  // squared errors
  __shared__ double teS[kRows];       // the rows' end times
  __shared__ int nsS[kRows];          // their sub-step counts
  __shared__ int badS[kRows];         // 1: no positive time or past the cap -> NaN
  const int d = a.d, dy = a.d + a.aug, nu = a.nu, H = a.H, in = dy + nu, B = a.B;
  const int64_t mi = blockIdx.y;  // member of the group (nlc_train.h GroupStrides; a single model is M = 1)
  const double* prm = a.batch.params + mi * a.gs.params;
  const NodeW w{prm + a.off[0], prm + a.off[1], prm + a.off[2], prm + a.off[3], prm + a.off[4], prm + a.off[5], H, dy, nu, in};
  double* tile_loss = a.tile_loss + mi * a.gs.ws;
  const int64_t* idx = a.batch.idx ? a.batch.idx + mi * a.gs.idx : nullptr;  // NULL (evaluation): rows 0 .. N - 1
  const int64_t drow = mi * a.gs.rows;
  const double* obs = a.batch.obs + drow * d;
  const double* window = a.batch.window + drow * B * nu;
  const double* tsp = a.batch.ts + drow;
  const double* target = a.batch.target + drow * d;
  const double loss_norm = 2.0 / ((double)a.batch.N * (double)d);  // MSELoss backward: 2 / numel * (input - target)
  const double nan = __builtin_nan("");
  // the slab and the partial exist in training only
  const NodeActLayout& L = a.L;
  double* ws = kTrain ? a.act + mi * a.gs.ws + (int64_t)blockIdx.x * a.A : nullptr;
  double* part = kTrain ? a.partial + mi * a.gs.ws + (int64_t)blockIdx.x * a.P : nullptr;
  bool summed = false;  // the partial holds this workgroup's earlier chunks

  for (int p = threadIdx.x; p < kRows * LH; p += kThreads) a1S[p] = a2S[p] = 0.0;  // rows past the live ones stay 0

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRows;
    const int nlive = a.batch.N - row0 < kRows ? (int)(a.batch.N - row0) : kRows;
    // ---- inputs (train_utils.py:698-715); rows past N are zeros with no sub-step, and their loss gradient is 0
    for (int p = threadIdx.x; p < kRows * (dy + nu + d + 1); p += kThreads) {
      const int r = p & (kRows - 1), e = p >> 4;
      const bool valid = r < nlive;
      const int64_t src = valid ? (idx ? idx[row0 + r] : row0 + r) : 0;
      if (e < dy) {
        xS[r * LX + e] = (valid && e < d) ? (obs[src * d + e] - a.norm.sm[e]) / a.norm.ss[e] : 0.0;
      } else if (e < dy + nu) {
        const int c = e - dy;
        uS[r * NLC_MAX_NU + c] = valid ? window[(src * B + (B - 1)) * nu + c] : 0.0;
      } else if (e < dy + nu + d) {
        const int c = e - dy - nu;
        tgS[r * LX + c] = valid ? target[src * d + c] : 0.0;
      } else {
        // the reference integrates every row to the time of the batch's first row (train_utils.py:719)
        const int64_t tsrc = a.row_times ? src : (idx ? idx[0] : 0);
        int bad = 0;
        const double te = valid ? tsp[tsrc] / a.time_div : 0.0;
        const int ns = !valid ? 0 : S == 1 ? node_euler_count(te, a.step_size, &bad) : node_rk_count(te, a.step_size, kMaxSub, &bad);
        teS[r] = te;
        nsS[r] = ns;
        badS[r] = valid ? bad : 0;
      }
    }
    __syncthreads();
    int kmax = 0;
    for (int r = 0; r < kRows; ++r) kmax = nsS[r] > kmax ? nsS[r] : kmax;
    kmax = kmax < kMaxSub ? kmax : kMaxSub;  // node_euler_count / node_rk_count already hold this; the slab relies on it
    const int r16 = threadIdx.x >> 4, q16 = threadIdx.x & 15;

    // ---- forward Euler
    if constexpr (S == 1) {
    for (int k = 0; k < kmax; ++k) {
      if (kTrain && threadIdx.x < kRows * LX) ws[L.Xt + (int64_t)k * kRows * LX + threadIdx.x] = xS[threadIdx.x];
      hidden_fwd(w, xS, uS, a1S, a2S, nlive);
      {
        const int ns = nsS[r16];
        const double hk = k < ns ? node_euler_width(teS[r16], a.step_size, ns, k) : 0.0;
        for (int i = 0; i < dy; ++i) {
          const double f = dot16(w.W4 + (int64_t)i * H, 1, a2S + r16 * LH, H) + w.b4[i];
          if (q16 == 0 && k < ns) xS[r16 * LX + i] += hk * f;
        }
      }
      __syncthreads();
    }
    } else {
      // ---- forward, S stages a sub-step: xS is the stage input Y_i, y and the slopes stay in rkS.  Thread t < RK owns
      // component t = r * LX + c of y, Y_i and every k_i; the slopes of a row are written by its lane q16 = 0
      double* yS = rkS;
      double* kS = rkS + RK;
      const int t = threadIdx.x;
      if (t < RK) yS[t] = xS[t];
      for (int k = 0; k < kmax; ++k) {
        const int nsr = t < RK ? nsS[t >> 3] : 0;
        const double hk = (t < RK && k < nsr) ? node_euler_width(teS[t >> 3], a.step_size, nsr, k) : 0.0;
        for (int st = 0; st < S; ++st) {
          if (t < RK) {
            const double Y = node_rk_stage_input(T, st, yS[t], hk, kS + t, RK);
            xS[t] = Y;
            if (kTrain) ws[L.Xt + ((int64_t)k * S + st) * RK + t] = Y;
          }
          __syncthreads();
          hidden_fwd(w, xS, uS, a1S, a2S, nlive);
          for (int i = 0; i < dy; ++i) {
            const double f = dot16(w.W4 + (int64_t)i * H, 1, a2S + r16 * LH, H) + w.b4[i];
            if (q16 == 0) kS[st * RK + r16 * LX + i] = f;
          }
          __syncthreads();
        }
        if (t < RK && k < nsr && (t & 7) < dy) yS[t] = node_rk_combine(T, yS[t], hk, kS + t, RK);
      }
      if (t < RK) xS[t] = yS[t];
      __syncthreads();
    }
    // ---- squared error of the first d columns (the augmented ones are dropped: their adjoint is 0) and dL/dx at the end
    for (int p = threadIdx.x; p < kRows * LX; p += kThreads) {
      const int r = p & (kRows - 1), c = p >> 4;
      const bool valid = r < nlive && c < d;
      const double diff = badS[r] ? nan : xS[r * LX + c] - tgS[r * LX + c];
      if (c < d) sqS[r * d + c] = valid ? diff * diff : 0.0;
      xbS[r * LX + c] = valid ? loss_norm * diff : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int i = 0; i < kRows * d; ++i) s += sqS[i];
      if (kTrain)
        tile_loss[blockIdx.x] = (tile == (int64_t)blockIdx.x ? 0.0 : tile_loss[blockIdx.x]) + s;
      else
        tile_loss[tile] = s;
    }
    if constexpr (kTrain) {
      // ---- backward through the sub-steps, kNodeChunk evaluations of the ODE function at a time (CS sub-steps of S stages,
      // last stage first): sample (kk, r) of a chunk is s = kk * nlive + r
      constexpr int CS = kNodeChunk / S;
      double* kbS = rkS + (1 + S) * RK;  // S > 1: kbar_i, component t = r * LX + c
      const int Q = (H + kWaves - 1) / kWaves;
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      for (int kend = kmax; kend > 0; kend -= CS) {
        const int kbeg = kend > CS ? kend - CS : 0;
        for (int k = kend - 1; k >= kbeg; --k) {
          if constexpr (S > 1) {
            // kbar_i = h b_i ybar' (zero where the row has no sub-step k); the stage's first barrier orders it
            if (threadIdx.x < RK) {
              const int r = threadIdx.x >> 3, i = threadIdx.x & 7;
              const int ns = nsS[r];
              const bool on = r < nlive && i < dy && k < ns;
              const double hk = on ? node_euler_width(teS[r], a.step_size, ns, k) : 0.0;
              for (int st = 0; st < S; ++st) kbS[st * RK + threadIdx.x] = on ? node_rk_kbar_init(T, st, hk, xbS[threadIdx.x]) : 0.0;
            }
          }
          for (int st = S - 1; st >= 0; --st) {
          const int64_t s0 = ((int64_t)(kend - 1 - k) * S + (S - 1 - st)) * nlive;
          if (threadIdx.x < kRows * LX) xS[threadIdx.x] = ws[L.Xt + ((int64_t)k * S + st) * kRows * LX + threadIdx.x];
          __syncthreads();
          hidden_fwd(w, xS, uS, a1S, a2S, nlive);
          // the sample's activations, its input and dL/df; a row past its own count adds zeros
          for (int p = threadIdx.x; p < nlive * H; p += kThreads) {
            const int r = p / H, j = p - r * H;
            ws[L.A1 + (s0 + r) * H + j] = a1S[r * LH + j];
            ws[L.A2 + (s0 + r) * H + j] = a2S[r * LH + j];
          }
          for (int p = threadIdx.x; p < nlive * in; p += kThreads) {
            const int r = p / in, c = p - r * in;
            ws[L.Z + (s0 + r) * in + c] = c < dy ? xS[r * LX + c] : uS[r * NLC_MAX_NU + c - dy];
          }
          if (threadIdx.x < kRows * LX) {
            const int r = threadIdx.x >> 3, i = threadIdx.x & 7;
            const int ns = nsS[r];
            const bool on = r < nlive && i < dy && k < ns;
            double v;
            if constexpr (S == 1)
              v = on ? node_out_delta(node_euler_width(teS[r], a.step_size, ns, k), xbS[r * LX + i]) : 0.0;
            else
              v = on ? kbS[st * RK + threadIdx.x] : 0.0;
            d3S[r * LX + i] = v;
            if (r < nlive) ws[L.D3 + (s0 + r) * LX + i] = v;
          }
          __syncthreads();
          // d2 = (W4^T d3) (1 - a2^2), in place
          for (int p = threadIdx.x; p < nlive * H; p += kThreads) {
            const int r = p / H, j = p - r * H;
            double g = 0.0;
            for (int i = 0; i < dy; ++i) g = fma(w.W4[(int64_t)i * H + j], d3S[r * LX + i], g);
            const double v = node_tanh_bwd(g, a2S[r * LH + j]);
            a2S[r * LH + j] = v;
            ws[L.D2 + (s0 + r) * H + j] = v;
          }
          __syncthreads();
          // d1 = (W2^T d2) (1 - a1^2), in place: a wave streams a quarter of the weight rows, a lane owns the columns
          // lane + 64 i, the four waves' addends meet in LDS in wave order
          for (int rb = 0; rb < nlive; rb += kBwdRows) {
            double acc[kSlots][kBwdRows];
#pragma unroll
            for (int i = 0; i < kSlots; ++i)
#pragma unroll
              for (int rr = 0; rr < kBwdRows; ++rr) acc[i][rr] = 0.0;
            const int j1 = (wave + 1) * Q < H ? (wave + 1) * Q : H;
            for (int j = wave * Q; j < j1; ++j) {
              const double* wrow = w.W2 + (int64_t)j * H;
              double dv[kBwdRows];
#pragma unroll
              for (int rr = 0; rr < kBwdRows; ++rr) dv[rr] = a2S[(rb + rr) * LH + j];
#pragma unroll
              for (int i = 0; i < kSlots; ++i) {
                const int l = lane + 64 * i;
                if (l < H) {
                  const double wv = wrow[l];
#pragma unroll
                  for (int rr = 0; rr < kBwdRows; ++rr) acc[i][rr] = fma(wv, dv[rr], acc[i][rr]);
                }
              }
            }
#pragma unroll
            for (int i = 0; i < kSlots; ++i) {
              const int l = lane + 64 * i;
              if (l < H) {
#pragma unroll
                for (int rr = 0; rr < kBwdRows; ++rr) pS[(wave * kBwdRows + rr) * LH + l] = acc[i][rr];
              }
            }
            __syncthreads();
            for (int p = threadIdx.x; p < kBwdRows * H; p += kThreads) {
              const int rr = p / H, l = p - rr * H, r = rb + rr;
              if (r < nlive) {
                double g = pS[rr * LH + l];
                for (int wv = 1; wv < kWaves; ++wv) g += pS[(wv * kBwdRows + rr) * LH + l];
                const double v = node_tanh_bwd(g, a1S[r * LH + l]);
                a1S[r * LH + l] = v;
                ws[L.D1 + (s0 + r) * H + l] = v;
              }
            }
            __syncthreads();
          }
          // dL/dx_k = dL/dx_{k+1} + W0[:, :dy]^T d1 (S > 1: ybar += Ybar_i, and kbar_j += h a_ij Ybar_i for j < i)
          if constexpr (S == 1) {
          for (int i = 0; i < dy; ++i) {
            const double g = dot16(w.W0 + i, in, a1S + r16 * LH, H);
            if (q16 == 0 && r16 < nlive) xbS[r16 * LX + i] += g;
          }
          } else {
            const int nsr = nsS[r16];
            const double hk = k < nsr ? node_euler_width(teS[r16], a.step_size, nsr, k) : 0.0;
            for (int i = 0; i < dy; ++i) {
              const double g = dot16(w.W0 + i, in, a1S + r16 * LH, H);
              if (q16 == 0 && r16 < nlive) {
                xbS[r16 * LX + i] += g;
                for (int j = 0; j < st; ++j) kbS[j * RK + r16 * LX + i] += node_rk_kbar_add(T, st, j, hk, g);
              }
            }
          }
          __syncthreads();
          }
        }
        // ---- the chunk's weight gradients: one pass over the partial, sums over its (evaluation, row) samples
        const int ns = (kend - kbeg) * S * nlive;
        const bool first = !summed;
        wgrad_mfma(part + a.off[0], H, in, ns, ws + L.D1, H, ws + L.Z, in, first);
        bgrad(part + a.off[1], H, ns, ws + L.D1, H, first);
        wgrad_mfma(part + a.off[2], H, H, ns, ws + L.D2, H, ws + L.A1, H, first);
        bgrad(part + a.off[3], H, ns, ws + L.D2, H, first);
        wgrad_mfma(part + a.off[4], dy, H, ns, ws + L.D3, LX, ws + L.A2, H, first);
        bgrad(part + a.off[5], dy, ns, ws + L.D3, LX, first);
        summed = true;
        __syncthreads();
      }
    }
    __syncthreads();
  }
  if constexpr (kTrain) {
    // no row of this workgroup had a sub-step: its partial is all zeros
    if (!summed)
      for (int64_t p = threadIdx.x; p < a.P; p += kThreads) part[p] = 0.0;
  }
}

}  // namespace

__global__ __launch_bounds__(kThreads) void node_train_fwd_bwd_kernel(const NodeTrainArgs a) { node_tiles<true, 0>(a, nullptr); }
__global__ __launch_bounds__(kThreads) void node_eval_kernel(const NodeTrainArgs a) { node_tiles<false, 0>(a, nullptr); }
// the multi-stage methods' instances
template <int METHOD>
__global__ __launch_bounds__(kThreads) void node_train_fwd_bwd_rk_kernel(const NodeTrainArgs a) {
  __shared__ double rkS[node_rk_lds_doubles(true, node_rk_stages(METHOD))];
  node_tiles<true, METHOD>(a, rkS);
}
template <int METHOD>
__global__ __launch_bounds__(kThreads) void node_eval_rk_kernel(const NodeTrainArgs a) {
  __shared__ double rkS[node_rk_lds_doubles(false, node_rk_stages(METHOD))];
  node_tiles<false, METHOD>(a, rkS);
}

hipError_t launch_node_train_fwd_bwd(const NodeTrainArgs& a, int method, int nblk, int M, hipStream_t s) {
  switch (method) {
    case 0: hipLaunchKernelGGL(node_train_fwd_bwd_kernel, dim3(nblk, M), dim3(kThreads), 0, s, a); break;
    case 1: hipLaunchKernelGGL(node_train_fwd_bwd_rk_kernel<1>, dim3(nblk, M), dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL(node_train_fwd_bwd_rk_kernel<2>, dim3(nblk, M), dim3(kThreads), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_node_eval(const NodeTrainArgs& a, int method, int G, int M, hipStream_t s) {
  switch (method) {
    case 0: hipLaunchKernelGGL(node_eval_kernel, dim3(G, M), dim3(kThreads), 0, s, a); break;
    case 1: hipLaunchKernelGGL(node_eval_rk_kernel<1>, dim3(G, M), dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL(node_eval_rk_kernel<2>, dim3(G, M), dim3(kThreads), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace train
}  // namespace nlc
