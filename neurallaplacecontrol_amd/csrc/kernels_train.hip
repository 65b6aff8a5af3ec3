// Fused training step of NeuralLaplaceModel with the Fourier ILT or one of the linear algorithms (fixed Talbot, Stehfest:
// the <true> instance of train_fwd_bwd_kernel, which differs in the query points and the line integral only): one iteration
// of the reference's training loop (train_utils.py:388-408: model(bs0, ba0, bts), MSELoss, backward, clip_grad_norm_,
// Adam.step), float64 throughout (model.double(), train_utils.py:267).  Three launches, no host synchronisation:
//
// blockIdx.y is the member of a group of same-shaped models (nlc_train.h GroupStrides; a single model is M = 1): every kernel
// moves its base pointers by the member's strides and then does what it does for one model, with no atomics and no read of
// another member's memory, so a member's bits do not depend on M or on its neighbours.
//
//   train_fwd_bwd_kernel  one workgroup per 16-row tile (a workgroup walks tiles b, b + G, ... when N needs more than
//                         kMaxBlocks tiles): rows gathered through the int64 index array, normalisation as
//                         nlc_model_forward, 2-layer reverse GRU with its gates taped, linear_out, per-row query points,
//                         representation MLP, sphere map, Fourier line integral at the row's own t, squared error; then
//                         the backward in reverse order: ILT, sphere map, MLP, linear_out, GRU backprop through time over
//                         both layers.  Weight gradients are sums over the tile's samples (rows; rows x window steps for the
//                         GRU) on the FP64 matrix cores (v_mfma_f64_16x16x4_f64), accumulated onto the workgroup's partial
//                         in state_dict blob order.
//   train_reduce_kernel   partials summed in workgroup order (no atomics: bit-reproducible), per-chunk sums of squares,
//                         the loss.
//   train_adam_kernel     per-tensor norms, their norm, clip_grad_norm_'s coefficient, torch.optim.Adam's update: clip_adam
//                         (nlc_train_dev.h) with the settings of its arguments.
// The reduce and Adam grids are the chunks of nlc_train.h's ChunkTable, walked by chunk_range.
//
// Elementary functions: gates and hidden activations use nlc_math.h's sigmoid_d / tanh_d (<= 4 ulp against libm on the
// whole line, tests/test_math_host.py); the sphere map's tanh is tanh_d; tan / sin / cos / exp / atan2 / asin of the query
// points and the line integral are the device library's.  tests/test_gpu_train.py holds the loss to 1e-12 relative and every
// gradient to 1e-9 of its tensor's max |grad| against float64 autograd on the CPU.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage; table in docs/training.md): train_fwd_bwd_kernel 256 VGPRs + 250
// AGPRs and 68 B/lane of scratch, not yet traced to its source (the linear instance: 230 AGPRs and none); one wave per
// SIMD.  The kernel is latency-bound at 2.3 ms per batch-16 iteration (docs/training.md): the next step is LDS-resident
// activations and MFMA forward products, not this scratch.
#include "nlc_train_nl_dev.h"

namespace nlc {
namespace train {

// kLinear: the fixed Talbot / Stehfest instance (a.lin_tab: nodes and weights).  Only the query points and the line integral
// differ; the Fourier instance never reads a.lin_tab and keeps its expressions and their order
template <bool kLinear>
__global__ __launch_bounds__(kThreads) void train_fwd_bwd_kernel(const TrainArgs a) {
  const int d = a.d, nin = a.nin, g = a.g, h = a.h, S = a.S, B = a.B;
  const int K0 = 2 * S + d + 2, O = 2 * d * S;
  const ActLayout& L = a.L;
  const int64_t mi = blockIdx.y;  // member of the group: its own blob, workspace region, index array and dataset rows
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
  double* tn = ws + L.tn;
  double* tgt = ws + L.tgt;
  double* sq = ws + L.sq;
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
  double* tile_loss = a.tile_loss + mi * a.gs.ws;
  const double loss_norm = 2.0 / ((double)a.batch.N * (double)d);  // MSELoss backward: 2 / numel * (input - target)

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const bool first = tile == (int)blockIdx.x;
    const int64_t row0 = (int64_t)tile * kRows;
    // ---- inputs: gathered rows, normalised as nlc_model_forward (w_nl.py:120-131); rows past N are zeros at t = 1 (finite
    // everywhere, and their loss gradient is 0)
    for (int p = threadIdx.x; p < kRows * (B * nin + d + 1); p += kThreads) {
      const int r = p & (kRows - 1), e = p >> 4;
      const bool valid = row0 + r < a.batch.N;
      // the member's rows: its slice of the index array, and of a stacked dataset (gs.rows = 0: the shared one).  The offset
      // goes onto the row index here, not onto four base pointers before the loop: those stayed live across the whole
      // kernel and took its scratch from 68 to 132 B/lane
      const int64_t src = (valid ? a.batch.idx[mi * a.gs.idx + row0 + r] : 0) + mi * a.gs.rows;
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
      dhA[p] = 0.0;
    }
    __syncthreads();
    // ---- query points s_k = gamma + i pi k / T (linear algorithms: node_k / t) of the row's t on the Riemann sphere (as
    // rep_inputs_kernel)
    for (int p = threadIdx.x; p < kRows * S; p += kThreads) {
      const int r = p & (kRows - 1), k = p >> 4;
      if constexpr (kLinear) {
        linear_query_point(a.lin_tab[k], a.lin_tab[S + k], tn[r], &a0[(int64_t)r * K0 + k], &a0[(int64_t)r * K0 + S + k]);
      } else {
        fourier_query_point(a.alpha, a.log_tol, tn[r], k, &a0[(int64_t)r * K0 + k], &a0[(int64_t)r * K0 + S + k]);
      }
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
    dense_tanh(prm + off[14], prm + off[15], a2, h, O, u);
    __syncthreads();
    // ---- sphere map + Fourier line integral at the row's own t, squared error, and their backward down to the last layer's
    // pre-activations: x = e^{gamma t} / T * sum_k w_k R_k c_k.  The linear algorithms: x = (1/t) sum_k R_k Re(W_k e^{i theta_k}),
    // no e^{gamma t} / T and no half weight on k = 0 (nlc_train.h linear_row_sum / linear_row_bwd)
    for (int p = threadIdx.x; p < kRows * d; p += kThreads) {
      const int r = p & (kRows - 1), c = p >> 4;
      if constexpr (kLinear) {
        const double t = tn[r];
        const double* wr = a.lin_tab + 2 * S;
        const double* wi = a.lin_tab + 3 * S;
        const double* yt = u + (int64_t)r * O + c * S;
        const double* yp = u + (int64_t)r * O + (d + c) * S;
        const double pred = linear_row_sum(yt, yp, wr, wi, S) / t;
        const bool valid = row0 + r < a.batch.N;
        const double diff = pred - tgt[r * d + c];
        sq[r * d + c] = valid ? diff * diff : 0.0;
        const double gs = valid ? (loss_norm * diff) / t : 0.0;
        linear_row_bwd(gs, yt, yp, wr, wi, S, d3 + (int64_t)r * O + c * S, d3 + (int64_t)r * O + (d + c) * S);
        continue;
      }
      const double srow = fourier_pred_factor(a.alpha, a.log_tol, tn[r]);
      const double* yt = u + (int64_t)r * O + c * S;
      const double* yp = u + (int64_t)r * O + (d + c) * S;
      double acc = 0.0;
      for (int k = 0; k < S; ++k) {
        double cv, cp;
        quarter(sphere_theta(yt[k]), k, &cv, &cp);
        const double R = tan(sphere_phi(yp[k]) / 2.0 + kPi / 4.0);
        acc += (k == 0 ? 0.5 : 1.0) * R * cv;
      }
      const double pred = srow * acc;
      const bool valid = row0 + r < a.batch.N;
      const double diff = pred - tgt[r * d + c];
      sq[r * d + c] = valid ? diff * diff : 0.0;
      const double gs = valid ? (loss_norm * diff) * srow : 0.0;
      double* dt = d3 + (int64_t)r * O + c * S;
      double* dp = d3 + (int64_t)r * O + (d + c) * S;
      for (int k = 0; k < S; ++k) {
        double cv, cp, gth, gph;
        quarter(sphere_theta(yt[k]), k, &cv, &cp);
        const double R = tan(sphere_phi(yp[k]) / 2.0 + kPi / 4.0);
        ilt_term_bwd(gs, k == 0 ? 0.5 : 1.0, R, cv, cp, &gth, &gph);
        dt[k] = sphere_theta_bwd(gth, yt[k]);
        dp[k] = sphere_phi_bwd(gph, yp[k]);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = first ? 0.0 : tile_loss[blockIdx.x];
      for (int i = 0; i < kRows * d; ++i) s += sq[i];
      tile_loss[blockIdx.x] = s;
    }
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
        double acc = first ? 0.0 : part[off[8] + p];
        for (int r = 0; r < kRows; ++r) acc += denc[r * 2 + c] * hB[(int64_t)r * g + i];
        part[off[8] + p] = acc;
      }
      if (threadIdx.x < 2) {
        const int c = threadIdx.x;
        double acc = first ? 0.0 : part[off[9] + c];
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
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void train_reduce_kernel(const ReduceArgs a) {
  const int b = blockIdx.x;
  const int64_t mi = blockIdx.y;  // member of the group: its own partials, tile losses, gradient, chunk sums and loss
  const double* partial = a.partial + mi * a.gs.ws;
  double* grad = a.grad + mi * a.gs.grad;
  const ChunkRange r = chunk_range(a.ct, b);
  double s = 0.0;
  for (int64_t e = r.e0 + threadIdx.x; e < r.e1; e += kThreads) {
    double gsum = 0.0;
    for (int k = 0; k < a.nblk; ++k) gsum += partial[(int64_t)k * a.P + e];
    grad[e] = gsum;
    s += gsum * gsum;
  }
  s = block_sum(s);
  if (threadIdx.x == 0) {
    a.sq[mi * a.gs.ws + b] = s;
    if (b == 0) {
      const double* tile_loss = a.tile_loss + mi * a.gs.ws;
      double l = 0.0;
      for (int k = 0; k < a.nblk; ++k) l += tile_loss[k];
      a.loss[mi] = l / ((double)a.N * (double)a.d);
    }
  }
}

__global__ __launch_bounds__(kThreads) void train_adam_kernel(const AdamArgs a) {
  clip_adam(a.params, a.m, a.v, a.grad, a.sq, a.gradnorm, a.ct, a.gs, a.max_norm, a.k, true);
}

hipError_t launch_train_fwd_bwd(const TrainArgs& a, int nblk, int M, hipStream_t s) {
  const auto kernel = a.lin_tab ? train_fwd_bwd_kernel<true> : train_fwd_bwd_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(nblk, M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_train_reduce(const ReduceArgs& a, int M, hipStream_t s) {
  hipLaunchKernelGGL(train_reduce_kernel, dim3(a.ct.cstart[kTensors], M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_train_adam(const AdamArgs& a, int M, hipStream_t s) {
  hipLaunchKernelGGL(train_adam_kernel, dim3(a.ct.cstart[kTensors], M), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace train
}  // namespace nlc
