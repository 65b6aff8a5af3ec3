// Host build of the element math of the fused training step (neurallaplacecontrol_amd/csrc/nlc_train.h) for
// tests/test_train_host.py (g++, no GPU).
#include "../../neurallaplacecontrol_amd/csrc/nlc_train.h"
using namespace nlc::train;
extern "C" {
// gru_cell_bwd over arrays: in (n, 6) [dh, r, z, n, hn, h_prev] -> out (n, 5) [gi_r, gi_z, gi_n, gh_n, dh_direct]
void nlc_t_gru_cell_bwd(const double* in, double* out, long n) {
  for (long i = 0; i < n; ++i) {
    const double* a = in + 6 * i;
    double* o = out + 5 * i;
    gru_cell_bwd(a[0], a[1], a[2], a[3], a[4], a[5], o, o + 1, o + 2, o + 3, o + 4);
  }
}
// sphere map backward: in (n, 2) [g, y] -> out (n, 2) [theta pre-activation grad, phi pre-activation grad]
void nlc_t_sphere_bwd(const double* in, double* out, long n) {
  for (long i = 0; i < n; ++i) {
    out[2 * i] = sphere_theta_bwd(in[2 * i], in[2 * i + 1]);
    out[2 * i + 1] = sphere_phi_bwd(in[2 * i], in[2 * i + 1]);
  }
}
void nlc_t_clip_coef(const double* in, double* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = clip_coef(in[2 * i], in[2 * i + 1]);
}
// Adam element: state (n, 3) [p, m, v] updated in place from g (n); k = [wd, omb1, beta2, omb2, step_size, bc2_sqrt, eps]
void nlc_t_adam(double* state, const double* g, const double* k, long n) {
  const AdamScalars s{k[0], k[1], k[2], k[3], k[4], k[5], k[6]};
  for (long i = 0; i < n; ++i) adam_element(state + 3 * i, state + 3 * i + 1, state + 3 * i + 2, g[i], s);
}
}
extern "C" {
// act_layout(d, nin, g, h, S, B): the 24 fields of ActLayout in declaration order (offsets, then total)
void nlc_t_act_layout(int d, int nin, int g, int h, int S, int B, long long* out) {
  const ActLayout L = act_layout(d, nin, g, h, S, B);
  const int64_t f[24] = {L.X0, L.H0, L.G0, L.H1, L.G1, L.a0, L.a1, L.a2, L.u, L.d3, L.d2, L.d1,
                         L.denc, L.tn, L.tgt, L.sq, L.DI0, L.DH0, L.DI1, L.DH1, L.DX1, L.dhA, L.dD, L.total};
  for (int i = 0; i < 24; ++i) out[i] = (long long)f[i];
}
// blob_offsets(d, nin, g, h, S): off[0..16]
void nlc_t_blob_offsets(int d, int nin, int g, int h, int S, long long* out) {
  int64_t off[kTensors + 1];
  blob_offsets(d, nin, g, h, S, off);
  for (int i = 0; i <= kTensors; ++i) out[i] = (long long)off[i];
}
// rnn_blob_offsets(d, nin, H, time_input): off[0..16] (six tensors, ten empty)
void nlc_t_rnn_blob_offsets(int d, int nin, int H, int time_input, long long* out) {
  int64_t off[kTensors + 1];
  rnn_blob_offsets(d, nin, H, time_input, off);
  for (int i = 0; i <= kTensors; ++i) out[i] = (long long)off[i];
}
static ChunkTable table_of(const long long* off) {
  ChunkTable c;
  for (int i = 0; i <= kTensors; ++i) c.off[i] = off[i];
  chunk_starts(c);
  return c;
}
// the ChunkTable of off[0..16]: cstart[0..16], and chunk_range of every chunk b: out (chunks, 3) [t, e0, e1]; out may be
// NULL to get the chunk count alone
int nlc_t_chunk_ranges(const long long* off, int* cstart, long long* out) {
  const ChunkTable c = table_of(off);
  for (int i = 0; i <= kTensors; ++i) cstart[i] = c.cstart[i];
  for (int b = 0; out && b < c.cstart[kTensors]; ++b) {
    const ChunkRange r = chunk_range(c, b);
    out[3 * b] = r.t;
    out[3 * b + 1] = (long long)r.e0;
    out[3 * b + 2] = (long long)r.e1;
  }
  return c.cstart[kTensors];
}
// a gradient's chunk sums of squares as train_reduce_kernel forms them (thread i of 256 sums elements e0 + i, e0 + i + 256,
// ... in order, then the fixed tree over the 256 sums): sq (chunks); then clip_total_norm of them
double nlc_t_clip_total(const long long* off, const double* grad, double* sq) {
  const ChunkTable c = table_of(off);
  for (int b = 0; b < c.cstart[kTensors]; ++b) {
    const ChunkRange r = chunk_range(c, b);
    double red[kThreads];
    for (int i = 0; i < kThreads; ++i) {
      double s = 0.0;
      for (int64_t e = r.e0 + i; e < r.e1; e += kThreads) s += grad[e] * grad[e];
      red[i] = s;
    }
    for (int w = kThreads / 2; w > 0; w >>= 1)
      for (int i = 0; i < w; ++i) red[i] += red[i + w];
    sq[b] = red[0];
  }
  return clip_total_norm(sq, c);
}
// the Fourier series' query points and prediction factor: t (n), k (nk) -> theta_s, phi_s (n, nk), factor (n)
void nlc_t_fourier(double alpha, double log_tol, const double* t, long n, const int* k, int nk, double* th, double* ph,
                   double* factor) {
  for (long i = 0; i < n; ++i) {
    for (int j = 0; j < nk; ++j) fourier_query_point(alpha, log_tol, t[i], k[j], &th[i * nk + j], &ph[i * nk + j]);
    factor[i] = fourier_pred_factor(alpha, log_tol, t[i]);
  }
}
}
