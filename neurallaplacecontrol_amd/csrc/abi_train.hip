// Host side of libnlc_hip.so, training unit: the fused training step of a NeuralLaplaceModel (kernels_train.hip) and of the
// DeltaTRNN / RNN baselines (kernels_train_rnn.hip), one iteration of the reference's loop, train_utils.py:388-408 (forward,
// MSELoss, backward, clip_grad_norm_, Adam.step).  The two models differ in the forward + backward launch and the blob's
// tensors; the workspace, the reduction and the Adam launch are written once.
#include <cmath>

#include "nlc_host.h"
#include "nlc_train.h"

using namespace nlc;
using namespace nlc::host;
using namespace nlc::train;

namespace {

struct Plan {
  int g, S, nblk, chunks, d;
  int64_t P, A, ntiles;
  int64_t off[kTensors + 1];
  int cstart[kTensors + 1];
};

// workgroups, partial size and the reduce / Adam chunking of a call with N rows, once p.off, p.A and p.d are set
void plan_rows(Plan& p, int64_t N) {
  p.P = p.off[kTensors];
  p.ntiles = (N + kRows - 1) / kRows;
  p.nblk = (int)(p.ntiles < kMaxBlocks ? p.ntiles : kMaxBlocks);
  p.chunks = chunk_starts(p.off, p.cstart);
}

// (slabs sized for the longest window)
Plan plan_of(const nlc_ctx* c, int64_t N) {
  Plan p{};
  const nlc_model_desc& md = c->md;
  p.g = md.h / 2;
  p.S = md.ilt.terms;
  p.d = md.d;
  blob_offsets(md.d, md.nin, p.g, md.h, p.S, p.off);
  p.A = act_layout(md.d, md.nin, p.g, md.h, p.S, kMaxB).total;
  plan_rows(p, N);
  return p;
}

Plan rnn_plan_of(const nlc_ctx* c, int64_t N) {
  Plan p{};
  const nlc_rnn_desc& rd = c->rd;
  p.d = rd.d;
  rnn_blob_offsets(rd.d, rd.nin, rd.hidden, rd.time_input, p.off);
  p.A = rnn_act_layout(rd.nin, rd.hidden, kMaxB).total;
  plan_rows(p, N);
  return p;
}

// scratch: [partials nblk * P | tile losses | slabs nblk * A | summed gradient P | chunk sums of squares]
struct WsPtrs {
  double *partial, *tile_loss, *act, *grad, *sq;
};
int64_t ws_doubles(const Plan& p, WsPtrs* w, void* base) {
  auto al = [](int64_t n) { return (n + 31) / 32 * 32; };
  int64_t o = 0;
  double* b = (double*)base;
  const int64_t o_part = o;
  o += al((int64_t)p.nblk * p.P);
  const int64_t o_loss = o;
  o += al(p.nblk);
  const int64_t o_act = o;
  o += al((int64_t)p.nblk * p.A);
  const int64_t o_grad = o;
  o += al(p.P);
  const int64_t o_sq = o;
  o += al(p.chunks);
  if (w && b) *w = WsPtrs{b + o_part, b + o_loss, b + o_act, b + o_grad, b + o_sq};
  return o;
}

int check_train(nlc_ctx* c, int64_t N, int B) {
  if (!c->has_model) return fail(c, NLC_ERR_STATE, "nlc_set_model has not been called");
  if (c->md.ilt.algo != NLC_ILT_FOURIER) return fail(c, NLC_ERR_UNSUPPORTED, "fused training step: fourier models only");
  if (c->md.ilt.scale != 2.0) return fail(c, NLC_ERR_UNSUPPORTED, "fused training step needs ILT scale == 2");
  if (B < 1 || B > kMaxB) return fail(c, NLC_ERR_UNSUPPORTED, "fused training step: window length must be in 1..16");
  if (N < 1) return fail(c, NLC_ERR_BAD_SHAPE, "fused training step: N must be >= 1");
  return NLC_OK;
}

// partials -> grad (blob order) and loss; sq gets the chunk sums of squares
int reduce(nlc_ctx* c, int64_t N, double* grad, double* loss, const Plan& p, const WsPtrs& w) {
  ReduceArgs r{};
  r.partial = w.partial;
  r.tile_loss = w.tile_loss;
  r.nblk = p.nblk;
  r.d = p.d;
  r.P = p.P;
  r.N = N;
  r.grad = grad;
  r.sq = w.sq;
  r.loss = loss;
  for (int i = 0; i <= kTensors; ++i) {
    r.off[i] = p.off[i];
    r.cstart[i] = p.cstart[i];
  }
  ProfScope ps(c, "train_reduce_kernel");
  NLC_HIP(c, launch_train_reduce(r, c->stream));
  return NLC_OK;
}

// clip_grad_norm_ + Adam.step() on the summed gradient in the workspace
int adam(nlc_ctx* c, const nlc_train_desc* desc, double* params, double* m, double* v, int64_t step, double* gradnorm,
         const Plan& p, const WsPtrs& w) {
  // the host-side scalars of torch.optim.Adam's foreach step (python floats there: beta ** step, (lr / bc1) * -1, bc2 ** 0.5)
  AdamArgs a{};
  a.params = params;
  a.m = m;
  a.v = v;
  a.grad = w.grad;
  a.sq = w.sq;
  a.max_norm = desc->max_grad_norm;
  const double bc1 = 1.0 - std::pow(desc->beta1, (double)step);
  const double bc2 = 1.0 - std::pow(desc->beta2, (double)step);
  a.k.wd = desc->weight_decay;
  a.k.omb1 = 1.0 - desc->beta1;
  a.k.beta2 = desc->beta2;
  a.k.omb2 = 1.0 - desc->beta2;
  a.k.step_size = (desc->lr / bc1) * -1.0;
  a.k.bc2_sqrt = std::pow(bc2, 0.5);
  a.k.eps = desc->eps;
  a.gradnorm = gradnorm;
  for (int i = 0; i <= kTensors; ++i) {
    a.off[i] = p.off[i];
    a.cstart[i] = p.cstart[i];
  }
  ProfScope ps(c, "train_adam_kernel");
  NLC_HIP(c, launch_train_adam(a, c->stream));
  return NLC_OK;
}

// forward + backward + reduce: grad (blob order) and loss; sq gets the chunk sums of squares
int loss_grad(nlc_ctx* c, const double* params, const double* obs, const double* window, const double* ts,
              const double* target, const int64_t* idx, int64_t N, int B, double* grad, double* loss, const Plan& p,
              const WsPtrs& w) {
  const nlc_model_desc& md = c->md;
  TrainArgs a{};
  a.d = md.d;
  a.nin = md.nin;
  a.g = p.g;
  a.h = md.h;
  a.S = p.S;
  a.B = B;
  a.time_div = md.time_div;
  a.alpha = md.ilt.alpha;
  a.log_tol = std::log(md.ilt.tol);
  for (int i = 0; i < md.d; ++i) {
    a.sm[i] = md.state_mean[i];
    a.ss[i] = md.state_std[i];
  }
  for (int i = 0; i < md.nin; ++i) {
    a.am[i] = md.action_mean[i];
    a.as[i] = md.action_std[i];
  }
  a.params = params;
  a.obs = obs;
  a.window = window;
  a.ts = ts;
  a.target = target;
  a.idx = idx;
  a.N = N;
  a.ntiles = (int)p.ntiles;
  a.P = p.P;
  a.A = p.A;
  a.L = act_layout(md.d, md.nin, p.g, md.h, p.S, B);
  a.partial = w.partial;
  a.tile_loss = w.tile_loss;
  a.act = w.act;
  for (int i = 0; i <= kTensors; ++i) a.off[i] = p.off[i];
  {
    ProfScope ps(c, "train_fwd_bwd_kernel");
    NLC_HIP(c, launch_train_fwd_bwd(a, p.nblk, c->stream));
  }
  return reduce(c, N, grad, loss, p, w);
}

int check_rnn_train(nlc_ctx* c, int64_t N, int B) {
  if (!c->has_rnn) return fail(c, NLC_ERR_STATE, "nlc_set_rnn_model has not been called");
  if (B < 1 || B > kMaxB) return fail(c, NLC_ERR_UNSUPPORTED, "fused training step: window length must be in 1..16");
  if (N < 1) return fail(c, NLC_ERR_BAD_SHAPE, "fused training step: N must be >= 1");
  return NLC_OK;
}

int rnn_loss_grad(nlc_ctx* c, const double* params, const double* obs, const double* window, const double* ts,
                  const double* target, const int64_t* idx, int64_t N, int B, double* grad, double* loss, const Plan& p,
                  const WsPtrs& w) {
  const nlc_rnn_desc& rd = c->rd;
  RnnTrainArgs a{};
  a.d = rd.d;
  a.nin = rd.nin;
  a.B = B;
  a.time_input = rd.time_input;
  a.time_div = rd.time_div;
  for (int i = 0; i < rd.d; ++i) {
    a.sm[i] = rd.state_mean[i];
    a.ss[i] = rd.state_std[i];
  }
  for (int i = 0; i < rd.nin; ++i) {
    a.am[i] = rd.action_mean[i];
    a.as[i] = rd.action_std[i];
  }
  a.params = params;
  a.obs = obs;
  a.window = window;
  a.ts = ts;
  a.target = target;
  a.idx = idx;
  a.N = N;
  a.ntiles = (int)p.ntiles;
  a.P = p.P;
  a.A = p.A;
  a.L = rnn_act_layout(rd.nin, rd.hidden, B);
  a.partial = w.partial;
  a.tile_loss = w.tile_loss;
  a.act = w.act;
  for (int i = 0; i <= kRnnTensors; ++i) a.off[i] = p.off[i];
  {
    ProfScope ps(c, "rnn_train_fwd_bwd_kernel");
    NLC_HIP(c, launch_rnn_train_fwd_bwd(a, rd.hidden, p.nblk, c->stream));
  }
  return reduce(c, N, grad, loss, p, w);
}

}  // namespace

// train_utils.py:388-408
extern "C" int64_t nlc_train_workspace_bytes(nlc_ctx* c, int64_t N) {
  if (!c || !c->has_model || N < 1) return -1;
  const Plan p = plan_of(c, N);
  return ws_doubles(p, nullptr, nullptr) * (int64_t)sizeof(double);
}

// train_utils.py:391-402 (zero_grad, forward, MSELoss, backward)
extern "C" int nlc_train_loss_grad(nlc_ctx* c, const double* params, const double* obs, const double* window,
                                   const double* ts, const double* target, const int64_t* idx, int64_t N, int B,
                                   double* grad, double* loss, void* ws) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (int rc = check_train(c, N, B)) return rc;
  if (!params || !obs || !window || !ts || !target || !idx || !grad || !loss || !ws)
    return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  NLC_HIP(c, hipSetDevice(c->device));
  const Plan p = plan_of(c, N);
  WsPtrs w;
  ws_doubles(p, &w, ws);
  return loss_grad(c, params, obs, window, ts, target, idx, N, B, grad, loss, p, w);
  NLC_GUARD_END(c)
}

// train_utils.py:391-404 (one whole iteration: + clip_grad_norm_ + optimizer.step())
extern "C" int nlc_train_step(nlc_ctx* c, const nlc_train_desc* desc, double* params, double* m, double* v, int64_t step,
                              const double* obs, const double* window, const double* ts, const double* target,
                              const int64_t* idx, int64_t N, int B, double* loss, double* gradnorm, void* ws) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (!desc) return fail(c, NLC_ERR_BAD_ARG, "NULL train desc");
  if (int rc = check_train(c, N, B)) return rc;
  if (step < 1) return fail(c, NLC_ERR_BAD_ARG, "Adam step count must be >= 1");
  if (!params || !m || !v || !obs || !window || !ts || !target || !idx || !loss || !ws)
    return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  NLC_HIP(c, hipSetDevice(c->device));
  const Plan p = plan_of(c, N);
  WsPtrs w;
  ws_doubles(p, &w, ws);
  if (int rc = loss_grad(c, params, obs, window, ts, target, idx, N, B, w.grad, loss, p, w)) return rc;
  return adam(c, desc, params, m, v, step, gradnorm, p, w);
  NLC_GUARD_END(c)
}

// ---- DeltaTRNN / RNN (train_utils.py:550-631): the same three entries and contract; params, m, v flat in
// nlc_set_rnn_model's blob order; ts may be NULL for a model without time input
// train_utils.py:388-408
extern "C" int64_t nlc_rnn_train_workspace_bytes(nlc_ctx* c, int64_t N) {
  if (!c || !c->has_rnn || N < 1) return -1;
  const Plan p = rnn_plan_of(c, N);
  return ws_doubles(p, nullptr, nullptr) * (int64_t)sizeof(double);
}

// train_utils.py:391-402 (zero_grad, forward, MSELoss, backward)
extern "C" int nlc_rnn_train_loss_grad(nlc_ctx* c, const double* params, const double* obs, const double* window,
                                       const double* ts, const double* target, const int64_t* idx, int64_t N, int B,
                                       double* grad, double* loss, void* ws) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (int rc = check_rnn_train(c, N, B)) return rc;
  if (!params || !obs || !window || (!ts && c->rd.time_input) || !target || !idx || !grad || !loss || !ws)
    return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  NLC_HIP(c, hipSetDevice(c->device));
  const Plan p = rnn_plan_of(c, N);
  WsPtrs w;
  ws_doubles(p, &w, ws);
  return rnn_loss_grad(c, params, obs, window, ts, target, idx, N, B, grad, loss, p, w);
  NLC_GUARD_END(c)
}

// train_utils.py:391-404 (one whole iteration: + clip_grad_norm_ + optimizer.step())
extern "C" int nlc_rnn_train_step(nlc_ctx* c, const nlc_train_desc* desc, double* params, double* m, double* v,
                                  int64_t step, const double* obs, const double* window, const double* ts,
                                  const double* target, const int64_t* idx, int64_t N, int B, double* loss, double* gradnorm,
                                  void* ws) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (!desc) return fail(c, NLC_ERR_BAD_ARG, "NULL train desc");
  if (int rc = check_rnn_train(c, N, B)) return rc;
  if (step < 1) return fail(c, NLC_ERR_BAD_ARG, "Adam step count must be >= 1");
  if (!params || !m || !v || !obs || !window || (!ts && c->rd.time_input) || !target || !idx || !loss || !ws)
    return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  NLC_HIP(c, hipSetDevice(c->device));
  const Plan p = rnn_plan_of(c, N);
  WsPtrs w;
  ws_doubles(p, &w, ws);
  if (int rc = rnn_loss_grad(c, params, obs, window, ts, target, idx, N, B, w.grad, loss, p, w)) return rc;
  return adam(c, desc, params, m, v, step, gradnorm, p, w);
  NLC_GUARD_END(c)
}
