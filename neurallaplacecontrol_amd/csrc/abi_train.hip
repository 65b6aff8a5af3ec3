// Host side of libnlc_hip.so, training unit: the fused training step of a NeuralLaplaceModel (kernels_train.hip; the Fourier
// ILT, or fixed Talbot / Stehfest with the node and weight tables of abi_ilt.hip's linear_tables) and of the
// DeltaTRNN / RNN (kernels_train_rnn.hip) and NODE (kernels_train_node.hip) baselines, one iteration of the reference's loop, train_utils.py:388-408 (forward,
// MSELoss, backward, clip_grad_norm_, Adam.step).  The models differ in the forward + backward launch and the blob's
// tensors; the workspace, the reduction and the Adam launch are written once.  Every entry is the group path: M same-shaped
// models (run_exp_multi.py:105-110) in the same three launches, the member on the grid's y axis; a single model is M = 1.
#include <cmath>
#include <iterator>

#include "nlc_host.h"
#include "nlc_train.h"
#include "nlc_train_dehoog.h"
#include "nlc_train_eval.h"
#include "nlc_train_members.h"
#include "nlc_train_node.h"

using namespace nlc;
using namespace nlc::host;
using namespace nlc::train;

namespace {

// the model families of the entries below: NeuralLaplaceModel, DeltaTRNN / RNN, NODE
enum Family { kFamNl, kFamRnn, kFamNode };

struct Plan {
  int g, S, nblk, chunks, d;
  int64_t P, A, ntiles;
  ChunkTable ct;         // the blob's tensors and their reduce / Adam chunks
  TrainWsLayout ws;      // one member's workspace region
  GroupStrides gs;  // for a group whose gradient lives in the workspace (a step); loss_grad overrides gs.grad
  int M;
  int row_times;  // NODE: every row integrates to its own time (0: to the batch's first row's, as the reference)
  bool dehoog;        // NL, option "train_dehoog": the de Hoog launch sequence (nlc_train_dehoog.h); dh is its workspace
  DehoogWsLayout dh;  // (set by plan_group: the ILT arrays hold the M members back to back)
};

// workgroups, partial size and the reduce / Adam chunking of a call with N rows, once p.ct.off, p.A and p.d are set
void plan_rows(Plan& p, int64_t N) {
  p.P = p.ct.off[kTensors];
  p.ntiles = (N + kRows - 1) / kRows;
  p.nblk = (int)(p.ntiles < kMaxBlocks ? p.ntiles : kMaxBlocks);
  p.chunks = chunk_starts(p.ct);
  p.ws = train_ws_layout(p.nblk, p.P, p.A, p.chunks);
}

// the members' strides of a call: M members, N index entries each, data_rows dataset rows apart (0: one shared dataset)
void plan_group(Plan& p, int M, int64_t N, int64_t data_rows) {
  p.M = M;
  p.gs = GroupStrides{p.P, p.ws.total, p.ws.total, N, data_rows};
  if (p.dehoog) p.dh = dehoog_ws_layout(M, N, p.d, p.S, p.ws.total);
}

// whether the ctx's NL model trains through the de Hoog launch sequence: a de Hoog model and option "train_dehoog" = 1
bool nl_dehoog(const nlc_ctx* c) { return c->nl.has && c->nl.md.ilt.algo == NLC_ILT_DEHOOG && c->opt.train_dehoog != 0; }

// (slabs sized for the longest window)
Plan plan_of(const nlc_ctx* c, int64_t N) {
  Plan p{};
  const nlc_model_desc& md = c->nl.md;
  p.g = md.h / 2;
  p.S = md.ilt.terms;
  p.d = md.d;
  blob_offsets(md.d, md.nin, p.g, md.h, p.S, p.ct.off);
  p.A = act_layout(md.d, md.nin, p.g, md.h, p.S, kMaxB).total;
  p.dehoog = nl_dehoog(c);
  plan_rows(p, N);
  return p;
}

Plan rnn_plan_of(const nlc_ctx* c, int64_t N) {
  Plan p{};
  const nlc_rnn_desc& rd = c->rnnm.rd;
  p.d = rd.d;
  rnn_blob_offsets(rd.d, rd.nin, rd.hidden, rd.time_input, p.ct.off);
  p.A = rnn_act_layout(rd.nin, rd.hidden, kMaxB).total;
  plan_rows(p, N);
  return p;
}

// (the slab is a function of the shape alone: it holds the tape of kNodeTrainMaxSub ODE-function inputs, whatever ts says and
// whichever method the ctx option "node_method" names)
Plan node_plan_of(const nlc_ctx* c, int64_t N) {
  Plan p{};
  const nlc_node_desc& nd = c->nodem.nd;
  p.d = nd.d;
  node_blob_offsets(nd.d, nd.augment_dim, nd.nu, nd.hidden, p.ct.off);
  p.A = node_act_layout(nd.hidden, nd.d + nd.augment_dim + nd.nu).total;
  plan_rows(p, N);
  return p;
}

Plan family_plan(const nlc_ctx* c, Family fam, int64_t N) {
  return fam == kFamRnn ? rnn_plan_of(c, N) : fam == kFamNode ? node_plan_of(c, N) : plan_of(c, N);
}

bool family_has(const nlc_ctx* c, Family fam) {
  return fam == kFamRnn ? c->rnnm.has : fam == kFamNode ? c->nodem.has : c->nl.has;
}

// member 0's arrays in the workspace (nlc_train.h TrainWsLayout; member m's are gs.ws doubles further on)
struct WsPtrs {
  double *partial, *tile_loss, *act, *grad, *sq;
  double* base;  // the workspace's first double (a de Hoog call's ILT arrays are offsets of Plan::dh from it)
};
WsPtrs ws_ptrs(const Plan& p, void* base) {
  double* b = (double*)base;
  return WsPtrs{b + p.ws.partial, b + p.ws.tile_loss, b + p.ws.act, b + p.ws.grad, b + p.ws.sq, b};
}

// whether the family's kernels read ts: all but an RNN without time input
bool need_ts(const nlc_ctx* c, Family fam) { return fam == kFamRnn ? c->rnnm.rd.time_input != 0 : true; }

// the NL model the kernels take: uploaded, and with one of the three ILT algorithms they are written for (fixed Talbot /
// Stehfest: fixed nodes and weights from linear_tables, the <true> instance of train_fwd_bwd_kernel); with option
// "train_dehoog" also de Hoog at the term counts its ILT kernels take, at any ILT scale (kernels_train_dehoog.hip)
int check_nl_model(nlc_ctx* c) {
  if (!c->nl.has) return fail(c, NLC_ERR_STATE, "nlc_set_model has not been called");
  const nlc_ilt_desc& ilt = c->nl.md.ilt;
  if (nl_dehoog(c)) {
    if (ilt.terms < 3 || ilt.terms > 33 || ilt.terms % 2 == 0)
      return fail(c, NLC_ERR_UNSUPPORTED, "fused training step (dehoog): ilt_reconstruction_terms must be odd, 3 .. 33");
  } else if (is_linear_ilt(ilt)) {
    // what linear_tables cannot build: an odd or too long Stehfest series, terms past the tables
    if (check_ilt(c, &ilt) != NLC_OK)
      return fail(c, NLC_ERR_UNSUPPORTED,
                  "fused training step: no node / weight tables for these terms (stehfest: even, 2 .. 20; fixed_tablot: 2 .. 129)");
  } else {
    if (ilt.algo != NLC_ILT_FOURIER)
      return fail(c, NLC_ERR_UNSUPPORTED, "fused training step: fourier, fixed_tablot and stehfest models only");
    if (ilt.scale != 2.0) return fail(c, NLC_ERR_UNSUPPORTED, "fused training step needs ILT scale == 2 (fourier)");
  }
  return NLC_OK;
}

// what every training and evaluation entry checks first, in this order: the family's model, the call's shape, the group
int check_call(nlc_ctx* c, Family fam, int M, int64_t data_rows, int64_t N, int B) {
  if (fam == kFamRnn && !c->rnnm.has) return fail(c, NLC_ERR_STATE, "nlc_set_rnn_model has not been called");
  if (fam == kFamNode && !c->nodem.has) return fail(c, NLC_ERR_STATE, "nlc_set_node_model has not been called");
  if (fam == kFamNl)
    if (int rc = check_nl_model(c)) return rc;
  // (a NODE reads the window's newest action only, but keeps the families' one contract)
  if (B < 1 || B > kMaxB) return fail(c, NLC_ERR_UNSUPPORTED, "fused training step: window length must be in 1..16");
  if (N < 1) return fail(c, NLC_ERR_BAD_SHAPE, "fused training step: N must be >= 1");
  // (de Hoog: one tile per workgroup, its slab lives across the ILT launches)
  if (fam == kFamNl && nl_dehoog(c) && N > kDehoogMaxRows)
    return fail(c, NLC_ERR_UNSUPPORTED, "fused training step (dehoog): at most 2048 rows in a call");
  if (M < 1) return fail(c, NLC_ERR_BAD_SHAPE, "fused training step: a group needs M >= 1 members");
  if (M > kMaxGroup) return fail(c, NLC_ERR_UNSUPPORTED, "fused training step: at most 65535 members in a group");
  if (data_rows < 0) return fail(c, NLC_ERR_BAD_SHAPE, "fused training step: data_row_stride must be >= 0");
  return NLC_OK;
}

// partials -> grad (blob order, members grad_stride apart) and loss [M]; sq gets the chunk sums of squares
int reduce(nlc_ctx* c, int64_t N, double* grad, int64_t grad_stride, double* loss, const Plan& p, const WsPtrs& w) {
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
  r.ct = p.ct;
  r.gs = p.gs;
  r.gs.grad = grad_stride;
  ProfScope ps(c, "train_reduce_kernel");
  NLC_HIP(c, launch_train_reduce(r, p.M, c->stream));
  return NLC_OK;
}

// the scalars of torch.optim.Adam's foreach step that a group shares at one step count (python floats there: beta ** step,
// bc2 ** 0.5); step_size needs a learning rate, see adam and adam_members
struct StepScalars {
  double omb1, beta2, omb2, eps, bc1, bc2_sqrt;
};
StepScalars step_scalars(const nlc_train_desc* desc, int64_t step) {
  const double bc1 = 1.0 - std::pow(desc->beta1, (double)step);
  const double bc2 = 1.0 - std::pow(desc->beta2, (double)step);
  return StepScalars{1.0 - desc->beta1, desc->beta2, 1.0 - desc->beta2, desc->eps, bc1, std::pow(bc2, 0.5)};
}

// clip_grad_norm_ + Adam.step() on the summed gradients in the workspace, per member
int adam(nlc_ctx* c, const nlc_train_desc* desc, double* params, double* m, double* v, int64_t step, double* gradnorm,
         const Plan& p, const WsPtrs& w) {
  const StepScalars s = step_scalars(desc, step);
  AdamArgs a{};
  a.params = params;
  a.m = m;
  a.v = v;
  a.grad = w.grad;
  a.sq = w.sq;
  a.max_norm = desc->max_grad_norm;
  // step_size on the host, as python's (lr / bc1) * -1
  a.k = AdamScalars{desc->weight_decay, s.omb1, s.beta2, s.omb2, (desc->lr / s.bc1) * -1.0, s.bc2_sqrt, s.eps};
  a.gradnorm = gradnorm;
  a.ct = p.ct;
  a.gs = p.gs;
  ProfScope ps(c, "train_adam_kernel");
  NLC_HIP(c, launch_train_adam(a, p.M, c->stream));
  return NLC_OK;
}

// the same launch with lr, weight decay, clip norm and the active flag per member, from device arrays (kernels_train_members.hip);
// desc gives the betas and eps, its lr / weight_decay / max_grad_norm are not read; step_size is formed on the device, as
// -(lr[m] / bc1) (nlc_train_members.h member_step_size: the bits of the host's expression above)
int adam_members(nlc_ctx* c, const nlc_train_desc* desc, const nlc_train_members* mem, double* params, double* m, double* v,
                 int64_t step, double* gradnorm, const Plan& p, const WsPtrs& w) {
  const StepScalars s = step_scalars(desc, step);
  MembersAdamArgs a{};
  a.params = params;
  a.m = m;
  a.v = v;
  a.grad = w.grad;
  a.sq = w.sq;
  a.lr = mem->lr_dev;
  a.wd = mem->wd_dev;
  a.max_norm = mem->max_norm_dev;
  a.active = mem->active_dev;
  a.omb1 = s.omb1;
  a.beta2 = s.beta2;
  a.omb2 = s.omb2;
  a.eps = s.eps;
  a.bc1 = s.bc1;
  a.bc2_sqrt = s.bc2_sqrt;
  a.gradnorm = gradnorm;
  a.ct = p.ct;
  a.gs = p.gs;
  ProfScope ps(c, "train_adam_members_kernel");
  NLC_HIP(c, launch_train_adam_members(a, p.M, c->stream));
  return NLC_OK;
}

// normalisation constants of a family's descriptor (nlc_model_desc or nlc_rnn_desc); entries past d / nin stay 0
template <class Desc>
void fill_norm(Norm& n, const Desc& m) {
  for (int i = 0; i < m.d; ++i) {
    n.sm[i] = m.state_mean[i];
    n.ss[i] = m.state_std[i];
  }
  for (int i = 0; i < m.nin; ++i) {
    n.am[i] = m.action_mean[i];
    n.as[i] = m.action_std[i];
  }
}

// what the four forward launches (training and evaluation, both families) share: the descriptor's shape and constants, the
// window length, the batch, and the plan's tiles, blob offsets and member strides
template <class Args, class Desc>
void fill_call(Args& a, const Desc& m, int B, const Batch& b, const Plan& p) {
  a.d = m.d;
  a.nin = m.nin;
  a.B = B;
  a.time_div = m.time_div;
  fill_norm(a.norm, m);
  a.batch = b;
  a.ntiles = (decltype(a.ntiles))p.ntiles;
  for (size_t i = 0; i < std::size(a.off); ++i) a.off[i] = p.ct.off[i];
  a.gs = p.gs;
}

// the NL model's own part of a launch: widths, the Fourier constants, or the tables of a linear algorithm
template <class Args>
int fill_nl(nlc_ctx* c, Args& a, const Plan& p) {
  const nlc_model_desc& md = c->nl.md;
  a.g = p.g;
  a.h = md.h;
  a.S = p.S;
  a.alpha = md.ilt.alpha;
  a.log_tol = std::log(md.ilt.tol);
  // one table for all members of a group (they share the descriptor); NULL selects the Fourier instance
  return is_linear_ilt(md.ilt) ? linear_tables(c, &md.ilt, &a.lin_tab) : NLC_OK;
}

// the workspace of a forward + backward launch
template <class Args>
void fill_train_ws(Args& a, const Plan& p, const WsPtrs& w) {
  a.P = p.P;
  a.A = p.A;
  a.partial = w.partial;
  a.tile_loss = w.tile_loss;
  a.act = w.act;
}

int nl_dehoog_launches(nlc_ctx* c, const Batch& b, int B, const Plan& p, const WsPtrs& w, bool backward);

int nl_fwd_bwd(nlc_ctx* c, const Batch& b, int B, const Plan& p, const WsPtrs& w) {
  if (p.dehoog) return nl_dehoog_launches(c, b, B, p, w, true);
  TrainArgs a{};
  fill_call(a, c->nl.md, B, b, p);
  if (int rc = fill_nl(c, a, p)) return rc;
  fill_train_ws(a, p, w);
  a.L = act_layout(p.d, c->nl.md.nin, p.g, c->nl.md.h, p.S, B);
  ProfScope ps(c, "train_fwd_bwd_kernel");
  NLC_HIP(c, launch_train_fwd_bwd(a, p.nblk, p.M, c->stream));
  return NLC_OK;
}

// the de Hoog step's launches 1 .. 3 (forward half, ILT, loss; what evaluation needs) and, with backward, 4 and 5.  The group is
// one batch of M * rows points for the two ILT launches
int nl_dehoog_launches(nlc_ctx* c, const Batch& b, int B, const Plan& p, const WsPtrs& w, bool backward) {
  const nlc_model_desc& md = c->nl.md;
  const DehoogWsLayout& dh = p.dh;
  const int64_t R = (int64_t)p.M * dh.rows;
  DehoogTrainArgs a{};
  fill_call(a.t, md, B, b, p);
  if (int rc = fill_nl(c, a.t, p)) return rc;
  fill_train_ws(a.t, p, w);
  a.t.L = act_layout(p.d, md.nin, p.g, md.h, p.S, B);
  a.scale = md.ilt.scale;
  a.rows = dh.rows;
  a.theta = w.base + dh.theta;
  a.phi = w.base + dh.phi;
  a.tq = w.base + dh.t;
  a.gtheta = w.base + dh.gtheta;
  a.gphi = w.base + dh.gphi;
  {
    ProfScope ps(c, "train_dehoog_fwd_kernel");
    NLC_HIP(c, launch_train_dehoog_fwd(a, p.nblk, p.M, c->stream));
  }
  {
    // (the times are normalised already: t_div stays 1)
    const IltArgs ia = ilt_args(md.ilt, a.theta, a.phi, a.tq, w.base + dh.pred, R, p.d);
    ProfScope ps(c, "ilt_dehoog_kernel");
    NLC_HIP(c, launch_ilt_dehoog(ia, c->stream));
  }
  {
    const DehoogLossArgs la{w.base + dh.pred, w.act, w.base + dh.gx, w.tile_loss, dh.rows, b.N, p.A, a.t.L.tgt, p.gs.ws, p.d};
    ProfScope ps(c, "train_dehoog_loss_kernel");
    NLC_HIP(c, launch_train_dehoog_loss(la, p.nblk, p.M, c->stream));
  }
  if (!backward) return NLC_OK;
  {
    const IltDehoogBwdArgs ba = ilt_dehoog_bwd_args(md.ilt, a.theta, a.phi, a.tq, w.base + dh.gx, w.base + dh.gtheta,
                                                    w.base + dh.gphi, R, p.d, w.base + dh.scratch);
    ProfScope ps(c, "ilt_dehoog_bwd_kernel");
    NLC_HIP(c, launch_ilt_dehoog_bwd(ba, c->stream));
  }
  ProfScope ps(c, "train_dehoog_bwd_kernel");
  NLC_HIP(c, launch_train_dehoog_bwd(a, p.nblk, p.M, c->stream));
  return NLC_OK;
}

int rnn_fwd_bwd(nlc_ctx* c, const Batch& b, int B, const Plan& p, const WsPtrs& w) {
  const nlc_rnn_desc& rd = c->rnnm.rd;
  RnnTrainArgs a{};
  fill_call(a, rd, B, b, p);
  a.time_input = rd.time_input;
  fill_train_ws(a, p, w);
  a.L = rnn_act_layout(rd.nin, rd.hidden, B);
  ProfScope ps(c, "rnn_train_fwd_bwd_kernel");
  NLC_HIP(c, launch_rnn_train_fwd_bwd(a, rd.hidden, p.nblk, p.M, c->stream));
  return NLC_OK;
}

// held-out loss (kernels_train_eval.hip): forward and squared error only; p.gs is the evaluation's (group_eval_entry)
int nl_eval(nlc_ctx* c, const Batch& b, int B, const Plan& p, double* tile_loss) {
  EvalArgs a{};
  fill_call(a, c->nl.md, B, b, p);
  if (int rc = fill_nl(c, a, p)) return rc;
  a.tile_loss = tile_loss;
  a.L = eval_lds_layout(p.d, c->nl.md.nin, p.g, c->nl.md.h, p.S, B);
  // one workgroup per compute unit: the kernel's registers leave room for one wave per SIMD, whatever its LDS
  ProfScope ps(c, "train_eval_kernel");
  NLC_HIP(c, launch_train_eval(a, eval_grid(a.ntiles, c->prop.multiProcessorCount, 1, p.M), p.M, c->stream));
  return NLC_OK;
}

int rnn_eval(nlc_ctx* c, const Batch& b, int B, const Plan& p, double* tile_loss) {
  const nlc_rnn_desc& rd = c->rnnm.rd;
  RnnEvalArgs a{};
  fill_call(a, rd, B, b, p);
  a.time_input = rd.time_input;
  a.tile_loss = tile_loss;
  const int per_cu = eval_per_cu(rnn_eval_lds_doubles(rd.hidden) * (int64_t)sizeof(double));
  ProfScope ps(c, "rnn_eval_kernel");
  NLC_HIP(c, launch_rnn_eval(a, rd.hidden, eval_grid(a.ntiles, c->prop.multiProcessorCount, per_cu, p.M), p.M, c->stream));
  return NLC_OK;
}

// nlc_node_desc as fill_call reads a descriptor: the state half of the constants, no normalised input (the ODE function takes
// the window's newest action raw)
struct NodeDescView {
  int d, nin;
  double time_div;
  const double *state_mean, *state_std, *action_mean, *action_std;
};

// the NODE's launch arguments, shared by training and evaluation (kernels_train_node.hip)
NodeTrainArgs node_args(const nlc_ctx* c, const Batch& b, int B, const Plan& p) {
  const nlc_node_desc& nd = c->nodem.nd;
  NodeTrainArgs a{};
  fill_call(a, NodeDescView{nd.d, 0, nd.time_div, nd.state_mean, nd.state_std, nullptr, nullptr}, B, b, p);
  a.aug = nd.augment_dim;
  a.nu = nd.nu;
  a.H = nd.hidden;
  a.step_size = nd.step_size;
  a.row_times = p.row_times;
  return a;
}

int node_fwd_bwd(nlc_ctx* c, const Batch& b, int B, const Plan& p, const WsPtrs& w) {
  NodeTrainArgs a = node_args(c, b, B, p);
  fill_train_ws(a, p, w);
  a.L = node_act_layout(a.H, a.d + a.aug + a.nu);
  ProfScope ps(c, "node_train_fwd_bwd_kernel");
  NLC_HIP(c, launch_node_train_fwd_bwd(a, c->opt.node_method, p.nblk, p.M, c->stream));
  return NLC_OK;
}

int node_eval(nlc_ctx* c, const Batch& b, int B, const Plan& p, double* tile_loss) {
  NodeTrainArgs a = node_args(c, b, B, p);
  a.tile_loss = tile_loss;
  const int per_cu = eval_per_cu(node_lds_doubles(false, nlc::node_rk_stages(c->opt.node_method)) * (int64_t)sizeof(double));
  ProfScope ps(c, "node_eval_kernel");
  NLC_HIP(c, launch_node_eval(a, c->opt.node_method, eval_grid(a.ntiles, c->prop.multiProcessorCount, per_cu, p.M), p.M, c->stream));
  return NLC_OK;
}

// ---- the three entries of a family, written once for all of them and for any M
int64_t group_workspace_bytes(nlc_ctx* c, Family fam, int M, int64_t N) {
  if (!c || !family_has(c, fam) || N < 1 || M < 1 || M > kMaxGroup) return -1;
  Plan p = family_plan(c, fam, N);
  if (!p.dehoog) return (int64_t)M * p.ws.total * (int64_t)sizeof(double);
  plan_group(p, M, N, 0);
  return p.dh.total * (int64_t)sizeof(double);
}

// checks (all on the host, before any launch, in the single entries' order: model state and shape, the group, the step count,
// NULL pointers), then forward + backward + reduce of every member.  A step (step != NULL: its Adam step count; more_null: one
// of its own pointers is NULL) keeps the summed gradients in the workspace; else they go to the caller's grad [M][P]
int group_loss_grad(nlc_ctx* c, Family fam, int M, int64_t data_rows, const double* params, const double* obs,
                    const double* window, const double* ts, const double* target, const int64_t* idx, int64_t N, int B,
                    double* grad, double* loss, void* ws, Plan* plan, int row_times, const int64_t* step = nullptr,
                    bool more_null = false) {
  if (int rc = check_call(c, fam, M, data_rows, N, B)) return rc;
  if (step && *step < 1) return fail(c, NLC_ERR_BAD_ARG, "Adam step count must be >= 1");
  if (!params || !obs || !window || (!ts && need_ts(c, fam)) || !target || !idx || (!step && !grad) || !loss || !ws || more_null)
    return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  NLC_HIP(c, hipSetDevice(c->device));
  Plan& p = *plan;
  p = family_plan(c, fam, N);
  plan_group(p, M, N, data_rows);
  p.row_times = row_times;
  const WsPtrs w = ws_ptrs(p, ws);
  const Batch b{params, obs, window, ts, target, idx, N};
  if (int rc = (fam == kFamRnn ? rnn_fwd_bwd : fam == kFamNode ? node_fwd_bwd : nl_fwd_bwd)(c, b, B, p, w)) return rc;
  return reduce(c, N, step ? w.grad : grad, step ? p.gs.ws : p.P, loss, p, w);
}

int group_loss_grad_entry(nlc_ctx* c, Family fam, int M, int64_t data_rows, const double* params, const double* obs,
                          const double* window, const double* ts, const double* target, const int64_t* idx, int64_t N,
                          int B, double* grad, double* loss, void* ws, int row_times = 0) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  Plan p;
  return group_loss_grad(c, fam, M, data_rows, params, obs, window, ts, target, idx, N, B, grad, loss, ws, &p, row_times);
  NLC_GUARD_END(c)
}

int group_step_entry(nlc_ctx* c, Family fam, const nlc_train_desc* desc, int M, int64_t data_rows, double* params, double* m,
                     double* v, int64_t step, const double* obs, const double* window, const double* ts,
                     const double* target, const int64_t* idx, int64_t N, int B, double* loss, double* gradnorm, void* ws,
                     int row_times = 0, bool per_member = false, const nlc_train_members* mem = nullptr) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (!desc) return fail(c, NLC_ERR_BAD_ARG, "NULL train desc");
  // (a _members entry: its struct and the four arrays count among the step's own pointers)
  const bool mem_null = per_member && (!mem || !mem->lr_dev || !mem->wd_dev || !mem->max_norm_dev || !mem->active_dev);
  Plan p;
  if (int rc = group_loss_grad(c, fam, M, data_rows, params, obs, window, ts, target, idx, N, B, nullptr, loss, ws, &p,
                               row_times, &step, !m || !v || mem_null))
    return rc;
  // only the last launch differs
  if (per_member) return adam_members(c, desc, mem, params, m, v, step, gradnorm, p, ws_ptrs(p, ws));
  return adam(c, desc, params, m, v, step, gradnorm, p, ws_ptrs(p, ws));
  NLC_GUARD_END(c)
}

// ---- held-out loss (kernels_train_eval.hip): the forward and the squared error of every member, then one reduction.  The
// checks are group_loss_grad's, in its order; idx may be NULL (rows 0 .. N - 1).  The workspace is the tile losses
// (nlc_train_eval.h eval_ws_layout), M regions back to back
int64_t group_eval_workspace_bytes(nlc_ctx* c, Family fam, int M, int64_t N) {
  if (!c || !family_has(c, fam) || N < 1 || M < 1 || M > kMaxGroup) return -1;
  // (de Hoog evaluates through the training step's forward half: its slabs and ILT arrays)
  if (fam == kFamNl && nl_dehoog(c)) return group_workspace_bytes(c, fam, M, N);
  return (int64_t)M * eval_ws_layout(N).total * (int64_t)sizeof(double);
}

int group_eval_entry(nlc_ctx* c, Family fam, int M, int64_t data_rows, const double* params, const double* obs,
                     const double* window, const double* ts, const double* target, const int64_t* idx, int64_t N, int B,
                     double* loss, void* ws, int row_times = 0) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (int rc = check_call(c, fam, M, data_rows, N, B)) return rc;
  if (!params || !obs || !window || (!ts && need_ts(c, fam)) || !target || !loss || !ws)
    return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  NLC_HIP(c, hipSetDevice(c->device));
  Plan p = family_plan(c, fam, N);
  const Batch b{params, obs, window, ts, target, idx, N};
  // the forward launch, and where it left member 0's tile losses: how many, and the doubles to the next member's
  EvalReduceArgs r{nullptr, 0, N, 0, p.d, loss};
  if (p.dehoog) {
    // launches 1 .. 3 of the training step on its own workspace layout (the forward tapes needlessly here)
    plan_group(p, M, N, data_rows);
    const WsPtrs w = ws_ptrs(p, ws);
    if (int rc = nl_dehoog_launches(c, b, B, p, w, false)) return rc;
    r.tile_loss = w.tile_loss;
    r.ntiles = p.nblk;
    r.ws = p.ws.total;
  } else {
    const EvalWsLayout w = eval_ws_layout(N);
    p.M = M;
    p.row_times = row_times;
    p.gs = GroupStrides{p.P, w.total, 0, N, data_rows};
    double* tile_loss = (double*)ws + w.tile_loss;
    if (int rc = (fam == kFamRnn ? rnn_eval : fam == kFamNode ? node_eval : nl_eval)(c, b, B, p, tile_loss)) return rc;
    r.tile_loss = tile_loss;
    r.ntiles = w.ntiles;
    r.ws = w.total;
  }
  // one reduction over each member's tile losses
  ProfScope ps(c, "eval_reduce_kernel");
  NLC_HIP(c, launch_eval_reduce(r, M, c->stream));
  return NLC_OK;
  NLC_GUARD_END(c)
}

}  // namespace

// ---- NeuralLaplaceModel.  A group (run_exp_multi.py:105-110: one model per (env, delay, model_name), times seeds) is M
// models of one descriptor: params / m / v / grad [M][P], idx [M][N], loss / gradnorm [M], data_row_stride 0 (one dataset)
// or the rows per member of a stacked one; the single entries are its M = 1 case
// train_utils.py:388-408, run_exp_multi.py:105-110
extern "C" int64_t nlc_train_group_workspace_bytes(nlc_ctx* c, int M, int64_t N) {
  return group_workspace_bytes(c, kFamNl, M, N);
}
// train_utils.py:391-402 per member, run_exp_multi.py:105-110
extern "C" int nlc_train_group_loss_grad(nlc_ctx* c, int M, int64_t data_row_stride, const double* params,
                                         const double* obs, const double* window, const double* ts, const double* target,
                                         const int64_t* idx, int64_t N, int B, double* grad, double* loss, void* ws) {
  return group_loss_grad_entry(c, kFamNl, M, data_row_stride, params, obs, window, ts, target, idx, N, B, grad, loss, ws);
}
// train_utils.py:391-404 per member, run_exp_multi.py:105-110
extern "C" int nlc_train_group_step(nlc_ctx* c, const nlc_train_desc* desc, int M, int64_t data_row_stride, double* params,
                                    double* m, double* v, int64_t step, const double* obs, const double* window,
                                    const double* ts, const double* target, const int64_t* idx, int64_t N, int B,
                                    double* loss, double* gradnorm, void* ws) {
  return group_step_entry(c, kFamNl, desc, M, data_row_stride, params, m, v, step, obs, window, ts, target, idx, N, B, loss,
                          gradnorm, ws);
}
// train_utils.py:388-408
extern "C" int64_t nlc_train_workspace_bytes(nlc_ctx* c, int64_t N) { return group_workspace_bytes(c, kFamNl, 1, N); }
// train_utils.py:391-402 (zero_grad, forward, MSELoss, backward)
extern "C" int nlc_train_loss_grad(nlc_ctx* c, const double* params, const double* obs, const double* window,
                                   const double* ts, const double* target, const int64_t* idx, int64_t N, int B,
                                   double* grad, double* loss, void* ws) {
  return group_loss_grad_entry(c, kFamNl, 1, 0, params, obs, window, ts, target, idx, N, B, grad, loss, ws);
}
// train_utils.py:391-404 (one whole iteration: + clip_grad_norm_ + optimizer.step())
extern "C" int nlc_train_step(nlc_ctx* c, const nlc_train_desc* desc, double* params, double* m, double* v, int64_t step,
                              const double* obs, const double* window, const double* ts, const double* target,
                              const int64_t* idx, int64_t N, int B, double* loss, double* gradnorm, void* ws) {
  return group_step_entry(c, kFamNl, desc, 1, 0, params, m, v, step, obs, window, ts, target, idx, N, B, loss, gradnorm, ws);
}

// ---- DeltaTRNN / RNN (train_utils.py:550-631): the same entries and contract; params, m, v flat in nlc_set_rnn_model's blob
// order; ts may be NULL for a model without time input
// train_utils.py:388-408, run_exp_multi.py:105-110
extern "C" int64_t nlc_rnn_train_group_workspace_bytes(nlc_ctx* c, int M, int64_t N) {
  return group_workspace_bytes(c, kFamRnn, M, N);
}
// train_utils.py:391-402 per member, run_exp_multi.py:105-110
extern "C" int nlc_rnn_train_group_loss_grad(nlc_ctx* c, int M, int64_t data_row_stride, const double* params,
                                             const double* obs, const double* window, const double* ts,
                                             const double* target, const int64_t* idx, int64_t N, int B, double* grad,
                                             double* loss, void* ws) {
  return group_loss_grad_entry(c, kFamRnn, M, data_row_stride, params, obs, window, ts, target, idx, N, B, grad, loss, ws);
}
// train_utils.py:391-404 per member, run_exp_multi.py:105-110
extern "C" int nlc_rnn_train_group_step(nlc_ctx* c, const nlc_train_desc* desc, int M, int64_t data_row_stride,
                                        double* params, double* m, double* v, int64_t step, const double* obs,
                                        const double* window, const double* ts, const double* target, const int64_t* idx,
                                        int64_t N, int B, double* loss, double* gradnorm, void* ws) {
  return group_step_entry(c, kFamRnn, desc, M, data_row_stride, params, m, v, step, obs, window, ts, target, idx, N, B, loss,
                          gradnorm, ws);
}
// train_utils.py:388-408
extern "C" int64_t nlc_rnn_train_workspace_bytes(nlc_ctx* c, int64_t N) { return group_workspace_bytes(c, kFamRnn, 1, N); }
// train_utils.py:391-402 (zero_grad, forward, MSELoss, backward)
extern "C" int nlc_rnn_train_loss_grad(nlc_ctx* c, const double* params, const double* obs, const double* window,
                                       const double* ts, const double* target, const int64_t* idx, int64_t N, int B,
                                       double* grad, double* loss, void* ws) {
  return group_loss_grad_entry(c, kFamRnn, 1, 0, params, obs, window, ts, target, idx, N, B, grad, loss, ws);
}
// train_utils.py:391-404 (one whole iteration: + clip_grad_norm_ + optimizer.step())
extern "C" int nlc_rnn_train_step(nlc_ctx* c, const nlc_train_desc* desc, double* params, double* m, double* v,
                                  int64_t step, const double* obs, const double* window, const double* ts,
                                  const double* target, const int64_t* idx, int64_t N, int B, double* loss, double* gradnorm,
                                  void* ws) {
  return group_step_entry(c, kFamRnn, desc, 1, 0, params, m, v, step, obs, window, ts, target, idx, N, B, loss, gradnorm, ws);
}

// ---- held-out loss of both families: the forward and MSE of the reference's validation loss on the training entries' data
// conventions; no gradient, no update.  loss [M]; idx may be NULL (rows 0 .. N - 1)
// overlay.py:112-115, :175-177, run_exp_multi.py:105-110
extern "C" int64_t nlc_train_group_eval_workspace_bytes(nlc_ctx* c, int M, int64_t N) {
  return group_eval_workspace_bytes(c, kFamNl, M, N);
}
// overlay.py:112-115, :175-177 per member, run_exp_multi.py:105-110
extern "C" int nlc_train_group_eval(nlc_ctx* c, int M, int64_t data_row_stride, const double* params, const double* obs,
                                    const double* window, const double* ts, const double* target, const int64_t* idx,
                                    int64_t N, int B, double* loss, void* ws) {
  return group_eval_entry(c, kFamNl, M, data_row_stride, params, obs, window, ts, target, idx, N, B, loss, ws);
}
// overlay.py:112-115, :175-177
extern "C" int64_t nlc_train_eval_workspace_bytes(nlc_ctx* c, int64_t N) { return group_eval_workspace_bytes(c, kFamNl, 1, N); }
// overlay.py:112-115, :175-177
extern "C" int nlc_train_eval(nlc_ctx* c, const double* params, const double* obs, const double* window, const double* ts,
                              const double* target, const int64_t* idx, int64_t N, int B, double* loss, void* ws) {
  return group_eval_entry(c, kFamNl, 1, 0, params, obs, window, ts, target, idx, N, B, loss, ws);
}
// overlay.py:112-115, :175-177, run_exp_multi.py:105-110
extern "C" int64_t nlc_rnn_train_group_eval_workspace_bytes(nlc_ctx* c, int M, int64_t N) {
  return group_eval_workspace_bytes(c, kFamRnn, M, N);
}
// overlay.py:112-115, :175-177 per member, run_exp_multi.py:105-110
extern "C" int nlc_rnn_train_group_eval(nlc_ctx* c, int M, int64_t data_row_stride, const double* params, const double* obs,
                                        const double* window, const double* ts, const double* target, const int64_t* idx,
                                        int64_t N, int B, double* loss, void* ws) {
  return group_eval_entry(c, kFamRnn, M, data_row_stride, params, obs, window, ts, target, idx, N, B, loss, ws);
}
// overlay.py:112-115, :175-177
extern "C" int64_t nlc_rnn_train_eval_workspace_bytes(nlc_ctx* c, int64_t N) { return group_eval_workspace_bytes(c, kFamRnn, 1, N); }
// overlay.py:112-115, :175-177
extern "C" int nlc_rnn_train_eval(nlc_ctx* c, const double* params, const double* obs, const double* window, const double* ts,
                                  const double* target, const int64_t* idx, int64_t N, int B, double* loss, void* ws) {
  return group_eval_entry(c, kFamRnn, 1, 0, params, obs, window, ts, target, idx, N, B, loss, ws);
}

// ---- NODE (train_utils.py:637-724): the RNN entries' signatures and contract plus row_times -- 0: every row of a member's batch
// integrates to the time of its first row, ts[idx[0]] (train_utils.py:719; what NODE.forward does), non-zero: each row to its
// own ts[idx[r]].  params, m, v flat in nlc_set_node_model's blob order; the model comes from nlc_set_node_model on the ctx.
// The workspace is a function of (M, N) and the shape alone: a row's sub-step count is at most 256, a row whose time is not
// positive or needs more gets a NaN squared error.  The single-model forms are M = 1, data_row_stride 0
// train_utils.py:388-408, run_exp_multi.py:105-110
extern "C" int64_t nlc_node_train_group_workspace_bytes(nlc_ctx* c, int M, int64_t N) {
  return group_workspace_bytes(c, kFamNode, M, N);
}
// train_utils.py:391-402 per member, run_exp_multi.py:105-110
extern "C" int nlc_node_train_group_loss_grad(nlc_ctx* c, int M, int64_t data_row_stride, const double* params,
                                              const double* obs, const double* window, const double* ts,
                                              const double* target, const int64_t* idx, int64_t N, int B, double* grad,
                                              double* loss, void* ws, int row_times) {
  return group_loss_grad_entry(c, kFamNode, M, data_row_stride, params, obs, window, ts, target, idx, N, B, grad, loss, ws,
                               row_times != 0);
}
// train_utils.py:391-404 per member, run_exp_multi.py:105-110
extern "C" int nlc_node_train_group_step(nlc_ctx* c, const nlc_train_desc* desc, int M, int64_t data_row_stride,
                                         double* params, double* m, double* v, int64_t step, const double* obs,
                                         const double* window, const double* ts, const double* target, const int64_t* idx,
                                         int64_t N, int B, double* loss, double* gradnorm, void* ws, int row_times) {
  return group_step_entry(c, kFamNode, desc, M, data_row_stride, params, m, v, step, obs, window, ts, target, idx, N, B, loss,
                          gradnorm, ws, row_times != 0);
}
// overlay.py:112-115, :175-177, run_exp_multi.py:105-110
extern "C" int64_t nlc_node_train_group_eval_workspace_bytes(nlc_ctx* c, int M, int64_t N) {
  return group_eval_workspace_bytes(c, kFamNode, M, N);
}
// overlay.py:112-115, :175-177 per member, run_exp_multi.py:105-110
extern "C" int nlc_node_train_group_eval(nlc_ctx* c, int M, int64_t data_row_stride, const double* params, const double* obs,
                                         const double* window, const double* ts, const double* target, const int64_t* idx,
                                         int64_t N, int B, double* loss, void* ws, int row_times) {
  return group_eval_entry(c, kFamNode, M, data_row_stride, params, obs, window, ts, target, idx, N, B, loss, ws, row_times != 0);
}

// ---- per-member settings (kernels_train_members.hip): the _group_step entries with lr, weight decay, clip norm and an active
// flag per member from device arrays [M]; desc gives the betas and eps (its lr, weight_decay and max_grad_norm are not read).
// The checks are the _group_step entries', in their order; a NULL struct or a NULL array in it is a NULL device pointer.  A
// member with active == 0 keeps its params / m / v untouched; its forward, backward, loss and gradnorm are still computed
// train_utils.py:391-404 per member, config.py (sweep_mode: learning_rate, weight_decay, clip_grad_norm)
extern "C" int nlc_train_group_step_members(nlc_ctx* c, const nlc_train_desc* desc, int M, int64_t data_row_stride,
                                            double* params, double* m, double* v, int64_t step, const double* obs,
                                            const double* window, const double* ts, const double* target, const int64_t* idx,
                                            int64_t N, int B, double* loss, double* gradnorm, void* ws,
                                            const nlc_train_members* members) {
  return group_step_entry(c, kFamNl, desc, M, data_row_stride, params, m, v, step, obs, window, ts, target, idx, N, B, loss,
                          gradnorm, ws, 0, true, members);
}
// train_utils.py:391-404 per member, config.py (sweep_mode)
extern "C" int nlc_rnn_train_group_step_members(nlc_ctx* c, const nlc_train_desc* desc, int M, int64_t data_row_stride,
                                                double* params, double* m, double* v, int64_t step, const double* obs,
                                                const double* window, const double* ts, const double* target,
                                                const int64_t* idx, int64_t N, int B, double* loss, double* gradnorm, void* ws,
                                                const nlc_train_members* members) {
  return group_step_entry(c, kFamRnn, desc, M, data_row_stride, params, m, v, step, obs, window, ts, target, idx, N, B, loss,
                          gradnorm, ws, 0, true, members);
}
// train_utils.py:391-404 per member, config.py (sweep_mode)
extern "C" int nlc_node_train_group_step_members(nlc_ctx* c, const nlc_train_desc* desc, int M, int64_t data_row_stride,
                                                 double* params, double* m, double* v, int64_t step, const double* obs,
                                                 const double* window, const double* ts, const double* target,
                                                 const int64_t* idx, int64_t N, int B, double* loss, double* gradnorm, void* ws,
                                                 int row_times, const nlc_train_members* members) {
  return group_step_entry(c, kFamNode, desc, M, data_row_stride, params, m, v, step, obs, window, ts, target, idx, N, B, loss,
                          gradnorm, ws, row_times != 0, true, members);
}

// the reference's waiting / patience counter per member, after nlc_train_keep_best in stream order; reads no model from the ctx
// train_utils.py:315-317, :439-448
extern "C" int nlc_train_patience(nlc_ctx* c, int M, const int32_t* improved, int64_t* waiting, int32_t* active,
                                  int64_t* stopped_at, double patience, int64_t tag) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (!improved || !waiting || !active || !stopped_at) return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  if (M < 1) return fail(c, NLC_ERR_BAD_SHAPE, "patience: a group needs M >= 1 members");
  if (M > kMaxGroup) return fail(c, NLC_ERR_UNSUPPORTED, "patience: at most 65535 members in a group");
  if (patience != patience) return fail(c, NLC_ERR_BAD_ARG, "patience: patience must not be NaN");
  NLC_HIP(c, hipSetDevice(c->device));
  const PatienceArgs a{improved, waiting, active, stopped_at, patience, tag, M};
  ProfScope ps(c, "train_patience_kernel");
  NLC_HIP(c, launch_train_patience(a, c->stream));
  return NLC_OK;
  NLC_GUARD_END(c)
}
