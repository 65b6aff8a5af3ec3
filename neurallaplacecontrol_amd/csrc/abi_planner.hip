// Host side of libnlc_hip.so, planner unit: MPPIDelay behind nlc_mppi_* (planners/mppi_delay.py:64-224) -- configure,
// workspace layout, phase 1 (sampling / bounding + the T-step rollout; Neural-Laplace dynamics in abi_planner_nl.hip),
// importance weights, and the merge / hand-over of phase 2.
#include "nlc_host.h"

using namespace nlc;
using namespace nlc::host;

extern "C" int nlc_mppi_configure(nlc_ctx* c, const nlc_mppi_desc* d) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (!d) return fail(c, NLC_ERR_BAD_ARG, "NULL desc");
  if (d->K < 1 || d->T < 1 || d->K_global < d->K || d->k_offset < 0 || d->k_offset + d->K > d->K_global)
    return fail(c, NLC_ERR_BAD_SHAPE, "bad K / K_global / k_offset / T");
  if (d->nu < 1 || d->nu > NLC_MAX_NU) return fail(c, NLC_ERR_UNSUPPORTED, "nu must be 1 or 2");
  // (caller-supplied dynamics: the library never touches a state, any nx goes)
  if (d->d < 1 || (d->d > NLC_MAX_D && d->dynamics != NLC_DYN_EXTERNAL)) return fail(c, NLC_ERR_BAD_SHAPE, "bad nx");
  if (d->B < 1) return fail(c, NLC_ERR_BAD_SHAPE, "action_buffer needs at least one row");
  if (!(d->lambda_ > 0.0) || d->u_scale == 0.0) return fail(c, NLC_ERR_BAD_ARG, "lambda_ must be > 0, u_scale != 0");
  if (d->u_per_command < 1 || d->u_per_command > d->T) return fail(c, NLC_ERR_BAD_ARG, "bad u_per_command");
  if (d->E < 0 || d->E > 65535) return fail(c, NLC_ERR_BAD_ARG, "episodes E must be in [0, 65535]");
  const int E = d->E < 1 ? 1 : d->E;
  if ((double)E * (double)d->K * d->T * d->nu > 2.0e9)
    return fail(c, NLC_ERR_BAD_SHAPE, "E*K*T*nu exceeds the planner's index range");
  // the env id selects the running cost and the oracle dynamics; with cost_external and NL dynamics nothing needs it
  const bool env_free = d->cost_external &&
                        (d->dynamics == NLC_DYN_NL || d->dynamics == NLC_DYN_DTRNN || d->dynamics == NLC_DYN_NODE) &&
                        d->env == -1;
  if (!env_free && (d->env < 0 || d->env > NLC_ENV_CARTPOLE_NOTRIG)) return fail(c, NLC_ERR_UNSUPPORTED, "unknown env id");
  static const int env_d[4] = {5, 3, 6, 4}, env_nu[4] = {1, 1, 2, 1};
  if (!env_free && d->dynamics != NLC_DYN_EXTERNAL && (d->d != env_d[d->env] || d->nu != env_nu[d->env]))
    return fail(c, NLC_ERR_BAD_SHAPE, "nx / nu do not match the env's observation");
  // the state_constraint / change_goal branches exist in the cartpole env class only (ctcartpole.py:311-329)
  if (d->cost_variant & ~NLC_COST_VARIANT_MASK) return fail(c, NLC_ERR_BAD_SHAPE, "unknown cost_variant bits");
  if (d->cost_variant != 0 && !d->cost_external && d->env != NLC_ENV_CARTPOLE && d->env != NLC_ENV_CARTPOLE_NOTRIG)
    return fail(c, NLC_ERR_UNSUPPORTED, "cost_variant: only the cartpole envs have a state_constraint / change_goal cost");
  if (d->cost_external && d->dynamics == NLC_DYN_EXTERNAL)
    return fail(c, NLC_ERR_BAD_ARG, "cost_external needs fused dynamics (NLC_DYN_NL / NLC_DYN_ORACLE / NLC_DYN_DTRNN)");
  if (d->dynamics == NLC_DYN_EXTERNAL) {
    // the caller owns dynamics and cost
  } else if (d->dynamics == NLC_DYN_NL) {
    if (!c->nl.has) return fail(c, NLC_ERR_STATE, "NL dynamics need nlc_set_model first");
    // nin == nu + 1: an encode_obs_time model; the rollout appends the harness's constant time channel
    if (c->nl.md.d != d->d || (c->nl.md.nin != d->nu && c->nl.md.nin != d->nu + 1))
      return fail(c, NLC_ERR_BAD_SHAPE, "model state/action dims differ from the planner's");
    if (int rc = check_dehoog_terms(c, c->nl.md.ilt)) return rc;
  } else if (d->dynamics == NLC_DYN_ORACLE) {
    if (d->delay < 0 || d->delay > d->B - 1)
      return fail(c, NLC_ERR_BAD_ARG, "oracle dynamics: delay must be in [0, action_buffer_size-1]");
  } else if (d->dynamics == NLC_DYN_DTRNN) {
    if (!c->rnnm.has) return fail(c, NLC_ERR_STATE, "Delta-t RNN dynamics need nlc_set_rnn_model first");
    if (c->rnnm.rd.d != d->d || c->rnnm.rd.nin != d->nu)
      return fail(c, NLC_ERR_BAD_SHAPE, "model state/action dims differ from the planner's");
  } else if (d->dynamics == NLC_DYN_NODE) {
    if (!c->nodem.has) return fail(c, NLC_ERR_STATE, "NODE dynamics need nlc_set_node_model first");
    if (c->nodem.nd.d != d->d || c->nodem.nd.nu != d->nu)
      return fail(c, NLC_ERR_BAD_SHAPE, "model state/action dims differ from the planner's");
    double h[8];
    if (node_substeps(d->ts_pred / c->nodem.nd.time_div, c->nodem.nd.step_size, h, 8) < 0)
      return fail(c, NLC_ERR_UNSUPPORTED, "ts_pred needs more than 8 sub-steps of the solver's grid (or is <= 0)");
  } else {
    return fail(c, NLC_ERR_UNSUPPORTED, "unknown dynamics id");
  }
  NLC_HIP(c, hipSetDevice(c->device));
  const size_t un = (size_t)E * d->T * d->nu;
  for (int i = 0; i < 2; ++i) {
    NLC_HIP(c, (hipError_t)c->U[i].hold(un));
    // on the ctx's stream and waited for below: hipMemset runs asynchronously on the NULL stream, which is not
    // ordered against a non-blocking stream -- it could land after the nlc_mppi_set_U copy that follows configure
    NLC_HIP(c, hipMemsetAsync(c->U[i].get(), 0, un * sizeof(double), c->stream));
  }
  NLC_HIP(c, hipStreamSynchronize(c->stream));
  c->ucur = 0;
  NLC_HIP(c, (hipError_t)c->small.hold(un + 2 * (size_t)E));
  c->pin = plan::pin_layout(E, d->d, d->B, d->nu, d->T);
  NLC_HIP(c, (hipError_t)c->pinned.grow(c->pin.total));
  std::memset(c->pinned.get(), 0, c->pinned.size() * sizeof(double));
  c->pd = *d;
  c->pd.E = E;
  c->nblk = weight_tiles(d->K);
  if (d->dynamics == NLC_DYN_NL) {
    // constant prediction time => the 2S sphere-coordinate inputs of layer 1 are constants: fold into the bias
    c->tn = d->ts_pred / c->nl.md.time_div;
    const int S = c->nl.S;
    std::vector<double> bf;
    fold_b1(c->nl, c->tn, bf);
    if (int rc = upload(c, c->nl.b1fold, bf.data(), bf.size())) return rc;
    if (is_linear_ilt(c->nl.md.ilt)) {
      // coefficient fragments of the LIN rollout instances: lane -> (dim = lane & 15, slot 4 g + (lane >> 4)), as Cp
      std::vector<double> tab;
      linear_tables_host(c->nl.md.ilt.algo, S, tab);
      const int ng = 2 * c->nl.net.nt3;
      std::vector<double> cp((size_t)2 * ng * 64, 0.0);
      for (int g = 0; g < ng; ++g)
        for (int lane = 0; lane < 64; ++lane) {
          const auto el = c->nl.slot_elems[(size_t)4 * g + (lane >> 4)];
          if (el.first != (lane & 15)) continue;
          cp[(size_t)g * 64 + lane] = tab[2 * S + el.second] / c->tn;
          cp[(size_t)(ng + g) * 64 + lane] = -tab[3 * S + el.second] / c->tn;
        }
      if (c->opt.test_lin_coeff_scale != 1.0) {  // tests only: the sweep's tolerance must catch this
        size_t at = 0;
        for (size_t i = 0; i < cp.size(); ++i)
          if (std::fabs(cp[i]) > std::fabs(cp[at])) at = i;
        cp[at] *= c->opt.test_lin_coeff_scale;  // (the largest weight: Stehfest's span many orders of magnitude)
      }
      if (int rc = upload(c, c->nl.cp_lin, cp.data(), cp.size())) return rc;
    }
  }
  c->prefix.last_used = false;
  if (d->dynamics == NLC_DYN_NL)
    if (int rc = gru_prefix_configure(c)) return rc;
  c->has_mppi = true;
  c->dh.reset();
  c->wait.reset();
  c->fused.new_problem();
  return NLC_OK;
  NLC_GUARD_END(c)
}

namespace nlc {
namespace host {
// fixed Talbot / Stehfest models whose rollout runs on the LIN instances of the rollout kernels (launch_nl_rollout_ht<HT, true>,
// at the widths of with_width in nlc_kernels.h) instead of the staged path
bool linear_on_rollout_kernels(const nlc_ctx* c) {
  return c->nl.has && is_linear_ilt(c->nl.md.ilt) &&
         (c->nl.md.h == 64 || c->nl.md.h == 128 || c->nl.md.h == 256) && c->opt.linear_fused != 0;
}

WsLayout ws_layout(const nlc_ctx* c) {
  const nlc_mppi_desc& d = c->pd;
  WsLayout w{};
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 63) / 64 * 64;
    return o;
  };
  const size_t KE = (size_t)d.K * d.E;  // all local samples
  w.tile_part = take((size_t)d.E * c->nblk * (2 + (size_t)d.T * d.nu));
  w.chunk_part = take((size_t)d.E * ((c->nblk + 63) / 64) * (2 + (size_t)d.T * d.nu));
  w.pa = take(d.dynamics == NLC_DYN_NL ? KE * d.T * 2 : 0);
  w.state0 = take(d.dynamics == NLC_DYN_EXTERNAL ? 0 : KE * d.d);
  w.abuf = take((size_t)d.E * d.B * d.nu);
  w.xcarry = take(d.dynamics == NLC_DYN_NL ? KE * d.d : 0);
  w.ccarry = take(d.dynamics == NLC_DYN_NL ? KE * 2 : 0);
  // (the staged buffers are laid out for every non-Fourier model, also when a linear-algorithm model runs on the LIN rollout
  // instances: the layout must not depend on an option that can change after the caller sized its workspace)
  const bool staged = d.dynamics == NLC_DYN_NL && c->nl.md.ilt.algo != NLC_ILT_FOURIER;
  // slot-major (8*nt3, KE), >= KE*d*S; the persistent step chain cuts it into private (8*nt3) x 64 blocks, one per 64 samples
  const size_t KE64 = (KE + 63) / 64 * 64;
  w.fre = take(staged ? KE64 * 8 * (size_t)c->nl.net.nt3 : 0);
  w.fim = take(staged ? KE64 * 8 * (size_t)c->nl.net.nt3 : 0);
  w.dx = take(staged ? KE * d.d : 0);
  w.tconst = take(staged ? 8 : 0);
  w.rq = take(d.dynamics == NLC_DYN_DTRNN ? KE * d.T * d.d : 0);  // hidden part of linear_out, (T, K, d)
  // fused one-launch planner body: tickets, per-CU census, one flag word per encoder tile (unsigned words)
  w.sync = take(d.dynamics == NLC_DYN_NL && !staged ? (fused_sync_words(d.T, (int64_t)KE) + 1) / 2 : 0);
  w.total = off;
  return w;
}

// Give-up bookkeeping of the fused body, once per look at the pinned block: reads and clears the word a rollout workgroup of
// the fused body sets when it gives up waiting for an encoder tile (`lost_here`) and the word merge_kernel sets when a gathered
// partial row is marked invalid (kPartialInvalidEta; `marked`: some rank gave up).  A give-up here puts the ctx on the
// two-launch body.  `command`: index of the command the words speak of; `count_marked`: a row another rank marked is a give-up
// this ctx saw as well (nlc_mppi_finish, which then re-runs the command; nlc_mppi_rollout records only its own).
struct GiveUp {
  bool lost_here, marked;
  bool any() const { return lost_here || marked; }
};
static bool take_word(unsigned* w) {
  if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == 0u) return false;
  *w = 0u;
  return true;
}
static GiveUp take_give_up(nlc_ctx* c, int64_t command, bool count_marked) {
  GiveUp g{};
  g.lost_here = take_word(pin_giveup_word(c));
  g.marked = take_word(pin_merge_status_word(c));
  if (g.lost_here) {
    c->fused.lost = true;
    c->fused.timeouts += 1;
  }
  if (g.lost_here || (g.marked && count_marked)) c->fused.last_giveup_command = command;
  return g;
}

WeightArgs make_weight_args(nlc_ctx* c, const nlc_mppi_buffers* buf) {
  const nlc_mppi_desc& d = c->pd;
  const WsLayout w = ws_layout(c);
  double* ws = (double*)buf->workspace;
  WeightArgs wa{};
  wa.Kep = d.K;
  wa.E = d.E;
  wa.T = d.T;
  wa.nu = d.nu;
  wa.lambda_ = d.lambda_;
  wa.cost = buf->cost_total;
  wa.noise = buf->noise;
  wa.tile_part = ws + w.tile_part;
  wa.chunk_part = ws + w.chunk_part;
  wa.partials = buf->partials;
  wa.nblk = c->nblk;
  return wa;
}

// what follows a rollout that left the running cost out: nothing for the caller's own cost (cost_external: it calls
// nlc_mppi_weights), else the cost variant's kernel on the stored states and the importance weights
int finish_rollout_costs(nlc_ctx* c, const nlc_mppi_buffers* buf, bool in_body) {
  const nlc_mppi_desc& d = c->pd;
  if (d.cost_external) return NLC_OK;
  if (cost_variant_of(d) && !in_body) {
    if (!buf->states) return fail(c, NLC_ERR_BAD_ARG, "this rollout body evaluates a cost_variant on buf->states");
    VariantCostArgs v{d.K * d.E, d.T, d.nu, d.d, d.env, cost_variant_of(d), d.u_scale, buf->states, buf->perturbed, buf->cost_total};
    ProfScope ps(c, "variant_cost_kernel");
    NLC_HIP(c, launch_variant_cost(v, c->stream));
  }
  return run_weights(c, buf);
}

int run_weights(nlc_ctx* c, const nlc_mppi_buffers* buf) {
  WeightArgs wa = make_weight_args(c, buf);
  // behind a fused launch that left the fold to us: its give-up word marks the partial rows here -- the launch of
  // THIS command only; a re-run on the two-launch body (last_body 2) must not read the word the failed launch left set
  if (c->last_body == 3 && buf->workspace && c->pd.dynamics == NLC_DYN_NL)
    wa.gave_up = reinterpret_cast<const unsigned*>((const double*)buf->workspace + ws_layout(c).sync) + kFusedTimeout;
  ProfScope ps(c, "weight_kernels");
  NLC_HIP(c, launch_weights(wa, c->stream));
  return NLC_OK;
}

// one launch: the perturb kernel shifts U on the fly (every (k, t) thread reads U_old[t + 1]; the episode's first local sample
// stores the shifted row) and stores the staged inputs; shift_U_kernel only when there is nothing to perturb
int launch_shift_perturb(nlc_ctx* c, RolloutCall& call) {
  PerturbArgs& p = call.p;
  p.fused_shift = (int64_t)p.K * p.T > 0;
  if (!p.fused_shift) {
    ProfScope ps(c, "shift_U_kernel");
    NLC_HIP(c, launch_shift_U(p, c->stream));
  }
  ProfScope ps(c, "perturb_kernel");
  NLC_HIP(c, launch_perturb(p, c->stream));
  return NLC_OK;
}

// the samples and the cost terms of the command's rollout, whichever body runs it; c->U[c->ucur].get() is the shifted sequence
SampleCostArgs sample_cost_args(const nlc_ctx* c, const RolloutCall& call) {
  const nlc_mppi_desc& d = c->pd;
  SampleCostArgs a{};
  a.K = call.KE;
  a.Kep = d.K;
  a.T = d.T;
  a.nu = d.nu;
  a.env = (d.cost_external || cost_variant_of(d)) ? -1 : d.env;  // (a variant's CV bodies: cost_in_body)
  a.state_per_sample = call.state_per_sample;
  a.state0 = call.state_dev;
  a.perturbed = call.buf->perturbed;
  a.noise = call.buf->noise;
  a.U = c->U[c->ucur].get();
  for (int i = 0; i < NLC_MAX_NU * NLC_MAX_NU; ++i) a.sigma_inv[i] = d.noise_sigma_inv[i];
  a.lambda_ = d.lambda_;
  a.u_scale = d.u_scale;
  a.noise_abs_cost = d.noise_abs_cost;
  a.states = call.buf->states;
  a.cost_total = call.buf->cost_total;
  return a;
}

// the command's sampling / bounding, apart from the inline inputs; c->U[c->ucur].get() is the sequence BEFORE the shift
PerturbArgs perturb_args(const nlc_ctx* c, const nlc_mppi_buffers* buf, int rng, uint64_t seed, uint64_t counter) {
  const nlc_mppi_desc& d = c->pd;
  PerturbArgs p{};
  p.K = d.K * d.E;  // all local samples, episode-major
  p.Kep = d.K;
  p.E = d.E;
  p.K_global = d.K_global;
  p.k_offset = d.k_offset;
  p.T = d.T;
  p.nu = d.nu;
  p.U_old = c->U[c->ucur].get();
  p.U_new = c->U[c->ucur ^ 1].get();
  p.noise = buf->noise;
  p.perturbed = buf->perturbed;
  p.actions = buf->actions;
  p.u_scale = d.u_scale;
  p.has_bounds = d.has_bounds;
  p.sample_null_action = d.sample_null_action;
  p.rng = rng;
  for (int i = 0; i < NLC_MAX_NU; ++i) {
    p.u_min[i] = d.u_min[i];
    p.u_max[i] = d.u_max[i];
    p.u_init[i] = d.u_init[i];
    p.mu[i] = d.noise_mu[i];
  }
  for (int i = 0; i < NLC_MAX_NU * NLC_MAX_NU; ++i) p.chol[i] = d.noise_chol[i];
  p.seed = seed;
  p.counter = counter;
  return p;
}

// phase 2 over the partial rows of G ranks; c->U[c->ucur].get() is the shifted sequence.  The pinned action, the sequence word and
// the sync block's clean-up are the caller's decisions.
MergeArgs merge_args(nlc_ctx* c, const nlc_mppi_buffers* buf, const double* gathered, int G, int rank) {
  const nlc_mppi_desc& d = c->pd;
  MergeArgs m{};
  m.Kep = d.K;
  m.E = d.E;
  m.T = d.T;
  m.nu = d.nu;
  m.G = G;
  m.rank = rank;
  m.u_per_command = d.u_per_command;
  m.lambda_ = d.lambda_;
  m.u_scale = d.u_scale;
  m.gathered = gathered;
  m.U = c->U[c->ucur].get();
  m.cost_nz = buf->cost_nz;
  m.omega = buf->omega;
  m.action = buf->action ? buf->action : c->small.get();
  m.beta_eta = c->small.get() + (size_t)d.E * d.T * d.nu;
  m.cost = buf->cost_total;
  m.status_pinned = pin_merge_status_word(c);
  return m;
}
}  // namespace host
}  // namespace nlc

extern "C" int64_t nlc_mppi_workspace_bytes(nlc_ctx* c) {
  if (!c || !c->has_mppi) return -1;
  return (int64_t)(ws_layout(c).total * sizeof(double));
}

extern "C" int nlc_mppi_set_U(nlc_ctx* c, const double* U) {
  if (!c) return NLC_ERR_BAD_ARG;
  if (!c->has_mppi) return fail(c, NLC_ERR_STATE, "planner not configured");
  if (!U) return fail(c, NLC_ERR_BAD_ARG, "NULL U");
  NLC_HIP(c, hipSetDevice(c->device));
  NLC_HIP(c, hipMemcpyAsync(c->U[c->ucur].get(), U, (size_t)c->pd.E * c->pd.T * c->pd.nu * sizeof(double), hipMemcpyHostToDevice,
                            c->stream));
  NLC_HIP(c, hipStreamSynchronize(c->stream));
  return NLC_OK;
}

extern "C" int nlc_mppi_set_goal_flipped(nlc_ctx* c, int flipped) {
  if (!c) return NLC_ERR_BAD_ARG;
  if (!c->has_mppi) return fail(c, NLC_ERR_STATE, "planner not configured");
  if (c->pd.env != NLC_ENV_CARTPOLE && c->pd.env != NLC_ENV_CARTPOLE_NOTRIG)
    return fail(c, NLC_ERR_UNSUPPORTED, "change_goal_flipped: only the cartpole envs have a change_goal cost");
  if (!(c->pd.cost_variant & NLC_COST_CHANGE_GOAL))
    return fail(c, NLC_ERR_STATE, "change_goal_flipped: the planner was not configured with NLC_COST_CHANGE_GOAL");
  // sample_cost_args reads the descriptor at every command: the next rollout's launches carry the new bit
  c->pd.cost_variant = flipped ? (c->pd.cost_variant | NLC_COST_GOAL_FLIPPED) : (c->pd.cost_variant & ~NLC_COST_GOAL_FLIPPED);
  return NLC_OK;
}

extern "C" int nlc_mppi_get_U(nlc_ctx* c, double* U) {
  if (!c) return NLC_ERR_BAD_ARG;
  if (!c->has_mppi) return fail(c, NLC_ERR_STATE, "planner not configured");
  if (!U) return fail(c, NLC_ERR_BAD_ARG, "NULL U");
  NLC_HIP(c, hipSetDevice(c->device));
  NLC_HIP(c, hipMemcpyAsync(U, c->U[c->ucur].get(), (size_t)c->pd.E * c->pd.T * c->pd.nu * sizeof(double), hipMemcpyDeviceToHost,
                            c->stream));
  NLC_HIP(c, hipStreamSynchronize(c->stream));
  return NLC_OK;
}

// The command's state(s) and action buffer(s) into the workspace (dynamics the library runs; not on a replay), or
// *inline_inputs: they ride in the perturb kernel's arguments
static int stage_inputs(nlc_ctx* c, RolloutCall& call, const double* state, const double* abuf_host, bool* inline_inputs) {
  const nlc_mppi_desc& d = c->pd;
  const int state_per_sample = call.state_per_sample;
  double* state_dev = call.state_dev;
  double* abuf_dev = call.abuf_dev;
  if (d.E > 1) {
    // batched episodes: the (E,d) states and (E,B,nu) action buffers usually live on the device already (a device-side
    // env loop); hipMemcpyDefault takes either kind of pointer
    const size_t ns = (size_t)(state_per_sample ? call.KE : d.E) * d.d;
    NLC_HIP(c, hipMemcpyAsync(state_dev, state, ns * sizeof(double), hipMemcpyDefault, c->stream));
    NLC_HIP(c, hipMemcpyAsync(abuf_dev, abuf_host, (size_t)d.E * d.B * d.nu * sizeof(double), hipMemcpyDefault,
                              c->stream));
    // a caller-owned HOST buffer may be a temporary: the copies out of it must have completed before we return
    if (!is_device_ptr(state) || !is_device_ptr(abuf_host)) NLC_HIP(c, hipStreamSynchronize(c->stream));
  } else if (!state_per_sample && d.B * d.nu <= kMaxInlineAbuf) {
    *inline_inputs = true;  // state and action_buffer travel in the shift kernel's arguments (below)
  } else {
    // small inputs go through pinned staging (truly asynchronous copies).  The staging slots are rewritten
    // only after the previous command's copies out of them have completed (stage_ev).
    if (c->side.stage_ev) NLC_HIP(c, hipEventSynchronize(c->side.stage_ev));
    double* pin_state = c->pinned.get() + c->pin.state;
    double* pin_abuf = c->pinned.get() + c->pin.abuf;
    std::memcpy(pin_abuf, abuf_host, (size_t)d.B * d.nu * sizeof(double));
    if (state_per_sample) {
      // (K, d) from caller-owned pageable memory: wait for the copy, the source may be a temporary
      NLC_HIP(c, hipMemcpyAsync(state_dev, state, (size_t)d.K * d.d * sizeof(double), hipMemcpyHostToDevice, c->stream));
      NLC_HIP(c, hipStreamSynchronize(c->stream));
    } else {
      std::memcpy(pin_state, state, (size_t)d.d * sizeof(double));
      NLC_HIP(c, hipMemcpyAsync(state_dev, pin_state, (size_t)d.d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    NLC_HIP(c, hipMemcpyAsync(abuf_dev, pin_abuf, (size_t)d.B * d.nu * sizeof(double), hipMemcpyHostToDevice,
                              c->stream));
    if (!c->side.stage_ev) NLC_HIP(c, hipEventCreateWithFlags(&c->side.stage_ev, hipEventDisableTiming));
    NLC_HIP(c, hipEventRecord(c->side.stage_ev, c->stream));
  }
  return NLC_OK;
}

// the rollout of the baseline dynamics: NODE, Delta-t RNN (encode launch + rollout launch), oracle
static int rollout_baseline(nlc_ctx* c, RolloutCall& call) {
  const nlc_mppi_desc& d = c->pd;
  c->last_body = d.dynamics == NLC_DYN_NODE ? 8 : (d.dynamics == NLC_DYN_DTRNN ? 7 : 6);
  const SampleCostArgs sc = sample_cost_args(c, call);
  if (d.dynamics == NLC_DYN_NODE) {
    NodeRolloutArgs r{sc};
    r.net = c->nodem.node;
    r.net.nsub = node_substeps(d.ts_pred / c->nodem.nd.time_div, c->nodem.nd.step_size, r.net.hsub, 8);
    ProfScope ps(c, "node_rollout_kernel");
    NLC_HIP(c, launch_node_rollout(r, c->nodem.node_ht, c->opt.node_method, c->stream));
  } else if (d.dynamics == NLC_DYN_DTRNN) {
    RnnArgs g = c->rnnm.rnn;
    g.mode = 1;
    g.perturbed = call.buf->perturbed;
    g.abuf = call.abuf_dev;
    g.u_scale = d.u_scale;
    g.T = d.T;
    g.B = d.B;
    g.Kep = d.K;
    g.K = call.KE;
    g.N = call.KE * d.T;
    g.out = call.ws + call.w.rq;
    {
      ProfScope ps(c, "rnn_encode_kernel");
      NLC_HIP(c, launch_rnn_encode(g, c->rnnm.rd.hidden, c->stream));
    }
    RnnRolloutArgs r{sc};
    r.head = c->rnnm.rnn_head;
    r.q = g.out;
    r.ts = d.ts_pred;
    ProfScope ps(c, "rnn_rollout_kernel");
    NLC_HIP(c, launch_rnn_rollout(r, c->stream));
  } else {
    OracleRolloutArgs r{sc};
    r.B = d.B;
    r.d = d.d;
    r.delay = d.delay;
    r.friction = d.friction;
    r.dyn_env = d.env;
    r.abuf = call.abuf_dev;
    r.ts = d.ts_pred;
    ProfScope ps(c, "oracle_rollout_kernel");
    NLC_HIP(c, launch_oracle_rollout(r, c->stream));
  }
  return NLC_OK;
}

// Phase 1 of a command.  `replay`: the command's fused launch gave up (hand-off timeout) -- run it again on the two-launch
// body from the inputs kept in c->fused.last / still staged in the workspace (nlc_mppi_finish).
static int mppi_rollout_impl(nlc_ctx* c, const double* state, int state_per_sample, const double* abuf_host,
                             const nlc_mppi_buffers* buf, int rng, uint64_t seed, uint64_t counter, bool replay) {
  NLC_GUARD_BEGIN
  if (!c->has_mppi) return fail(c, NLC_ERR_STATE, "planner not configured");
  const nlc_mppi_desc& d = c->pd;
  const bool external = d.dynamics == NLC_DYN_EXTERNAL;
  if ((!external && (!state || !abuf_host)) || !buf) return fail(c, NLC_ERR_BAD_ARG, "NULL argument");
  if (!buf->noise || !buf->perturbed || !buf->cost_total || !buf->cost_nz || !buf->partials || !buf->workspace)
    return fail(c, NLC_ERR_BAD_ARG, "NULL required device buffer");
  if (d.cost_external && !buf->states) return fail(c, NLC_ERR_BAD_ARG, "cost_external needs buf->states");
  NLC_HIP(c, hipSetDevice(c->device));
  if (!replay) c->commands += 1;
  c->last_body = 0;
  if (!replay) {  // (a device-resident caller never synchronised inside nlc_mppi_finish)
    // `marked` is set on every rank of a sharded planner: they all fail here, none waits in a collective
    if (take_give_up(c, c->commands - 2 /* the command before this one */, false).any())
      return fail(c, NLC_ERR_HIP, "fused planner body: the PREVIOUS command timed out waiting inside the launch (on this or "
                                  "another rank; its action was NaN and U was left alone); later commands run the two-launch body");
  }
  RolloutCall call{};
  call.buf = buf;
  call.w = ws_layout(c);
  call.ws = (double*)buf->workspace;
  call.state_dev = call.ws + call.w.state0;
  call.abuf_dev = call.ws + call.w.abuf;
  call.KE = d.K * d.E;  // all local samples, episode-major
  call.state_per_sample = state_per_sample;
  call.rng = rng;
  call.replay = replay;
  double* state_dev = call.state_dev;
  double* abuf_dev = call.abuf_dev;
  bool inline_inputs = false;
  if (replay)
    inline_inputs = c->fused.last.inline_inputs;  // otherwise the inputs are still staged in the workspace
  else if (!external)
    if (int rc = stage_inputs(c, call, state, abuf_host, &inline_inputs)) return rc;
  PerturbArgs& p = call.p;
  p = perturb_args(c, buf, rng, seed, counter);
  if (inline_inputs) {
    p.n_state_in = d.d;
    p.n_abuf_in = d.B * d.nu;
    p.state_dst = state_dev;
    p.abuf_dst = abuf_dev;
    std::memcpy(p.state_in, state, (size_t)d.d * sizeof(double));
    std::memcpy(p.abuf_in, abuf_host, (size_t)d.B * d.nu * sizeof(double));
  }
  if (!replay) {
    FusedState::LastCommand& L = c->fused.last;
    L.valid = !external;
    L.inline_inputs = inline_inputs;
    L.fused = false;
    L.state_per_sample = state_per_sample;
    L.rng = rng;
    L.seed = seed;
    L.counter = counter;
    if (inline_inputs) {
      std::memcpy(L.state_in, p.state_in, sizeof(L.state_in));
      std::memcpy(L.abuf_in, p.abuf_in, sizeof(L.abuf_in));
    }
  }
  c->ucur ^= 1;  // from here on c->U[c->ucur].get() is the shifted sequence the kernels below produce
  call.inline_inputs = inline_inputs;
  const bool lin_direct = d.dynamics == NLC_DYN_NL && linear_on_rollout_kernels(c);
  const bool nl_fourier = d.dynamics == NLC_DYN_NL && (c->nl.md.ilt.algo == NLC_ILT_FOURIER || lin_direct);  // one rollout kernel
  // (the fused planner body's argument block carries the sampling arguments to the device itself: rollout_nl launches the
  // perturb kernel on the paths that still need it)
  if (!nl_fourier)
    if (int rc2 = launch_shift_perturb(c, call)) return rc2;
  if (external) {
    c->last_body = 9;
    return NLC_OK;  // the caller runs the horizon loop, then nlc_mppi_weights
  }
  if (d.dynamics == NLC_DYN_NL) return rollout_nl(c, call);
  if (int rc = rollout_baseline(c, call)) return rc;
  return finish_rollout_costs(c, buf);
  NLC_GUARD_END(c)
}

extern "C" int nlc_mppi_rollout(nlc_ctx* c, const double* state, int state_per_sample, const double* abuf_host,
                                const nlc_mppi_buffers* buf, int rng, uint64_t seed, uint64_t counter) {
  if (!c) return NLC_ERR_BAD_ARG;
  return mppi_rollout_impl(c, state, state_per_sample, abuf_host, buf, rng, seed, counter, false);
}

extern "C" int nlc_mppi_weights(nlc_ctx* c, const nlc_mppi_buffers* buf) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (!c->has_mppi) return fail(c, NLC_ERR_STATE, "planner not configured");
  if (!buf || !buf->noise || !buf->cost_total || !buf->cost_nz || !buf->partials || !buf->workspace)
    return fail(c, NLC_ERR_BAD_ARG, "NULL required device buffer");
  NLC_HIP(c, hipSetDevice(c->device));
  return run_weights(c, buf);
  NLC_GUARD_END(c)
}

namespace {

// the library's own collective: one all-gather of this rank's partial rows on the command's stream
int native_all_gather(nlc_ctx* c, const nlc_mppi_buffers* buf, int G, int rank, const double** gathered) {
  const nlc_mppi_desc& d = c->pd;
  if (!c->comm) return fail(c, NLC_ERR_BAD_ARG, "gathered_dev is NULL and no communicator (nlc_comm_init)");
  if (G != c->comm_world || rank != c->comm_rank) return fail(c, NLC_ERR_BAD_ARG, "G / rank differ from the communicator's");
  if (!buf->partials) return fail(c, NLC_ERR_BAD_ARG, "NULL buf->partials");
  const size_t per_rank = (size_t)d.E * (size_t)(2 + d.T * d.nu);
  NLC_HIP(c, (hipError_t)c->comm_gather.grow(per_rank * (size_t)G));
  ProfScope ps(c, "rccl_all_gather");
  const int rc = rccl()->AllGather(buf->partials, c->comm_gather.get(), per_rank, kNcclFloat64, c->comm, c->stream);
  if (rc != 0) return fail(c, NLC_ERR_COMM, std::string("ncclAllGather: ") + rccl()->GetErrorString(rc));
  *gathered = c->comm_gather.get();
  return NLC_OK;
}

inline double now_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3;
}

// Host wait for the action of a single planner.  host_spin 1: spin on the pinned sequence word the merge kernel stores
// behind the action.  host_spin 2: sleep through most of the command first -- the shortest of the last eight waits predicts
// this one -- and spin only for the rest: the core is free for the harness's other workers (run_exp_multi.py:145 fans out a
// Pool(12) over one GPU) at the price of a timer wake-up when the prediction is off.  host_spin 0 / batched planners /
// profiling: hipStreamSynchronize (which, measured, busy-waits as well: profiles/r4_host_spin_contention.json).
int wait_for_action(nlc_ctx* c, bool spin, const unsigned long long* seq_word) {
  if (spin) {
    const unsigned long long want = c->wait.seq;
    const double t0 = now_us();
    if (c->opt.host_spin == 2 && c->wait.hist_n >= 2) {
      double pred = c->wait.hist_us[0];
      for (int i = 1; i < c->wait.hist_n; ++i) pred = pred < c->wait.hist_us[i] ? pred : c->wait.hist_us[i];
      double margin = pred * 0.15 > c->opt.host_spin_margin_us ? pred * 0.15 : c->opt.host_spin_margin_us;
      if (c->wait.nap_margin_us > margin) margin = c->wait.nap_margin_us;  // grown by earlier oversleeps (below)
      const double nap = pred - margin;
      if (nap >= 50.0 && __atomic_load_n(seq_word, __ATOMIC_ACQUIRE) != want) {
        timespec req;
        req.tv_sec = (time_t)(nap * 1e-6);
        req.tv_nsec = (long)((nap - (double)req.tv_sec * 1e6) * 1e3);
        nanosleep(&req, nullptr);
        // the timer's wake-up latency is the host's, not ours to know: if the action was already there when we woke, the nap
        // was too long -- wake earlier from now on; while it is not, drift back towards the configured margin
        if (__atomic_load_n(seq_word, __ATOMIC_ACQUIRE) == want)
          c->wait.nap_margin_us = margin * 1.5 + 20.0;
        else
          c->wait.nap_margin_us = margin * 0.995;
      }
    }
    for (unsigned long long it = 0; it < 400000000ull; ++it) {  // ~ seconds: then fall back to the runtime's wait
      // acquire: the action words the kernel stored BEFORE the sequence number are read after it
      if (__atomic_load_n(seq_word, __ATOMIC_ACQUIRE) == want) {
        c->wait.hist_us[c->wait.hist_at] = now_us() - t0;
        c->wait.hist_at = (c->wait.hist_at + 1) % 8;
        if (c->wait.hist_n < 8) c->wait.hist_n += 1;
        return NLC_OK;
      }
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
  }
  NLC_HIP(c, hipStreamSynchronize(c->stream));
  return NLC_OK;
}

}  // namespace

extern "C" int nlc_mppi_finish(nlc_ctx* c, const double* gathered, int G, int rank, const nlc_mppi_buffers* buf,
                               double* action_host) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  if (!c->has_mppi) return fail(c, NLC_ERR_STATE, "planner not configured");
  if (!buf || !buf->cost_nz) return fail(c, NLC_ERR_BAD_ARG, "NULL argument");
  if (!action_host && !buf->action) return fail(c, NLC_ERR_BAD_ARG, "neither action_host nor buf->action given");
  if (G < 1 || rank < 0 || rank >= G) return fail(c, NLC_ERR_BAD_ARG, "bad G / rank");
  const nlc_mppi_desc& d = c->pd;
  NLC_HIP(c, hipSetDevice(c->device));
  const bool native = gathered == nullptr;
  if (native)
    if (int rc = native_all_gather(c, buf, G, rank, &gathered)) return rc;
  if (!buf->cost_total) return fail(c, NLC_ERR_BAD_ARG, "NULL buf->cost_total");
  MergeArgs m = merge_args(c, buf, gathered, G, rank);
  // the returned action is stored by the kernel straight into pinned (host-coherent) memory: the only thing left
  // on the host's critical path is the wait for it
  double* pin_act = c->pinned.get() + c->pin.action;
  m.action_pinned = action_host ? pin_act : nullptr;
  unsigned long long* seq_word = pin_seq_word(c);
  const bool spin = action_host && c->opt.host_spin && d.E == 1 && !c->profiling;
  auto launch_merge_now = [&]() -> int {
    if (spin) {
      m.seq_pinned = seq_word;
      m.seq = ++c->wait.seq;
    }
    if (c->fused.sync_dirty && buf->workspace && !c->opt.fused_keep_sync) {
      // last launch of the command: leave the fused body's tickets / flags zeroed for the next one
      m.zero_words = reinterpret_cast<unsigned*>((double*)buf->workspace + ws_layout(c).sync);
      m.n_zero_words = (int64_t)fused_sync_words(d.T, d.K * d.E);
    }
    ProfScope ps(c, "merge_kernel");
    NLC_HIP(c, launch_merge(m, c->stream));
    if (m.zero_words) {
      c->fused.sync_clean_ws = buf->workspace;
      c->fused.sync_dirty = false;
    }
    return NLC_OK;
  };
  if (int rc = launch_merge_now()) return rc;
  if (!action_host) return NLC_OK;  // device-resident caller: no wait; a lost command surfaces at the next nlc_mppi_rollout
  const size_t na = (size_t)d.E * d.u_per_command * d.nu;
  if (int rc = wait_for_action(c, spin, seq_word)) return rc;
  // A wave of the fused body gave up waiting for another workgroup of its launch (the device was not this planner's alone,
  // or fewer workgroups were resident than the host assumed): that launch's results are not valid.
  //   * here: the pinned give-up word is set; this ctx runs the two-launch body from now on;
  //   * on ANY rank of a sharded planner: the shard's partial row is marked (kPartialInvalidEta) and travels through the
  //     all-gather, so merge_kernel on EVERY rank has skipped the update and set the merge-status word.
  // Every rank therefore takes the same decision: re-run the command on the two-launch body from the inputs the ctx keeps
  // (the control sequence's ping-pong partner is untouched), gather again, merge again.
  const GiveUp gu = take_give_up(c, c->commands - 1 /* this command */, true);
  if (gu.any()) {
    if (G > 1 && !gu.marked)  // (a sharded command whose weights were folded outside the launch: the peers cannot know)
      return fail(c, NLC_ERR_HIP, "fused planner body: a workgroup timed out waiting inside the launch and the shard's partials "
                                  "were not marked; command lost (later commands run the two-launch body)");
    if (d.cost_external || !c->fused.last.valid || !buf->workspace || !buf->partials)
      return fail(c, NLC_ERR_HIP, "fused planner body: a workgroup timed out waiting inside the launch; command lost "
                                  "(later commands run the two-launch body)");
    c->fused.fallbacks += 1;
    c->ucur ^= 1;  // back to the control sequence before this command's shift
    const FusedState::LastCommand L = c->fused.last;
    if (int rc = mppi_rollout_impl(c, L.state_in, L.state_per_sample, L.abuf_in, buf, L.rng, L.seed, L.counter, true)) return rc;
    m.U = c->U[c->ucur].get();
    if (G == 1) {
      m.gathered = buf->partials;
    } else if (native) {
      if (int rc = native_all_gather(c, buf, G, rank, &gathered)) return rc;
      m.gathered = gathered;
    } else {
      // the caller owns the collective: buf->partials hold the re-run's values -- gather them again, call again
      c->err = "the command was re-run on the two-launch body: all-gather buf->partials again and call nlc_mppi_finish again";
      return NLC_AGAIN;
    }
    if (int rc = launch_merge_now()) return rc;
    if (int rc = wait_for_action(c, spin, seq_word)) return rc;
    if (take_word(pin_merge_status_word(c))) return fail(c, NLC_ERR_STATE, "partials still marked invalid after the re-run");
  }
  std::memcpy(action_host, pin_act, na * sizeof(double));
  return NLC_OK;
  NLC_GUARD_END(c)
}
