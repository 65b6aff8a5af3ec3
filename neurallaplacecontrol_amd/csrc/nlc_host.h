// Internal header of the host side of libnlc_hip.so (the abi_*.hip translation units): the context object behind the opaque
// nlc_ctx handle of include/nlc.h, status / HIP-error helpers, per-launch event profiling, and the few helpers more than one
// unit needs.  Nothing here is part of the ABI.
//   abi_ctx.hip         context, options, stream binding, device info, profiling read-out
//   abi_comm.hip        optional library-owned RCCL communicator (bound with dlopen)
//   abi_ilt.hip         stand-alone ILT entry points (laplace_reconstruct pieces) + tables of the linear algorithms
//   abi_model.hip       NL model upload (MFMA fragment packing), GRU encode, model forward, representation function
//   abi_baselines.hip   env step, Delta-t RNN and NODE baseline models
//   abi_planner.hip     nlc_mppi_*: configure, workspace layout, phase 1 (sampling + rollout), weights, finish
//   abi_planner_nl.hip  phase 1 with Neural-Laplace dynamics: staged (de Hoog / linear), one-launch fused body, two launches
//   abi_train.hip       fused training step, held-out loss and loss gradient of the NL and Delta-t RNN models (groups of them)
//   abi_train_select.hip  keep_best / restore_best: the best weights of a group's members, kept on the device
//   abi_synth.hip       synthetic transition dataset, generated on the device
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <time.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "nlc_devbuf.h"
#include "nlc_gru_prefix.h"
#include "nlc_kernels.h"
#include "nlc_pack.h"
#include "nlc_plan.h"

namespace nlc {
int nl_pick_nt3(int need);

namespace host {

struct ProfEntry {
  std::string name;
  double total_ms = 0.0;
  int64_t launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// a model's packed weights on the host, as one block for upload_arena
struct DeviceArena {
  std::vector<double> host;
  size_t push(const std::vector<double>& v) {
    // 64-double (512 B) alignment so every fragment row starts on a cache line
    const size_t off = (host.size() + 63) / 64 * 64;
    host.resize(off);
    host.insert(host.end(), v.begin(), v.end());
    return off;
  }
};

// ---- the planner's state, by group (members of nlc_ctx)

// nlc_set_option; defaults as documented in include/nlc.h
struct PlannerOptions {
  int rollout_variant = 0;          // 0 auto, 1 wave-per-tile, 2 latency-split (two launches), 3 fused one-launch body
  int repfunc_split = 1;            // staged de Hoog planner: latency-split representation kernel (h = 128)
  int gru_coop = -1;                // stand-alone GRU encodes: cooperative (one tile per workgroup) kernel 1 / 0, -1 auto
  int gru_prefix = -1;              // two-launch body, wave-per-tile encoder: clipped leading GRU steps from a table (nlc_gru_prefix.h): -1 auto, 0 / 1
  int gru_gemm = 0;                 // 1: encoder hidden-state GEMMs on the INT8 matrix pipe (kernels_gru_i8.hip), g == 64 only
  int horizon_chunks = 1;           // Fourier planner, wave-per-tile body (K > 8192): GRU encode of later horizon chunks beside the rollout of earlier ones
  int dehoog_gru_chunks = 0;        // staged de Hoog planner: GRU encode in this many horizon chunks beside the step chain (0 / 1: one launch up front)
  int dehoog_gru_lds_pad = 49152;   // unused dynamic LDS of those chunk launches (bytes): 32 KB + 48 KB -> two workgroups per CU
  int dehoog_chain = -1;            // de Hoog planner: the step chain as one persistent launch (kernels_dehoog_chain.hip): -1 auto, 0 / 1
  int dehoog_chain_phases = 3;      // tools only: 1 / 2 = only the representation / QD phase of the chain kernel runs (timing)
  int dehoog_streams = 0;           // staged de Hoog planner: parts of the population on streams of their own (0 auto)
  int linear_fused = 1;             // fixed Talbot / Stehfest models: LIN instances of the rollout kernels (0: the staged path)
  int train_dehoog = 0;             // training entries: 1 = de Hoog NL models take the fused step (kernels_train_dehoog.hip); 0: refused
  int node_method = 0;              // every NODE entry: the fixed-grid solver (nlc_node_rk.h): 0 euler, 1 midpoint, 2 rk4
  int host_spin = 1;                // nlc_mppi_finish with a host action pointer: 1 spin on a pinned word the merge kernel
                                    // stores, 2 sleep through the predicted wait first, 0 hipStreamSynchronize
  double host_spin_margin_us = 150.0;  // host_spin 2: the host wakes this long (or 15 % of the predicted wait) before the predicted end
  // fused one-launch body.  fused.blocks_per_cu: 0 auto (3 while chains sit on at most half of the CUs, else 4), 3 or 4;
  // fused.roll_cap: 0 auto (one chain per 16-sample tile, at most one per CU); fused.chain_first_tiles: tiles per wave a chain's
  // workgroup encodes before it starts walking (-1 auto); fused.partner_tiles: tiles per wave after which a chain's CU partner
  // sleeps (-1: never, -2 auto); fused.tile_step_ratio > 0: the adaptive partner rule (measured slower:
  // profiles/r3_fused_small_shard.md), 0 = static schedule
  nlc::plan::FusedKnobs fused;
  int64_t fused_max_samples = 4096; // auto: populations up to this size take the fused body (one chain per CU at most)
  int fused_inline = 3;             // sampling / bounding and the weight reduction inside the launch
  int64_t fused_spin_limit = 1 << 18;  // polls (~2 us each) before a waiting wave of the fused body gives up (~0.5 s)
  int fused_keep_sync = 0;          // tools only: the merge kernel leaves the sync block as the launch left it (timeline dumps)
  int fused_test_drop_tile = -1;    // tests only: this encoder tile is never published (forces the timeout path)
  double test_lin_coeff_scale = 1.0;  // tests only: the largest w_re / t coefficient of the LIN fragments is scaled by this
  // tools only (tools/rollout_giveback.py): something BETWEEN the encoder launch and the rollout launch of the two-launch body
  double dbg_gap_us = 0.0;          // one wavefront spinning on the constant 100 MHz counter for this long (an idle GPU)
  double dbg_l2_mb = 0.0;           // a read sweep over this many MB of scratch (evicts the L2s)
};

// the fused one-launch body's occupancy cache, sync-block bookkeeping and give-up record
struct FusedState {
  int blocks_per_cu = -1;        // occupancy of the fused kernel's 4-per-CU instance (queried once per hidden width)
  int blocks_per_cu3 = -1;       // ... of its 3-per-CU instance
  int occ_h = 0;                 // hidden width the two occupancies were queried for
  bool lost = false;             // a fused command gave up (hand-off timeout): later commands take the two-launch body
  int64_t fallbacks = 0;         // commands re-run on the two-launch body after such a timeout
  int64_t timeouts = 0;          // fused launches of THIS ctx that gave up (re-run or lost)
  int64_t last_giveup_command = -1;  // value of nlc_ctx::commands (0-based) at the last give-up seen by this ctx, -1 = none
  const void* sync_clean_ws = nullptr;  // workspace whose fused sync block the last merge kernel left zeroed
  bool sync_dirty = false;       // a fused launch has used the sync block since
  // the last command's inputs, kept for a re-run on the two-launch body (nlc_mppi_finish, after a fused timeout)
  struct LastCommand {
    bool valid = false, inline_inputs = false, fused = false;
    int state_per_sample = 0, rng = 0;
    uint64_t seed = 0, counter = 0;
    double state_in[NLC_MAX_D] = {0};
    double abuf_in[nlc::kMaxInlineAbuf] = {0};
  } last;
  // nlc_mppi_configure: nothing of the previous problem's commands is left to clean up after or to replay.  The occupancy
  // cache (a property of the model's width), `lost` and the counters (of the ctx's life) stay.
  void new_problem() {
    sync_clean_ws = nullptr;
    sync_dirty = false;
    last.valid = false;
  }
  // nlc_set_option "rollout_variant": an explicit choice re-arms the fused body after a timeout
  void rearm() { lost = false; }
};

// de Hoog planner, "dehoog_chain" and "dehoog_streams" both on auto: the chain's form is measured over the planner's first
// commands (abi_planner_nl.hip; the decision rule is nlc_plan.h dehoog_pick)
struct DehoogCalib {
  int n = 0, choice = -1, pending = -1, pending_round = 0;
  double t0 = 0.0;
  float ms[3][2] = {{1e30f, 1e30f}, {1e30f, 1e30f}, {1e30f, 1e30f}};  // [candidate][round & 1]: the last two rounds
  hipEvent_t ev[2] = {nullptr, nullptr};
  // nlc_mppi_configure: measured again for the new problem (the event pair is kept)
  void reset() {
    n = 0;
    choice = pending = -1;
    for (auto& v : ms) v[0] = v[1] = 1e30f;
  }
  void destroy() {
    for (hipEvent_t& e : ev) {
      if (e) hipEventDestroy(e);
      e = nullptr;
    }
  }
};

// "gru_prefix" (nlc_gru_prefix.h): the table sits in the model's arena (c->nl.arena, reserved by nlc_set_model) and is built by
// nlc_mppi_configure -- a new model, other bounds / u_scale / normalisation or another B all pass through there; the window
// lists and their counters are the ctx's own buffer, grown at the first command that needs it
struct GruPrefixState {
  size_t arena_off = 0;          // table, out_tab, the table build's 16 synthetic windows and the products, in doubles from the arena's base
  const char* why_not = "gru_prefix: planner not configured";  // out of scope (nullptr: the table is built)
  unsigned long long img_max = 0, img_min = 0;
  DevDoubles lists;              // counters (one 64-double row) + kLists lists
  bool last_used = false;        // the last command's encoder launch started from the table
  int last_B = 0;
};

// host_spin: the wait for the action in nlc_mppi_finish
struct HostWait {
  unsigned long long seq = 0;  // sequence number of the last command handed to the spin protocol (never reset: the pinned word
                               // keeps the last one stored)
  double hist_us[8] = {0};     // the last waits for the action (their minimum predicts the next one)
  int hist_n = 0, hist_at = 0;
  double nap_margin_us = 0.0;  // host_spin 2: the margin in use (grows when a nap overshoots the action's arrival)
  // nlc_mppi_configure, nlc_set_option "host_spin": a new problem size or mode, a new wait to predict
  void reset() {
    hist_n = hist_at = 0;
    nap_margin_us = 0.0;
  }
};

// streams and events beside the ctx's stream, created on first use and kept until nlc_destroy
struct SideStreams {
  hipStream_t gru_stream = nullptr;      // GRU encode in horizon chunks (low priority)
  std::vector<hipEvent_t> ev_gru;        // ... latents of chunk ch are there
  std::vector<hipStream_t> aux_streams;  // staged step chain: parts 1 .. P-1 of the population
  hipEvent_t ev_fork = nullptr;
  std::vector<hipEvent_t> ev_join;
  hipEvent_t stage_ev = nullptr;         // recorded after the staged H2D copies of a command
  void destroy() {
    if (stage_ev) hipEventDestroy(stage_ev);
    if (ev_fork) hipEventDestroy(ev_fork);
    for (hipEvent_t e : ev_join) hipEventDestroy(e);
    for (hipStream_t s : aux_streams) hipStreamDestroy(s);
    for (hipEvent_t e : ev_gru) hipEventDestroy(e);
    if (gru_stream) hipStreamDestroy(gru_stream);
    *this = SideStreams{};
  }
};

// ---- the uploaded models, by family (members of nlc_ctx).  A setter builds a local group and moves it into the ctx once
// every check, allocation and copy has succeeded: the move frees the previous model's buffers, and a fresh group's defaults
// are what a new model invalidates inside the group.  Outside it the setter clears has_mppi (RNN / NODE: of their own
// dynamics) and, for NL, the gru_prefix table.  The pointers inside gru / net / rnn / node are kernel arguments.
struct NlModel {
  bool has = false;
  nlc_model_desc md{};
  int g = 0, S = 0, P = 0;
  DevDoubles arena;     // packed weights + the room of the gru_prefix table
  nlc::GruArgs gru{};   // weight pointers + normalisation filled in
  nlc::NlNetArgs net{}; // general-t variant (b1 = raw bias)
  std::vector<double> W1s_host, b1_host;  // for folding the constant sphere inputs (fold_b1)
  DevInts slot_dev;                       // (8*nt3) layer-3 slot -> c*S + k (de Hoog path)
  DevInts eidx_dev;                       // (d*S) inverse: term k of dim c -> slot (slot-major F of the planner path)
  std::vector<std::pair<int, int>> slot_elems;  // (dim, term) of every layer-3 slot (nlc_pack.h)
  DevDoubles lin_tab;                     // nodes / weights of the linear ILT algorithms, cached per (algo, terms)
  int lin_algo = -1, lin_S = 0;
  DevDoubles b1fold;                      // (h): layer 1's bias with the sphere inputs of the planner's ts_pred folded in
  DevDoubles cp_lin;                      // [2][2 nt3][64]: w_re / t and -w_im / t coefficient fragments (configure time)
  DevDoubles b1fold_fwd;                  // (h): the same fold for nlc_model_forward_const_t's query time
  double fwd_tn = -1.0;                   // normalised time b1fold_fwd was folded for
  std::vector<double> fwd_fold_host;      // its host copy (kept alive for the asynchronous upload)
};

// Delta-t RNN baseline
struct RnnModel {
  bool has = false;
  nlc_rnn_desc rd{};
  DevDoubles arena;
  nlc::RnnArgs rnn{};
  nlc::RnnHead rnn_head{};
};

// NODE baseline
struct NodeModel {
  bool has = false;
  nlc_node_desc nd{};
  DevDoubles arena;
  nlc::NodeNetArgs node{};
  int node_ht = 0;
};

}  // namespace host
}  // namespace nlc

struct nlc_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  hipDeviceProp_t prop;

  // models
  nlc::host::NlModel nl;
  nlc::host::RnnModel rnnm;
  nlc::host::NodeModel nodem;

  // planner
  bool has_mppi = false;
  nlc_mppi_desc pd{};
  nlc::host::DevDoubles U[2];
  int ucur = 0;
  nlc::host::DevDoubles small;  // action (<= T*nu) + beta_eta (2)
  double tn = 0.0;
  int nblk = 0;
  int64_t commands = 0;                 // nlc_mppi_rollout calls since nlc_create
  int last_body = 0;                    // body phase 1 of the last command ran on (nlc_get_stat "rollout_body")

  bool profiling = false;
  std::vector<nlc::host::ProfEntry> prof;
  std::vector<hipEvent_t> event_pool;

  // pinned host block of the configured planner (nlc_plan.h): staging for the per-command small transfers, the action, and the
  // control words the kernels store
  nlc::host::PinnedDoubles pinned;
  nlc::plan::PinLayout pin{};
  // the planner's state by group; each group's reset rule is its own (who calls which: nlc_mppi_configure, nlc_set_option,
  // nlc_destroy)
  nlc::host::PlannerOptions opt;
  nlc::host::FusedState fused;
  nlc::host::DehoogCalib dh;
  nlc::host::HostWait wait;
  nlc::host::SideStreams side;
  nlc::host::GruPrefixState prefix;
  // tools only (options "dbg_gap_us" / "dbg_l2_mb")
  nlc::host::DevDoubles dbg_scratch;
  // optional native collective (nlc_comm_init): an RCCL communicator over the ranks of a K-sharded planner
  void* comm = nullptr;
  int comm_world = 0, comm_rank = 0;
  nlc::host::DevDoubles comm_gather;  // (world, E, 2+T*nu) receive buffer of the per-command all-gather
};

namespace nlc {
namespace host {

extern thread_local std::string g_create_error;  // nlc_last_error(NULL): failures before a ctx exists

inline int fail(nlc_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define NLC_HIP(c, expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess)                                                                         \
      return fail((c), NLC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
  } while (0)

#define NLC_GUARD_BEGIN try {
#define NLC_GUARD_END(c)                                                       \
  }                                                                            \
  catch (const std::exception& e) {                                            \
    return fail((c), NLC_ERR_STATE, std::string("exception: ") + e.what());    \
  }                                                                            \
  catch (...) {                                                                \
    return fail((c), NLC_ERR_STATE, "unknown exception");                      \
  }

// ---- profiling: hipEvent pair around one launch, on the launch stream
struct ProfScope {
  nlc_ctx* c;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ProfEntry* entry = nullptr;
  hipEvent_t take_event() {
    if (!c->event_pool.empty()) {
      hipEvent_t e = c->event_pool.back();
      c->event_pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
  }
  hipStream_t st;
  ProfScope(nlc_ctx* ctx, const char* name, hipStream_t stream = nullptr, bool use_given = false)
      : c(ctx), st(use_given ? stream : ctx->stream) {
    if (!c->profiling) return;
    for (auto& p : c->prof)
      if (p.name == name) entry = &p;
    if (!entry) {
      c->prof.push_back(ProfEntry{});
      c->prof.back().name = name;
      entry = &c->prof.back();
    }
    e0 = take_event();
    e1 = take_event();
    hipEventRecord(e0, st);
  }
  ~ProfScope() {
    if (!entry) return;
    hipEventRecord(e1, st);
    entry->pending.emplace_back(e0, e1);
    entry->launches += 1;
  }
};

void prof_flush(nlc_ctx* c);

struct Blob {
  const double* p;
  int64_t left;
  const double* take(int64_t n) {
    if (n > left) throw std::runtime_error("weight blob too short");
    const double* r = p;
    p += n;
    left -= n;
    return r;
  }
};

bool is_device_ptr(const void* p);
// b holds exactly n elements, copied from src (a synchronous copy); a failure leaves it empty
template <class T>
int upload(nlc_ctx* c, Buf<T, DeviceMem>& b, const T* src, size_t n) {
  NLC_HIP(c, (hipError_t)b.hold(n));
  const hipError_t e = hipMemcpy(b.get(), src, n * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) b.reset();
  return e == hipSuccess ? NLC_OK : fail(c, NLC_ERR_HIP, std::string("weight upload: ") + hipGetErrorString(e));
}
inline int upload_arena(nlc_ctx* c, const DeviceArena& ar, DevDoubles& b) { return upload(c, b, ar.host.data(), ar.host.size()); }
bool gru_use_coop(const nlc_ctx* c, int64_t n_windows);
// the window-mode GRU encode of N windows of B actions -> out (N, 2), on the ctx's stream
int encode_windows(nlc_ctx* c, const double* window, int64_t N, int B, double* out);

// ---- abi_ilt.hip
int check_ilt(nlc_ctx* c, const nlc_ilt_desc* d);
// fixed Talbot / Stehfest: the two algorithms that are linear in F (nodes and weights from linear_tables)
inline bool is_linear_ilt(const nlc_ilt_desc& ilt) { return ilt.algo == NLC_ILT_FIXED_TALBOT || ilt.algo == NLC_ILT_STEHFEST; }
// the term counts the de Hoog kernels take (any count goes for the other algorithms)
inline int check_dehoog_terms(nlc_ctx* c, const nlc_ilt_desc& ilt) {
  if (ilt.algo == NLC_ILT_DEHOOG && (ilt.terms < 3 || ilt.terms > 33 || ilt.terms % 2 == 0))
    return fail(c, NLC_ERR_UNSUPPORTED, "dehoog: ilt_reconstruction_terms must be odd, 3 .. 33 (2M+1 terms)");
  return NLC_OK;
}
void sphere_inputs(const nlc_ilt_desc& ilt, double tn, std::vector<double>& sph);
// layer 1's bias of model m with the constant sphere inputs of the normalised time tn folded in (nlc_devbuf.h)
inline void fold_b1(const NlModel& m, double tn, std::vector<double>& out) {
  std::vector<double> sph;
  sphere_inputs(m.md.ilt, tn, sph);
  fold_b1(m.W1s_host.data(), m.b1_host.data(), m.md.h, m.S, sph.data(), out);
}
void linear_tables_host(int algo, int S, std::vector<double>& h);
int linear_tables(nlc_ctx* c, const nlc_ilt_desc* d, const double** tab);
// The ILT kernels' argument blocks, filled by name: the arrays, the shape and the contour's options, with t_div = 1,
// t_stride = 1 and everything else zero / NULL.  A call site then sets what its algorithm adds (fre / fim, eidx, lin_wr /
// lin_wi, t_div, t_stride, scratch); the launchers set rpp / iters.
template <class A>
inline A ilt_args_common(const nlc_ilt_desc& ilt, const double* theta, const double* phi, const double* t, int64_t N, int d) {
  A a{};
  a.theta = theta;
  a.phi = phi;
  a.t = t;
  a.N = N;
  a.d = d;
  a.S = ilt.terms;
  a.alpha = ilt.alpha;
  a.log_tol = std::log(ilt.tol);
  a.scale = ilt.scale;
  return a;
}
inline IltArgs ilt_args(const nlc_ilt_desc& ilt, const double* theta, const double* phi, const double* t, double* x, int64_t N,
                        int d) {
  IltArgs a = ilt_args_common<IltArgs>(ilt, theta, phi, t, N, d);
  a.x = x;
  a.t_div = 1.0;
  a.t_stride = 1;
  return a;
}
template <class A = IltBwdArgs>
inline A ilt_bwd_args(const nlc_ilt_desc& ilt, const double* theta, const double* phi, const double* t, const double* gx,
                      double* gtheta, double* gphi, int64_t N, int d) {
  A a = ilt_args_common<A>(ilt, theta, phi, t, N, d);
  a.gx = gx;
  a.gtheta = gtheta;
  a.gphi = gphi;
  return a;
}
inline IltDehoogBwdArgs ilt_dehoog_bwd_args(const nlc_ilt_desc& ilt, const double* theta, const double* phi, const double* t,
                                            const double* gx, double* gtheta, double* gphi, int64_t N, int d, void* scratch) {
  IltDehoogBwdArgs a = ilt_bwd_args<IltDehoogBwdArgs>(ilt, theta, phi, t, gx, gtheta, gphi, N, d);
  a.t_div = 1.0;
  a.scratch = scratch;
  return a;
}

// ---- abi_baselines.hip
int node_substeps(double t_end, double step, double* h, int max_n);

// ---- abi_comm.hip: RCCL, bound at run time
struct Rccl {
  typedef struct { char internal[NLC_COMM_ID_BYTES]; } UniqueId;  // = ncclUniqueId (rccl.h: 128 opaque bytes)
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;  // the id is passed BY VALUE (rccl.h)
  int (*CommDestroy)(void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  std::string why;
  bool ok = false;
};
Rccl* rccl();
constexpr int kNcclFloat64 = 8;  // rccl.h: ncclFloat64 = ncclDouble = 8

// ---- abi_planner.hip
bool linear_on_rollout_kernels(const nlc_ctx* c);
struct WsLayout {
  size_t tile_part, chunk_part, pa, state0, abuf, xcarry, ccarry, fre, fim, dx, tconst, rq, sync, total;
};
WsLayout ws_layout(const nlc_ctx* c);
// the control words of the pinned block (nlc_plan.h PinLayout)
inline unsigned* pin_giveup_word(nlc_ctx* c) { return reinterpret_cast<unsigned*>(c->pinned.get() + c->pin.giveup); }
inline unsigned long long* pin_seq_word(nlc_ctx* c) { return reinterpret_cast<unsigned long long*>(c->pinned.get() + c->pin.seq); }
inline unsigned* pin_merge_status_word(nlc_ctx* c) { return reinterpret_cast<unsigned*>(c->pinned.get() + c->pin.merge_status); }
WeightArgs make_weight_args(nlc_ctx* c, const nlc_mppi_buffers* buf);
int run_weights(nlc_ctx* c, const nlc_mppi_buffers* buf);
// The configured cost variant, 0 with cost_external; a flipped bit without NLC_COST_CHANGE_GOAL selects nothing.
inline int cost_variant_of(const nlc_mppi_desc& d) {
  if (d.cost_external || !(d.cost_variant & (NLC_COST_STATE_CONSTRAINT | NLC_COST_CHANGE_GOAL))) return 0;
  return d.cost_variant;
}
// A cost variant runs INSIDE the latency-split rollout and the one-launch body, on their CV
// instances (cost_in_body puts env and the bits into the argument block).  Every other body leaves the running cost out
// (env = -1, as for the caller's own cost with cost_external) and variant_cost_kernel evaluates it on the stored states
// before the weights (finish_rollout_costs with in_body = false).
template <class A>
void cost_in_body(A& a, const nlc_mppi_desc& d) {
  if (cost_variant_of(d)) {
    a.env = d.env;
    a.cost_variant = cost_variant_of(d);
  }
}
int finish_rollout_costs(nlc_ctx* c, const nlc_mppi_buffers* buf, bool in_body = false);

// One phase-1 call (nlc_mppi_rollout, or its re-run after a fused time-out) as the dynamics-specific parts see it
struct RolloutCall {
  const nlc_mppi_buffers* buf;
  PerturbArgs p;         // sampling / bounding arguments, filled in by the caller
  WsLayout w;
  double* ws;            // buf->workspace
  double* state_dev;     // staged state(s) and action buffer(s) inside the workspace
  double* abuf_dev;
  int64_t KE;            // all local samples, episode-major
  int state_per_sample, rng;
  bool inline_inputs;    // state and action_buffer ride in the perturb kernel's arguments
  bool replay;           // re-run of the last command on the two-launch body
};
int launch_shift_perturb(nlc_ctx* c, RolloutCall& call);
SampleCostArgs sample_cost_args(const nlc_ctx* c, const RolloutCall& call);  // once the shifted U is current
// ---- abi_planner_nl.hip
int rollout_nl(nlc_ctx* c, RolloutCall& call);
// "gru_prefix": the table of a freshly configured NL planner (or the reason there is none); doubles nlc_set_model reserves
int gru_prefix_configure(nlc_ctx* c);
// table, out_tab (62), the build's windows; then the products (a multiple of 4 doubles from the base: v4d loads)
inline size_t gru_prefix_products_off(int g) { return (size_t)nlc::prefix::kEntries * 2 * g + 64 + (size_t)16 * nlc::prefix::kMaxB; }
inline size_t gru_prefix_arena_doubles(int g) {
  return gru_prefix_products_off(g) + (size_t)nlc::prefix::products_doubles(g);
}

}  // namespace host
}  // namespace nlc
