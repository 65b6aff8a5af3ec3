// Host side of libnlc_hip.so, planner unit, Neural-Laplace dynamics: phase 1 of a command after the sampling arguments are
// set (abi_planner.hip) -- the hoisted GRU encode and one of three rollout forms: the staged step chain (de Hoog and, as an
// option, fixed Talbot / Stehfest models), the one-launch fused body of a small shard, or GRU launch + rollout launch.
#include "nlc_host.h"

using namespace nlc;
using namespace nlc::host;

namespace {

// tools only (options "dbg_gap_us" / "dbg_l2_mb", tools/rollout_giveback.py): what sits between the encoder launch and the rollout
// launch when the question is what the SECOND kernel inherits from the first -- clocks, cache contents
__global__ void dbg_spin_kernel(unsigned long long ticks_100mhz) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks_100mhz) __builtin_amdgcn_s_sleep(8);
}
__global__ void dbg_touch_kernel(const double* __restrict__ p, size_t n, double* __restrict__ sink) {
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc += p[i];
  if (acc == 12345.678) *sink = acc;
}
int dbg_between(nlc_ctx* c) {
  if (c->opt.dbg_gap_us > 0.0) hipLaunchKernelGGL(dbg_spin_kernel, dim3(1), dim3(64), 0, c->stream, (unsigned long long)(c->opt.dbg_gap_us * 100.0));
  if (c->opt.dbg_l2_mb > 0.0) {
    const size_t bytes = (size_t)(c->opt.dbg_l2_mb * 1048576.0);
    const size_t n = bytes / 8 + 1;  // the sweep's doubles and its sink
    if (c->dbg_scratch.size() < n) {
      NLC_HIP(c, (hipError_t)c->dbg_scratch.hold(n));
      NLC_HIP(c, hipMemsetAsync(c->dbg_scratch.get(), 0, n * sizeof(double), c->stream));
    }
    hipLaunchKernelGGL(dbg_touch_kernel, dim3(2048), dim3(256), 0, c->stream, c->dbg_scratch.get(), bytes / 8, c->dbg_scratch.get() + bytes / 8);
  }
  return NLC_OK;
}

inline double now_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + (double)ts.tv_nsec * 1e-9;
}

// the context's fork / join events and side streams are created on first use and kept: this one if it is still null ...
int ensure(nlc_ctx* c, hipEvent_t& e) {
  if (!e) NLC_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return NLC_OK;
}
int ensure(nlc_ctx* c, hipStream_t& s) {
  if (!s) NLC_HIP(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return NLC_OK;
}
// ... or a vector of them grown to n
template <class H>
int grow(nlc_ctx* c, std::vector<H>& v, int n) {
  while ((int)v.size() < n) {
    H h = nullptr;
    if (int rc = ensure(c, h)) return rc;
    v.push_back(h);
  }
  return NLC_OK;
}

// the block's fields into an argument block that spells them out itself (RolloutArgs, DehoogChainArgs: nlc_kernels.h); Kep,
// which the latter has not, is the caller's
template <class A>
void put_sample_cost(A& a, const SampleCostArgs& s) {
  a.K = s.K;
  a.T = s.T;
  a.nu = s.nu;
  a.env = s.env;
  a.state_per_sample = s.state_per_sample;
  a.state0 = s.state0;
  a.perturbed = s.perturbed;
  a.noise = s.noise;
  a.U = s.U;
  std::memcpy(a.sigma_inv, s.sigma_inv, sizeof(a.sigma_inv));
  a.lambda_ = s.lambda_;
  a.u_scale = s.u_scale;
  a.noise_abs_cost = s.noise_abs_cost;
  a.states = s.states;
  a.cost_total = s.cost_total;
}

// GRU encode in C horizon chunks of Tc steps on a low-priority stream of its own, forked behind what c->stream holds (the
// perturb kernel, the staged inputs); ev_gru[ch] tells the consumer that the latents of chunk ch are there
int gru_encode_chunks(nlc_ctx* c, GruArgs& g, int64_t KE, int C, int Tc, bool coop, unsigned lds_pad) {
  const int T = c->pd.T;
  if (!c->side.gru_stream) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = lowest priority: the consumer's workgroups go first
    NLC_HIP(c, hipStreamCreateWithPriority(&c->side.gru_stream, hipStreamNonBlocking, lo));
  }
  if (int rc = ensure(c, c->side.ev_fork)) return rc;
  if (int rc = grow(c, c->side.ev_gru, C)) return rc;
  NLC_HIP(c, hipEventRecord(c->side.ev_fork, c->stream));
  NLC_HIP(c, hipStreamWaitEvent(c->side.gru_stream, c->side.ev_fork, 0));
  for (int ch = 0; ch < C; ++ch) {
    g.t0 = ch * Tc;
    g.Tc = (g.t0 + Tc <= T) ? Tc : T - g.t0;
    if (g.Tc <= 0) break;
    g.N = KE * g.Tc;
    {
      ProfScope ps(c, "gru_encode_kernel", c->side.gru_stream, true);
      NLC_HIP(c, launch_gru_encode(g, c->nl.g, c->side.gru_stream, coop, lds_pad));
    }
    NLC_HIP(c, hipEventRecord(c->side.ev_gru[ch], c->side.gru_stream));
  }
  return NLC_OK;
}

// De Hoog planner with "dehoog_chain" and "dehoog_streams" both on auto and a population large enough for two streams to be
// considered: which form runs the chain is MEASURED.  The staged launches on two streams are the fastest form on most boxes
// of the pool (158 planning steps/s at configs[4]'s size against 151 on one stream and 150 for the persistent kernel) but the
// slowest on others, where launches on two streams do not overlap (134, same kernels, same per-launch durations:
// profiles/r4_dehoog_chain.md).  The first commands of a planner therefore run the candidates in turns -- same bits whichever
// runs -- with an event pair around the chain (read back one command later, when the caller has long waited for that
// command's action: no synchronisation is added), and the planner keeps the fastest (nlc_plan.h dehoog_pick).
// *variant: 0 two streams, 1 one stream, 2 persistent kernel, -1 not calibrating; *timing: this command is a measurement --
// dh.ev[0] is recorded here, the caller records dh.ev[1] behind the chain.
int dehoog_calibrate(nlc_ctx* c, int64_t KE, bool chain_ok, int* variant, bool* timing) {
  DehoogCalib& dh = c->dh;
  *variant = -1;
  *timing = false;
  if (!(c->pd.E == 1 && c->opt.dehoog_chain < 0 && c->opt.dehoog_streams == 0 && KE >= 8192 && !c->profiling)) return NLC_OK;
  const int ncand = chain_ok ? 3 : 2;
  if (dh.pending >= 0 && dh.ev[0] && dh.ev[1]) {  // the previous command's measurement
    float ms = 0.f;
    if (hipEventSynchronize(dh.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, dh.ev[0], dh.ev[1]) == hipSuccess)
      dh.ms[dh.pending][dh.pending_round & 1] = ms;
    dh.pending = -1;
  }
  if (dh.choice < 0) dh.choice = plan::dehoog_pick(dh.n, ncand, now_s() - dh.t0, dh.ms);
  if (dh.choice >= 0) {
    *variant = dh.choice;
    return NLC_OK;
  }
  if (dh.n == 0) dh.t0 = now_s();
  *variant = dh.n % ncand;
  dh.pending = *variant;
  dh.pending_round = dh.n / ncand;
  dh.n += 1;
  for (int e = 0; e < 2; ++e)
    if (!dh.ev[e]) NLC_HIP(c, hipEventCreate(&dh.ev[e]));
  NLC_HIP(c, hipEventRecord(dh.ev[0], c->stream));
  *timing = true;
  return NLC_OK;
}

// the whole step chain as ONE persistent launch (kernels_dehoog_chain.hip): a workgroup owns 64 samples for all T steps, F
// stays with the CU that wrote it
int launch_dehoog_chain(nlc_ctx* c, RolloutCall& call, const SampleCostArgs& sc, const RolloutArgs& r, double* pa) {
  DehoogChainArgs ca{};
  put_sample_cost(ca, sc);
  ca.net = r.net;
  ca.pa = pa;
  ca.tn = c->tn;
  ca.slot = c->nl.slot_dev.get();
  ca.eidx = c->nl.eidx_dev.get();
  ca.fre = call.ws + call.w.fre;  // one private (8 nt3) x 64 block per 64 samples
  ca.fim = call.ws + call.w.fim;
  ca.phases = c->opt.dehoog_chain_phases;
  ProfScope ps(c, "nl_dehoog_chain_kernel");
  NLC_HIP(c, launch_nl_dehoog_chain(ca, c->opt.dehoog_chain == 2 ? 2 : 4, c->stream));
  return NLC_OK;
}

// The step chain as launches: two per horizon step -- [tail of step t-1 +] representation function -> F, then de Hoog (or the
// slot-major linear ILT) -> dx; the tail of the LAST step is a launch of its own.
// The population is cut into P contiguous parts (nlc_plan.h staged_partition) whose 2 T + 1 launches run on P streams.  A
// sample's chain never leaves its part, so the parts need no ordering among themselves, and the two kernels of a step bound
// different pipes -- the representation launch the FP64 MFMA (util 0.42: dependent layers), the QD launch the FP64 VALU at
// 1.25 wavefronts per SIMD (active 0.39) -- so while one part's QD pass runs, another part's representation launch fills the
// matrix pipe (option "dehoog_streams": 1 = one stream).  With C > 1 a part's launches wait for the GRU chunk (ev_gru) that
// holds their horizon step.
int launch_staged_steps(nlc_ctx* c, RolloutCall& call, const SampleCostArgs& sc, const RolloutArgs& r, double* pa,
                        const double* lin_tab, const plan::Parts& parts, const plan::Chunks& ck) {
  const nlc_mppi_desc& d = c->pd;
  const WsLayout& w = call.w;
  double* ws = call.ws;
  const int64_t KE = call.KE;
  const int P = parts.P;
  SideStreams& side = c->side;
  double* tconst = ws + w.tconst;
  RepFuncArgs rf{};
  rf.net = r.net;
  rf.N = KE;
  rf.obs_stride = d.d;
  rf.Kep = d.K;
  rf.pa_stride = (int64_t)d.T * 2;
  rf.tn = c->tn;
  rf.general_t = 0;
  rf.slot = c->nl.slot_dev.get();
  rf.fre = ws + w.fre;
  rf.fim = ws + w.fim;
  // F travels slot-major between the two kernels of a step: four 128-B runs per store instruction of the MFMA
  // epilogue, one full line per de Hoog load (kernels_ilt.hip, FMODE 2)
  rf.slot_major = 1;
  rf.split = c->nl.md.h == 128 && c->opt.repfunc_split != 0;
  IltArgs ia = ilt_args(c->nl.md.ilt, nullptr, nullptr, tconst, ws + w.dx, KE, d.d);
  ia.fre = rf.fre;
  ia.fim = rf.fim;
  ia.t_stride = 0;  // one prediction time for every sample
  ia.eidx = c->nl.eidx_dev.get();
  StepTailArgs st{sc};
  st.d = d.d;
  st.x = r.xcarry;
  st.dx = ws + w.dx;
  st.ccarry = r.ccarry;
  if (P > 1) {
    if (int rc = grow(c, side.aux_streams, P - 1)) return rc;
    if (int rc = ensure(c, side.ev_fork)) return rc;
    if (int rc = grow(c, side.ev_join, P - 1)) return rc;
    NLC_HIP(c, hipEventRecord(side.ev_fork, c->stream));  // behind the GRU encode and the staged inputs
    for (int h = 1; h < P; ++h) NLC_HIP(c, hipStreamWaitEvent(side.aux_streams[h - 1], side.ev_fork, 0));
  }
  const size_t f_per_sample = 8 * (size_t)c->nl.net.nt3;
  RepFuncArgs rfs[4];
  IltArgs ias[4];
  StepTailArgs sts[4];
  for (int h = 0; h < P; ++h) {  // part h: samples [o, o + n)
    const int64_t o = parts.off[h], n = parts.n[h];
    StepTailArgs& stp = sts[h];
    stp = st;
    static_cast<SampleCostArgs&>(stp) = st.part(o, n, d.d);
    stp.x = st.x + o * d.d;
    stp.dx = st.dx + o * d.d;
    stp.ccarry = st.ccarry + o * 2;
    RepFuncArgs& rfp = rfs[h];
    rfp = rf;
    rfp.N = n;
    rfp.Kep = stp.Kep;
    rfp.fre = rf.fre + (size_t)o * f_per_sample;  // slot-major (8 nt3, n) block of the part
    rfp.fim = rf.fim + (size_t)o * f_per_sample;
    IltArgs& iap = ias[h];
    iap = ia;
    iap.N = n;
    iap.x = ia.x + o * d.d;
    iap.fre = rfp.fre;
    iap.fim = rfp.fim;
  }
  auto stream_of = [&](int h) { return h == 0 ? c->stream : side.aux_streams[h - 1]; };
  for (int t = 0; t < d.T; ++t) {
    for (int h = 0; h < P; ++h) {
      if (parts.n[h] <= 0) continue;
      hipStream_t sh = stream_of(h);
      if (ck.C > 1 && t % ck.Tc == 0) NLC_HIP(c, hipStreamWaitEvent(sh, side.ev_gru[t / ck.Tc], 0));  // latents of this chunk
      RepFuncArgs& rp = rfs[h];
      rp.obs = sts[h].state0;
      rp.obs_per_sample = (t == 0) ? call.state_per_sample : 1;
      rp.pa = pa + ((size_t)parts.off[h] * d.T + (size_t)t) * 2;
      rp.tail_prev = t > 0;
      if (t > 0) {
        rp.tail = sts[h];
        rp.tail.t = t - 1;
        rp.tail.first = t - 1 == 0;
        rp.tail.last = 0;
      }
      {
        ProfScope ps(c, "nl_repfunc_kernel", sh, true);
        NLC_HIP(c, launch_nl_repfunc(rp, sh));
      }
      if (!lin_tab) {
        ProfScope ps(c, "ilt_dehoog_kernel", sh, true);
        NLC_HIP(c, launch_ilt_dehoog(ias[h], sh));
      } else {
        const IltArgs& ih = ias[h];
        const IltLinSlotArgs il{ih.fre, ih.fim, ih.eidx, ih.t, ih.x, ih.N, ih.d, ih.S, lin_tab + 2 * ih.S, lin_tab + 3 * ih.S};
        ProfScope ps(c, "ilt_linear_slot_kernel", sh, true);
        NLC_HIP(c, launch_ilt_linear_slot(il, sh));
      }
    }
  }
  for (int h = 0; h < P; ++h) {
    if (parts.n[h] <= 0) continue;
    hipStream_t sh = stream_of(h);
    sts[h].t = d.T - 1;
    sts[h].first = d.T == 1;
    sts[h].last = 1;
    {
      ProfScope ps(c, "step_tail_kernel", sh, true);
      NLC_HIP(c, launch_step_tail(sts[h], sh));
    }
    if (h > 0) {
      NLC_HIP(c, hipEventRecord(side.ev_join[h - 1], sh));
      NLC_HIP(c, hipStreamWaitEvent(c->stream, side.ev_join[h - 1], 0));
    }
  }
  return NLC_OK;
}

// staged planner path (BASELINE configs[4]): hoisted GRU, then the step chain -- as launches per horizon step or as one
// persistent launch; fixed_tablot / stehfest models (option linear_fused = 0) take the same path with the slot-major linear
// ILT in de Hoog's place.  Everything stays on the device.
int rollout_nl_staged(nlc_ctx* c, RolloutCall& call, const SampleCostArgs& sc, GruArgs& g, RolloutArgs& r, double* pa) {
  const nlc_mppi_desc& d = c->pd;
  const int64_t KE = call.KE;
  const bool dehoog = c->nl.md.ilt.algo == NLC_ILT_DEHOOG;
  const double* lin_tab = nullptr;
  if (!dehoog)
    if (int rc = linear_tables(c, &c->nl.md.ilt, &lin_tab)) return rc;
  // option "dehoog_chain": -1 auto, 0 the staged launches, 1 (2: two workgroups per CU) the persistent kernel required
  const bool chain_ok = dehoog && d.E == 1 && nl_dehoog_chain_available(c->nl.md.h, c->nl.net.nt3, c->nl.S);
  if (c->opt.dehoog_chain >= 1 && !chain_ok)
    return fail(c, NLC_ERR_UNSUPPORTED, "dehoog_chain: single planner, hidden_units 128 and 17 or 33 de Hoog terms only");
  int calib_variant = -1;
  bool timing = false;
  if (int rc = dehoog_calibrate(c, KE, chain_ok, &calib_variant, &timing)) return rc;
  const bool chain = chain_ok && (c->opt.dehoog_chain >= 1 || calib_variant == 2);
  // GRU encode: one launch up front, or (option "dehoog_gru_chunks" C > 1; auto: off) C horizon chunks on a
  // stream of their own that run BESIDE the step chain.  The chunks use the cooperative kernel at reduced occupancy (lds_pad)
  // so that the chain's workgroups find room.
  const plan::Chunks ck = plan::horizon_chunks(d.E == 1 && !chain ? c->opt.dehoog_gru_chunks : 1, d.T);
  if (ck.C == 1) {
    g.t0 = 0;
    g.Tc = d.T;
    g.N = KE * d.T;
    ProfScope ps(c, "gru_encode_kernel");
    NLC_HIP(c, launch_gru_encode(g, c->nl.g, c->stream, gru_use_coop(c, g.N)));
  }
  c->last_body = chain ? 5 : 4;
  if (chain) {
    if (int rc = launch_dehoog_chain(c, call, sc, r, pa)) return rc;
  } else {
    NLC_HIP(c, hipMemcpyAsync(call.ws + call.w.tconst, &c->tn, sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (ck.C > 1) {
      // (cooperative kernel at reduced occupancy unless "gru_coop" = 0 asks for the wave-per-tile one)
      const bool coop = c->opt.gru_coop != 0;
      if (int rc = gru_encode_chunks(c, g, KE, ck.C, ck.Tc, coop, coop ? (unsigned)c->opt.dehoog_gru_lds_pad : 0u)) return rc;
    }
    int P = d.E == 1 ? c->opt.dehoog_streams : 1;
    if (P == 0) P = KE >= 8192 ? 2 : 1;  // auto ...
    if (calib_variant == 0) P = 2;       // ... or what the calibration runs / chose
    if (calib_variant == 1) P = 1;
    if (int rc = launch_staged_steps(c, call, sc, r, pa, lin_tab, plan::staged_partition(KE, P), ck)) return rc;
  }
  if (timing) NLC_HIP(c, hipEventRecord(c->dh.ev[1], c->stream));
  return finish_rollout_costs(c, call.buf);  // (neither form of the step chain has an instance for a cost variant)
}

// one persistent launch for a small shard (kernels_fused.hip): GRU encode and split rollout as roles of one grid, with the
// sampling and the weight fold inside when the command allows.  Returns through *weights_done whether the launch folded the
// importance weights itself.
int rollout_nl_fused(nlc_ctx* c, RolloutCall& call, GruArgs& g, RolloutArgs& r, bool* weights_done) {
  const nlc_mppi_desc& d = c->pd;
  const nlc_mppi_buffers* buf = call.buf;
  const WsLayout& w = call.w;
  double* ws = call.ws;
  const int64_t KE = call.KE;
  const int rng = call.rng;
  const bool inline_inputs = call.inline_inputs;
  PerturbArgs& p = call.p;
  const plan::FusedSchedule s = plan::fused_schedule(c->prop.multiProcessorCount, KE, d.T, c->nl.md.h, c->fused.blocks_per_cu,
                                                     c->fused.blocks_per_cu3, c->opt.fused);
  FusedArgs f{};
  f.r = r;
  f.r.t_begin = 0;
  f.r.t_end = d.T;
  f.g = g;
  f.g.t0 = 0;
  f.g.Tc = d.T;
  f.g.N = KE * d.T;
  FusedCtl& fc = f.ctl;
  fc.sync = reinterpret_cast<unsigned*>(ws + w.sync);
  fc.timeout_host = pin_giveup_word(c);
  fc.ntk = s.ntk;
  fc.n_enc = s.n_enc;
  fc.roll_cap = s.roll_cap;
  fc.adaptive_q8 = s.adaptive_q8;
  fc.pool_wgs = s.pool_wgs;
  fc.chain_first_tiles = s.chain_first_tiles;
  fc.partner_tiles = s.partner_tiles;
  fc.spin_limit = (unsigned)c->opt.fused_spin_limit;
  fc.test_drop_tile = c->opt.fused_test_drop_tile;
  // Single planner: the weight reduction runs inside the launch, and with device noise and the command's inputs in
  // the kernel arguments so does the sampling -- command() is then this launch + merge_kernel.
  fc.inline_weights = (c->opt.fused_inline & 1) && d.E == 1 && !d.cost_external;
  fc.inline_perturb = (c->opt.fused_inline & 2) && d.E == 1 && inline_inputs && rng == 1 && d.B <= kFusedMaxInlineB;
  unsigned* sync_words = reinterpret_cast<unsigned*>(ws + w.sync);
  const size_t n_sync = fused_sync_words(d.T, KE);
  if (fc.inline_perturb) {
    // tickets / flags start at zero: the previous command's merge kernel left them so (else: one memset)
    if (c->fused.sync_clean_ws != buf->workspace) NLC_HIP(c, hipMemsetAsync(sync_words, 0, n_sync * sizeof(unsigned), c->stream));
  } else {
    p.zero_words = sync_words;
    p.n_zero_words = (int64_t)n_sync;
    if (int rc = launch_shift_perturb(c, call)) return rc;
  }
  c->fused.sync_clean_ws = nullptr;
  c->fused.sync_dirty = true;
  c->fused.last.fused = true;
  c->last_body = 3;
  f.p = p;
  if (fc.inline_weights) f.w = make_weight_args(c, buf);
  {
    ProfScope ps(c, "nl_plan_fused_kernel");
    NLC_HIP(c, launch_nl_plan_fused(f, c->nl.g, s.grid, s.built, c->stream));
  }
  *weights_done = fc.inline_weights != 0;
  return NLC_OK;
}

// "gru_prefix" for the encoder launch of the two-launch body over N windows: *use, or (option 1) the reason it cannot be.  On
// *use the perturb kernel is told to zero the list counters, as it zeroes the fused body's sync block.
int gru_prefix_begin(nlc_ctx* c, RolloutCall& call, const GruArgs& g, int64_t N, int chunks, bool* use, GruPrefixArgs* px) {
  *use = false;
  if (c->opt.gru_prefix == 0) return NLC_OK;
  GruPrefixState& ps = c->prefix;
  const char* why = ps.why_not;
  if (!why && ps.last_B != g.B) why = "gru_prefix: the table was built for another action-buffer length";
  if (!why && chunks != 1) why = "gru_prefix: not with the encoder in horizon chunks (horizon_chunks)";
  if (!why && gru_use_coop(c, N)) why = "gru_prefix: this launch takes the cooperative encoder (gru_coop)";
  if (!why && g.use_i8) why = "gru_prefix: the FP64 encoder only (gru_gemm is 1)";
  if (!why) why = prefix::out_of_scope(g.nact, g.nin, 1, g.B, N, true);
  if (why) return c->opt.gru_prefix == 1 ? fail(c, NLC_ERR_UNSUPPORTED, why) : NLC_OK;
  const int64_t stride = (N + 63) / 64 * 64;
  const size_t need = 64 + (size_t)prefix::kLists * (size_t)stride / 2;  // doubles: a row of counters, then 32-bit lists
  if (need > ps.lists.size()) {
    NLC_HIP(c, hipStreamSynchronize(c->stream));  // (an earlier command may still read the buffer this replaces)
    NLC_HIP(c, (hipError_t)ps.lists.hold(need));
  }
  double* base = c->nl.arena.get() + ps.arena_off;
  px->table = base;
  px->out_tab = base + (size_t)prefix::kEntries * 2 * c->nl.g;
  px->products = base + gru_prefix_products_off(c->nl.g);
  px->counts = reinterpret_cast<unsigned*>(ps.lists.get());
  px->lists = reinterpret_cast<unsigned*>(ps.lists.get() + 64);
  px->list_stride = stride;
  px->img_max = ps.img_max;
  px->img_min = ps.img_min;
  call.p.zero_words = px->counts;
  call.p.n_zero_words = 16;
  *use = true;
  return NLC_OK;
}

// GRU launch + rollout launch (wave-per-tile or latency-split body), optionally in horizon chunks on two streams
int rollout_nl_two_launch(nlc_ctx* c, RolloutCall& call, GruArgs& g, RolloutArgs& r, int variant) {
  const nlc_mppi_desc& d = c->pd;
  const int64_t KE = call.KE;
  bool use_prefix = false;
  GruPrefixArgs px{};
  {
    const int chunks = plan::horizon_chunks((variant != 2 && KE > 8192 && d.E == 1) ? c->opt.horizon_chunks : 1, d.T).C;
    if (int rc = gru_prefix_begin(c, call, g, KE * d.T, chunks, &use_prefix, &px)) return rc;
  }
  if (int rc2 = nlc::host::launch_shift_perturb(c, call)) return rc2;
  // Horizon chunks (round 3, option "horizon_chunks"): the encoder input does not depend on the state, so the GRU
  // encode of horizon steps [c Tc, (c + 1) Tc) can run on a stream of its own while the rollout walks the chunk before
  // it.  The two kernels bound different things -- the encoder the FP64 MFMA pipe (95 % busy, two waves per SIMD), the
  // wave-per-tile rollout the latency of ONE wave per SIMD (85 % busy) -- and since round 3 one wave of each fits a
  // SIMD's registers (216 + 288 <= 512), so the encoder fills the rollout's issue bubbles.  State and cost sums travel
  // between the rollout's chunk launches in xcarry / ccarry: same bits as the single launch.
  const plan::Chunks ck = plan::horizon_chunks((variant != 2 && KE > 8192 && d.E == 1) ? c->opt.horizon_chunks : 1, d.T);
  const int C = ck.C, Tc = ck.Tc;
  if (C == 1) {
    g.t0 = 0;
    g.Tc = d.T;
    g.N = KE * d.T;
    if (use_prefix) {
      {
        ProfScope ps(c, "gru_prefix_index_kernel");
        NLC_HIP(c, launch_gru_prefix_index(g, px, c->stream));
      }
      ProfScope ps(c, "gru_encode_kernel");
      NLC_HIP(c, launch_gru_encode_prefix(g, px, c->nl.g, c->stream));
      c->prefix.last_used = true;
    } else {
      ProfScope ps(c, "gru_encode_kernel");
      NLC_HIP(c, launch_gru_encode(g, c->nl.g, c->stream, gru_use_coop(c, g.N)));
    }
    if (c->opt.dbg_gap_us > 0.0 || c->opt.dbg_l2_mb > 0.0)
      if (int rc3 = dbg_between(c)) return rc3;
    r.t_begin = 0;
    r.t_end = d.T;
    ProfScope ps(c, "nl_rollout_kernel");
    NLC_HIP(c, launch_nl_rollout(r, c->stream, variant));
  } else {
    if (int rc = gru_encode_chunks(c, g, KE, C, Tc, false, 0u)) return rc;
    for (int ch = 0; ch < C; ++ch) {
      r.t_begin = ch * Tc;
      r.t_end = (r.t_begin + Tc <= d.T) ? r.t_begin + Tc : d.T;
      if (r.t_begin >= r.t_end) break;
      NLC_HIP(c, hipStreamWaitEvent(c->stream, c->side.ev_gru[ch], 0));
      ProfScope ps(c, "nl_rollout_kernel");
      NLC_HIP(c, launch_nl_rollout(r, c->stream, 1));
    }
  }
  return NLC_OK;
}

}  // namespace

// The prefix-state table (nlc_gru_prefix.h) of the planner nlc_mppi_configure has just described in c->pd: one wavefront runs
// the 16 patterns of four clipped actions through the encoder's own step body.  The tile is fed the bound images exactly as a
// clipped action reaches the encoder: perturbed holds u_max / u_scale, the encoder multiplies by u_scale and normalises.
int nlc::host::gru_prefix_configure(nlc_ctx* c) {
  const nlc_mppi_desc& d = c->pd;
  GruPrefixState& ps = c->prefix;
  ps.last_B = d.B;
  ps.last_used = false;
  const double img[2] = {prefix::bound_image(d.u_max[0], d.u_scale), prefix::bound_image(d.u_min[0], d.u_scale)};
  bool finite = true;
  for (double v : img) finite = finite && std::isfinite((d.u_scale * v - c->nl.gru.mean[0]) / c->nl.gru.std[0]);
  ps.why_not = prefix::out_of_scope(d.nu, c->nl.md.nin, d.has_bounds, d.B, 0, finite);
  if (ps.why_not) return NLC_OK;
  ps.img_max = prefix::bits_of(img[0]);
  ps.img_min = prefix::bits_of(img[1]);
  std::vector<double> syn((size_t)16 * d.B, 0.0);  // column c, GRU step s (window element B - 1 - s): bit s of c picks u_min
  for (int col = 0; col < 16; ++col)
    for (int s = 0; s < prefix::cap(d.B); ++s) syn[(size_t)col * d.B + (d.B - 1 - s)] = img[(col >> s) & 1];
  double* base = c->nl.arena.get() + ps.arena_off;
  GruPrefixArgs px{};
  px.table = base;
  px.out_tab = base + (size_t)prefix::kEntries * 2 * c->nl.g;
  px.products = base + gru_prefix_products_off(c->nl.g);
  double* syn_dev = px.out_tab + 64;
  NLC_HIP(c, hipMemcpy(syn_dev, syn.data(), syn.size() * sizeof(double), hipMemcpyHostToDevice));
  GruArgs a = c->nl.gru;
  a.mode = 1;
  a.perturbed = syn_dev;
  a.abuf = syn_dev;  // (never read: every element of window (k, B - 1) is a perturbed one)
  a.u_scale = d.u_scale;
  a.T = a.Tc = d.B;
  a.t0 = 0;
  a.Kep = 16;
  a.N = 16;
  a.B = d.B;
  a.nact = 1;
  a.out = nullptr;
  NLC_HIP(c, launch_gru_prefix_table(a, px, c->nl.g, c->stream));
  NLC_HIP(c, hipStreamSynchronize(c->stream));
  return NLC_OK;
}

int nlc::host::rollout_nl(nlc_ctx* c, RolloutCall& call) {
  const nlc_mppi_desc& d = c->pd;
  const nlc_mppi_buffers* buf = call.buf;
  const WsLayout& w = call.w;
  double* ws = call.ws;
  const int64_t KE = call.KE;
  const bool replay = call.replay;
  const bool lin_direct = linear_on_rollout_kernels(c);
  double* pa = ws + w.pa;
  GruArgs g = c->nl.gru;
  g.mode = 1;
  g.perturbed = buf->perturbed;
  g.abuf = call.abuf_dev;
  g.u_scale = d.u_scale;
  g.T = d.T;
  g.B = d.B;
  g.Kep = d.K;
  g.nact = d.nu;
  g.out = pa;
  const SampleCostArgs sc = sample_cost_args(c, call);
  RolloutArgs r{};
  put_sample_cost(r, sc);
  r.Kep = sc.Kep;
  r.net = c->nl.net;
  r.net.b1 = c->nl.b1fold.get();
  r.B = d.B;
  r.pa = pa;
  r.tn = c->tn;
  r.xcarry = ws + w.xcarry;
  r.ccarry = ws + w.ccarry;
  if (lin_direct) {
    if (!c->nl.cp_lin.get()) return fail(c, NLC_ERR_STATE, "linear-algorithm coefficient tables missing (nlc_mppi_configure)");
    const size_t ng = (size_t)2 * c->nl.net.nt3 * 64;
    r.net.Cp = c->nl.cp_lin.get();
    r.net.Cp2 = c->nl.cp_lin.get() + ng;
    r.net.lin = 1;
  }
  c->prefix.last_used = false;
  const char* prefix_two_launch_only = "gru_prefix: the encoder launch of the two-launch body only (rollout_variant 1 / 2)";
  if (c->nl.md.ilt.algo != NLC_ILT_FOURIER && !lin_direct) {
    if (c->opt.gru_prefix == 1) return fail(c, NLC_ERR_UNSUPPORTED, prefix_two_launch_only);
    return rollout_nl_staged(c, call, sc, g, r, pa);
  }
  // rollout_variant (nlc_set_option): 0 auto, 1 wave-per-tile, 2 latency-split, 3 fused one-launch body
  int variant = c->opt.rollout_variant;
  const int h_ = c->nl.md.h;
  const bool fused_ok = (h_ == 64 || h_ == 128 || h_ == 256) && 2 * c->nl.g == h_ && c->nl.net.nt3 <= 21 &&
                        KE * d.T * 16 < (int64_t)1 << 31 && !lin_direct;  // (no LIN instance of the one-launch body)
  if (variant == 3 && !fused_ok) return fail(c, NLC_ERR_UNSUPPORTED, "fused planner body: model shape not instantiated");
  // instances per width: 3 and 4 workgroups per CU at hidden_units 64 / 128, 2 at 256 (68 KB of LDS per workgroup)
  const int bpc_hi = h_ == 256 ? 2 : 4, bpc_lo = h_ == 256 ? 2 : 3;
  if (fused_ok && (c->fused.blocks_per_cu < 0 || c->fused.occ_h != h_)) {
    int bpc = 0;
    NLC_HIP(c, fused_max_resident_blocks(h_, bpc_hi, &bpc));
    c->fused.blocks_per_cu = bpc;
    NLC_HIP(c, fused_max_resident_blocks(h_, bpc_lo, &bpc));
    c->fused.blocks_per_cu3 = bpc;
    c->fused.occ_h = h_;
  }
  // The fused body's rollout workgroups wait for encoder workgroups of the SAME launch, so every workgroup must be
  // resident and there must be workgroups left to encode beside one chain per CU: at least two per CU.  It
  // also assumes the device to itself (include/nlc.h): after one hand-off timeout the ctx stays on the two-launch body.
  if (variant == 3 && c->fused.blocks_per_cu < 2)
    return fail(c, NLC_ERR_UNSUPPORTED, "fused planner body: fewer than two workgroups of the kernel fit a CU");
  // A K-sharded planner takes the fused body by itself only when the weight fold runs inside the launch: a give-up then marks
  // the shard's partial row, which every rank sees after the all-gather (nlc_mppi_finish re-runs the command everywhere).
  const bool sharded = d.K_global > d.K;
  const bool fold_inside = (c->opt.fused_inline & 1) && d.E == 1 && !d.cost_external;
  if (variant == 0 && fused_ok && c->fused.blocks_per_cu >= 2 && KE <= c->opt.fused_max_samples && (!sharded || fold_inside)) variant = 3;
  if (variant == 3 && (replay || c->fused.lost)) variant = 2;
  // the one-launch body and the latency-split body have an instance for a cost variant; the wave-per-tile body has not
  const bool in_body = variant == 3 || variant == 2 || (variant == 0 && KE <= 8192);
  if (in_body) cost_in_body(r, d);
  if (variant == 3) {
    if (c->opt.gru_prefix == 1) return fail(c, NLC_ERR_UNSUPPORTED, prefix_two_launch_only);
    bool weights_done = false;
    if (int rc2 = rollout_nl_fused(c, call, g, r, &weights_done)) return rc2;
    if (weights_done) return NLC_OK;
  } else {
    if (int rc2 = rollout_nl_two_launch(c, call, g, r, variant)) return rc2;
    // (launch_nl_rollout: 2 = latency-split, 1 = wave-per-tile, 0 = its own pick: split up to 8192 samples)
    c->last_body = (variant == 2 || (variant == 0 && KE <= 8192)) ? 2 : 1;
  }
  return finish_rollout_costs(c, buf, in_body);
}
