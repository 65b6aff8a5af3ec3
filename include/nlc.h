/*
 * nlc.h -- C ABI of libnlc_hip.so: the MI355X (gfx950) planning hot path of Neural Laplace Control.
 *
 * The reference (samholt/NeuralLaplaceControl) is pure Python and has NO FFI layer; its boundary for
 * this path is three Python call sites.  Each entry point below names the reference interface it
 * replaces (file:line, relative to the reference tree).  The Python mirror of those interfaces
 * (neurallaplacecontrol_amd/) binds these symbols with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every function returns an int status (NLC_OK = 0, negative = error); text via nlc_last_error().
 *     No C++ exception crosses this boundary.
 *   - "_dev" pointers are DEVICE pointers (HBM of the ctx's GPU; e.g. torch.Tensor.data_ptr()),
 *     "_host" pointers are host pointers.  All payloads are float64, row-major, contiguous.
 *   - the caller owns every pointer for the duration of the call only; the ctx copies what it keeps.
 *   - kernels are enqueued on the stream given to nlc_set_stream() (until then: a stream the ctx created).
 *     Functions that return host data synchronise that stream before returning; the others are
 *     asynchronous with respect to the host, ordered on the stream.
 *   - a ctx is not thread-safe: one ctx per (process, device).  HIP is initialised lazily inside
 *     nlc_create(), never at library load (spawn-safe, cf. run_exp_multi.py:145,207).
 */
#ifndef NLC_H_
#define NLC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLC_ABI_VERSION 20

#define NLC_OK 0
#define NLC_ERR_BAD_ARG (-1)
#define NLC_ERR_BAD_SHAPE (-2)
#define NLC_ERR_HIP (-3)
#define NLC_ERR_UNSUPPORTED (-4)
#define NLC_ERR_STATE (-5)
#define NLC_ERR_COMM (-6) /* RCCL reported an error (message in nlc_last_error) */
/* nlc_mppi_finish only, caller-owned collective (gathered_dev != NULL, G > 1): the command was re-run on the two-launch body on
 * every rank; buf->partials hold the new rows -- all-gather them again and call nlc_mppi_finish again.  Not an error. */
#define NLC_AGAIN 1

#define NLC_MAX_NU 2   /* action dims (cartpole/pendulum 1, acrobot 2) */
#define NLC_MAX_NIN 3  /* GRU input dims = nu + encode_obs_time */
#define NLC_MAX_D 8    /* observation dims (3..6 in the reference envs) */

/* ILT algorithms (torchlaplace `ilt_algorithm`, call site w_nl.py:141) */
#define NLC_ILT_FOURIER 0
#define NLC_ILT_DEHOOG 1
/* the closed-form LINEAR algorithms torchlaplace also offers (reference knob config.py:36 nl_ilt_algorithm): stand-alone
 * reconstruction (nlc_ilt_rep_inputs / nlc_ilt_reconstruct / its backward), nlc_model_forward, and the planner -- on LIN
 * instances of the rollout kernels by default, on the staged all-HIP path with option "linear_fused" = 0 (see nlc_set_option) */
#define NLC_ILT_FIXED_TALBOT 2 /* "fixed_tablot": Abate & Valko, M = terms nodes, r = 2M/5 (mpmath FixedTalbot) */
#define NLC_ILT_STEHFEST 3     /* "stehfest": Gaver-Stehfest, terms even (mpmath Stehfest) */

/* env running costs (mppi_with_model.py:145-171 -> ctcartpole.py:289-346, ctpendulum.py:139-155,
 * ctacrobot.py:233-255) and oracle dynamics (oracle.py:11-224) */
#define NLC_ENV_CARTPOLE 0
#define NLC_ENV_PENDULUM 1
#define NLC_ENV_ACROBOT 2
/* cartpole WITHOUT the trig observation: CTCartpole(obs_trans=False), nx = 4, state [x, xdot, theta, thetadot]
 * (ctcartpole.py:60; reward branch :297-300; oracle dynamics branch oracle.py:38-44, 80-86) -- BASELINE's literal
 * "state_dim=4".  Planner only (running cost, oracle dynamics, NL dynamics); nlc_env_step keeps the three harness envs. */
#define NLC_ENV_CARTPOLE_NOTRIG 3
/* the non-default branches of the harness running_cost (mppi_with_model.py:146-162 -> ctcartpole.py:311-329), a bit set;
 * cartpole envs only.  The closure's `if state_constraint / elif change_goal`: with NLC_COST_STATE_CONSTRAINT set the two
 * goal bits are not looked at. */
#define NLC_COST_STATE_CONSTRAINT 1 /* position error e0^2 + exp(10 e0 + 7): a soft wall on the cart (ctcartpole.py:327-329) */
#define NLC_COST_CHANGE_GOAL 2      /* goal x = -2 instead of 0 (ctcartpole.py:313-317) */
#define NLC_COST_GOAL_FLIPPED 4     /* with NLC_COST_CHANGE_GOAL: goal x = +2 (the global change_goal_flipped, :153-158) */
#define NLC_COST_VARIANT_MASK 7

/* rollout dynamics */
#define NLC_DYN_NL 0     /* state + NeuralLaplaceModel(state, window, ts_pred)  (mppi_with_model.py:103-122) */
#define NLC_DYN_ORACLE 1 /* oracle.{cartpole,pendulum,acrobot}_dynamics_dt_delay (mppi_with_model.py:129-143) */
#define NLC_DYN_EXTERNAL 2 /* caller-supplied dynamics/cost callables: the caller runs the horizon loop
                              (mppi_delay.py:271-296) itself between nlc_mppi_rollout and nlc_mppi_weights */
#define NLC_DYN_DTRNN 3    /* state + DeltaTRNN(state, window, ts_pred): the reference's Delta-t RNN baseline
                              (train_utils.py:589-631) behind the same harness closure (mppi_with_model.py:103-122) */
#define NLC_DYN_NODE 4     /* state + NODE(state, window, ts_pred): the neural-ODE baseline (train_utils.py:664-724) */

typedef struct nlc_ctx nlc_ctx;

/* ---- context -------------------------------------------------------------------------------- */
int nlc_abi_version(void);
int nlc_create(int device, nlc_ctx** out);
void nlc_destroy(nlc_ctx* ctx);
const char* nlc_last_error(const nlc_ctx* ctx); /* ctx may be NULL: error of the last failed nlc_create */
/* hipStream_t to enqueue on from now on, used as given: NULL is HIP's legacy default (null) stream, which
 * is what torch.cuda.current_stream().cuda_stream reports for torch's default stream. */
int nlc_set_stream(nlc_ctx* ctx, void* hip_stream);
int nlc_synchronize(nlc_ctx* ctx);
/* Planner tuning knobs (none changes a result beyond last-bit rounding of the reductions they do not touch; they pick
 * which hand-written rollout body a command of NLC_DYN_NL / Fourier runs):
 *   "rollout_variant"    0 auto (default) | 1 one wavefront per 16-sample tile | 2 latency-split, one workgroup per tile
 *                        | 3 fused one-launch body (GRU encode + split rollout as roles of one persistent grid)
 *   "fused_max_samples"  auto picks the fused body up to this many local samples (default 4096: one chain per CU; one
 *                        GPU's shard of BASELINE configs[1] at 4 and 8 GPUs)
 *   "fused_roll_cap"     rollout workgroups the fused body starts right away, one per CU (0 = auto: one per 16-sample
 *                        tile, at most one per CU)
 *   "repfunc_split"      staged de Hoog planner: the per-step representation launch as one workgroup per 16-sample tile
 *                        (1, default; 60 vs 76 us per step at K = 16384, S = 33) or one wavefront per tile (0)
 *   "gru_coop"           stand-alone GRU encodes (nlc_gru_encode, nlc_model_forward, the two-launch planner bodies) with the
 *                        cooperative kernel -- one 16-window tile per workgroup, one gate chunk per wavefront, a third of
 *                        the latency -- 1 / 0; -1 = auto (default): up to 50 000 windows at hidden_units 128, 8 192 at 64, always at 256
 *   "gru_prefix"         two-launch planner bodies, wave-per-tile FP64 encoder, one action dimension without a time channel
 *                        (nu == nin == 1) and action bounds: MPPI stores a clipped action as exactly u_max / u_scale or
 *                        u_min / u_scale, and the encoder consumes a window newest action first from h = 0, so while the consumed
 *                        actions are clipped the hidden states are constants of (weights, bounds, u_scale, normalisation,
 *                        pattern).  nlc_mppi_configure builds a table of the 2 + 4 + 8 + 16 states after one to four such steps
 *                        (30 KB in the model's arena; rebuilt by every configure, which a new model forces) and, for every state a
 *                        tile can start from, the hidden-side products W_hh H (+ bias) of the step that follows it: 6 g doubles
 *                        per entry, 90 KB reserved at hidden_units 128, of which B = 4 uses 42 KB.  Per command an index
 *                        pass behind perturb_kernel sorts the windows by the length of their clipped prefix (0 .. min(B, 4)) and
 *                        the encoder launch runs only the remaining steps of each, the first of them without its two
 *                        hidden-side GEMMs -- same step code, every gate sums its hidden side first, bit-identical latents
 *                        (csrc/nlc_gru_prefix.h).  -1 (default): whenever the launch is in scope, silently not otherwise;
 *                        0: never (the plain launch); 1: required -- NLC_ERR_UNSUPPORTED from nlc_mppi_rollout when the command
 *                        runs another body (fused, staged), the cooperative or int8-sliced encoder, horizon chunks, nu or nin
 *                        other than 1, no bounds, B > 32, more than 2^27 windows, or a bound whose normalised image is not finite
 *   "gru_gemm"           EXPERIMENTAL.  0 (default): the GRU encoder's hidden-state GEMMs on FP64 MFMAs.  1: the same GEMMs as
 *                        int8-sliced fixed-point products on the INT8 matrix pipe (csrc/kernels_gru_i8.hip, nlc_i8gemm.h; models with
 *                        hidden_units = 128, the stand-alone encode launches that take the wave-sized form -- more than 50 000
 *                        windows, or all of them with gru_coop = 0; the one-launch planner body keeps its FP64 encoder role): GRU states and row-scaled weights as 54-bit fixed point in seven signed 8-bit digits, one
 *                        v_mfma_i32_16x16x64_i8 per digit pair, exact integer accumulation, FP64 recombination.  Latents
 *                        agree with the FP64 kernel's to 3e-16; against the exact product either form is within 5 x 2^-53 of
 *                        the row's sum of |w h| (tools/i8gemm_check.hip).  2.5 ms against 3.0 ms for BASELINE configs[1]'s encode
 *   "horizon_chunks"     Fourier planner, wave-per-tile body (more than 8192 local samples): the GRU encode in this many horizon
 *                        chunks on a low-priority stream of its own, each chunk's rollout launch behind its event, so that the
 *                        encoder of later steps runs beside the rollout of earlier ones (one wave of each kernel fits a SIMD:
 *                        216 + 288 VGPRs).  1 (default) = one encode launch, one rollout launch.  Same bits for every value;
 *                        measured 4.224 vs 4.270 ms at 3 chunks (K = 16384) -- the two kernels leave each other little to fill
 *                        (95 % / 85 % of the issue slots busy), and per-launch times of overlapped kernels say nothing about
 *                        either, so the default and the reported roofline stay with the two plain launches.
 *   "dehoog_chain"       de Hoog planner (single planner, hidden_units 128, 17 or 33 terms): 1 = the whole step chain as ONE
 *                        persistent launch (kernels_dehoog_chain.hip: a workgroup of eight waves owns 64 samples for all T
 *                        steps -- representation MLP of its four tiles in one pass, QD table one wavefront per dim, state / cost
 *                        tail; F_k stays with the CU that wrote it); 2 = the same with four waves per 32 samples, two workgroups
 *                        per CU; 0 = the staged 2 T + 1 launches below; -1 (default) = auto.  Same bits for every value.
 *                        AUTO (this knob and "dehoog_streams" both on auto, >= 8192 local samples): the planner MEASURES -- its
 *                        first commands run the candidate forms (staged on two streams, staged on one, persistent kernel) in
 *                        turns for at least four rounds and half a second, an event pair around the chain, and it keeps the
 *                        fastest.  On most boxes that is the staged path on two streams (155-159 planning steps/s at BASELINE
 *                        configs[4]'s size vs 151 on one stream and 150 for the persistent kernel); on a box whose streams do not
 *                        overlap two streams measure 134 and auto settles on one (profiles/r4_dehoog_chain.md).
 *                        ("dehoog_chain_phases": tools only, 1 / 2 = only the representation / only the QD phase of that kernel
 *                        runs -- a timing breakdown, meaningless results)
 *   "dehoog_streams"     staged planner (NLC_ILT_DEHOOG models; fixed Talbot / Stehfest models take the same path and the
 *                        same options): the population is cut into this many contiguous parts
 *                        whose per-step launches run on streams of their own -- one part's FP64-VALU-bound QD pass beside
 *                        another part's MFMA-bound representation launch; 0 = auto (2 from 8192 samples), 1 = one stream.
 *                        Same bits for every value.
 *   "dehoog_gru_chunks"  the same planner: GRU encode in this many horizon chunks on a further stream, beside the step chain
 *                        (cooperative kernel at reduced occupancy, "dehoog_gru_lds_pad" bytes of unused LDS); 0 / 1 (default):
 *                        one launch up front -- measured no faster (the chip is busy either way).
 *   "host_spin"          nlc_mppi_finish with action_host (single planner): 1 (default) = the merge kernel stores a sequence
 *                        number behind the action in pinned host memory and the host spins on that word (sub-microsecond
 *                        hand-over, one busy core for the length of a command); 2 = the host first sleeps through most of the
 *                        wait -- the shortest of its last eight waits predicts this one, it wakes "host_spin_margin_us"
 *                        (default 150; at least 15 % of the prediction) early -- and spins only for the rest, leaving the core
 *                        to the harness's other workers (run_exp_multi.py:145 fans out a Pool(12) on one GPU);
 *                        0 = hipStreamSynchronize (measured: the runtime busy-waits as well, and wakes 5-9 us later).
 *                        After the call ONLY the action is valid; the stream may still be finishing omega / cost_nz (they are
 *                        stream-ordered for every later call; nlc_synchronize before reading them from the host).
 *   "fused_blocks_per_cu"  fused body: the instance compiled for 3 (168 VGPRs) or 4 (128 VGPRs) workgroups per CU; 0 = auto
 *                        (3 while rollout chains sit on at most half of the CUs, else 4)
 *   "fused_inline"       fused body, single planner (E <= 1), bit mask: 1 = the importance-weight reduction (:210-216) runs
 *                        inside the launch (every rollout tile folds its 16 samples when their costs are final, the last one
 *                        folds the tiles); 2 = with device noise (rng == 1) and host-side state / action_buffer the sampling
 *                        and bounding (:319-328) run in the encoder role; 3 (default; 1 is accepted as 3) = both -- a command
 *                        is then two launches (this one + the merge after the shard all-gather) instead of five; 0 = separate
 *                        launches.  Same bits either way.
 *   "fused_spin_limit"   polls (~2 us each) before a waiting wave of the fused body gives up (default 2^18, ~0.5 s)
 *   "linear_fused"       NLC_ILT_FIXED_TALBOT / NLC_ILT_STEHFEST models: 1 (default) = the rollout runs on LIN instances of the
 *                        rollout kernels (two epilogue MFMAs per slot group, coefficient fragments folded for the constant
 *                        prediction time at nlc_mppi_configure); 0 = the staged path de Hoog models take
 *   "train_dehoog"       training and evaluation entries of the NL family (nlc_train_*): 0 (default) = an NLC_ILT_DEHOOG model is
 *                        refused with NLC_ERR_UNSUPPORTED, as ever; 1 = it is accepted at odd ilt terms 3 .. 33 and any ILT
 *                        scale, and a call runs the forward half of the step, the de Hoog ILT, the loss, the ILT's backward
 *                        and the backward half as five launches before the reduction and Adam (csrc/nlc_train_dehoog.h).
 *                        One 16-row tile per workgroup: N <= 2048 rows per member and call, a larger N is
 *                        NLC_ERR_UNSUPPORTED; an even term count likewise.  The workspace sizes the *_workspace_bytes entries
 *                        return (nlc_train_group_eval_workspace_bytes included) are then the de Hoog layout's.  Other
 *                        algorithms are not affected
 *   "node_method"        the NODE's fixed-grid solver (train_utils.py:101-125 --node_method, :717-723 odeint(method=...)): 0
 *                        (default) euler, 1 midpoint, 2 rk4 -- torchdiffeq's 3/8 rule; tableaus in csrc/nlc_node_rk.h.  Any other
 *                        value: NLC_ERR_BAD_ARG.  Every NODE entry of the ctx reads it at the call: nlc_node_forward,
 *                        nlc_mppi_configure / the NLC_DYN_NODE rollout, and the nlc_node_train_group_* entries.  nlc_node_desc
 *                        does not carry it (its size is unchanged)
 *   "fused_keep_sync"    tools only: the merge kernel does not zero the fused body's sync block (tools/fused_debug.py reads
 *                        the launch's progress counters / timeline from it); the next command pays a memset instead
 *   "test_lin_coeff_scale"  tests only: the largest coefficient of the LIN rollout instances' folded w_re / t fragment is
 *                        scaled by this at the next nlc_mppi_configure (1 = off): the parity sweep's bound must catch 1 + 1e-6
 *   "fused_test_drop_tile"  tests only: the encoder tile with this ticket is never published (-1 = none): forces the
 *                        hand-off timeout and the re-run on the two-launch body
 *   "fused_chain_first_tiles"  encoder tiles every such workgroup encodes before its chain starts (-1 = auto: 1)
 *   "fused_partner_tiles"  the OTHER workgroups of that CU stop drawing encoder tiles after this many each and sleep until
 *                        the chain is done (an encoder wave beside a chain doubles the chain's step time); -1 = never,
 *                        -2 = auto (1 .. 4 with the share of CUs that walk a chain: fit to MI355X measurements)
 * The fused body assumes the device to itself: its rollout workgroups wait for encoder workgroups of the SAME launch, so
 * all of its workgroups must be resident at once (auto picks it only when at least two fit a CU).  Every wait is bounded: on
 * a time-out the launch marks its shard's partial row invalid (eta_r = -1), which travels through the shard all-gather, so
 * merge_kernel on EVERY rank skips the update and tells its host: every rank re-runs the command on the two-launch body inside
 * nlc_mppi_finish (library-side costs, host action pointer given; with a caller-owned collective the call returns NLC_AGAIN
 * for the second all-gather) -- no rank is left waiting in a collective.  Otherwise (device-resident action, cost callables)
 * the loss is reported as NLC_ERR_HIP by this or the next call, on every rank.  The ctx that timed out keeps to the
 * two-launch body from then on (setting "rollout_variant" again re-arms it).
 * Unknown names / out-of-range values: NLC_ERR_BAD_ARG. */
int nlc_set_option(nlc_ctx* ctx, const char* name, double value);
/* Read-only counters of the ctx's planner (ABI v9), so that a caller -- and the reference's deployment of several planner
 * processes on ONE GPU (run_exp_multi.py:145-165 fans out Pool(12) workers of K = 1000, config.py:52) -- can see which body
 * its commands run on and whether the fused body's bounded waits ever expired:
 *   "rollout_body"         body phase 1 of the LAST command ran on: 1 wave-per-tile | 2 latency-split | 3 fused one-launch
 *                          | 4 staged step chain (de Hoog / linear algorithms) | 5 persistent de Hoog chain | 6 oracle
 *                          | 7 Delta-t RNN | 8 NODE | 9 caller's callables; 0 = no command yet
 *   "fused_timeouts"       fused launches of this ctx that gave up waiting (each one: a re-run, or a lost command)
 *   "fused_fallbacks"      commands re-run on the two-launch body inside nlc_mppi_finish (give-up here OR on another rank)
 *   "fused_lost"           1 = this ctx has left the fused body for good ("rollout_variant" re-arms it)
 *   "last_giveup_command"  0-based index of the last command (count of nlc_mppi_rollout calls) that saw a give-up, -1 = none
 *   "commands"             nlc_mppi_rollout calls so far
 *   "comm_world", "comm_rank"  size / rank of the library-owned RCCL communicator (0 / -1 = none: nlc_comm_init not called)
 *   "fused_blocks_per_cu"  resident workgroups per CU the occupancy query returned for the fused kernel (-1 = not queried yet)
 *   "fused_spin_limit"     the option's current value
 *   "gru_prefix"           1 when the LAST command's encoder launch started from the prefix-state table (option "gru_prefix")
 *   "gru_prefix_windows_l0" .. "_l4"  that command's windows by the number of leading GRU steps taken from the table (0 when
 *                          the table was not used); they sum to E K T.  Reading one waits for the command's launches
 *   "gru_prefix_table_tiles"  that command's 16-window tiles that started from the table and took their first step's hidden-side
 *                          products from it: sum over the lengths 1 .. min(B, 5) - 1 of ceil(windows / 16).  Waits likewise
 *   "latents_offset"       offset, in doubles, of the (E K, T, 2) GRU latents inside nlc_mppi_buffers.workspace (-1: no NL planner)
 *   "gru_gemm"             1 when encode launches run the int8-sliced kernel (option "gru_gemm" = 1 and a hidden_units = 128 model)
 *   "gru_i8_launches"      launches of the int8-sliced encoder kernel in this PROCESS so far (any ctx): the option alone does not say
 *                          that a launch took it -- cooperative and fused launches keep their FP64 encoder
 *   "model_nt3"            16-wide output tiles of the representation MLP's last layer as packed by nlc_set_model (the bench's
 *                          issued-flop count needs it), 0 = no model
 * Unknown names: NLC_ERR_BAD_ARG. */
int nlc_get_stat(nlc_ctx* ctx, const char* name, double* out);
/* device properties the bench reports next to its roofline numbers */
int nlc_device_info(nlc_ctx* ctx, char* name, int name_len, int* num_cus, int* clock_mhz, double* hbm_gib);

/* ---- ILT: torchlaplace.laplace_reconstruct (external; call sites w_nl.py:137-144,
 *      w_latent_ode.py:88-94).  Parity unpinned vs upstream torchlaplace: alpha/tol/scale and the
 *      [theta_s | phi_s | p] input order are the recalled defaults, exposed here as parameters. ---- */
typedef struct {
  int32_t algo;  /* NLC_ILT_* */
  int32_t terms; /* S = ilt_reconstruction_terms (de Hoog: odd, 2M+1 <= 33; Stehfest: even <= 20) */
  double alpha;  /* fourier 1e-3, dehoog 1e-10 (unused by the linear algorithms, as are tol and scale) */
  double tol;    /* 10*alpha */
  double scale;  /* 2.0 */
} nlc_ilt_desc;

/* Contour evaluation + Riemann-sphere projection + concat: rows [theta_s(0..S-1) | phi_s(0..S-1) | p]
 * for every (batch row b, time point j).  t_dev is (B*Tt) if t_batched else (Tt) shared by all rows.
 * out_dev: (B, Tt, 2S+P). */
int nlc_ilt_rep_inputs(nlc_ctx* ctx, const nlc_ilt_desc* desc, const double* p_dev, const double* t_dev,
                       int t_batched, int64_t B, int64_t Tt, int P, double* out_dev);
/* Sphere -> complex map and line integral: theta_dev, phi_dev (N, d, S) rep-func outputs, t_dev (N)
 * -> x_dev (N, d).  HBM-bound streaming kernel for Fourier; algorithmic bytes (2dS+d)*8 per point. */
int nlc_ilt_reconstruct(nlc_ctx* ctx, const nlc_ilt_desc* desc, const double* theta_dev, const double* phi_dev,
                        const double* t_dev, int64_t N, int d, double* x_dev);

/* Backward of nlc_ilt_reconstruct with respect to the representation-function outputs, every algorithm: the
 * reference trains the rep func THROUGH torchlaplace.laplace_reconstruct by autograd (train_utils.py:388-407 ->
 * w_nl.py:137-144).  grad_x_dev (N, d) upstream gradient -> grad_theta_dev, grad_phi_dev (N, d, S).  No gradient
 * with respect to t.  Fourier / fixed Talbot / Stehfest: HBM-bound streaming kernels, algorithmic bytes 4dS*8 per point.
 * de Hoog: reverse mode through the quotient-difference table, taped in stream-ordered scratch of the call
 * (hipMallocAsync / hipFreeAsync on the bound stream: 7.5 KB per row in flight at S = 33 -- 466 complex values: the q columns,
 * the even e columns, the continued fraction's recurrence -- for at most 1024 resident wavefronts of 64 rows: 0.49 GB). */
int nlc_ilt_reconstruct_backward(nlc_ctx* ctx, const nlc_ilt_desc* desc, const double* theta_dev,
                                 const double* phi_dev, const double* t_dev, const double* grad_x_dev, int64_t N,
                                 int d, double* grad_theta_dev, double* grad_phi_dev);

/* ---- model: NeuralLaplaceModel (w_nl.py:66-145), ReverseGRUEncoder (:14-29),
 *      LaplaceRepresentationFunc (:32-63) ------------------------------------------------------- */
typedef struct {
  int32_t d;   /* state_dim (obs dim) */
  int32_t nin; /* GRU input dim = action_dim + encode_obs_time (w_nl.py:19-20) */
  int32_t h;   /* hidden_units (GRU hidden = h/2, w_nl.py:92) */
  nlc_ilt_desc ilt;
  double time_div; /* ts_pred is divided by this: dt*8 if normalize&&normalize_time else 1 (w_nl.py:122) */
  double state_mean[NLC_MAX_D], state_std[NLC_MAX_D];       /* identity (0,1) if !normalize */
  double action_mean[NLC_MAX_NIN], action_std[NLC_MAX_NIN]; /* (0,3) if !normalize (w_nl.py:129) */
} nlc_model_desc;

/* weights_host: float64 blob, tensors in the reference's state_dict order:
 *   gru.weight_ih_l0 (3g,nin) weight_hh_l0 (3g,g) bias_ih_l0 (3g) bias_hh_l0 (3g)
 *   gru.weight_ih_l1 (3g,g)   weight_hh_l1 (3g,g) bias_ih_l1 (3g) bias_hh_l1 (3g)
 *   linear_out.weight (2,g) linear_out.bias (2)
 *   linear_tanh_stack.0.weight (h,2S+d+2) .0.bias (h) .2.weight (h,h) .2.bias (h)
 *   .4.weight (2dS,h) .4.bias (2dS)
 * n_doubles must equal nlc_model_blob_size(desc).  The ctx repacks them into MFMA fragment order.
 * desc->ilt.algo: every implemented algorithm runs nlc_gru_encode, nlc_rep_func, nlc_model_forward and the planner
 * (NLC_DYN_NL; Fourier: fused rollout kernel, the others: staged all-HIP path); nlc_model_forward_const_t is Fourier only. */
int64_t nlc_model_blob_size(const nlc_model_desc* desc);
int nlc_set_model(nlc_ctx* ctx, const nlc_model_desc* desc, const double* weights_host, int64_t n_doubles);
/* ReverseGRUEncoder.forward on the model's normalised input: window_dev (N, B, nin) raw
 * (un-normalised) actions, B = window length (action_buffer_size, config.py:58) -> out_dev (N, 2) */
int nlc_gru_encode(nlc_ctx* ctx, const double* window_dev, int64_t N, int B, double* out_dev);
/* NeuralLaplaceModel.forward: obs_dev (N,d), window_dev (N,B,nin), ts_dev (N) raw ts_pred
 * -> out_dev (N,d) predicted state difference.  ws_dev: scratch of nlc_model_workspace_bytes(N). */
int64_t nlc_model_workspace_bytes(nlc_ctx* ctx, int64_t N);
int nlc_model_forward(nlc_ctx* ctx, const double* obs_dev, const double* window_dev, const double* ts_dev,
                      int64_t N, int B, double* out_dev, void* ws_dev);
/* The same with ONE query time for every row (what the harness closure passes: ts_pred = dt, mppi_with_model.py:74,
 * 120): the 2S sphere-coordinate inputs of the representation MLP are then constants and are folded into its first
 * bias on the host (once per value of ts_pred), as nlc_mppi_configure does for the fused planner.  Fourier models. */
int nlc_model_forward_const_t(nlc_ctx* ctx, const double* obs_dev, const double* window_dev, double ts_pred, int64_t N,
                              int B, double* out_dev, void* ws_dev);
/* a8 alone: LaplaceRepresentationFunc.forward (w_nl.py:55-63) on N explicit input rows
 * rep_in_dev (N, 2S + d + 2) = [theta_s (S) | phi_s (S) | latent p (d+2)] -- whatever sphere coordinates the caller
 * supplies, as torchlaplace hands them to the module -- -> theta_dev, phi_dev (N, d, S) with theta = pi tanh(.),
 * phi = (pi/2) tanh(.) (:59-62).  Same MFMA kernel as the de Hoog path's representation stage. */
int nlc_rep_func(nlc_ctx* ctx, const double* rep_in_dev, int64_t N, double* theta_dev, double* phi_dev);

/* ---- training: one iteration of the reference's loop over a NeuralLaplaceModel (train_utils.py:388-408, float64 as
 *      model.double() at :267): pred = model(bs0, ba0, bts); loss = MSELoss(pred.squeeze(), bsd.squeeze()); backward;
 *      clip_grad_norm_(params, max_grad_norm); Adam.step().  The shape comes from nlc_set_model on the same ctx; the kernels
 *      take what it takes with the Fourier ILT (scale 2) and with the linear algorithms, fixed Talbot and Stehfest (any scale:
 *      they have none; x = (1/t) Re sum_k W_k F(delta_k / t) with the node / weight tables of the forward).  de Hoog, a
 *      Stehfest series the tables do not hold (odd, or past 20 terms), or B > 16: NLC_ERR_UNSUPPORTED on the host, before
 *      any launch.
 *   params_dev, grad_dev, m_dev, v_dev: flat device arrays of nlc_model_blob_size doubles in nlc_set_model's blob order.
 *   obs_dev (M, d), window_dev (M, B, nin) raw actions, ts_dev (M) raw ts_pred, target_dev (M, d) = bsn - bs0 of the dataset;
 *   idx_dev (N) int64 row indices into them (the reference's permutation[iter*bs : iter*bs+bs], no gather copy).
 *   ws_dev: scratch of nlc_train_workspace_bytes(ctx, N).  Asynchronous on the ctx's stream; bit-reproducible (no
 *   floating-point atomics). */
typedef struct {
  double lr;            /* Adam lr (train_utils.py:281: config.learning_rate) */
  double beta1, beta2;  /* Adam betas (0.9, 0.999) */
  double eps;           /* Adam eps (1e-8) */
  double weight_decay;  /* L2 added to the clipped gradient inside the step, as torch.optim.Adam (0) */
  double max_grad_norm; /* clip_grad_norm_'s max_norm (config.clip_grad_norm = 0.1); <= 0: no clipping */
} nlc_train_desc;
int64_t nlc_train_workspace_bytes(nlc_ctx* ctx, int64_t N);
/* loss and gradient only (train_utils.py:391-402): grad_dev (blob order) = d loss / d params, loss_dev (0-dim) = the MSE */
int nlc_train_loss_grad(nlc_ctx* ctx, const double* params_dev, const double* obs_dev, const double* window_dev,
                        const double* ts_dev, const double* target_dev, const int64_t* idx_dev, int64_t N, int B,
                        double* grad_dev, double* loss_dev, void* ws_dev);
/* the whole iteration (train_utils.py:391-404): params_dev, m_dev (exp_avg), v_dev (exp_avg_sq) updated in place; step = the
 * Adam step count of this update (1 for the first); loss_dev the MSE before the update, gradnorm_dev (may be NULL) the total
 * gradient norm before clipping (clip_grad_norm_'s return value). */
int nlc_train_step(nlc_ctx* ctx, const nlc_train_desc* desc, double* params_dev, double* m_dev, double* v_dev, int64_t step,
                   const double* obs_dev, const double* window_dev, const double* ts_dev, const double* target_dev,
                   const int64_t* idx_dev, int64_t N, int B, double* loss_dev, double* gradnorm_dev, void* ws_dev);
/* ---- grouped training: M models of one descriptor in the same three launches, the member on the grid's y axis.  The
 *      reference trains one model per (env, delay, model_name) (run_exp_multi.py:105-110), times seeds; for a fixed env and
 *      family these share the architecture and the normalisation constants and differ in weights and data, and one model's
 *      iteration (train_utils.py:388-408) occupies one compute unit.  Contract of the three entries above, plus:
 *   params_dev, m_dev, v_dev, grad_dev: [M][P] (P = nlc_model_blob_size); idx_dev: [M][N]; loss_dev, gradnorm_dev: [M]
 *   (gradnorm_dev may be NULL); one nlc_train_desc and one Adam step count for the whole group.
 *   data_row_stride: 0 = every member reads the same obs / window / ts / target; R > 0 = they are stacked, member m reads
 *   rows [m R, (m + 1) R) (its idx entries index within them).
 *   ws_dev: nlc_train_group_workspace_bytes(ctx, M, N) = M x the single-model layout, each region 256-byte aligned.
 *   The refusals of the single entries apply; M < 1 or data_row_stride < 0: NLC_ERR_BAD_SHAPE; M > 65535 (the grid's y
 *   limit): NLC_ERR_UNSUPPORTED; all on the host before any launch.  No atomics and no cross-member reads: a member's
 *   results are bit-identical whatever M and its neighbours are, and the single entries are the M = 1, stride 0 case. */
/* train_utils.py:388-408, run_exp_multi.py:105-110 */
int64_t nlc_train_group_workspace_bytes(nlc_ctx* ctx, int M, int64_t N);
/* train_utils.py:391-402 per member, run_exp_multi.py:105-110 */
int nlc_train_group_loss_grad(nlc_ctx* ctx, int M, int64_t data_row_stride, const double* params_dev, const double* obs_dev,
                              const double* window_dev, const double* ts_dev, const double* target_dev,
                              const int64_t* idx_dev, int64_t N, int B, double* grad_dev, double* loss_dev, void* ws_dev);
/* train_utils.py:391-404 per member, run_exp_multi.py:105-110 */
int nlc_train_group_step(nlc_ctx* ctx, const nlc_train_desc* desc, int M, int64_t data_row_stride, double* params_dev,
                         double* m_dev, double* v_dev, int64_t step, const double* obs_dev, const double* window_dev,
                         const double* ts_dev, const double* target_dev, const int64_t* idx_dev, int64_t N, int B,
                         double* loss_dev, double* gradnorm_dev, void* ws_dev);

/* ---- held-out loss: the forward and MSE of the reference's validation loss (overlay.py:112-115
 *      get_val_loss_delay_precomputed; :175-177: model(s0, a0, ts), then the loss) on the data conventions of the training
 *      entries above, with no backward, no update and no (N, d) prediction.  loss_dev [M] = mean squared error of member m over
 *      its N rows; idx_dev [M][N] as for a step, or NULL: every member takes rows 0 .. N - 1.  Contract and host-side refusals
 *      of nlc_train_group_loss_grad (de Hoog and B > 16: NLC_ERR_UNSUPPORTED; N < 1, M < 1, data_row_stride < 0:
 *      NLC_ERR_BAD_SHAPE; M > 65535: NLC_ERR_UNSUPPORTED; no model: NLC_ERR_STATE), all before any launch.
 *   ws_dev: nlc_train_group_eval_workspace_bytes(ctx, M, N): the tile losses only, M regions of ceil(N / 16) doubles, each
 *   rounded up to a multiple of 256 bytes.  Asynchronous on the ctx's stream; no floating-point atomics: a member's loss does
 *   not depend on the grid, on M or on its neighbours; the single entries are the M = 1, stride 0 case. */
/* overlay.py:112-115, :175-177, run_exp_multi.py:105-110 */
int64_t nlc_train_group_eval_workspace_bytes(nlc_ctx* ctx, int M, int64_t N);
/* overlay.py:112-115, :175-177 per member, run_exp_multi.py:105-110 */
int nlc_train_group_eval(nlc_ctx* ctx, int M, int64_t data_row_stride, const double* params_dev, const double* obs_dev,
                         const double* window_dev, const double* ts_dev, const double* target_dev,
                         const int64_t* idx_dev /* NULL: rows 0..N-1 */, int64_t N, int B, double* loss_dev /* [M] */,
                         void* ws_dev);
/* overlay.py:112-115, :175-177 */
int64_t nlc_train_eval_workspace_bytes(nlc_ctx* ctx, int64_t N);
/* overlay.py:112-115, :175-177 */
int nlc_train_eval(nlc_ctx* ctx, const double* params_dev, const double* obs_dev, const double* window_dev,
                   const double* ts_dev, const double* target_dev, const int64_t* idx_dev /* NULL: rows 0..N-1 */, int64_t N,
                   int B, double* loss_dev, void* ws_dev);

/* ---- baseline models: DeltaTRNN (train_utils.py:589-631; factory :56-74) and RNN (:550-586; factory :77-98);
 *      rnn_hidden_units config.py:43 ------
 * out, _ = GRU(nin -> hidden, 1 layer, batch_first)(window_n); dx = linear_out(cat(out[:, -1], obs_n, ts_n)). */
typedef struct {
  int32_t d;      /* state_dim */
  int32_t nin;    /* GRU input dim = action_dim (+1 for an encode_obs_time model; forward API only) */
  int32_t hidden; /* hidden_units: 64, 128 or 160 */
  int32_t time_input; /* 1: DeltaTRNN (linear_out sees ts); 0: the plain RNN baseline (train_utils.py:550-586), whose
                       * linear_out is (d, H+d) and which ignores ts_pred */
  /* The caller resolves the reference's branch structure (train_utils.py:618-626; the `else` of the raw-input branch
   * belongs to `if self.normalize_time`): normalised branch -> the model's buffers and time_div = dt*8; raw branch
   * (normalize_time False) -> state (0, 1), action (0, 3), time_div 1. */
  double time_div;
  double state_mean[NLC_MAX_D], state_std[NLC_MAX_D];
  double action_mean[NLC_MAX_NIN], action_std[NLC_MAX_NIN];
} nlc_rnn_desc;
/* weights_host: float64 blob in the reference's state_dict order:
 *   gru.weight_ih_l0 (3H,nin) gru.weight_hh_l0 (3H,H) gru.bias_ih_l0 (3H) gru.bias_hh_l0 (3H)
 *   linear_out.weight (d, H+d+time_input) linear_out.bias (d) */
int64_t nlc_rnn_blob_size(const nlc_rnn_desc* desc);
int nlc_set_rnn_model(nlc_ctx* ctx, const nlc_rnn_desc* desc, const double* weights_host, int64_t n_doubles);
/* DeltaTRNN.forward: obs_dev (N,d), window_dev (N,B,nin) raw actions, ts_dev (N) raw ts_pred -> out_dev (N,d)
 * predicted state difference.  ws_dev: N*d doubles of scratch. */
int nlc_rnn_forward(nlc_ctx* ctx, const double* obs_dev, const double* window_dev, const double* ts_dev, int64_t N,
                    int B, double* out_dev, void* ws_dev);
/* ---- training of these two models: the same iteration (train_utils.py:388-408 over DeltaTRNN.forward :618-631 /
 *      RNN.forward :577-586), signatures and contract as nlc_train_workspace_bytes / nlc_train_loss_grad / nlc_train_step
 *      above (nlc_train_desc is reused).  The shape comes from nlc_set_rnn_model on the same ctx (without it: NLC_ERR_STATE);
 *      B outside 1..16: NLC_ERR_UNSUPPORTED; N < 1: NLC_ERR_BAD_SHAPE; all checked on the host before any launch.
 *   params_dev, grad_dev, m_dev, v_dev: nlc_rnn_blob_size doubles in nlc_set_rnn_model's blob order.
 *   ts_dev is read only by a time_input model (may be NULL otherwise). */
int64_t nlc_rnn_train_workspace_bytes(nlc_ctx* ctx, int64_t N);
/* train_utils.py:391-402 */
int nlc_rnn_train_loss_grad(nlc_ctx* ctx, const double* params_dev, const double* obs_dev, const double* window_dev,
                            const double* ts_dev, const double* target_dev, const int64_t* idx_dev, int64_t N, int B,
                            double* grad_dev, double* loss_dev, void* ws_dev);
/* train_utils.py:391-404 */
int nlc_rnn_train_step(nlc_ctx* ctx, const nlc_train_desc* desc, double* params_dev, double* m_dev, double* v_dev,
                       int64_t step, const double* obs_dev, const double* window_dev, const double* ts_dev,
                       const double* target_dev, const int64_t* idx_dev, int64_t N, int B, double* loss_dev,
                       double* gradnorm_dev, void* ws_dev);
/* grouped training of these two models: layout and contract of nlc_train_group_* above (P = nlc_rnn_blob_size) */
/* train_utils.py:388-408, run_exp_multi.py:105-110 */
int64_t nlc_rnn_train_group_workspace_bytes(nlc_ctx* ctx, int M, int64_t N);
/* train_utils.py:391-402 per member, run_exp_multi.py:105-110 */
int nlc_rnn_train_group_loss_grad(nlc_ctx* ctx, int M, int64_t data_row_stride, const double* params_dev,
                                  const double* obs_dev, const double* window_dev, const double* ts_dev,
                                  const double* target_dev, const int64_t* idx_dev, int64_t N, int B, double* grad_dev,
                                  double* loss_dev, void* ws_dev);
/* train_utils.py:391-404 per member, run_exp_multi.py:105-110 */
int nlc_rnn_train_group_step(nlc_ctx* ctx, const nlc_train_desc* desc, int M, int64_t data_row_stride, double* params_dev,
                             double* m_dev, double* v_dev, int64_t step, const double* obs_dev, const double* window_dev,
                             const double* ts_dev, const double* target_dev, const int64_t* idx_dev, int64_t N, int B,
                             double* loss_dev, double* gradnorm_dev, void* ws_dev);

/* held-out loss of these two models: layout and contract of nlc_train_group_eval above (P = nlc_rnn_blob_size; ts_dev may be
 * NULL for a model without time input) */
/* overlay.py:112-115, :175-177, run_exp_multi.py:105-110 */
int64_t nlc_rnn_train_group_eval_workspace_bytes(nlc_ctx* ctx, int M, int64_t N);
/* overlay.py:112-115, :175-177 per member, run_exp_multi.py:105-110 */
int nlc_rnn_train_group_eval(nlc_ctx* ctx, int M, int64_t data_row_stride, const double* params_dev, const double* obs_dev,
                             const double* window_dev, const double* ts_dev, const double* target_dev,
                             const int64_t* idx_dev /* NULL: rows 0..N-1 */, int64_t N, int B, double* loss_dev /* [M] */,
                             void* ws_dev);
/* overlay.py:112-115, :175-177 */
int64_t nlc_rnn_train_eval_workspace_bytes(nlc_ctx* ctx, int64_t N);
/* overlay.py:112-115, :175-177 */
int nlc_rnn_train_eval(nlc_ctx* ctx, const double* params_dev, const double* obs_dev, const double* window_dev,
                       const double* ts_dev, const double* target_dev, const int64_t* idx_dev /* NULL: rows 0..N-1 */,
                       int64_t N, int B, double* loss_dev, void* ws_dev);

/* ---- snapshot selection: keep the parameters of the best loss seen so far, per member, on the device -- the reference saves
 *      model.state_dict() whenever a window's loss beats best_loss (train_utils.py:439-448) and reports best_val_loss (:491).
 *      Independent of the model family (the NL and RNN trainers share it) and of any model in the ctx.
 *   loss_dev, best_loss_dev [M]; params_dev, best_params_dev [M][P]; best_tag_dev [M]; improved_dev [M] int32, or NULL.
 *   Member m improves iff loss[m] < best_loss[m]: strict; a NaN loss never improves and a NaN best is never replaced; start
 *   best_loss at +inf (+inf then never improves, -inf does once).  On improvement best_params[m][:] = params[m][:],
 *   best_loss[m] = loss[m], best_tag[m] = tag, improved[m] = 1; otherwise nothing of member m is written but improved[m] = 0.
 *   Two launches on the ctx's stream, no atomics, no host synchronisation: the copy (member on the grid's y axis, best_loss
 *   read-only, a member that did not improve costs two 8-byte reads per workgroup), then one thread per member commits
 *   best_loss, best_tag and improved.  Rows of odd P are copied with 8-byte accesses where they are not 16-byte aligned.
 *   Refused on the host before any launch: a NULL pointer other than improved_dev, params_dev == best_params_dev:
 *   NLC_ERR_BAD_ARG; M < 1 or P < 1: NLC_ERR_BAD_SHAPE; M > 65535 (the grid's y limit): NLC_ERR_UNSUPPORTED. */
/* train_utils.py:439-448 (save on improvement), :491 (best_val_loss) */
int nlc_train_keep_best(nlc_ctx* ctx, int M, int64_t P, const double* loss_dev, const double* params_dev,
                        double* best_loss_dev, double* best_params_dev, int64_t* best_tag_dev, int64_t tag,
                        int32_t* improved_dev /* (M), may be NULL */);

/* ---- baseline model: NODE (train_utils.py:664-724; ODE function xOdeFuncInXAndU :637-661; factory :101-125;
 * node_hidden_units 270, node_augment_dim 1, node_method "euler": config.py:40-42).
 *   x = cat((obs - mean)/std, zeros(augment_dim)); u = window[:, -1, :] (raw);
 *   out = odeint(f(., u), x, [0, ts_pred[0] / time_div], method, step_size)[-1][:, :d]
 * torchdiffeq's fixed-grid solvers are restated (grid t_k = k*step_size, last point = the end time; method = the ctx option
 * "node_method": euler, midpoint, or rk4 = the 3/8 rule; one sub-step Y_i = y + h sum_j a_ij k_j, k_i = f(Y_i),
 * y' = y + h sum_i b_i k_i, csrc/nlc_node_rk.h): grid and solvers alike
 * PARITY UNPINNED vs upstream torchdiffeq (absent offline); everything else is pinned against the reference classes.
 * A prediction time may need at most 8 sub-steps in nlc_node_forward and the planner, whatever the method. */
typedef struct {
  int32_t d;           /* state_dim */
  int32_t nu;          /* action_dim */
  int32_t hidden;      /* hidden_units, <= 272 */
  int32_t augment_dim; /* d + augment_dim <= 8, d + augment_dim + nu <= 12 */
  double time_div;     /* dt*8 if normalize_time else 1 (train_utils.py:701-702) */
  double step_size;    /* options["step_size"] = 0.05 (:722) */
  double state_mean[NLC_MAX_D], state_std[NLC_MAX_D]; /* (0, 1) if !normalize */
} nlc_node_desc;
/* weights_host: float64 blob in state_dict order: x_ode_func_in_x_and_u.linear_tanh_stack.{0,2,4}.{weight,bias}:
 *   (H, d+aug+nu) (H) (H, H) (H) (d+aug, H) (d+aug) */
int64_t nlc_node_blob_size(const nlc_node_desc* desc);
int nlc_set_node_model(nlc_ctx* ctx, const nlc_node_desc* desc, const double* weights_host, int64_t n_doubles);
/* NODE.forward: obs_dev (N,d), action_dev (N,nu) = window[:, -1, :], ts_pred = the FIRST row's raw prediction time
 * (the reference integrates every row to ts_pred[0], :719) -> out_dev (N,d) integrated normalised state. */
int nlc_node_forward(nlc_ctx* ctx, const double* obs_dev, const double* action_dev, double ts_pred, int64_t N,
                     double* out_dev);
/* ---- training of the NODE: the same iteration (train_utils.py:388-408 over NODE.forward :696-724; the loss is the MSE of
 *      the integrated normalised state against target), signatures and contract of nlc_rnn_train_group_* above plus row_times.
 *      The model comes from nlc_set_node_model on the same ctx (without it: NLC_ERR_STATE); N < 1 or M < 1:
 *      NLC_ERR_BAD_SHAPE; M > 65535 or B outside 1..16: NLC_ERR_UNSUPPORTED; all checked on the host before any launch.
 *   params_dev, grad_dev, m_dev, v_dev [M][P], P = nlc_node_blob_size, in nlc_set_node_model's blob order (unpadded).
 *   window_dev (rows, B, nu): the newest action window[:, B-1, :] is read, raw.  ts_dev (rows): raw prediction times.
 *   row_times == 0: every row of a member's batch integrates to the time of its first row, ts[idx[0]] (:719, what NODE.forward
 *   does); != 0: each row to its own ts[idx[r]].  The sub-step counts are formed on the device (torchdiffeq's fixed grid:
 *   ceil(t / step_size + 1) points); nothing reads ts on the host.  A row takes at most 256 evaluations of the ODE function
 *   (256 euler, 128 midpoint, 64 rk4 sub-steps; the stage inputs are taped where Euler tapes its states): the workspace is a
 *   function of (M, N) and the model's shape alone and the same for every method, and a row whose time is not positive, is NaN,
 *   or needs more sub-steps gets a NaN squared error (so the member's loss is NaN) and touches no memory outside the workspace.
 *   The backward of a sub-step: kbar_i = h b_i ybar'; for i = s .. 1: Ybar_i = J_f(Y_i)^T kbar_i, kbar_j += h a_ij Ybar_i (j < i);
 *   ybar = ybar' + sum_i Ybar_i.
 *   The single-model forms are M = 1, data_row_stride = 0.  Three launches (training) or two (evaluation) on the ctx's stream,
 *   no atomics, no host synchronisation. */
/* train_utils.py:388-408, run_exp_multi.py:105-110 */
int64_t nlc_node_train_group_workspace_bytes(nlc_ctx* ctx, int M, int64_t N);
/* train_utils.py:391-402 per member, run_exp_multi.py:105-110 */
int nlc_node_train_group_loss_grad(nlc_ctx* ctx, int M, int64_t data_row_stride, const double* params_dev,
                                   const double* obs_dev, const double* window_dev, const double* ts_dev,
                                   const double* target_dev, const int64_t* idx_dev, int64_t N, int B, double* grad_dev,
                                   double* loss_dev, void* ws_dev, int row_times);
/* train_utils.py:391-404 per member, run_exp_multi.py:105-110 */
int nlc_node_train_group_step(nlc_ctx* ctx, const nlc_train_desc* desc, int M, int64_t data_row_stride, double* params_dev,
                              double* m_dev, double* v_dev, int64_t step, const double* obs_dev, const double* window_dev,
                              const double* ts_dev, const double* target_dev, const int64_t* idx_dev, int64_t N, int B,
                              double* loss_dev, double* gradnorm_dev, void* ws_dev, int row_times);
/* overlay.py:112-115, :175-177, run_exp_multi.py:105-110 */
int64_t nlc_node_train_group_eval_workspace_bytes(nlc_ctx* ctx, int M, int64_t N);
/* overlay.py:112-115, :175-177 per member, run_exp_multi.py:105-110 */
int nlc_node_train_group_eval(nlc_ctx* ctx, int M, int64_t data_row_stride, const double* params_dev, const double* obs_dev,
                              const double* window_dev, const double* ts_dev, const double* target_dev,
                              const int64_t* idx_dev /* NULL: rows 0..N-1 */, int64_t N, int B, double* loss_dev /* [M] */,
                              void* ws_dev, int row_times);

/* ---- per-member settings and patience of a group: a sweep over learning rate, weight decay or clip norm (config.py:
 *      sweep_mode, learning_rate, weight_decay, clip_grad_norm) as one group, each member stopping when it stops improving
 *      (waiting / patience, train_utils.py:315-317, :439-448).
 *   The three _members entries are their _group_step with a trailing nlc_train_members: four device arrays [M] read by the
 *   clip + Adam launch in place of desc's lr, weight_decay and max_grad_norm (which are then not read; the betas, eps and the
 *   step count stay one per group).  max_norm <= 0: no clipping; wd == 0: no decay term.  A member with active == 0 is frozen:
 *   its rows of params_dev, m_dev and v_dev are neither read nor written by the update; its forward, backward and reduction
 *   still run, so loss_dev and gradnorm_dev report it.  An active member's results are bit-identical to _group_step's with
 *   its scalars.  The checks are _group_step's, in their order; a NULL struct or a NULL array in it: NLC_ERR_BAD_ARG, before
 *   any launch. */
typedef struct {
  const double* lr_dev;       /* [M] learning rates */
  const double* wd_dev;       /* [M] weight decays */
  const double* max_norm_dev; /* [M] clip_grad_norm_'s max_norm; <= 0: no clipping */
  const int32_t* active_dev;  /* [M] 0: frozen */
} nlc_train_members;
/* train_utils.py:391-404 per member, config.py (sweep_mode) */
int nlc_train_group_step_members(nlc_ctx* ctx, const nlc_train_desc* desc, int M, int64_t data_row_stride, double* params_dev,
                                 double* m_dev, double* v_dev, int64_t step, const double* obs_dev, const double* window_dev,
                                 const double* ts_dev, const double* target_dev, const int64_t* idx_dev, int64_t N, int B,
                                 double* loss_dev, double* gradnorm_dev, void* ws_dev, const nlc_train_members* members);
/* train_utils.py:391-404 per member, config.py (sweep_mode) */
int nlc_rnn_train_group_step_members(nlc_ctx* ctx, const nlc_train_desc* desc, int M, int64_t data_row_stride,
                                     double* params_dev, double* m_dev, double* v_dev, int64_t step, const double* obs_dev,
                                     const double* window_dev, const double* ts_dev, const double* target_dev,
                                     const int64_t* idx_dev, int64_t N, int B, double* loss_dev, double* gradnorm_dev,
                                     void* ws_dev, const nlc_train_members* members);
/* train_utils.py:391-404 per member, config.py (sweep_mode) */
int nlc_node_train_group_step_members(nlc_ctx* ctx, const nlc_train_desc* desc, int M, int64_t data_row_stride,
                                      double* params_dev, double* m_dev, double* v_dev, int64_t step, const double* obs_dev,
                                      const double* window_dev, const double* ts_dev, const double* target_dev,
                                      const int64_t* idx_dev, int64_t N, int B, double* loss_dev, double* gradnorm_dev,
                                      void* ws_dev, int row_times, const nlc_train_members* members);
/* The reference's early-stopping counter at one check, per member and on the device, after nlc_train_keep_best in stream
 * order (improved_dev is its flags): an active member that improved gets waiting = 0; else, if waiting > patience, active = 0
 * and stopped_at = tag; else waiting += 1.  A member with active == 0 is left alone.  patience may be +inf (the reference's
 * default: nobody stops).  Needs no model in the ctx.  Refused on the host before any launch: a NULL pointer or a NaN
 * patience: NLC_ERR_BAD_ARG; M < 1: NLC_ERR_BAD_SHAPE; M > 65535: NLC_ERR_UNSUPPORTED. */
/* train_utils.py:315-317, :439-448 */
int nlc_train_patience(nlc_ctx* ctx, int M, const int32_t* improved_dev, int64_t* waiting_dev, int32_t* active_dev,
                       int64_t* stopped_at_dev, double patience, int64_t tag);

/* ---- planner: MPPIDelay (planners/mppi_delay.py:54-381) ------------------------------------- */
typedef struct {
  int64_t K;        /* samples owned by THIS ctx (its shard of the population) */
  int64_t K_global; /* whole population (== K on one GPU) */
  int64_t k_offset; /* global index of this shard's first sample (Philox counters, sample_null_action) */
  int32_t T;        /* horizon */
  int32_t nu;       /* action dims */
  int32_t d;        /* nx */
  int32_t B;        /* rows of action_buffer */
  double lambda_;
  double u_scale;
  int32_t has_bounds; /* u_min/u_max given (mppi_delay.py:143-153) */
  double u_min[NLC_MAX_NU], u_max[NLC_MAX_NU];
  double u_init[NLC_MAX_NU];
  double noise_mu[NLC_MAX_NU];
  double noise_sigma[NLC_MAX_NU * NLC_MAX_NU];     /* covariance, row-major nu x nu */
  double noise_sigma_inv[NLC_MAX_NU * NLC_MAX_NU]; /* torch.inverse(noise_sigma) (:157) */
  double noise_chol[NLC_MAX_NU * NLC_MAX_NU];      /* lower Cholesky factor (device RNG only) */
  int32_t sample_null_action; /* :322-323 */
  int32_t noise_abs_cost;     /* :329-330 */
  int32_t u_per_command;      /* :217-220 */
  int32_t dynamics;           /* NLC_DYN_* */
  int32_t env;                /* NLC_ENV_* running cost (and oracle dynamics) */
  int32_t delay;              /* oracle dynamics: action applied = window[-(delay+1)] */
  int32_t friction;           /* oracle cartpole only */
  int32_t E;                  /* episodes: independent planning problems batched in this ctx, each with its own
                               * state, action_buffer, U and K samples (0 or 1 = one problem = the reference's
                               * MPPIDelay; > 1 = the dataset collector's many episodes,
                               * mppi_dataset_collector.py:224-321,402-424, planned side by side) */
  int32_t cost_external;      /* 1: the dynamics run fused but the caller evaluates running_cost / terminal cost itself
                               * (arbitrary harness closures, e.g. the state_constraint / change_goal branches of
                               * mppi_with_model.py:145-171): nlc_mppi_rollout leaves only the perturbation cost
                               * (:343-344) in buf->cost_total and stops before the weights; the caller adds its cost
                               * (buf->states must be given) and calls nlc_mppi_weights.  env is then used by oracle
                               * dynamics only and may be -1 with NL dynamics. */
  int32_t cost_variant;       /* NLC_COST_* bits of the in-kernel running cost: the state_constraint / change_goal branches of
                               * the harness closure (mppi_with_model.py:42-43, 146-162; mppi_dataset_collector.py:45-46,
                               * 137-156) on NLC_ENV_CARTPOLE / NLC_ENV_CARTPOLE_NOTRIG.  0 = the default branch (:163).
                               * Any bit on another env: NLC_ERR_UNSUPPORTED; bits outside NLC_COST_VARIANT_MASK:
                               * NLC_ERR_BAD_SHAPE; both before any launch.  Ignored with cost_external.  The
                               * latency-split and one-launch bodies evaluate a variant in compile-time instances of
                               * their own; behind every other body one launch evaluates it on the stored rollout
                               * (buf->states must then be given), before the importance weights.  A flipped bit
                               * without NLC_COST_CHANGE_GOAL selects nothing. */
  double ts_pred;             /* raw dt handed to the dynamics (mppi_with_model.py:74) */
} nlc_mppi_desc;

/* caller-owned device buffers the kernels read/write (the Python mirror keeps them as the public
 * attributes .noise .perturbed_action .states .actions .cost_total .cost_total_non_zero .omega).
 * With E > 1 episodes every buffer gains a leading E: per-sample ones are (E,K,...), partials
 * (E, 2+T*nu), action (E, u_per_command*nu); U is (E,T,nu). */
typedef struct {
  double* noise;      /* (K,T,nu) in: raw N(mu,Sigma) draw when rng == 0; out: bounded noise (:328) */
  double* perturbed;  /* (K,T,nu) out: bounded perturbed action, normalised units (:325-326) */
  double* states;     /* (K,T,d)  out, may be NULL */
  double* actions;    /* (K,T,nu) out = perturbed (actions/u_scale, :340), may be NULL */
  double* cost_total; /* (K) out */
  double* cost_nz;    /* (K) out: exp(-(cost-beta)/lambda) */
  double* omega;      /* (K) out: cost_nz/eta, may be NULL */
  double* partials;   /* (2+T*nu) out: this shard's (beta_r, eta_r, S_r[t,j]) */
  double* action;     /* (u_per_command*nu) out: the returned action, on the device; may be NULL */
  void* workspace;    /* nlc_mppi_workspace_bytes() bytes of scratch */
} nlc_mppi_buffers;

/* NLC_DYN_NL: the model's GRU input dim must be nu, or nu+1 for an encode_obs_time model -- the rollout then
 * appends the constant time channel B-1 .. 0 the harness closure builds (mppi_with_model.py:110-119).
 * NLC_DYN_DTRNN: needs nlc_set_rnn_model first; GRU input dim == nu (the closure adds the time channel for
 * model_name == "nl" only).  NLC_DYN_NODE: needs nlc_set_node_model first. */
int nlc_mppi_configure(nlc_ctx* ctx, const nlc_mppi_desc* desc);
int64_t nlc_mppi_workspace_bytes(nlc_ctx* ctx);
int nlc_mppi_set_U(nlc_ctx* ctx, const double* U_host); /* (E,T,nu) control sequence(s), :161-164 */
int nlc_mppi_get_U(nlc_ctx* ctx, double* U_host);
/* The reference's running_cost reads the global change_goal_flipped on EVERY call (mppi_with_model.py:153-158, set by the
 * evaluation loop :231-232, 251-253): sets or clears NLC_COST_GOAL_FLIPPED of the configured planner -- one host word, no
 * launch, no reconfiguration; U, the command counter and the noise stream are untouched.  Commands from the next
 * nlc_mppi_rollout on see it.  NLC_ERR_STATE without a configured planner or without
 * NLC_COST_CHANGE_GOAL in its cost_variant; NLC_ERR_UNSUPPORTED on a non-cartpole env. */
int nlc_mppi_set_goal_flipped(nlc_ctx* ctx, int flipped);
/* Phase 1 of command(): shift U (:199-200), sample/perturb/bound (:319-335), hoisted GRU encode,
 * T-step rollout + running cost (:232-313), perturbation cost (:343-344), and this shard's
 * softmax partials (beta_r, eta_r, S_r) into buf->partials.
 *   state_host: (d) or (K,d) if state_per_sample (:243-246); action_buffer_host: (B,nu).
 *   E > 1: state (E,d) or (E,K,d), action_buffer (E,B,nu); both may then be host OR device pointers.
 *   rng: 0 = buf->noise holds the caller's raw draw; 1 = device Philox4x32-10(seed, counter): sample k of episode e, horizon
 *   step t takes the block of counter words (kg lo, kg hi, t, counter lo) under the key (seed lo, seed hi ^ counter hi), with
 *   kg = e * K_global + k_offset + k the GLOBAL sample index, so a draw does not depend on the sharding.  The block's words
 *   0, 1 and 2, 3 make two 53-bit uniforms u1, u2 in (0, 1), z = sqrt(-2 ln u1) (cos, sin)(2 pi u2 - pi), and
 *   eps = noise_mu + noise_chol z (the lower factor; nu = 1 takes z[0]). */
int nlc_mppi_rollout(nlc_ctx* ctx, const double* state_host, int state_per_sample,
                     const double* action_buffer_host, const nlc_mppi_buffers* buf, int rng, uint64_t seed,
                     uint64_t counter);
/* NLC_DYN_EXTERNAL / cost_external: nlc_mppi_rollout stops after the perturbation / after the rollout; once the
 * caller has completed buf->cost_total (rollout cost + perturbation cost, :339-344) this computes the softmax
 * partials.
 * Non-finite costs (this call and the weights inside nlc_mppi_rollout alike): a +inf cost weighs exactly 0 at every level
 * of the fold -- also when a whole 16-sample tile, 64-tile chunk, episode or shard is +inf -- so the partials are those of
 * the population without these samples, as the reference's one-level softmax gives them.  A NaN or -inf cost makes
 * eta_r NaN; a shard whose costs are all +inf has (beta_r, eta_r, S_r) = (+inf, 0, 0). */
int nlc_mppi_weights(nlc_ctx* ctx, const nlc_mppi_buffers* buf);
/* Phase 2: merge G shard partials (gathered_dev: (G, E, 2+T*nu); pass buf->partials and G=1 on one GPU; NULL: gather
 * them with the ctx's own communicator, see the multi-GPU note below),
 * omega, U[t] += sum_k omega_k noise[k,t] (:210-216) and return action = U[:u_per_command]*u_scale
 * (:217-224) into action_host (E*u_per_command*nu) -- the call waits until the ACTION is in host memory (see "host_spin":
 * cost_nz / omega may still be in flight on the stream; nlc_synchronize before reading them from the host) -- and/or into
 * buf->action on the device.  With action_host == NULL nothing is copied back and the call does not synchronise.
 * Returns NLC_AGAIN (> 0, not an error) when a sharded command had to be re-run and the caller owns the collective.
 * Non-finite costs: a shard with beta_r = +inf is merged with scale exactly 0; +inf samples get cost_nz = omega = 0 and the
 * action is finite whenever one cost of the population is.  A NaN or -inf cost anywhere, or +inf costs everywhere
 * (eta = 0), give a NaN action and NaN U, as in the reference: poisoned costs are never turned into a finite action. */
int nlc_mppi_finish(nlc_ctx* ctx, const double* gathered_dev, int G, int rank, const nlc_mppi_buffers* buf,
                    double* action_host);
/* Multi-GPU: the one exchange of a K-sharded command is the all-gather of buf->partials ((2+T*nu) doubles per rank and
 * episode) between nlc_mppi_rollout and nlc_mppi_finish (reference reduction :210-216).  Two ways:
 *   (1) the caller brings the collective and passes `gathered_dev`: torch.distributed over RCCL in the Python mirror
 *       (sharding.py, the default there), MPI_Allgather / its own RCCL communicator for a C caller -- the library does not
 *       compete with the host framework for the collective stream, ranks or device selection;
 *   (2) the library's own communicator (SURVEY 8b's sketch): rank 0 draws an id with nlc_comm_unique_id and ships the
 *       NLC_COMM_ID_BYTES bytes to every rank by any means, every rank calls nlc_comm_init on its ctx (its device), and
 *       nlc_mppi_finish with gathered_dev == NULL then runs ONE ncclAllGather on the command's own stream before the
 *       merge -- no host hop between the rollout and the action.  RCCL is bound at run time (dlopen of librccl.so.1; the
 *       copy already in the process is used if there is one); without it these return NLC_ERR_UNSUPPORTED.
 * nlc_comm_unique_id has no ctx: its error text is returned by nlc_last_error(NULL). */
#define NLC_COMM_ID_BYTES 128
int nlc_comm_unique_id(void* id_out);
int nlc_comm_init(nlc_ctx* ctx, int rank, int world, const void* id);
int nlc_comm_destroy(nlc_ctx* ctx);
/* Collective: every rank all-gathers its rank number over the communicator and checks the result on the host (the Python
 * mirror runs it once after nlc_comm_init and falls back to torch.distributed's collective if any rank fails). */
int nlc_comm_self_test(nlc_ctx* ctx);

/* ---- env side of the evaluation loop: the reference steps ONE env per process on the host,
 * step_env (mppi_with_model.py:193-216) = get_action (delay buffer, :25-28) + env.integrate_system(2, g, s0)
 * (base_env.py:136-173; solver "euler" overlay.py:39, ts = [0, dt]: one Euler step of torch_rhs on the reduced
 * state) + get_obs (:83-89).  Here E independent envs advance on the device, next to a batched planner (E > 1), so a
 * control step needs no host round trip.
 *   state_dev (E, n) reduced states (cartpole [x, xdot, theta, thetadot], pendulum [theta, thetadot], acrobot
 *   [theta1, theta2, v1, v2]), updated in place; action_buffer_dev (E, B, nu) rolled in place, the new action
 *   appended, row -(delay+1) applied; action_dev (E, nu); obs_dev (E, d) trig observation of the new state;
 *   reward_dev (E) diff_reward(new state, applied action), may be NULL. */
int nlc_env_step(nlc_ctx* ctx, int env, int friction, double dt, int delay, int64_t E, int B, int nu,
                 double* state_dev, double* action_buffer_dev, const double* action_dev, double* obs_dev,
                 double* reward_dev);
/* get_obs (base_env.py:83-89): obs_dev (E, d) = torch_transform_states(state_dev (E, n)) */
int nlc_env_obs(nlc_ctx* ctx, int env, int64_t E, const double* state_dev, double* obs_dev);

/* ---- expert-data collection (mppi_dataset_collector.py:33-321): one control step of the collector's loop() / step_env()
 * (:192-222, 241-268) for E envs side by side, recorded into the dataset (s0, a0, sn, ts) the trainers consume.  In the
 * order of the reference: s0 = the observation the planner was given (:245-246); the expert's command plus uniform action
 * noise, clipped (:250-254), or a uniform random action (model_name "random", :255-256); get_action /
 * get_action_with_encode_obs_time (:20-30); the step's interval tsn by ts_grid (base_env.py:103-120); one Euler step of
 * size tsn (base_env.py:136-173, solver "euler"); reward = diff_reward(new state, applied action) (base_env.py:164), added
 * to the env's episode return (:269); the time channel ages by tsn (:206-208); Gaussian observation noise on the reduced
 * state, which persists (env.set_state_, :209-210); sn, a0 = the whole buffer, ts = tsn (:266-268).
 * Random draws are Philox4x32-10 keyed by `seed` with counter (global episode lo, hi, it, stream): they depend on the
 * episode and the step only, never on E or on how the episodes are batched (docs/collector.md). */
#define NLC_TS_GRID_FIXED 0   /* tsn = dt */
#define NLC_TS_GRID_UNIFORM 1 /* tsn = rand * 2 dt  ("uniform" / "random") */
#define NLC_TS_GRID_EXP 2     /* tsn ~ Exponential(rate 1/dt) */
#define NLC_POLICY_PLANNER 0  /* action_dev holds the planner's commands */
#define NLC_POLICY_RANDOM 1   /* uniform in [action_low, action_high]; action_dev is not read */
typedef struct nlc_collect_desc {
  int32_t env;       /* NLC_ENV_CARTPOLE / _PENDULUM / _ACROBOT */
  int32_t friction;
  double dt;
  int32_t delay;     /* the applied action is buffer row B - 1 - delay */
  int32_t B;         /* action buffer rows */
  int64_t E;         /* envs of this launch */
  int32_t nu;        /* action dims (must be the env's) */
  int32_t time_channel; /* 1: encode_obs_time -- the buffer has nu + 1 columns, the last is the observation time */
  int32_t ts_grid;   /* NLC_TS_GRID_* */
  int32_t policy;    /* NLC_POLICY_* */
  double action_noise; /* collect_expert_random_action_noise; < 0 = None: no noise and no clip */
  double obs_noise;    /* observation_noise (0 = off) */
  double action_low, action_high; /* env.action_space.low[0] / high[0] */
  int32_t steps_per_episode; /* iter_ (:373): rows per episode */
  uint64_t seed;
} nlc_collect_desc;
/* it: control step in [0, steps_per_episode); episode_base: global index of env 0's episode.  Env e writes dataset row
 * (episode_base + e) * steps_per_episode + it (episode-major, :426-439); the four dataset pointers are the bases of
 * arrays that hold at least (episode_base + E) * steps_per_episode rows.
 *   state_dev (E, n), abuf_dev (E, B, nu + time_channel), ret_dev (E): updated in place (ret_dev += reward)
 *   action_dev (E, nu) or NULL with NLC_POLICY_RANDOM
 *   s0_dev, sn_dev (rows, d); a0_dev (rows, B, nu + time_channel); ts_dev (rows)
 * NLC_ERR_BAD_SHAPE: E < 1 (E == 0 is refused too), B < 1, delay outside [0, B-1], nu > NLC_MAX_NU or not the env's, it or
 * episode_base out of range; NLC_ERR_BAD_ARG: unknown ts_grid / policy, NULL pointer, NULL action_dev with
 * NLC_POLICY_PLANNER.  Nothing is launched after a refusal. */
int nlc_collect_step(nlc_ctx* ctx, const nlc_collect_desc* desc, int it, int64_t episode_base, double* state_dev,
                     double* abuf_dev, const double* action_dev_or_null, double* ret_dev, double* s0_dev, double* a0_dev,
                     double* sn_dev, double* ts_dev);

/* ---- synthetic transition dataset (overlay.py:664-737, generate_irregular_data_delay_time_multi with rand=True; states and
 * actions from compute_state_actions, :603-631; one Euler step per row, batch_integrate_system, base_env.py:231-280).
 * A dataset is TI time blocks x A actions x S states, row r = (ti * A + i) * S + j.  Per row: the reduced state j of block
 * ti, (2u - 1) * state_max per component; action i of block ti, (2u - 1) * action_high per action dim; the block's
 * interval tsn by ts_grid (drawn once per block); s0 = observation of the state, sn = observation after one Euler step of
 * size tsn, ts = tsn; a0 = a (B, nu + time_channel) buffer of uniform fills (2u - 1) * action_high whose row B - 1 - delay
 * is the row's action, the time column, where there is one, B - 1 .. 0 (:718-731).
 * Random draws are Philox4x32-10 keyed by `seed`; the counters depend on (ti, j) (state), (ti, i) (action), ti (interval)
 * and (global row r, buffer row) (fill) only, never on the launch shape or on which blocks a call covers
 * (docs/synthetic.md).  With `reuse` the states and actions of every block are block 0's (:695-702). */
typedef struct nlc_synth_desc {
  int32_t env;       /* NLC_ENV_CARTPOLE / _PENDULUM / _ACROBOT */
  int32_t friction;
  double dt;
  int32_t delay;     /* the row's action is buffer row B - 1 - delay */
  int32_t B;         /* action buffer rows */
  int32_t nu;        /* action dims (must be the env's) */
  int32_t time_channel; /* 1: encode_obs_time -- the buffer has nu + 1 columns, the last is B - 1 .. 0 */
  int32_t ts_grid;   /* NLC_TS_GRID_* */
  int32_t reuse;     /* reuse_state_actions_when_sampling_times */
  int64_t S;         /* states per time block */
  int64_t A;         /* actions per time block */
  double action_high;
  double state_max[4]; /* the box of the reduced state; the first n (4, pendulum 2) are read */
  uint64_t seed;
} nlc_synth_desc;
/* Writes time blocks [ti_begin, ti_end) to rows [(ti - ti_begin) * A * S, (ti - ti_begin + 1) * A * S) of
 *   s0_dev, sn_dev ((ti_end - ti_begin) A S, d); a0_dev (.., B, nu + time_channel); ts_dev (..)
 * so that calls over consecutive block ranges concatenate to the call over their union, bit for bit.
 * NLC_ERR_UNSUPPORTED: an env other than the three above; ti_end * A * S >= 2^40 (global rows are counter words and int64
 * element indices), or a call of more than (2^31 - 1) * 256 rows.  NLC_ERR_BAD_SHAPE: B < 1, delay outside
 * [0, B-1], nu not the env's, S < 1, A < 1, ti_begin < 0, ti_end <= ti_begin or ti_end >= 2^31.  NLC_ERR_BAD_ARG: NULL
 * pointer, unknown ts_grid, dt, action_high or a state_max that is not > 0.  Every field is checked on the host and nothing
 * is launched after a refusal. */
int nlc_synth_generate(nlc_ctx* ctx, const nlc_synth_desc* desc, int64_t ti_begin, int64_t ti_end, double* s0_dev,
                       double* a0_dev, double* sn_dev, double* ts_dev);

/* ---- in-library kernel timing (hipEvent pairs on the launch stream) ------------------------- */
int nlc_profile_enable(nlc_ctx* ctx, int on);
int nlc_profile_reset(nlc_ctx* ctx);
int nlc_profile_count(nlc_ctx* ctx);
int nlc_profile_read(nlc_ctx* ctx, int idx, char* name, int name_len, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* NLC_H_ */
