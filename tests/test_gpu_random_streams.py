"""GPU: every device random draw, value for value, against the independent Philox reference (tests/philox_ref.py), whose
counters are built from the documents: the planner's sampling (perturb_kernel, and the fused body's inline sampling), the
expert collector's control step (collect_step_kernel) and the synthetic dataset (synth_kernel).

Uniform-derived values -- box samples, fills, applied actions, the fixed / uniform intervals, the time column -- are compared
for exact equality (the units are built with -ffp-contract=off; each value is a short chain of single-rounding operations).
`exp` intervals are held to 4 ulp of the extended-precision value, standard normals to 4e-15 max(rad, 1) and a coloured
planner draw to sum_j |L_ij| 4e-15 max(rad, 1) + 4 ulp(|eps_i|) (philox_ref.eps_bound; twice the bound derived from the
device's operations), observations to the device env step's rtol 1e-11 / atol 1e-12.  Every test asserts how many elements
it compared."""

import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref as pr

pytestmark = pytest.mark.gpu

SEEDS = [7, 2**32 + 5]
OBS_TOL = dict(rtol=1e-11, atol=1e-12)  # the device env step and observation (tests/test_gpu_synthetic.py)
LD = np.longdouble


def _ulp_err(got, want_ld):
    """|got - want| in ulps of want (want in extended precision)."""
    want = np.asarray(want_ld, dtype=LD)
    return np.asarray(np.abs(np.asarray(got, dtype=LD) - want) / pr.ulp(want.astype(np.float64)), dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- the planner
PLANNER_CASES = {  # nu: (env, nx, Sigma, mu)
    1: ("oderl-pendulum", 3, [[0.64]], None),
    2: ("oderl-acrobot", 6, [[1.0, 0.3], [0.3, 0.5]], [0.2, -0.1]),  # full covariance, non-zero off-diagonal and mean
}


def _cholesky(sigma):
    """The lower factor, from its definition (1 x 1 and 2 x 2)."""
    s = np.asarray(sigma, dtype=np.float64)
    L = np.zeros_like(s)
    L[0, 0] = np.sqrt(s[0, 0])
    if s.shape[0] == 2:
        L[1, 0] = s[1, 0] / L[0, 0]
        L[1, 1] = np.sqrt(s[1, 1] - L[1, 0] * L[1, 0])
    return L


def _check_eps(noise, kg, T, seed, counter, mu, L, where):
    """noise (K, T, nu) of global samples kg (K) against planner_eps; returns (elements compared, largest error / bound)."""
    got = noise.detach().cpu().numpy()
    nu = got.shape[-1]
    kk, tt = np.meshgrid(np.asarray(kg, dtype=np.int64), np.arange(T), indexing="ij")
    want, rad = pr.planner_eps(kk, tt, seed, counter, mu, L, with_rad=True)
    assert got.shape == want.shape == (len(kg), T, nu), (got.shape, want.shape, where)
    bound = pr.eps_bound(rad, L, want.astype(np.float64))
    ratio = np.asarray(np.abs(got.astype(LD) - want), dtype=np.float64) / bound
    assert np.all(ratio <= 1.0), (where, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))
    return got.size, float(ratio.max())


def _oracle_planner(nlc, nu, K, T, seed, **kw):
    env, nx, sigma, mu = PLANNER_CASES[nu]
    sig = torch.tensor(sigma, dtype=torch.float64)
    p = nlc.MPPIDelay(nlc.OracleDynamics(env, 0.05, 0), nlc.EnvCost(env), nx, sig, K, T, "cuda", lambda_=1.0, u_scale=1,
                      noise_mu=None if mu is None else torch.tensor(mu, dtype=torch.float64),
                      U_init=torch.zeros(T, nu, dtype=torch.float64), noise_rng="philox", seed=seed, **kw)
    return p, env, (np.zeros(nu) if mu is None else np.array(mu)), _cholesky(sigma)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("nu", [1, 2])
def test_planner_draws_equal_the_documented_stream(nlc, nu, seed):
    """MPPIDelay, noise_rng="philox", oracle dynamics, no bounds, u_scale = 1, K = 300 (no multiple of 256), T = 3: every
    element of `noise` of commands 0 and 1, and of a command after `_commands = 2^32 + 1` (the counter's high word, XORed
    into the key), equals planner_eps(kg, t, seed, command, mu, L).  The published noise is (U + eps) - U, so U is set to
    zero before every command: noise is then the raw draw, bit for bit.  Then the same planner as a shard past 2^32:
    K_local = 300 at k_offset = 2^32 - 150 of K_global = 2^32 + 150 -- the compared global indices straddle 2^32 (the high
    counter word of kg).
    Measured on an MI355X: largest error / bound 0.125 (nu = 1), 0.126 (nu = 2), over both seeds."""
    K, T = 300, 3
    p, env, mu, L = _oracle_planner(nlc, nu, K, T, seed)
    st, ab = nlc.initial_state(env), torch.zeros(4, nu, dtype=torch.float64)
    compared, worst = 0, 0.0
    for command in (0, 1, 2**32 + 1):
        p._commands = command
        p.U = torch.zeros(T, nu, dtype=torch.float64)
        p.command(st, ab)
        n, r = _check_eps(p.noise, np.arange(K), T, seed, command, mu, L, (nu, seed, command))
        compared, worst = compared + n, max(worst, r)
    assert compared == 3 * K * T * nu
    # a shard whose global sample indices cross 2^32
    q, _, _, _ = _oracle_planner(nlc, nu, K, T, seed)
    q.K, q.K_local, q.k_offset = 2**32 + 150, K, 2**32 - 150
    q.U = torch.zeros(T, nu, dtype=torch.float64)
    q._commands = 1
    q.command(st, ab)
    kg = q.k_offset + np.arange(K, dtype=np.int64)
    assert kg.min() < 2**32 <= kg.max() and int((kg < 2**32).sum()) == 150
    n, r = _check_eps(q.noise, kg, T, seed, 1, mu, L, (nu, seed, "shard past 2^32"))
    assert n == K * T * nu
    # and the low half of the shard is NOT what the indices without their high word give (a dropped word would pass above
    # only if it were dropped in the reference too)
    low = pr.planner_eps(kg[150:, None] - 2**32, np.arange(T)[None, :], seed, 1, mu, L).astype(np.float64)
    assert not np.any(low == q.noise.cpu().numpy()[150:])
    print(f"planner nu={nu} seed={seed}: {compared + n} elements, largest error / bound {max(worst, r):.3f}")


def test_batched_planner_episode_e_continues_at_e_times_K(nlc):
    """BatchedMPPIDelay, E = 3, K = 100, nu = 2: episode e's noise is planner_eps(e K + k, t, ...), commands 0
    and 1.  Measured on an MI355X: largest error / bound 0.123."""
    E, K, T, nu, seed = 3, 100, 3, 2, 7
    env, nx, sigma, mu = PLANNER_CASES[nu]
    L = _cholesky(sigma)
    p = nlc.BatchedMPPIDelay(nlc.OracleDynamics(env, 0.05, 0), nlc.EnvCost(env), nx, torch.tensor(sigma, dtype=torch.float64), E, K,
                             T, "cuda", lambda_=1.0, u_scale=1, noise_mu=torch.tensor(mu, dtype=torch.float64),
                             U_init=torch.zeros(E, T, nu, dtype=torch.float64), noise_rng="philox", seed=seed)
    st = nlc.initial_state(env).repeat(E, 1)
    ab = torch.zeros(E, 4, nu, dtype=torch.float64)
    compared, worst = 0, 0.0
    for command in (0, 1):
        p.U = torch.zeros(E, T, nu, dtype=torch.float64)
        p.command(st, ab)
        assert p.noise.shape == (E, K, T, nu)
        for e in range(E):
            n, r = _check_eps(p.noise[e], e * K + np.arange(K), T, seed, command, np.array(mu), L, ("batched", e, command))
            compared, worst = compared + n, max(worst, r)
    assert compared == 2 * E * K * T * nu
    print(f"batched planner: {compared} elements, largest error / bound {worst:.3f}")


def test_fused_body_inline_sampling_equals_the_documented_stream(nlc):
    """An NLDynamics planner on the one-launch fused body, which samples inside its launch (no perturb_kernel): the
    smallest configuration of test_fused_inline_sampling_and_weights_bit_identical (cartpole, K = 48, T = 9, hidden 128),
    without bounds and with u_scale = 1 and U = 0 so that the published `noise` is the raw draw.
    Measured on an MI355X: largest error / bound 0.126."""
    from gpu_common import build_model
    from oracle import nl_model as onl

    env, K, T, seed = "oderl-cartpole", 48, 9, 2**32 + 5
    st = onl.ENV_STATS[env]
    d, nu, A = st["d"], st["nu"], st["act_high"]
    model = build_model(nlc, onl.make_synthetic_state_dict(0, d, nu, 128, 17, st["state_std"], [A / 2], tame=True))
    sigma = [[0.64]]
    p = nlc.MPPIDelay(nlc.NLDynamics(model, 0.05), nlc.EnvCost(env), d, torch.tensor(sigma, dtype=torch.float64), K, T, "cpu",
                      lambda_=0.7, u_scale=1, noise_rng="philox", seed=seed, U_init=torch.zeros(T, nu, dtype=torch.float64),
                      planner_options={"rollout_variant": 3, "fused_inline": 1})
    state, ab = nlc.initial_state(env), torch.zeros(4, nu, dtype=torch.float64)
    compared, worst = 0, 0.0
    p.command(state, ab)  # (the first command also uploads and configures: keep its launches out of the profile below)
    for command in (0, 1):
        p._commands = command
        p.U = torch.zeros(T, nu, dtype=torch.float64)
        p.ctx.profile_reset()
        p.ctx.profile(True)
        p.command(state, ab)
        p.ctx.profile(False)
        assert set(p.ctx.profile_read()) == {"nl_plan_fused_kernel", "merge_kernel"}, "the draw under test is the fused body's own"
        n, r = _check_eps(p.noise, np.arange(K), T, seed, command, np.zeros(1), _cholesky(sigma), ("fused", command))
        compared, worst = compared + n, max(worst, r)
    assert compared == 2 * K * T * nu
    print(f"fused inline sampling: {compared} elements, largest error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------- the collector
COLLECT_E, COLLECT_BASE, COLLECT_STEPS, COLLECT_B, COLLECT_DELAY = 300, 5, 3, 4, 1


def _step_rows(col, it):
    E, st = col.E, col.storage
    rows = (COLLECT_BASE + np.arange(E)) * COLLECT_STEPS + it
    return [t[torch.as_tensor(rows)].cpu() for t in (st.s0, st.a0, st.sn, st.ts)]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("env", ["oderl-cartpole", "oderl-pendulum"])
def test_collector_draws_equal_the_documented_streams(nlc, env, seed):
    """ExpertCollector, E = 300 envs at episode_base = 5 (global episodes 5 .. 304), three steps, cartpole (n = 4: both
    observation-noise blocks) and pendulum (n = 2), B = 4, delay 1.
    A: given actions, action noise 1.0 with its clip, the `uniform` grid, observation_noise = 0.01 -- ts == 2 dt u (stream 0)
    and the step's action a0[row, B - 1] == clip(a + (2u - 1) high) (stream 1) exactly; sn == the oracle observation of
    (the quiet state, stepped on the CPU from the state before with the applied action a0[row, B - 1 - delay] and ts, +
    0.01 z), z components 0, 1 from stream 2 and 2, 3 from stream 3, and the stored state likewise.
    B: policy="random" on the `exp` grid -- the action == low + (high - low) u (stream 4) exactly, ts within 4 ulp of
    -dt ln u in extended precision.
    The high word of the episode index cannot be reached here: storage is indexed by the global row, so an episode past 2^32
    needs that many rows; the counter builder's high word is covered by tests/test_philox_host.py.
    Measured on an MI355X: largest exp-interval error 1.27 ulp (both envs, both seeds)."""
    from neurallaplacecontrol_amd.envs import ENV_DIMS
    from oracle import envs as oenvs

    E, B, delay, dt = COLLECT_E, COLLECT_B, COLLECT_DELAY, 0.05
    nx, nu, high = ENV_DIMS[env]
    n = oenvs.STATE_DIM[env]
    kw = dict(action_buffer_size=B, steps_per_episode=COLLECT_STEPS, seed=seed, episode_base=COLLECT_BASE, dt=dt)
    a = nlc.ExpertCollector(env, delay, E, ts_grid="uniform", random_action_noise=1.0, observation_noise=0.01, **kw)
    b = nlc.ExpertCollector(env, delay, E, ts_grid="exp", policy="random", **kw)
    g = torch.Generator().manual_seed(3)
    acts = (torch.rand(COLLECT_STEPS, E, nu, dtype=torch.float64, generator=g) * 2 - 1) * high
    episode = COLLECT_BASE + np.arange(E)
    compared = dict(ts=0, action=0, sn=0, policy=0, exp=0)
    worst_ulp = 0.0
    for it in range(COLLECT_STEPS):
        draws = pr.collector_draws(seed, episode, it)
        # ---- A
        before = a.state.cpu()
        a.collect_step(acts[it].cuda())
        s0, a0, sn, ts = _step_rows(a, it)
        assert np.array_equal(ts.numpy(), (2.0 * dt) * draws["interval"]), (env, seed, it)
        u = draws["action_noise"][:, :nu]
        want = np.clip(acts[it].numpy() + ((2.0 * u - 1.0) * high) * 1.0, -high, high)
        assert np.array_equal(a0[:, B - 1, :nu].numpy(), want), (env, seed, it)
        assert int((np.abs(want) == high).sum()) > 0 and int((np.abs(want) < high).sum()) > 0  # clipped and not
        quiet, _, _ = oenvs.env_step(env, before, a0[:, B - 1 - delay, :nu], ts.view(E, 1))
        noisy = torch.as_tensor((quiet.numpy().astype(LD) + LD(0.01) * draws["obs_noise"][:, :n]).astype(np.float64))
        where = dict(err_msg=str((env, seed, it)))
        np.testing.assert_allclose(sn.numpy(), oenvs.env_obs(env, noisy).numpy(), **OBS_TOL, **where)
        np.testing.assert_allclose(a.state.cpu().numpy(), noisy.numpy(), **OBS_TOL, **where)
        assert float((noisy - quiet).abs().min()) > 0.0 and float((noisy - quiet).abs().max()) > 1e-2  # the noise is there
        compared["ts"] += ts.numel()
        compared["action"] += want.size
        compared["sn"] += sn.numel()
        # ---- B
        b.collect_step(None)
        _, b0, _, bts = _step_rows(b, it)
        assert np.array_equal(b0[:, B - 1, :nu].numpy(), -high + (high - -high) * draws["policy"][:, :nu]), (env, seed, it)
        err = _ulp_err(bts.numpy(), pr.exp_interval(draws["interval"], dt))
        assert np.all(err <= 4.0), (env, seed, it, float(err.max()))
        worst_ulp = max(worst_ulp, float(err.max()))
        compared["policy"] += E * nu
        compared["exp"] += bts.numel()
    assert compared == dict(ts=3 * E, action=3 * E * nu, sn=3 * E * nx, policy=3 * E * nu, exp=3 * E)
    print(f"collector {env} seed={seed}: {compared}, largest exp-interval error {worst_ulp:.2f} ulp")


# ---------------------------------------------------------------------------------------------------- the synthetic dataset
SYNTH_SPD = {"oderl-cartpole": 2, "oderl-pendulum": 3, "oderl-acrobot": 2}  # 640 / 810 / 640 rows: the smallest with > 256


def _check_synth(env, data, seed, A, S, begin, B, delay, enc, reuse, grid, dt, where):
    """(s0, a0, sn, ts) of time blocks [begin, ..) against synth_draws; returns the element counts and the largest exp error."""
    from neurallaplacecontrol_amd.envs import ENV_DIMS
    from neurallaplacecontrol_amd.synthetic import STATE_MAX
    from oracle import envs as oenvs

    nx, nu, high = ENV_DIMS[env]
    smax = np.array(STATE_MAX[env])
    n = smax.size
    s0, a0, sn, ts = (t.cpu().numpy() for t in data)
    R = s0.shape[0]
    r = begin * A * S + np.arange(R, dtype=np.int64)  # the GLOBAL row
    q, j = np.divmod(r, S)
    ti, i = np.divmod(q, A)
    fills = [bb for bb in range(B) if bb != B - 1 - delay]
    rr, bb = np.meshgrid(r, np.arange(B), indexing="ij")
    d = pr.synth_draws(seed, ti[:, None], i[:, None], j[:, None], rr, bb, reuse)
    state = pr.box(d["state"][:, 0, :n], smax)
    np.testing.assert_allclose(s0, oenvs.env_obs(env, torch.as_tensor(state)).numpy(), **OBS_TOL, err_msg=str(where))
    assert np.array_equal(a0[:, B - 1 - delay, :nu], pr.box(d["action"][:, 0, :nu], high)), where
    assert np.array_equal(a0[:, fills, :nu], pr.box(d["fill"][:, fills, :nu], high)), where
    if enc:
        assert a0.shape[2] == nu + 1 and np.array_equal(a0[:, :, nu], np.broadcast_to(np.arange(B - 1, -1, -1.0), (R, B))), where
    else:
        assert a0.shape[2] == nu
    worst = 0.0
    u = d["interval"][:, 0]
    if grid == "fixed":
        assert np.array_equal(ts[:, 0], np.full(R, dt)), where
    elif grid == "uniform":
        assert np.array_equal(ts[:, 0], (2.0 * dt) * u), where
    else:
        err = _ulp_err(ts[:, 0], pr.exp_interval(u, dt))
        assert np.all(err <= 4.0), (where, float(err.max()))
        worst = float(err.max())
    assert len(set(ti.tolist())) >= 1 and sn.shape == s0.shape
    return dict(s0=s0.size, action=R * nu, fill=R * len(fills) * nu, time=R * B * int(enc), ts=R), worst, r


@pytest.mark.parametrize("env", ["oderl-cartpole", "oderl-pendulum", "oderl-acrobot"])
def test_synthetic_draws_equal_the_stream_table(nlc, env):
    """generate_synthetic_dataset at the smallest samples_per_dim with more than one 256-row workgroup (cartpole and acrobot 2:
    640 rows, pendulum 3: 810), reuse on and off x ts_grid fixed / uniform / exp x encode_obs_time on and off x delay 0 and
    B - 1, the whole dataset or the slice blocks=(3, 7): s0 against the oracle observation of the box sample of streams 0, 1
    at (j, ti), the action row of a0 (stream 2 at (i, ti)) and every fill entry (stream 4 at (global row, buffer row)) exactly,
    the time column, and ts (stream 3 at (0, ti)) -- exactly on the fixed and uniform grids, within 4 ulp on exp.
    Measured on an MI355X: largest exp-interval error 0.75 ulp (all three envs)."""
    from neurallaplacecontrol_amd.envs import ENV_DIMS

    spd, B, dt, seed = SYNTH_SPD[env], 4, 0.05, 2**32 + 5
    TI, A, S = nlc.synthetic_dataset_shape(env, spd)
    nx, nu, _ = ENV_DIMS[env]
    assert TI * A * S > 256
    total = dict(s0=0, action=0, fill=0, time=0, ts=0)
    want = dict(total)
    worst, case = 0.0, 0
    for reuse in (False, True):
        for grid in ("fixed", "uniform", "exp"):
            for enc in (False, True):
                for delay in (0, B - 1):
                    blocks = None if case % 2 == 0 else (3, 7)
                    case += 1
                    data = nlc.generate_synthetic_dataset(env, delay, spd, action_buffer_size=B, encode_obs_time=enc,
                                                          reuse_state_actions_when_sampling_times=reuse, dt=dt, ts_grid=grid,
                                                          seed=seed, blocks=blocks)
                    begin, R = (0, TI * A * S) if blocks is None else (3, 4 * A * S)
                    assert data[0].shape[0] == R
                    where = (env, reuse, grid, enc, delay, blocks)
                    cnt, w, _ = _check_synth(env, data, seed, A, S, begin, B, delay, enc, reuse, grid, dt, where)
                    worst = max(worst, w)
                    for k, v in dict(s0=R * nx, action=R * nu, fill=R * (B - 1) * nu, time=R * B * int(enc), ts=R).items():
                        want[k] += v
                        total[k] += cnt[k]
    assert case == 24 and total == want and all(v > 0 for v in total.values())
    print(f"synthetic {env}: {total}, largest exp-interval error {worst:.2f} ulp")


def test_synthetic_fill_counter_carries_the_high_word_of_the_global_row(nlc):
    """One descriptor-level nlc_synth_generate call, made as generate_synthetic_dataset makes it: pendulum, A = S = 256,
    blocks (65535, 65537) -- 131 072 rows whose global row index crosses 2^32 in the middle (the entry accepts the shape: TI A S
    stays below 2^40), B = 2, delay 0: the fill of buffer row 0 (stream 4 at (global row, 0)) exactly, with the action row,
    s0 and the uniform-grid ts; and the rows past 2^32 are not what the row index without its high word gives."""
    from neurallaplacecontrol_amd import _lib
    from neurallaplacecontrol_amd.laplace import default_ctx
    from neurallaplacecontrol_amd.synthetic import STATE_MAX

    env, A, S, B, delay, dt, seed = "oderl-pendulum", 256, 256, 2, 0, 0.05, 7
    begin, end = 65535, 65537
    R = (end - begin) * A * S
    assert R == 131072 <= 150000
    smax = STATE_MAX[env]
    desc = _lib.SynthDesc(env=_lib.ENV_IDS[env], friction=0, dt=dt, delay=delay, B=B, nu=1, time_channel=0,
                          ts_grid=_lib.TS_GRIDS["uniform"], reuse=0, S=S, A=A, action_high=2.0,
                          state_max=(C.c_double * 4)(*smax, 0.0, 0.0), seed=seed)
    mk = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")  # noqa: E731
    data = mk(R, 3), mk(R, B, 1), mk(R, 3), mk(R, 1)
    ctx = default_ctx(torch.cuda.current_device())
    ctx.launch(ctx.lib.nlc_synth_generate, C.byref(desc), begin, end, *(_lib.ptr(t) for t in data))
    torch.cuda.synchronize()
    cnt, _, r = _check_synth(env, data, seed, A, S, begin, B, delay, False, False, "uniform", dt, "rows across 2^32")
    assert int(r[0]) == 2**32 - 65536 and int(r[-1]) == 2**32 + 65535 and int((r >= 2**32).sum()) == 65536
    assert cnt == dict(s0=R * 3, action=R, fill=R, time=0, ts=R)
    wrapped = pr.box(pr.synth_draws(seed, 0, 0, 0, r[65536:] - 2**32, 0, False)["fill"][:, 0], 2.0)  # (buffer row 0 is the fill)
    assert wrapped.shape == (65536,) and not np.any(wrapped == data[1][65536:, 0, 0].cpu().numpy())
