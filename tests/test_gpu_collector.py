"""GPU: the expert-data collector's control step (collect_step_kernel behind nlc_collect_step, ExpertCollector,
collect_expert_dataset) against BatchedEnv (bit for bit in quiet mode), the CPU restatement of the env step (oracle/envs.py,
pinned to the real env classes by G10), the reference's time-channel lines, and the distributions of its draws."""

import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENVS = ["oderl-cartpole", "oderl-pendulum", "oderl-acrobot"]
BUFFERS = [(4, 0), (4, 3), (1, 0)]  # (B, delay)
SIZES = [1, 257]  # one lane; one lane past a workgroup
STEPS = 4
G10_TOL = dict(rtol=1e-11, atol=1e-12)  # test_env_step_vs_reference_env_golden's tolerance for the device env step


def _actions(E, nu, high, seed, steps=STEPS):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(steps, E, nu, dtype=torch.float64, generator=g) * 2 - 1) * high).cuda()


def _rows(t, E, steps):
    return t.view(E, steps, *t.shape[1:])


@pytest.mark.parametrize("friction", [False, True])
@pytest.mark.parametrize("env", ENVS)
def test_quiet_mode_is_batched_env_step(nlc, env, friction):
    """ts_grid="fixed", no action noise (None: no clip either), no observation noise, given actions: state, observation,
    reward (as the running return), action buffer and the recorded rows are torch.equal to a BatchedEnv stepped with the
    same actions -- collect_step_kernel and env_step_kernel share their dynamics bit for bit."""
    for B, delay in BUFFERS:
        for E in SIZES:
            col = nlc.ExpertCollector(env, delay, E, ts_grid="fixed", random_action_noise=None, observation_noise=0.0,
                                      friction=friction, action_buffer_size=B, steps_per_episode=STEPS, seed=3)
            ref = nlc.BatchedEnv(env, E, dt=0.05, action_delay=delay, action_buffer_size=B, friction=friction, seed=3)
            assert torch.equal(col.state, ref.state)
            acts = _actions(E, col.nu, col.action_high, 10 * B + delay)
            total = torch.zeros(E, dtype=torch.float64, device="cuda")
            obs_before = ref.get_obs().clone()
            for it in range(STEPS):
                col.collect_step(acts[it])
                obs, rew = ref.step(acts[it])
                total = total + rew
                where = (env, friction, B, delay, E, it)
                assert torch.equal(col.state, ref.state), where
                assert torch.equal(col.env.get_obs(), obs), where
                assert torch.equal(col.action_buffer, ref.action_buffer), where
                assert torch.equal(col._ret, total), where
                s0, a0, sn, ts = (_rows(t, E, STEPS)[:, it] for t in (col.storage.s0, col.storage.a0, col.storage.sn, col.storage.ts))
                assert torch.equal(s0, obs_before) and torch.equal(sn, obs) and torch.equal(a0, ref.action_buffer), where
                assert torch.equal(ts, torch.full_like(ts, 0.05)), where
                obs_before = obs.clone()
            assert torch.equal(col.returns, total)
            assert col.dataset()[3].shape == (E * STEPS, 1)


@pytest.mark.parametrize("env", ENVS)
def test_recorded_rows_are_consistent_with_the_oracle(nlc, env):
    """exp grid, action noise 1.0: oracle.envs.env_step(state before, the applied action a0[row, B-1-delay, :nu], ts[row])
    reproduces the state after, sn[row] and the step's reward (difference of the running return) at G10's tolerance; s0[row]
    is the observation before the step; within an episode sn[row] == s0[row + 1] bit for bit; the applied action lies in
    the action space and every interval is positive."""
    from oracle import envs as oenvs

    for B, delay in BUFFERS:
        for E in SIZES:
            col = nlc.ExpertCollector(env, delay, E, ts_grid="exp", random_action_noise=1.0, action_buffer_size=B,
                                      steps_per_episode=STEPS, seed=5)
            acts = _actions(E, col.nu, col.action_high, 7)
            for it in range(STEPS):
                before, obs_before, ret_before = col.state.cpu(), col.env.get_obs().cpu(), col._ret.cpu()
                col.collect_step(acts[it])
                s0, a0, sn, ts = (_rows(t, E, STEPS)[:, it].cpu()
                                  for t in (col.storage.s0, col.storage.a0, col.storage.sn, col.storage.ts))
                at = a0[:, B - 1 - delay, : col.nu]
                assert float(at.abs().max()) <= col.action_high and float(ts.min()) > 0.0
                s1, o1, r1 = oenvs.env_step(env, before, at, ts.view(E, 1))
                where = dict(err_msg=str((env, B, delay, E, it)))
                np.testing.assert_allclose(col.state.cpu().numpy(), s1.numpy(), **G10_TOL, **where)
                np.testing.assert_allclose(sn.numpy(), o1.numpy(), **G10_TOL, **where)
                np.testing.assert_allclose((col._ret.cpu() - ret_before).numpy(), r1.numpy(), **G10_TOL, **where)
                assert torch.equal(s0, obs_before)
            s0, _, sn, _ = col.dataset()
            assert torch.equal(_rows(sn, E, STEPS)[:, :-1], _rows(s0, E, STEPS)[:, 1:])


def _time_channel_reference(tsr, B, dt):
    """The reference's lines in float64 on the CPU from the recorded intervals tsr (episodes, steps), in its addition order:
    from flip(arange(B)) * dt; per step roll, last = 0 (get_action_with_encode_obs_time), += tsn, last = 0 (step_env).
    Returns the column after every step, (episodes, steps, B)."""
    t = (torch.flip(torch.arange(B), (0,)).double() * dt).repeat(tsr.shape[0], 1)
    out = []
    for it in range(tsr.shape[1]):
        t = torch.roll(t, -1, dims=1)
        t[:, -1] = 0
        t += tsr[:, it : it + 1]
        t[:, -1] = 0
        out.append(t.clone())
    return torch.stack(out, dim=1)


@pytest.mark.parametrize("env", ENVS)
def test_time_channel_follows_the_reference_recurrence(nlc, env):
    """encode_obs_time: a0[..., nu] after every step equals the reference's lines evaluated in float64 on the CPU from the
    recorded ts, in the same addition order (roll, last = 0; += tsn, last = 0; from flip(arange(B)) * dt): torch.equal.
    The action columns, s0, sn and ts do not depend on the flag."""
    dt = 0.05
    for B, delay in BUFFERS:
        for E in SIZES:
            kw = dict(ts_grid="exp", random_action_noise=1.0, action_buffer_size=B, steps_per_episode=STEPS, seed=9, dt=dt)
            col = nlc.ExpertCollector(env, delay, E, encode_obs_time=True, **kw)
            plain = nlc.ExpertCollector(env, delay, E, encode_obs_time=False, **kw)
            nu = col.nu
            acts = _actions(E, nu, col.action_high, 11)
            assert torch.equal(col.action_buffer[0, :, nu].cpu(), torch.flip(torch.arange(B), (0,)).double() * dt)
            for it in range(STEPS):
                col.collect_step(acts[it])
                plain.collect_step(acts[it])
            (s0, a0, sn, ts), (p0, pa, pn, pt) = col.dataset(), plain.dataset()
            assert a0.shape == (E * STEPS, B, nu + 1) and pa.shape == (E * STEPS, B, nu)
            assert torch.equal(a0[..., :nu], pa) and torch.equal(s0, p0) and torch.equal(sn, pn) and torch.equal(ts, pt)
            tcol = _rows(a0[..., nu].cpu(), E, STEPS)
            want = _time_channel_reference(_rows(ts.cpu(), E, STEPS)[..., 0], B, dt)
            for it in range(STEPS):
                assert torch.equal(tcol[:, it], want[:, it]), (env, B, delay, E, it)
            assert torch.equal(col.action_buffer[..., nu].cpu(), want[:, -1])


# ---------------------------------------------------------------------------------------------------- draw distributions
N_BIG = 65536


@pytest.fixture(scope="module")
def big(nlc):
    """One acrobot collector (nu = 2, four state components: both uniforms of a block, both blocks of the observation
    noise) of 65 536 envs; the tests launch single steps through its descriptor with the settings they need."""
    return nlc.ExpertCollector("oderl-acrobot", 0, N_BIG, steps_per_episode=1, seed=17)


def _one_step(col, actions, **desc):
    col.storage.reserve(col.E)
    col._launch(col._desc(**desc), actions, it=0)
    return col.storage


def test_interval_distributions(big):
    """Bounds are 5 standard errors of the statistic under the nominal distribution (N = 65 536).  exp: X ~ Exp(mean dt),
    sd(X) = dt, E X^2 = 2 dt^2, sd(X^2) = sqrt(24 - 4) dt^2.  uniform: X ~ U(0, 2 dt), sd = 2 dt / sqrt(12)."""
    dt, N = big.dt, N_BIG
    zero = torch.zeros(N, 2, dtype=torch.float64, device="cuda")
    ts = _one_step(big, zero, ts_grid=2).ts[:N].clone()
    assert float(ts.min()) > 0.0
    assert abs(float(ts.mean()) - dt) <= 5 * dt / math.sqrt(N)
    assert abs(float((ts * ts).mean()) - 2 * dt * dt) <= 5 * math.sqrt(20.0) * dt * dt / math.sqrt(N)
    tu = _one_step(big, zero, ts_grid=1).ts[:N].clone()
    assert float(tu.min()) > 0.0 and float(tu.max()) < 2 * dt
    assert abs(float(tu.mean()) - dt) <= 5 * (2 * dt / math.sqrt(12.0)) / math.sqrt(N)
    assert not torch.equal(ts, tu)


def test_action_noise_distribution_and_clip(big):
    """Planner action 0: the applied action is the noise, uniform in +-A with A = high * scale: mean 0 (sd A / sqrt(3)),
    second moment A^2 / 3 (sd of x^2: A^2 sqrt(1/5 - 1/9)), the two action dims uncorrelated (sd of the product of two
    independent such draws: A^2 / 3).  Planner action = high: nothing exceeds high, and what the noise pushed up sits on it."""
    N, high = N_BIG, big.action_high
    zero = torch.zeros(N, 2, dtype=torch.float64, device="cuda")
    for scale in (1.0, 0.25):
        A = high * scale
        x = _one_step(big, zero, action_noise=scale, ts_grid=0).a0[:N, -1, :].clone()
        assert float(x.abs().max()) <= A
        for j in range(2):
            assert abs(float(x[:, j].mean())) <= 5 * A / math.sqrt(3.0) / math.sqrt(N)
            assert abs(float((x[:, j] ** 2).mean()) - A * A / 3) <= 5 * A * A * math.sqrt(1 / 5 - 1 / 9) / math.sqrt(N)
        assert abs(float((x[:, 0] * x[:, 1]).mean())) <= 5 * (A * A / 3) / math.sqrt(N)
    top = _one_step(big, torch.full_like(zero, high), action_noise=1.0, ts_grid=0).a0[:N, -1, :]
    assert float(top.max()) == high and float(top.min()) >= 0.0
    frac = float((top == high).double().mean())
    assert abs(frac - 0.5) <= 5 * 0.5 / math.sqrt(2 * N)
    # None: neither noise nor clip
    raw = _one_step(big, torch.full_like(zero, 2 * high), action_noise=-1.0, ts_grid=0).a0[:N, -1, :]
    assert torch.equal(raw, torch.full_like(raw, 2 * high))


def test_observation_noise_distribution(big):
    """observation_noise = 0.1 on the reduced state: z = (state - noiseless state) / 0.1 has mean 0 (sd 1 / sqrt(N)) and
    variance 1 (sd of z^2: sqrt(2)) per component; the correlation between components, and between envs e and e + 1, is
    within 5 / sqrt(N) (the product of two independent standard normals has sd 1).  sn is the observation of the noisy
    state; the reward (the return) does not see the noise."""
    N = N_BIG
    zero = torch.zeros(N, 2, dtype=torch.float64, device="cuda")
    start, ab0 = big.state.clone(), big.action_buffer.clone()

    def run(obs_noise):
        big.env.state.copy_(start)
        big.action_buffer.copy_(ab0)
        big._ret.zero_()
        st = _one_step(big, zero, obs_noise=obs_noise, ts_grid=0, action_noise=-1.0)
        return big.state.clone(), st.sn[:N].clone(), big._ret.clone()

    clean, sn_clean, ret_clean = run(0.0)
    noisy, sn_noisy, ret_noisy = run(0.1)
    big.env.state.copy_(start)
    big.action_buffer.copy_(ab0)
    assert torch.equal(ret_clean, ret_noisy) and not torch.equal(sn_clean, sn_noisy)
    z = (noisy - clean) / 0.1
    se = 1 / math.sqrt(N)
    for i in range(4):
        assert abs(float(z[:, i].mean())) <= 5 * se, i
        assert abs(float((z[:, i] ** 2).mean()) - 1.0) <= 5 * math.sqrt(2.0) * se, i
        assert abs(float((z[:-1, i] * z[1:, i]).mean())) <= 5 * se, i
        for j in range(i + 1, 4):
            assert abs(float((z[:, i] * z[:, j]).mean())) <= 5 * se, (i, j)
    big.env.state.copy_(noisy)
    assert torch.equal(big.env.get_obs(), sn_noisy)
    big.env.state.copy_(start)


def test_random_policy_distribution(big):
    """policy = random: no actions are read; the applied action is uniform in [low, high] (mean 0, sd high / sqrt(3))."""
    N, high = N_BIG, big.action_high
    x = _one_step(big, None, policy=1, ts_grid=0).a0[:N, -1, :].clone()
    assert float(x.max()) <= high and float(x.min()) >= -high
    for j in range(2):
        assert abs(float(x[:, j].mean())) <= 5 * high / math.sqrt(3.0) / math.sqrt(N)
        assert abs(float((x[:, j] ** 2).mean()) - high * high / 3) <= 5 * high * high * math.sqrt(1 / 5 - 1 / 9) / math.sqrt(N)
    noise = _one_step(big, torch.zeros(N, 2, dtype=torch.float64, device="cuda"), action_noise=1.0, ts_grid=0).a0[:N, -1, :]
    assert not torch.equal(x, noise)  # a stream of its own


# ---------------------------------------------------------------------------------------------------- determinism
def _collect(nlc, env, E, base, seed, acts, storage=None):
    col = nlc.ExpertCollector(env, 1, E, ts_grid="exp", random_action_noise=1.0, observation_noise=0.05, encode_obs_time=True,
                              steps_per_episode=STEPS, seed=seed, episode_base=base, storage=storage)
    for it in range(STEPS):
        col.collect_step(acts[it, base : base + E])
    return col


@pytest.mark.parametrize("env", ENVS)
def test_determinism_and_batching_invariance(nlc, env):
    """Given actions: the same seed twice gives bit-identical datasets, another seed differs, and 8 episodes in one batch
    equal two batches of 4 with episode_base 0 and 4, row for row (draws depend on (seed, global episode, step) only; env e
    of a collector at episode_base b resets from the stream of global episode b + e)."""
    from neurallaplacecontrol_amd.envs import ENV_DIMS

    _, nu, high = ENV_DIMS[env]
    acts = _actions(8, nu, high, 21)
    a, b, c = (_collect(nlc, env, 8, 0, s, acts) for s in (0, 0, 1))
    for x, y in zip(a.dataset(), b.dataset()):
        assert torch.equal(x, y)
    assert torch.equal(a.returns, b.returns)
    assert all(not torch.equal(x, y) for x, y in zip(a.dataset(), c.dataset()))
    lo = _collect(nlc, env, 4, 0, 0, acts)
    hi = _collect(nlc, env, 4, 4, 0, acts, storage=lo.storage)
    assert lo.storage.episodes == 8 and hi.dataset()[0].shape[0] == 8 * STEPS
    for x, y in zip(a.dataset(), lo.dataset()):
        assert torch.equal(x, y)
    assert torch.equal(a.returns, lo.returns)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_dataset_untouched(nlc):
    from neurallaplacecontrol_amd._lib import NlcError

    col = nlc.ExpertCollector("oderl-cartpole", 1, 3, steps_per_episode=STEPS, seed=2)
    acts = _actions(3, 1, 3.0, 1)
    col.collect_step(acts[0])
    snap = [t.clone() for t in (col.storage.s0, col.storage.a0, col.storage.sn, col.storage.ts, col.state, col.action_buffer, col._ret)]
    for over, msg in ((dict(delay=4), "delay must be in"), (dict(delay=-1), "delay must be in"), (dict(nu=3), "nu must be in"),
                      (dict(ts_grid=7), "unknown ts_grid"), (dict(policy=5), "unknown policy"), (dict(E=0), "E must be >= 1"),
                      (dict(B=0), "delay must be in")):
        with pytest.raises(NlcError, match=msg):
            col._launch(col._desc(**over), acts[1])
    with pytest.raises(NlcError, match="planner policy needs actions"):
        col.collect_step(None)
    col.ts_grid = "lattice"
    with pytest.raises(NlcError, match="unknown ts_grid"):
        col.collect_step(acts[1])
    col.ts_grid = "exp"
    with pytest.raises(ValueError):
        nlc.ExpertCollector("oderl-cartpole", 4, 3, action_buffer_size=4)
    torch.cuda.synchronize()
    now = (col.storage.s0, col.storage.a0, col.storage.sn, col.storage.ts, col.state, col.action_buffer, col._ret)
    assert all(torch.equal(x, y) for x, y in zip(snap, now)) and col._it == 1
    col.collect_step(acts[1])  # and the collector goes on
    assert col._it == 2


# ---------------------------------------------------------------------------------------------------- end to end
def test_collect_expert_dataset_end_to_end(nlc, tmp_path):
    """8 episodes of 5 steps in batches of 3: two full batches and a short one of 2 (a planner of its own size)."""
    from oracle import envs as oenvs

    env, delay, seed = "oderl-cartpole", 2, 4
    torch.manual_seed(0)
    data = nlc.collect_expert_dataset(env, delay, collect_samples=40, steps_per_episode=5, roll_outs=64, time_steps=5,
                                      num_envs=3, save_path=str(tmp_path), seed=seed)
    s0, a0, sn, ts = data
    assert s0.shape == (40, 5) and a0.shape == (40, 4, 1) and sn.shape == (40, 5) and ts.shape == (40, 1)
    assert all(t.dtype == torch.float64 and t.is_cuda for t in data)
    assert data.returns.shape == (8,) and bool(torch.isfinite(data.returns).all()) and bool(torch.isfinite(sn).all())
    assert float(ts.min()) > 0 and float(a0.abs().max()) <= 3.0
    # episode-major: within every episode sn[row] is s0[row + 1]; every episode starts from ITS reset observation: global
    # episode g starts from the first draw of RandomState(seed + g), whichever batch and lane ran it
    assert torch.equal(sn.view(8, 5, 5)[:, :-1], s0.view(8, 5, 5)[:, 1:])
    first = s0.view(8, 5, 5)[:, 0].cpu()
    for g in range(8):
        st = oenvs.env_reset(env, np.random.RandomState(seed + g))
        np.testing.assert_allclose(first[g].numpy(), oenvs.env_obs(env, st).numpy(), **G10_TOL)
    # the file: the reference's name, CPU tensors, equal
    name = nlc.replay_buffer_file_name(env, delay, "oracle", False, 4, "exp", 1.0, 0.0, False)
    assert os.listdir(tmp_path) == [name]
    loaded = torch.load(os.path.join(tmp_path, name))
    assert isinstance(loaded, tuple) and len(loaded) == 4
    assert all(not t.is_cuda and torch.equal(t, d.cpu()) for t, d in zip(loaded, data))
    # the trainers take the tensors as they are
    torch.manual_seed(1)
    model = nlc.DeltaTRNN(5, 1, hidden_units=64, state_mean=np.zeros(5), state_std=np.ones(5), action_mean=np.zeros(1),
                          action_std=np.ones(1), normalize=True, normalize_time=True).double().cuda()
    losses = nlc.RNNTrainer(model).run(*data, torch.randperm(40)[:32].cuda(), 16)
    assert losses.shape == (2,) and bool(torch.isfinite(losses).all())


def test_run_episodes_random_policy_and_single_episode(nlc):
    """run_episodes without a planner (policy="random") over two batches, and a one-episode collector driven by a single
    MPPIDelay (what collect_expert_dataset builds when one episode remains)."""
    col = nlc.ExpertCollector("oderl-pendulum", 0, 5, policy="random", steps_per_episode=3, seed=1).run_episodes(2)
    s0, a0, sn, ts = col.dataset()
    assert s0.shape == (30, 3) and a0.shape == (30, 4, 1) and col.returns.shape == (10,) and col.episode_base == 10
    assert float(a0.abs().max()) <= 2.0 and torch.equal(sn.view(10, 3, 3)[:, :-1], s0.view(10, 3, 3)[:, 1:])
    data = nlc.collect_expert_dataset("oderl-pendulum", 1, collect_samples=4, steps_per_episode=4, roll_outs=32, time_steps=4,
                                      num_envs=8)
    assert data[0].shape == (4, 3) and data.returns.shape == (1,) and bool(torch.isfinite(data.returns).all())


def test_run_episodes_does_not_depend_on_the_batching_without_a_planner(nlc):
    """policy="random" with observation noise and the time channel: every draw and every reset is keyed by the global episode
    index, so two batches of 4 episodes (run_episodes(2) at E = 4) equal one batch of 8, bit for bit.  (With a planner the
    planner's own sampling noise is per batch, and only the collector's draws are invariant.)"""
    kw = dict(policy="random", observation_noise=0.05, encode_obs_time=True, steps_per_episode=STEPS, seed=6)
    for env in ENVS:
        one = nlc.ExpertCollector(env, 1, 8, **kw).run_episodes(1)
        two = nlc.ExpertCollector(env, 1, 4, **kw).run_episodes(2)
        assert one.dataset()[0].shape[0] == 8 * STEPS
        for x, y in zip(one.dataset(), two.dataset()):
            assert torch.equal(x, y), env
        assert torch.equal(one.returns, two.returns), env


def test_collect_expert_dataset_with_the_time_channel(nlc, tmp_path):
    """encode_obs_time=True end to end, 5 episodes of 4 steps in batches of 2 and a single last episode: with oracle
    dynamics the planner is handed the (B, nu + 1) buffer and drops the time column itself; with a learned encode_obs_time
    NL model it is handed the action columns and NLDynamics appends the constant channel B-1 .. 0.  In both the recorded
    time column follows the reference recurrence on the recorded ts, the action columns stay in the action space, and the
    file carries the reference's name for the model's kind."""
    from gpu_common import GOLD, load_sd

    from neurallaplacecontrol_amd.collector import _model_name

    env, delay, B, dt = "oderl-cartpole", 1, 4, 0.05
    sd = load_sd(np.load(f"{GOLD}/g5_nl_obs_time_cartpole.npz"))
    model = nlc.NeuralLaplaceModel(5, 1, 5, hidden_units=128, s_recon_terms=17, ilt_algorithm="fourier", encode_obs_time=True,
                                   state_mean=np.zeros(5), state_std=np.ones(5), action_mean=np.array([0]),
                                   action_std=np.array([1.0]), normalize=True, normalize_time=True).double()
    model.load_state_dict(sd)
    model = model.cuda()
    for dynamics, name in (("oracle", "oracle"), (model, "nl")):
        out = tmp_path / name
        data = nlc.collect_expert_dataset(env, delay, collect_samples=20, steps_per_episode=4, roll_outs=64, time_steps=5,
                                          num_envs=2, dynamics=dynamics, encode_obs_time=True, save_path=str(out), seed=3)
        s0, a0, sn, ts = data
        assert a0.shape == (20, B, 2) and ts.shape == (20, 1) and bool(torch.isfinite(data.returns).all())
        assert float(a0[..., 0].abs().max()) <= 3.0 and float(a0[..., 0].abs().max()) > 0.0
        want = _time_channel_reference(ts.cpu().view(5, 4), B, dt)
        assert torch.equal(a0[..., 1].cpu().view(5, 4, B), want), name
        assert torch.equal(sn.view(5, 4, 5)[:, :-1], s0.view(5, 4, 5)[:, 1:])
        assert os.listdir(out) == [nlc.replay_buffer_file_name(env, delay, name, True, B, "exp", 1.0, 0.0, False)]
    # the other kinds of model the reference names; an explicit model_name wins
    rnn = nlc.DeltaTRNN(5, 1, hidden_units=64, state_mean=np.zeros(5), state_std=np.ones(5), action_mean=np.zeros(1),
                        action_std=np.ones(1), normalize=True, normalize_time=True).double().cuda()
    assert _model_name("planner", rnn) == "delta_t_rnn" and _model_name("planner", nlc.NLDynamics(rnn, dt)) == "delta_t_rnn"
    assert _model_name("random", rnn) == "random" and _model_name("planner", model) == "nl"
    with pytest.raises(ValueError, match="model_name"):
        nlc.collect_expert_dataset(env, delay, collect_samples=4, steps_per_episode=4, dynamics=torch.nn.Identity(),
                                   save_path=str(tmp_path / "none"))
    assert not (tmp_path / "none").exists()
