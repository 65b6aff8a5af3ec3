"""GPU: the synthetic transition dataset (synth_kernel behind nlc_synth_generate, generate_synthetic_dataset) against the CPU
restatement of the env step (oracle/envs.py, pinned to the real env classes by G10), the reference's row layout
(overlay.py:664-737, base_env.py:263-276), the distributions of its draws, and the trainers that consume it."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENVS = ["oderl-cartpole", "oderl-pendulum", "oderl-acrobot"]
BUFFERS = [(4, 0), (4, 3), (1, 0)]  # (B, delay)
DIMS = {"oderl-cartpole": (5, 1, 3.0, 4), "oderl-pendulum": (3, 1, 2.0, 2), "oderl-acrobot": (6, 2, 5.0, 4)}  # d, nu, high, n
G10_TOL = dict(rtol=1e-11, atol=1e-12)  # test_env_step_vs_reference_env_golden's tolerance for the device env step
SPD = 3  # S = 81 (pendulum 9), A = 3, TI = 30


def _applied(a0, B, delay, nu):
    return a0[:, B - 1 - delay, :nu]


def _oracle_check(env, data, B, delay, friction, where):
    """Every row: oracle.envs.env_obs2state(s0) stepped by oracle.envs.env_step with the applied action and ts gives sn."""
    from oracle import envs as oenvs

    nu = DIMS[env][1]
    s0, a0, sn, ts = (t.cpu() for t in data)
    _, o1, _ = oenvs.env_step(env, oenvs.env_obs2state(env, s0), _applied(a0, B, delay, nu), ts, friction)
    err = (sn - o1).abs()
    print(f"{where}: rows {s0.shape[0]} max abs err {float(err.max()):.3e} "
          f"max err / (atol + rtol |ref|) {float((err / (1e-12 + 1e-11 * o1.abs())).max()):.3e}")
    np.testing.assert_allclose(sn.numpy(), o1.numpy(), **G10_TOL, err_msg=str(where))


# ---------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("friction", [False, True])
@pytest.mark.parametrize("env", ENVS)
def test_rows_are_consistent_with_the_oracle(nlc, env, friction):
    """exp grid, samples_per_dim = 3, every (B, delay): the observation s0 taken back to the reduced state
    (oracle.envs.env_obs2state: the atan2 round trip), one oracle Euler step of size ts[row] with the applied action
    a0[row, B-1-delay, :nu], observed again, reproduces sn at G10's tolerance."""
    for B, delay in BUFFERS:
        data = nlc.generate_synthetic_dataset(env, delay, SPD, action_buffer_size=B, ts_grid="exp", friction=friction, seed=5)
        _oracle_check(env, data, B, delay, friction, (env, friction, B, delay))


def test_rows_are_consistent_with_the_oracle_across_workgroup_boundaries(nlc):
    """Cartpole, samples_per_dim = 5: S = 625 is no multiple of the 256 rows of a workgroup, so workgroups straddle action
    and time-block boundaries (and the last one is short): 50 x 5 x 625 rows against the oracle, and the layout."""
    env, B, delay = "oderl-cartpole", 4, 1
    data = nlc.generate_synthetic_dataset(env, delay, 5, action_buffer_size=B, ts_grid="exp", seed=2)
    assert data[0].shape == (50 * 5 * 625, 5)
    _oracle_check(env, data, B, delay, False, (env, "S=625"))
    _check_structure(env, data, 50, 5, 625, B, delay, False)


# ---------------------------------------------------------------------------------------------------- structure
def _check_structure(env, data, TI, A, S, B, delay, enc):
    d, nu, high, _ = DIMS[env]
    s0, a0, sn, ts = data
    R, W = TI * A * S, nu + int(enc)
    assert s0.shape == (R, d) and a0.shape == (R, B, W) and sn.shape == (R, d) and ts.shape == (R, 1)
    assert all(t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() for t in data)
    assert bool(torch.isfinite(s0).all()) and bool(torch.isfinite(sn).all())
    s0b = s0.view(TI, A, S, d)
    assert torch.equal(s0b, s0b[:, :1].expand(TI, A, S, d)), "rows with the same j share s0 across actions"
    at = _applied(a0, B, delay, nu).reshape(TI, A, S, nu)
    assert torch.equal(at, at[:, :, :1].expand(TI, A, S, nu)), "rows with the same i share the applied action"
    tsb = ts.view(TI, A * S)
    assert torch.equal(tsb, tsb[:, :1].expand(TI, A * S)) and float(ts.min()) > 0.0, "ts is constant within a block"
    assert float(a0[..., :nu].abs().max()) <= high
    if enc:
        col = torch.arange(B - 1, -1, -1, dtype=torch.float64, device=a0.device)
        assert torch.equal(a0[..., nu], col.expand(R, B))
    return s0b, at, tsb


@pytest.mark.parametrize("enc", [False, True])
@pytest.mark.parametrize("env", ENVS)
def test_structure_of_a_dataset(nlc, env, enc):
    """The reference's shapes and row order for every (B, delay), on the fixed grid (ts == 0.05 exactly) and on exp; states,
    actions and intervals of different blocks differ (nothing is reused unasked)."""
    TI, A, S = nlc.synthetic_dataset_shape(env, SPD)
    assert (TI, A, S) == (30, 3, 3 ** DIMS[env][3])
    for B, delay in BUFFERS:
        for grid in ("fixed", "exp"):
            data = nlc.generate_synthetic_dataset(env, delay, SPD, action_buffer_size=B, encode_obs_time=enc, ts_grid=grid, seed=1)
            s0b, at, tsb = _check_structure(env, data, TI, A, S, B, delay, enc)
            if grid == "fixed":
                assert torch.equal(data[3], torch.full_like(data[3], 0.05))
            else:
                assert len(set(tsb[:, 0].tolist())) == TI
            assert not torch.equal(s0b[0], s0b[1]) and not torch.equal(at[0], at[1])
            assert not torch.equal(at[:, 0], at[:, 1]) and not torch.equal(s0b[:, :, 0], s0b[:, :, 1])


@pytest.mark.parametrize("env", ENVS)
def test_reuse_state_actions_when_sampling_times(nlc, env):
    """reuse_state_actions_when_sampling_times (overlay.py:695-702): s0 and the applied action of block ti equal block 0's,
    and block 0 is the plain dataset's block 0; the buffer fills and, on exp, the intervals still differ per block."""
    d, nu, _, _ = DIMS[env]
    B, delay = 4, 1
    TI, A, S = nlc.synthetic_dataset_shape(env, SPD)
    kw = dict(action_buffer_size=B, ts_grid="exp", seed=9)
    data = nlc.generate_synthetic_dataset(env, delay, SPD, reuse_state_actions_when_sampling_times=True, **kw)
    plain = nlc.generate_synthetic_dataset(env, delay, SPD, **kw)
    s0b, at, tsb = _check_structure(env, data, TI, A, S, B, delay, False)
    assert torch.equal(s0b, s0b[:1].expand_as(s0b)) and torch.equal(at, at[:1].expand_as(at))
    assert all(torch.equal(x[: A * S], y[: A * S]) for x, y in zip(data, plain))
    assert torch.equal(data[3], plain[3]) and len(set(tsb[:, 0].tolist())) == TI
    fills = data[1].view(TI, A * S, B, nu)[:, :, B - 1, :]  # (delay = 1: the last buffer row is a fill)
    assert not torch.equal(fills[0], fills[1]) and not torch.equal(data[1], plain[1])
    assert torch.equal(fills, plain[1].view(TI, A * S, B, nu)[:, :, B - 1, :]), "the fills do not depend on reuse"


# ---------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("env,spd", [("oderl-cartpole", SPD), ("oderl-pendulum", SPD), ("oderl-acrobot", SPD), ("oderl-cartpole", 5)])
def test_determinism_and_chunk_invariance(nlc, env, spd):
    """The same seed gives torch.equal datasets; blocks=(0, 7) and blocks=(7, TI) concatenate to the full call bit for bit
    (S = 625: the chunks' workgroups cover other rows than the full call's); another seed differs in every tensor."""
    TI = nlc.synthetic_dataset_shape(env, spd)[0]
    kw = dict(action_buffer_size=4, encode_obs_time=True, ts_grid="exp", seed=11)
    full = nlc.generate_synthetic_dataset(env, 2, spd, **kw)
    again = nlc.generate_synthetic_dataset(env, 2, spd, **kw)
    assert all(torch.equal(x, y) for x, y in zip(full, again))
    head = nlc.generate_synthetic_dataset(env, 2, spd, blocks=(0, 7), **kw)
    tail = nlc.generate_synthetic_dataset(env, 2, spd, blocks=(7, TI), **kw)
    assert head[0].shape[0] * TI == full[0].shape[0] * 7
    for x, h, t in zip(full, head, tail):
        assert torch.equal(x, torch.cat((h, t), dim=0))
    other = nlc.generate_synthetic_dataset(env, 2, spd, **dict(kw, seed=12))
    assert not any(torch.equal(x, y) for x, y in zip(full, other))


# ---------------------------------------------------------------------------------------------------- distributions
@pytest.fixture(scope="module")
def big(nlc):
    """Cartpole, samples_per_dim = 6 on the exp grid: 60 blocks x 6 actions x 1296 states = 466 560 rows."""
    return tuple(t.cpu() for t in nlc.generate_synthetic_dataset("oderl-cartpole", 1, 6, action_buffer_size=4, ts_grid="exp", seed=3))


def _uniform_moments(x, mx, what):
    """x ~ U(-mx, mx): mean 0 (sd mx / sqrt(3)), second moment mx^2 / 3 (sd of x^2: mx^2 sqrt(1/5 - 1/9)); 5 standard errors."""
    N = x.numel()
    assert float(x.abs().max()) <= mx, what
    assert abs(float(x.mean())) <= 5 * mx / math.sqrt(3.0) / math.sqrt(N), what
    assert abs(float((x * x).mean()) - mx * mx / 3) <= 5 * mx * mx * math.sqrt(1 / 5 - 1 / 9) / math.sqrt(N), what


def test_state_and_action_distributions(big):
    """Over the 60 x 1296 = 77 760 distinct (ti, j): every reduced-state component (the angle through atan2 of the
    observation) is uniform on its box [5, 20, pi32, 30]; components and neighbouring states are uncorrelated (the product of
    two independent such draws has sd max_a max_b / 3).  The 360 distinct actions are uniform on [-3, 3]."""
    from neurallaplacecontrol_amd.synthetic import STATE_MAX

    TI, A, S = 60, 6, 1296
    s0 = big[0].view(TI, A, S, 5)[:, 0].reshape(TI * S, 5)
    st = torch.stack([s0[:, 0], s0[:, 1], torch.atan2(s0[:, 3], s0[:, 2]), s0[:, 4]], dim=1)
    mx = STATE_MAX["oderl-cartpole"]
    N = st.shape[0]
    assert N >= 65536
    for c in range(4):
        _uniform_moments(st[:, c], mx[c], f"state {c}")
        assert abs(float((st[:-1, c] * st[1:, c]).mean())) <= 5 * (mx[c] * mx[c] / 3) / math.sqrt(N - 1), c
        for e in range(c + 1, 4):
            assert abs(float((st[:, c] * st[:, e]).mean())) <= 5 * (mx[c] * mx[e] / 3) / math.sqrt(N), (c, e)
    act = _applied(big[1], 4, 1, 1).view(TI, A, S)[:, :, 0].reshape(-1)
    assert act.numel() == 360
    _uniform_moments(act, 3.0, "action")


def test_buffer_fill_distribution(big):
    """The three fill rows of every buffer (B = 4, delay = 1: rows 0, 1, 3) are uniform on [-3, 3] over the 466 560 rows, and
    uncorrelated between buffer rows and between neighbouring dataset rows."""
    a0 = big[1][..., 0]
    N = a0.shape[0]
    for b in (0, 1, 3):
        _uniform_moments(a0[:, b], 3.0, f"fill {b}")
        assert abs(float((a0[:-1, b] * a0[1:, b]).mean())) <= 5 * 3.0 / math.sqrt(N - 1), b
    for b, e in ((0, 1), (0, 3), (1, 3)):
        assert abs(float((a0[:, b] * a0[:, e]).mean())) <= 5 * 3.0 / math.sqrt(N), (b, e)


def test_interval_means(nlc, big):
    """Over TI = 60 blocks the mean interval is within 5 standard errors of dt: 5 dt / sqrt(3 x 60) on the uniform grid
    (sd 2 dt / sqrt(12)), 5 dt / sqrt(60) on exp (sd dt); uniform intervals lie in (0, 2 dt)."""
    dt, TI, rows = 0.05, 60, 6 * 1296
    te = big[3].view(TI, rows)[:, 0]
    assert float(te.min()) > 0.0 and abs(float(te.mean()) - dt) <= 5 * dt / math.sqrt(TI)
    tu = nlc.generate_synthetic_dataset("oderl-pendulum", 0, 6, ts_grid="uniform", seed=3)[3].cpu().view(TI, -1)[:, 0]
    assert float(tu.min()) > 0.0 and float(tu.max()) < 2 * dt
    assert abs(float(tu.mean()) - dt) <= 5 * dt / math.sqrt(3 * TI)


# ---------------------------------------------------------------------------------------------------- refusals
def _raw_call(nlc, ctx, outs, begin, end, **over):
    from neurallaplacecontrol_amd import _lib

    f = dict(env=0, friction=0, dt=0.05, delay=1, B=4, nu=1, time_channel=0, ts_grid=0, reuse=0, S=81, A=3, action_high=3.0,
             state_max=(C.c_double * 4)(5.0, 20.0, 3.1415927410125732, 30.0), seed=0)
    f.update(over)
    desc = _lib.SynthDesc(**f)
    with ctx.stream():
        return ctx.lib.nlc_synth_generate(ctx.h, C.byref(desc), begin, end, *(_lib.ptr(t) for t in outs))


def test_refusals_before_any_launch(nlc):
    """Each refused input gives the documented error and leaves pre-filled output arrays untouched; a valid call on the same
    ctx then fills them."""
    from neurallaplacecontrol_amd import _lib

    ctx = _lib.Ctx(torch.cuda.current_device())
    R = 2 * 3 * 81
    outs = [torch.full(s, -7.0, dtype=torch.float64, device="cuda") for s in ((R, 5), (R, 4, 1), (R, 5), (R, 1))]
    bad_shape, unsupported, bad_arg = -2, -4, -1
    cases = [
        (dict(env=3), (0, 2), unsupported),  # oderl-cartpole-notrig: not one of the three harness envs
        (dict(env=7), (0, 2), unsupported),
        (dict(delay=4), (0, 2), bad_shape),  # delay >= B
        (dict(delay=-1), (0, 2), bad_shape),
        (dict(B=0, delay=0), (0, 2), bad_shape),
        (dict(nu=2), (0, 2), bad_shape),
        (dict(S=0), (0, 2), bad_shape),
        (dict(A=-3), (0, 2), bad_shape),
        ({}, (-1, 2), bad_shape),
        ({}, (2, 2), bad_shape),
        ({}, (3, 2), bad_shape),
        ({}, (0, 2**31), bad_shape),
        (dict(S=2**20, A=2**10), (0, 2**10), unsupported),  # TI A S = 2^40: at the limit
        (dict(S=2**39, A=2**39), (0, 2), unsupported),  # a product that overflows int64
        (dict(ts_grid=3), (0, 2), bad_arg),
        (dict(dt=0.0), (0, 2), bad_arg),
    ]
    for over, (begin, end), code in cases:
        assert _raw_call(nlc, ctx, outs, begin, end, **over) == code, (over, begin, end)
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs)
    # the Python entry refuses before it allocates or launches
    with pytest.raises(NotImplementedError, match="grid mode"):
        nlc.generate_synthetic_dataset("oderl-cartpole", 1, SPD, rand=False)
    with pytest.raises(ValueError, match="unknown env"):
        nlc.generate_synthetic_dataset("oderl-hopper", 1, SPD)
    with pytest.raises(ValueError, match="unknown env"):
        nlc.generate_synthetic_dataset("oderl-cartpole-notrig", 1, SPD)
    with pytest.raises(ValueError, match="delay"):
        nlc.generate_synthetic_dataset("oderl-cartpole", 4, SPD, action_buffer_size=4)
    for blocks in ((-1, 2), (0, 31), (30, 31), (4, 4)):
        with pytest.raises(ValueError, match="blocks"):
            nlc.generate_synthetic_dataset("oderl-cartpole", 1, SPD, blocks=blocks)
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs)
    # and the same ctx and arrays take a valid call: the raw entry equals the Python function
    assert _raw_call(nlc, ctx, outs, 3, 5, seed=4) == 0
    want = nlc.generate_synthetic_dataset("oderl-cartpole", 1, SPD, action_buffer_size=4, blocks=(3, 5), seed=4)
    assert all(torch.equal(x, y) for x, y in zip(outs, want))


# ---------------------------------------------------------------------------------------------------- end to end
def _ref_loop(model, data, perm, bs, iters):
    """train_utils.py:391-408 on the model's grad-mode path: MSE, clip_grad_norm_(0.1), Adam(1e-4)."""
    s0, a0, sn, ts = data
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    out = []
    for i in range(iters):
        ind = perm[i * bs : (i + 1) * bs]
        opt.zero_grad()
        pred = model(s0[ind], a0[ind], ts[ind])
        loss = torch.nn.MSELoss()(pred.squeeze(), (sn[ind] - s0[ind]).squeeze())
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)
        opt.step()
        out.append(loss.item())
    return torch.tensor(out, dtype=torch.float64)


def test_dataset_goes_straight_into_the_trainers(nlc):
    """A cartpole dataset of samples_per_dim = 3 (7 290 rows, exp grid) into NLTrainer.run and RNNTrainer.run as it is, 20
    iterations at batch 16 on small golden-shape models: the losses are finite and match the same trainers' grad-mode path
    (the reference loop on a twin, on the same tensors) to the 1e-9 relative docs/training.md states for run()."""
    from gpu_common import build_model

    from oracle import nl_model as onl

    bs, iters = 16, 20
    data = nlc.generate_synthetic_dataset("oderl-cartpole", 2, SPD, action_buffer_size=4, ts_grid="exp", seed=8)
    assert data[0].shape[0] == 7290
    perm = torch.randperm(7290, generator=torch.Generator().manual_seed(5))[: bs * iters].cuda()
    st = onl.ENV_STATS["oderl-cartpole"]
    sd = onl.make_synthetic_state_dict(3, st["d"], st["nu"], 128, 17, st["state_std"], [st["act_high"] / 2], tame=True)
    torch.manual_seed(1)
    rnn_kw = dict(hidden_units=64, state_mean=np.zeros(5), state_std=np.asarray(st["state_std"], dtype=np.float64),
                  action_mean=np.zeros(1), action_std=np.array([st["act_high"] / 2]), normalize=True, normalize_time=True)
    rnn_sd = nlc.DeltaTRNN(5, 1, **rnn_kw).double().state_dict()

    def make_rnn():
        m = nlc.DeltaTRNN(5, 1, **rnn_kw).double()
        m.load_state_dict(rnn_sd)
        return m.cuda()

    pairs = [("nl", nlc.NLTrainer, lambda: build_model(nlc, sd)), ("rnn", nlc.RNNTrainer, make_rnn)]
    for name, trainer, make in pairs:
        model, twin = make(), make()
        losses = trainer(model, lr=1e-4, clip_grad_norm=0.1).run(*data, perm, batch_size=bs)
        assert losses.shape == (iters,) and bool(torch.isfinite(losses).all()), name
        ref = _ref_loop(twin, data, perm, bs, iters)
        rel = float(((losses.cpu() - ref).abs() / ref.abs()).max())
        print(f"{name}: run() vs the grad-mode loop over {iters} iterations, loss rel err {rel:.3e}")
        assert rel <= 1e-9, f"{name}: loss rel err {rel:.3e}"
