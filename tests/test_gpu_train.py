"""GPU: the fused training step (NLTrainer / nlc_train_step) against autograd through the CPU oracle and against the
reference's training loop on the existing grad-mode path (train_utils.py:388-408)."""

import copy
import warnings

import numpy as np
import pytest
import torch
from train_compare import assert_grad_close

pytestmark = pytest.mark.gpu


def _stats(env):
    from oracle import nl_model as onl

    return onl.ENV_STATS["oderl-" + env]


def _sd(env, h, S, enc=False, seed=3, tame=True):
    from oracle import nl_model as onl

    st = _stats(env)
    return onl.make_synthetic_state_dict(seed, st["d"], st["nu"], h, S, st["state_std"], [st["act_high"] / 2],
                                         encode_obs_time=enc, tame=tame)


def _model(nlc, sd, env, h, S, enc=False, algo="fourier"):
    st = _stats(env)
    d, nu = st["d"], st["nu"]
    m = nlc.NeuralLaplaceModel(
        d, nu, d, hidden_units=h, s_recon_terms=S, ilt_algorithm=algo, encode_obs_time=enc, state_mean=np.zeros(d),
        state_std=np.ones(d), action_mean=np.array([0] * nu), action_std=np.array([1.0]), normalize=True, normalize_time=True,
    ).double()
    m.load_state_dict(sd)
    return m.to("cuda")


def _data(env, M, B, enc=False, seed=17):
    """A synthetic dataset in the reference's layout: s0 (M, d), a0 (M, B, nin), sn (M, d), ts (M, 1)."""
    st = _stats(env)
    d, nu, A = st["d"], st["nu"], st["act_high"]
    g = torch.Generator().manual_seed(seed)
    std = torch.tensor(st["state_std"], dtype=torch.float64)
    s0 = torch.randn(M, d, dtype=torch.float64, generator=g) * std
    a0 = (torch.rand(M, B, nu, dtype=torch.float64, generator=g) * 2 - 1) * A
    if enc:  # the harness's time channel (mppi_with_model.py:110-119)
        tch = torch.flip(torch.arange(B), (0,)).view(1, B, 1).repeat(M, 1, 1).to(torch.float64)
        a0 = torch.cat((a0, tch), dim=2)
    sn = s0 + torch.randn(M, d, dtype=torch.float64, generator=g) * 0.05 * std
    ts = torch.rand(M, 1, dtype=torch.float64, generator=g) * 0.08 + 0.02
    return s0, a0, sn, ts


def _ref_step(model, opt, bs0, ba0, bts, bsd, clip):
    """train_utils.py:391-408 on the model's existing grad-mode path."""
    opt.zero_grad()
    pred = model(bs0, ba0, bts)
    loss = torch.nn.MSELoss()(pred.squeeze(), bsd.squeeze())
    loss.backward()
    if clip > 0:
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
    opt.step()
    return loss.item()


def _close_to_scale(got, ref, tol, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    sc = float(ref.abs().max()) + 1e-300
    err = float((got - ref).abs().max())
    assert err <= tol * sc, f"{what}: max err {err:.3e} > {tol:g} x {sc:.3e}"


# (env, h, S, N, B, encode_obs_time)
LG_CASES = [
    ("cartpole", 128, 17, 16, 4, False),
    ("cartpole", 64, 33, 1, 4, False),
    ("pendulum", 64, 17, 203, 4, True),
    ("pendulum", 256, 33, 16, 1, False),
    ("acrobot", 128, 33, 203, 4, False),
    ("acrobot", 256, 17, 16, 16, False),
    ("cartpole", 64, 17, 4096, 4, True),
    ("acrobot", 64, 17, 4096, 2, False),
]


@pytest.mark.parametrize("env,h,S,N,B,enc", LG_CASES)
def test_loss_and_grad_vs_oracle_autograd(nlc, env, h, S, N, B, enc):
    """loss_and_grad: the loss to 1e-12 relative and every parameter gradient to 1e-9 of its block's max |grad| (each GRU gate
    block, each theta / phi half of the last layer: tests/train_compare.py), against autograd through
    oracle.nl_model.nl_forward + ((pred - target)^2).mean() on the CPU."""
    from oracle import nl_model as onl

    sd = _sd(env, h, S, enc)
    s0, a0, sn, ts = _data(env, N, B, enc)
    target = sn - s0
    names = [k for k in sd if k.startswith(("action_encoder.", "laplace_rep_func."))]
    leaves = {k: (v.clone().requires_grad_() if k in names else v) for k, v in sd.items()}
    ref_loss = ((onl.nl_forward(leaves, s0, a0, ts, S=S) - target) ** 2).mean()
    ref_loss.backward()
    model = _model(nlc, sd, env, h, S, enc)
    tr = nlc.NLTrainer(model)
    assert tr.fused
    loss = tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), target.cuda())
    assert loss.dim() == 0 and loss.is_cuda
    assert abs(float(loss) - float(ref_loss)) <= 1e-12 * abs(float(ref_loss))
    for k, p in model.named_parameters():
        assert_grad_close(k, p.grad, leaves[k].grad, 1e-9)


@pytest.mark.parametrize("clip,wd", [(0.1, 0.0), (1e6, 0.0), (0.1, 1e-2), (0.0, 0.0)])
def test_one_step_vs_clip_and_adam(nlc, clip, wd):
    """step() == the grad-mode forward + clip_grad_norm_(clip) + torch.optim.Adam(lr=1e-4) on a twin model: parameters,
    exp_avg and exp_avg_sq to 1e-12 of each tensor's magnitude (clip active, inactive, off, and with weight decay)."""
    env, h, S = "cartpole", 128, 17
    sd = _sd(env, h, S)
    s0, a0, sn, ts = _data(env, 16, 4)
    bsd = (sn - s0).cuda()
    model, twin = _model(nlc, sd, env, h, S), _model(nlc, sd, env, h, S)
    tr = nlc.NLTrainer(model, lr=1e-4, weight_decay=wd, clip_grad_norm=clip)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4, weight_decay=wd)
    ref_loss = _ref_step(twin, opt, s0.cuda(), a0.cuda(), ts.cuda(), bsd, clip)
    loss = tr.step(s0.cuda(), a0.cuda(), ts.cuda(), bsd)
    assert abs(float(loss) - ref_loss) <= 1e-12 * abs(ref_loss)
    sd_tr = tr.state_dict()
    sd_ref = opt.state_dict()
    named_twin = dict(twin.named_parameters())
    for i, (k, p) in enumerate(model.named_parameters()):
        _close_to_scale(p, named_twin[k], 1e-12, k)
        for key in ("exp_avg", "exp_avg_sq"):
            _close_to_scale(sd_tr["state"][i][key], sd_ref["state"][i][key], 1e-12, f"{k} {key}")
        assert float(sd_tr["state"][i]["step"]) == 1.0


def test_clip_is_active_at_the_test_shape(nlc):
    """The one-step test's clip = 0.1 case really clips (total gradient norm above 0.1), and the 1e6 case does not."""
    env, h, S = "cartpole", 128, 17
    s0, a0, sn, ts = _data(env, 16, 4)
    model = _model(nlc, _sd(env, h, S), env, h, S)
    tr = nlc.NLTrainer(model)
    tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), (sn - s0).cuda())
    total = float(torch.cat([p.grad.reshape(-1) for p in model.parameters()]).norm())
    assert 0.1 < total < 1e6


def _roundoff_misses(got, ref, grads_ref, tol, what):
    """Parameters within tol of max |p|; an element that misses must belong to a gradient that is roundoff-sized at some
    iteration: |g| below 1e-12 of its tensor's max |g| there (Adam divides by sqrt(v) + eps, so such an element's step is
    set by roundoff)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    sc = float(ref.abs().max()) + 1e-300
    bad = (got - ref).abs() > tol * sc
    if not bool(bad.any()):
        return 0
    tiny = torch.zeros_like(bad)
    for g in grads_ref:
        tiny |= g.abs() <= 1e-12 * (float(g.abs().max()) + 1e-300)
    assert bool(tiny[bad].all()), f"{what}: {int(bad.sum())} elements miss {tol:g} x {sc:.3e} without a roundoff-sized gradient"
    return int(bad.sum())


def test_run_200_iterations_vs_reference_loop(nlc):
    """run() over 200 iterations of a fixed permutation == the reference loop on the grad-mode path: every loss to 1e-9
    relative, final parameters to 1e-9 of max |p| (roundoff-sized-gradient elements shown to be so)."""
    env, h, S, bs, iters = "cartpole", 128, 17, 16, 200
    sd = _sd(env, h, S)
    s0, a0, sn, ts = _data(env, bs * iters + 5, 4)
    perm = torch.randperm(s0.shape[0], generator=torch.Generator().manual_seed(5))
    model, twin = _model(nlc, sd, env, h, S), _model(nlc, sd, env, h, S)
    tr = nlc.NLTrainer(model, lr=1e-4, clip_grad_norm=0.1)
    losses = tr.run(s0.cuda(), a0.cuda(), sn.cuda(), ts.cuda(), perm.cuda(), batch_size=bs)
    assert losses.shape == (iters,) and losses.is_cuda
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    s0c, a0c, snc, tsc = s0.cuda(), a0.cuda(), sn.cuda(), ts.cuda()
    ref, grads = [], {k: [] for k, _ in twin.named_parameters()}
    for i in range(iters):
        ind = perm[i * bs : i * bs + bs].cuda()
        ref.append(_ref_step(twin, opt, s0c[ind], a0c[ind], tsc[ind], snc[ind] - s0c[ind], 0.1))
        for k, p in twin.named_parameters():
            grads[k].append(p.grad.detach().cpu().clone())
    ref = torch.tensor(ref, dtype=torch.float64)
    rel = ((losses.cpu() - ref).abs() / ref.abs()).max()
    assert float(rel) <= 1e-9, f"loss rel err {float(rel):.3e}"
    named_twin = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        _roundoff_misses(p, named_twin[k], grads[k], 1e-9, k)


def test_run_is_bit_reproducible(nlc):
    env, h, S, bs = "acrobot", 128, 17, 16
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, 40 * bs, 4))
    perm = torch.randperm(s0.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
    out = []
    for _ in range(2):
        model = _model(nlc, sd, env, h, S)
        tr = nlc.NLTrainer(model)
        losses = tr.run(s0, a0, sn, ts, perm, batch_size=bs)
        out.append((losses.cpu(), [p.detach().cpu().clone() for p in model.parameters()]))
    assert torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)


def test_optimizer_state_round_trips_with_adam(nlc):
    """5 fused steps, state_dict() into torch.optim.Adam, 5 reference steps == 10 fused steps; and the way back: an Adam
    state loaded into a trainer continues the reference's trajectory."""
    env, h, S, bs = "cartpole", 64, 17, 16
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, 10 * bs, 4))
    batches = [(s0[i * bs:(i + 1) * bs], a0[i * bs:(i + 1) * bs], ts[i * bs:(i + 1) * bs],
                sn[i * bs:(i + 1) * bs] - s0[i * bs:(i + 1) * bs]) for i in range(10)]
    full = _model(nlc, sd, env, h, S)
    tr_full = nlc.NLTrainer(full)
    for b in batches:
        tr_full.step(*b)
    mixed = _model(nlc, sd, env, h, S)
    tr = nlc.NLTrainer(mixed)
    for b in batches[:5]:
        tr.step(*b)
    opt = torch.optim.Adam(mixed.parameters(), lr=1e-4)
    opt.load_state_dict(tr.state_dict())
    for b in batches[5:]:
        _ref_step(mixed, opt, *b, 0.1)
    named = dict(mixed.named_parameters())
    for k, p in full.named_parameters():
        _close_to_scale(named[k], p, 1e-9, k)
    # torch Adam -> trainer
    ref = _model(nlc, sd, env, h, S)
    opt2 = torch.optim.Adam(ref.parameters(), lr=1e-4)
    for b in batches[:5]:
        _ref_step(ref, opt2, *b, 0.1)
    back = _model(nlc, {k: v.detach().cpu() for k, v in ref.state_dict().items()}, env, h, S)
    tr2 = nlc.NLTrainer(back)
    tr2.load_state_dict(opt2.state_dict())
    for b in batches[5:]:
        _ref_step(ref, opt2, *b, 0.1)
        tr2.step(*b)
    named = dict(back.named_parameters())
    for k, p in ref.named_parameters():
        _close_to_scale(named[k], p, 1e-9, k)


def test_lr_change_between_calls(nlc):
    env, h, S = "pendulum", 64, 17
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, 32, 4))
    model, twin = _model(nlc, sd, env, h, S), _model(nlc, sd, env, h, S)
    tr = nlc.NLTrainer(model)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for i in range(2):
        b = (s0[16 * i:16 * i + 16], a0[16 * i:16 * i + 16], ts[16 * i:16 * i + 16], sn[16 * i:16 * i + 16] - s0[16 * i:16 * i + 16])
        _ref_step(twin, opt, *b, 0.1)
        sched.step()
        tr.step(*b)
        tr.lr = opt.param_groups[0]["lr"]
    named = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        _close_to_scale(p, named[k], 1e-12, k)


def test_trained_weights_reach_forward_and_planner(nlc):
    """After run(): model(...) under no_grad and MPPIDelay.command() -- on a planner built BEFORE training -- equal the same
    calls on a model freshly built from model.state_dict() to 1e-12."""
    env, h, S, bs = "cartpole", 128, 17, 16
    st = _stats(env)
    d, nu, A = st["d"], st["nu"], st["act_high"]
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, 20 * bs, 4))
    model = _model(nlc, sd, env, h, S)

    def planner(m, U0, raw):
        mppi = nlc.MPPIDelay(nlc.NLDynamics(m, 0.05), nlc.EnvCost("oderl-" + env), d, nlc.noise_sigma(nu), 256, 10, "cpu",
                             lambda_=1.0, u_min=torch.tensor(-A), u_max=torch.tensor(A), u_scale=A, U_init=U0.clone())
        mppi.noise_dist = type("Replay", (), {"sample": staticmethod(lambda shape: raw)})()
        return mppi

    gen = torch.Generator().manual_seed(0)
    raw = torch.randn(256, 10, nu, dtype=torch.float64, generator=gen)
    U0 = torch.randn(10, nu, dtype=torch.float64, generator=gen) * 0.1
    state, ab = nlc.initial_state("oderl-" + env), torch.zeros(4, nu, dtype=torch.float64)
    early = planner(model, U0, raw)
    before = early.command(state, ab)
    tr = nlc.NLTrainer(model, lr=1e-3)
    tr.run(s0, a0, sn, ts, torch.arange(s0.shape[0]).cuda(), batch_size=bs)
    fresh = _model(nlc, {k: v.detach().cpu() for k, v in model.state_dict().items()}, env, h, S)
    with torch.no_grad():
        y = model(s0[:64], a0[:64], ts[:64])
        y_ref = fresh(s0[:64], a0[:64], ts[:64])
    np.testing.assert_allclose(y.cpu().numpy(), y_ref.cpu().numpy(), rtol=1e-12, atol=1e-14)
    early.U = U0.clone()
    after = early.command(state, ab)
    ref = planner(fresh, U0, raw).command(state, ab)
    np.testing.assert_allclose(after.cpu().numpy(), ref.cpu().numpy(), rtol=1e-12, atol=1e-14)
    assert not torch.equal(after.cpu(), before.cpu())


def test_fallback_dehoog_warns_once_and_matches_reference_loop(nlc):
    from oracle import nl_model as onl

    env, h, S, bs = "cartpole", 128, 9, 16
    st = _stats(env)
    sd = onl.make_synthetic_state_dict(3, st["d"], st["nu"], h, S, st["state_std"], [st["act_high"] / 2], tame="dehoog")
    s0, a0, sn, ts = (t.cuda() for t in _data(env, 5 * bs, 4))
    model, twin = _model(nlc, sd, env, h, S, algo="dehoog"), _model(nlc, sd, env, h, S, algo="dehoog")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(model)
        losses = tr.run(s0, a0, sn, ts, torch.arange(s0.shape[0]).cuda(), batch_size=bs)
        tr.step(s0[:bs], a0[:bs], ts[:bs], sn[:bs] - s0[:bs])
    mine = [w for w in rec if "NLTrainer" in str(w.message)]
    assert len(mine) == 1 and not tr.fused
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    ref = [_ref_step(twin, opt, s0[i * bs:(i + 1) * bs], a0[i * bs:(i + 1) * bs], ts[i * bs:(i + 1) * bs],
                     sn[i * bs:(i + 1) * bs] - s0[i * bs:(i + 1) * bs], 0.1) for i in range(5)]
    np.testing.assert_allclose(losses.cpu().numpy(), ref, rtol=1e-12)
    assert tr.state_dict()["state"][0]["step"] == 6


def test_trainer_rejects_float32_and_host_models(nlc):
    env, h, S = "cartpole", 64, 17
    model = _model(nlc, _sd(env, h, S), env, h, S)
    with pytest.raises(NotImplementedError, match="float64"):
        nlc.NLTrainer(copy.deepcopy(model).float())
    with pytest.raises(RuntimeError, match="GPU"):
        nlc.NLTrainer(copy.deepcopy(model).cpu())


# ----------------------------------------------------------------------------------------------------------------------
# Shape-domain sweep: synthetic models of any (d, nu) the library accepts, against float64 autograd through the oracle.

def _gen_setup(d, nu, enc, h, S, B, N, normalize=True, normalize_time=True, mean=False, ilt=None, tscale=1.0, seed=0):
    """Synthetic weights (make_synthetic_state_dict, tamed), normalisation buffers (state / action std drawn per dim, means
    non-zero if `mean`) and a dataset: s0 (N, d), a0 (N, B, nin) (+ the harness's time channel if `enc`), ts (N, 1) in
    tscale x the default row-time range [0.02, 0.1), target (N, d)."""
    from oracle import nl_model as onl

    nin = nu + int(enc)
    rng = np.random.RandomState(seed)
    std = rng.uniform(0.5, 3.0, d)
    sd = onl.make_synthetic_state_dict(seed, d, nu, h, S, list(std), [1.0], encode_obs_time=enc, tame=True)
    sm = rng.uniform(-1.0, 1.0, d) if mean else np.zeros(d)
    sd["state_mean"] = torch.tensor(sm, dtype=torch.float64)
    sd["action_mean"] = torch.tensor(rng.uniform(-0.5, 0.5, nin) if mean else np.zeros(nin), dtype=torch.float64)
    sd["action_std"] = torch.tensor(rng.uniform(0.5, 2.0, nin), dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + 1)
    s0 = torch.tensor(sm) + torch.randn(N, d, dtype=torch.float64, generator=g) * torch.tensor(std)
    a0 = (torch.rand(N, B, nu, dtype=torch.float64, generator=g) * 2 - 1) * 2.0
    if enc:
        tch = torch.flip(torch.arange(B), (0,)).view(1, B, 1).repeat(N, 1, 1).to(torch.float64)
        a0 = torch.cat((a0, tch), dim=2)
    ts = (torch.rand(N, 1, dtype=torch.float64, generator=g) * 0.08 + 0.02) * tscale
    tgt = torch.randn(N, d, dtype=torch.float64, generator=g) * 0.05 * torch.tensor(std)
    return sd, (s0, a0, ts, tgt)


def _gen_model(nlc, sd, d, nu, enc, h, S, normalize=True, normalize_time=True, ilt=None, algo="fourier"):
    nin = nu + int(enc)
    m = nlc.NeuralLaplaceModel(
        d, nu, d, hidden_units=h, s_recon_terms=S, ilt_algorithm=algo, encode_obs_time=enc, state_mean=np.zeros(d),
        state_std=np.ones(d), action_mean=np.zeros(nin), action_std=np.ones(nin), normalize=normalize,
        normalize_time=normalize_time,
    ).double()
    m.load_state_dict(sd)
    m.ilt_options = ilt
    return m.to("cuda")


def _oracle_loss_grads(sd, data, S, normalize=True, normalize_time=True, ilt=None):
    """Float64 autograd through oracle.nl_model.nl_forward + ((pred - target)^2).mean() on the CPU."""
    from oracle import nl_model as onl

    s0, a0, ts, tgt = data
    names = [k for k in sd if k.startswith(("action_encoder.", "laplace_rep_func."))]
    leaves = {k: (v.clone().requires_grad_() if k in names else v) for k, v in sd.items()}
    pred = onl.nl_forward(leaves, s0, a0, ts, S=S, normalize=normalize, normalize_time=normalize_time, ilt_options=ilt)
    loss = ((pred.reshape(tgt.shape) - tgt) ** 2).mean()
    loss.backward()
    return loss.detach(), {k: leaves[k].grad for k in names}


def _max_terms(d):
    """Largest S nlc_set_model takes for a Fourier model of state dim d: the ILT tables' 129 terms, and the last layer's
    2 d S outputs in at most 25 output tiles (nlc_pack.h ilt_tiles_needed, kernels_nl.hip nl_pick_nt3)."""
    def tiles(S):
        n_even, n_odd = d * ((S + 1) // 2), d * (S // 2)
        return ((n_even + 3) // 4 + (n_odd + 3) // 4 + 1) // 2
    return max(S for S in range(1, 130) if tiles(S) <= 25)


# (label, d, nu, enc, h, S, B, N, normalize, normalize_time, mean, ilt_options, tscale)
# K0 = 2S + d + 2 (layer-0 inputs), O = 2dS (last-layer outputs): the MFMA weight-gradient tiles' M / K
SWEEP_FIXED = [
    ("d1_S16_O32_B3_N15", 1, 1, False, 64, 16, 3, 15, True, True, False, None, 1.0),
    ("d2_nu2_S4_B5_N17", 2, 2, False, 128, 4, 5, 17, True, True, True, None, 1.0),
    ("d4_S13_K0_32_B7", 4, 1, False, 128, 13, 7, 33, True, True, False, None, 1.0),
    ("d5_S13_K0_33_O130_B15", 5, 1, False, 64, 13, 15, 16, True, True, False, None, 1.0),
    ("d3_nu3_S3_B5", 3, 3, False, 64, 3, 5, 20, True, True, True, None, 1.0),
    ("d2_nu2_enc_raw_S32_O128", 2, 2, True, 128, 32, 4, 17, False, False, False, None, 1.0),
    ("d1_Smax", 1, 1, False, 64, _max_terms(1), 2, 16, True, True, False, None, 1.0),
    ("d6_Smax", 6, 2, False, 128, _max_terms(6), 3, 20, True, True, False, None, 1.0),
    ("d2_S62_K0_128", 2, 1, True, 64, 62, 1, 17, True, True, False, None, 1.0),
    ("d3_S62_K0_129_h256", 3, 1, False, 256, 62, 2, 15, True, True, False, None, 1.0),
    ("d4_S16_O128_B16", 4, 1, False, 64, 16, 16, 16, True, True, False, None, 1.0),
    ("d2_S8_O32_N1_h256", 2, 1, False, 256, 8, 1, 1, True, True, False, None, 1.0),
    ("N2048_128_tiles", 3, 1, False, 64, 9, 3, 2048, True, True, False, None, 1.0),
    ("N2049_ragged_second", 2, 1, False, 64, 7, 5, 2049, True, True, True, None, 1.0),
    ("N4103_ragged_third", 4, 2, False, 64, 5, 3, 4103, True, True, False, None, 1.0),
    ("normalize_time_off", 3, 1, False, 128, 17, 4, 40, True, False, True, None, 1.0),
    ("normalize_off", 5, 1, False, 64, 17, 4, 40, False, True, False, None, 1.0),
    ("ilt_alpha_tol", 3, 2, False, 128, 17, 4, 40, True, True, True, {"alpha": 0.05, "tol": 1e-4}, 1.0),
    ("t_0.2x", 5, 1, False, 128, 17, 4, 40, True, True, False, None, 0.2),
    ("t_4x_enc", 5, 1, True, 64, 33, 4, 40, True, True, True, None, 4.0),
]


def _random_train_cases(n=12, seed=2026):
    rng = np.random.RandomState(seed)
    cases = []
    for i in range(n):
        d, nu = int(rng.randint(1, 7)), int(rng.randint(1, 4))
        enc = bool(nu < 3 and rng.rand() < 0.3)
        h = [64, 128, 256][rng.randint(3)]
        S = int(rng.randint(1, min(40, _max_terms(d)) + 1))
        B, N = int(rng.randint(1, 17)), int(rng.randint(1, 300))
        normalize, normalize_time, mean = bool(rng.rand() < 0.75), bool(rng.rand() < 0.75), bool(rng.rand() < 0.5)
        ilt = None if rng.rand() < 0.7 else {"alpha": float(rng.uniform(1e-4, 0.1)), "tol": float(10 ** rng.uniform(-6, -2))}
        tscale = float(rng.choice([0.2, 0.5, 1.0, 2.0, 4.0]))
        cases.append((f"rand{i}", d, nu, enc, h, S, B, N, normalize, normalize_time, mean, ilt, tscale))
    return cases


SWEEP_CASES = SWEEP_FIXED + _random_train_cases()
# cases held to the condition-aware bound (the oracle's own response to a 1e-13 input perturbation), with the reason
SWEEP_CONDITION_AWARE = {}


@pytest.mark.parametrize("case", SWEEP_CASES, ids=[c[0] for c in SWEEP_CASES])
def test_loss_and_grad_shape_sweep_vs_oracle(nlc, case):
    """loss_and_grad over the shape domain the library accepts: d 1..6, GRU input dim 1..3 (with and without the time
    channel), widths 64 / 128 / 256, even / odd / largest S, MFMA weight-gradient dims at and one past a multiple of 16,
    odd windows, N ragged against the 16-row tile and past 128 tiles (a workgroup's second and third tile, ragged),
    normalize / normalize_time off, non-zero means, non-default ILT alpha / tol, row times 0.2x .. 4x.  Loss to 1e-12
    relative, every gradient block (tests/train_compare.py) to 1e-9 of its own max."""
    label, d, nu, enc, h, S, B, N, normalize, normalize_time, mean, ilt, tscale = case
    sd, data = _gen_setup(d, nu, enc, h, S, B, N, normalize, normalize_time, mean, ilt, tscale, seed=len(label) + 7 * d + S)
    ref_loss, ref_grads = _oracle_loss_grads(sd, data, S, normalize, normalize_time, ilt)
    model = _gen_model(nlc, sd, d, nu, enc, h, S, normalize, normalize_time, ilt)
    tr = nlc.NLTrainer(model)
    assert tr.fused
    loss = tr.loss_and_grad(*(t.cuda() for t in data))
    sens = None
    if label in SWEEP_CONDITION_AWARE:
        s0, a0, ts, tgt = data
        probe = (s0 * (1 + 1e-13), a0 * (1 + 1e-13), ts * (1 + 1e-13), tgt)
        _, pg = _oracle_loss_grads(sd, probe, S, normalize, normalize_time, ilt)
        sens = {k: (pg[k] - ref_grads[k]).abs() for k in ref_grads}
    rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    assert rel <= 1e-12, f"loss rel err {rel:.3e}"
    for k, p in model.named_parameters():
        assert_grad_close(k, p.grad, ref_grads[k], 1e-9, sens=None if sens is None else sens[k])


def test_sweep_covers_the_issue_edges():
    """The listed sweep keeps the edges it was built for (a guard against editing them away)."""
    ds = {c[1] for c in SWEEP_CASES}
    assert {1, 2, 4} <= ds
    assert any(c[2] == 3 for c in SWEEP_CASES) and any(c[2] == 2 and c[3] and not c[8] for c in SWEEP_CASES)
    assert {3, 4, 16, 32, _max_terms(1)} <= {c[5] for c in SWEEP_CASES}
    assert any(c[1] == 6 and c[5] == _max_terms(6) for c in SWEEP_CASES)
    k0 = {2 * c[5] + c[1] + 2 for c in SWEEP_CASES}
    o = {2 * c[1] * c[5] for c in SWEEP_CASES}
    assert {32, 33, 128, 129} <= k0 and {32, 128} <= o
    assert {3, 5, 7, 15} <= {c[6] for c in SWEEP_CASES}
    assert {15, 17, 2048, 2049, 4103} <= {c[7] for c in SWEEP_CASES}
    assert any(not c[8] for c in SWEEP_CASES) and any(c[8] and not c[9] for c in SWEEP_CASES)
    assert any(c[10] for c in SWEEP_CASES) and any(c[11] for c in SWEEP_CASES)
    assert {0.2, 4.0} <= {c[12] for c in SWEEP_CASES}


# ----------------------------------------------------------------------------------------------------------------------
# Optimiser, run(), gradnorm, fallback shapes

def _batch(s0, a0, sn, ts, i, bs):
    sl = slice(i * bs, (i + 1) * bs)
    return s0[sl], a0[sl], ts[sl], sn[sl] - s0[sl]


def _assert_adam_state_equal(model, twin, tr, opt, tol, steps):
    sd_tr, sd_ref = tr.state_dict(), opt.state_dict()
    named_twin = dict(twin.named_parameters())
    for i, (k, p) in enumerate(model.named_parameters()):
        _close_to_scale(p, named_twin[k], tol, k)
        for key in ("exp_avg", "exp_avg_sq"):
            _close_to_scale(sd_tr["state"][i][key], sd_ref["state"][i][key], tol, f"{k} {key}")
        assert float(sd_tr["state"][i]["step"]) == float(sd_ref["state"][i]["step"]) == steps, k


def test_steps_with_non_default_adam_hyperparameters(nlc):
    """5 step()s with betas (0.3, 0.95) -- torch.lerp's other branch in the moment update --, eps 1e-3 and weight decay
    1e-2 == the grad-mode forward + clip_grad_norm_ + torch.optim.Adam with the same settings: parameters and both moments
    to 1e-12 of each tensor's magnitude."""
    env, h, S, bs = "cartpole", 128, 17, 16
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, 5 * bs, 4))
    model, twin = _model(nlc, sd, env, h, S), _model(nlc, sd, env, h, S)
    kw = dict(lr=1e-3, betas=(0.3, 0.95), eps=1e-3, weight_decay=1e-2)
    tr = nlc.NLTrainer(model, clip_grad_norm=0.1, **kw)
    opt = torch.optim.Adam(twin.parameters(), **kw)
    for i in range(5):
        b = _batch(s0, a0, sn, ts, i, bs)
        ref = _ref_step(twin, opt, *b, 0.1)
        loss = tr.step(*b)
        assert abs(float(loss) - ref) <= 1e-12 * abs(ref)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 5)


def _perm_cases():
    g = np.random.RandomState(9)
    dup = torch.as_tensor(g.randint(0, 300, size=16 * 12))  # draws with replacement: duplicates, unsorted, not every row
    return {
        "duplicates_subset": (300, dup, 16),
        "bs7": (7 * 15 + 3, torch.randperm(7 * 15 + 3, generator=torch.Generator().manual_seed(3)), 7),
        "bs20": (20 * 10 + 5, torch.randperm(20 * 10 + 5, generator=torch.Generator().manual_seed(4)), 20),
        "bs2100": (2 * 2100 + 13, torch.randperm(2 * 2100 + 13, generator=torch.Generator().manual_seed(5)), 2100),
    }


@pytest.mark.parametrize("which", ["duplicates_subset", "bs7", "bs20", "bs2100"])
def test_run_permutations_and_batch_sizes_vs_reference_loop(nlc, which):
    """run() == the reference loop (_ref_step per batch) for a permutation with duplicates that is an unsorted strict
    subset of the rows, batch sizes 7 and 20, and batches of 2100 rows (one iteration walks 132 tiles, more than the 128
    workgroups): losses to 1e-9 relative, final parameters as in test_run_200_iterations_vs_reference_loop."""
    M, perm, bs = _perm_cases()[which]
    if which == "duplicates_subset":
        assert len(set(perm.tolist())) < perm.numel() and len(set(perm.tolist())) < M
        assert not bool((perm[1:] >= perm[:-1]).all())
    env, h, S = "acrobot", 64, 17
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, M, 3))
    model, twin = _model(nlc, sd, env, h, S), _model(nlc, sd, env, h, S)
    tr = nlc.NLTrainer(model, lr=1e-3, clip_grad_norm=0.1)
    losses = tr.run(s0, a0, sn, ts, perm.cuda(), batch_size=bs)
    iters = perm.numel() // bs
    assert losses.shape == (iters,)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    ref, grads = [], {k: [] for k, _ in twin.named_parameters()}
    for i in range(iters):
        ind = perm[i * bs : (i + 1) * bs].cuda()
        ref.append(_ref_step(twin, opt, s0[ind], a0[ind], ts[ind], sn[ind] - s0[ind], 0.1))
        for k, p in twin.named_parameters():
            grads[k].append(p.grad.detach().cpu().clone())
    ref = torch.tensor(ref, dtype=torch.float64)
    rel = ((losses.cpu() - ref).abs() / ref.abs()).max()
    assert float(rel) <= 1e-9, f"loss rel err {float(rel):.3e}"
    named_twin = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        _roundoff_misses(p, named_twin[k], grads[k], 1e-9, k)
    assert float(tr.state_dict()["state"][0]["step"]) == iters


def test_train_step_gradnorm_equals_clip_grad_norm(nlc):
    """nlc_train_step's gradnorm output (include/nlc.h, ABI 10), called through ctypes on the trainer's ctx, equals the
    total norm torch.nn.utils.clip_grad_norm_ returns on the same gradients (those of loss_and_grad: the same kernels)
    to 1e-12 relative."""
    import ctypes as C

    env, h, S, N, B = "pendulum", 128, 17, 40, 4
    s0, a0, sn, ts = (t.cuda() for t in _data(env, N, B))
    model = _model(nlc, _sd(env, h, S), env, h, S)
    tr = nlc.NLTrainer(model)
    tr.loss_and_grad(s0, a0, ts, sn - s0)
    ref = float(torch.nn.utils.clip_grad_norm_(list(model.parameters()), 1e300))
    obs, win, tsd, tgt = tr._data(s0, a0, ts, sn - s0)
    flat = torch.cat([p.detach().reshape(-1) for p in tr._params]).contiguous()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    loss = torch.empty((), dtype=torch.float64, device="cuda")
    gnorm = torch.full((), float("nan"), dtype=torch.float64, device="cuda")
    idx = torch.arange(N, dtype=torch.int64, device="cuda")
    ws = tr._workspace(N)
    ctx = tr._ctx
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.device(0):
        ctx.use_torch_stream()
        ctx.check(ctx.lib.nlc_train_step(ctx.h, C.byref(tr._desc()), p(flat), p(m), p(v), 1, p(obs), p(win), p(tsd), p(tgt),
                                         p(idx), N, B, p(loss), p(gnorm), p(ws)))
    got = float(gnorm)
    assert 0.1 < ref, "the test wants a clipping case"
    assert abs(got - ref) <= 1e-12 * ref, f"gradnorm {got!r} vs clip_grad_norm_ {ref!r}"


@pytest.mark.parametrize("d,h", [(5, 96), (7, 128)])
def test_fallback_shapes_warn_once_and_match_reference_loop(nlc, d, h):
    """Shapes nlc_set_model refuses (a width the kernels are not instantiated for, a state dim past 6): one warning at
    construction, and run() + step() equal the reference loop on a twin (losses to 1e-12 relative), step count included."""
    S, bs, nu = 9, 16, 1
    sd, (s0, a0, ts, tgt) = _gen_setup(d, nu, False, h, S, 4, 5 * bs, seed=d + h)
    s0, a0, ts = s0.cuda(), a0.cuda(), ts.cuda()
    sn = s0 + tgt.cuda()
    model, twin = _gen_model(nlc, sd, d, nu, False, h, S), _gen_model(nlc, sd, d, nu, False, h, S)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(model)
        losses = tr.run(s0, a0, sn, ts, torch.arange(s0.shape[0]).cuda(), batch_size=bs)
        tr.step(*_batch(s0, a0, sn, ts, 0, bs))
    mine = [w for w in rec if "NLTrainer" in str(w.message)]
    assert len(mine) == 1 and not tr.fused
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    ref = [_ref_step(twin, opt, *_batch(s0, a0, sn, ts, i, bs), 0.1) for i in range(5)]
    _ref_step(twin, opt, *_batch(s0, a0, sn, ts, 0, bs), 0.1)
    np.testing.assert_allclose(losses.cpu().numpy(), ref, rtol=1e-12)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 6)


# ----------------------------------------------------------------------------------------------------------------------
# Regressions: each of these failed before the trainer fixes that came with them.

def test_window_longer_than_16_falls_back_to_the_reference(nlc):
    """A B = 20 window (the kernels take 1..16) runs the grad-mode forward + clip_grad_norm_ + Adam with one warning,
    instead of raising: loss_and_grad, step and run equal the reference; and a sequence mixing B = 4 (fused) and B = 20
    (grad-mode) batches on one trainer keeps one Adam state -- parameters, moments and the step count equal a twin on
    torch.optim.Adam."""
    env, h, S, bs = "cartpole", 64, 17, 16
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, 6 * bs, 20))
    model, twin = _model(nlc, sd, env, h, S), _model(nlc, sd, env, h, S)
    b = _batch(s0, a0, sn, ts, 0, bs)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(model)
        assert tr.fused
        loss = tr.loss_and_grad(*b)
        grads = {k: p.grad.clone() for k, p in model.named_parameters()}
        tr.loss_and_grad(*b)
    assert len([w for w in rec if "NLTrainer" in str(w.message)]) == 1
    twin.zero_grad()
    ref = torch.nn.functional.mse_loss(twin(b[0], b[1], b[2]).squeeze(), b[3].squeeze())
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref))
    for k, p in twin.named_parameters():
        assert_grad_close(k, grads[k], p.grad, 1e-12)
    # step + run
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    refs = [_ref_step(twin, opt, *_batch(s0, a0, sn, ts, i, bs), 0.1) for i in range(4)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = [float(tr.step(*_batch(s0, a0, sn, ts, 0, bs)))]
        got += tr.run(s0[bs:], a0[bs:], sn[bs:], ts[bs:], torch.arange(3 * bs).cuda(), batch_size=bs).cpu().tolist()
    np.testing.assert_allclose(got, refs, rtol=1e-12)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 4)
    # mixed windows on one trainer
    model, twin = _model(nlc, sd, env, h, S), _model(nlc, sd, env, h, S)
    tr = nlc.NLTrainer(model, lr=1e-3)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, B in enumerate((4, 20, 4, 20, 4, 4)):
            s0b, a0b, tsb, bsd = _batch(s0, a0, sn, ts, i, bs)
            a0b = a0b[:, -B:].contiguous()
            ref = _ref_step(twin, opt, s0b, a0b, tsb, bsd, 0.1)
            loss = tr.step(s0b, a0b, tsb, bsd)
            assert abs(float(loss) - ref) <= 1e-12 * abs(ref), (i, B)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 6)


def test_refused_call_leaves_the_adam_step_count(nlc):
    """A call the library refuses on the host (N = 0: check_train, before any launch) leaves the step count alone, and the
    next step still equals torch.optim.Adam's (bias corrections of step 2, not 3)."""
    from neurallaplacecontrol_amd import _lib
    from neurallaplacecontrol_amd.training import _f64_ptr, _i64_ptr

    env, h, S, bs = "pendulum", 64, 17, 16
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, 2 * bs, 4))
    model, twin = _model(nlc, sd, env, h, S), _model(nlc, sd, env, h, S)
    tr = nlc.NLTrainer(model)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    b0, b1 = _batch(s0, a0, sn, ts, 0, bs), _batch(s0, a0, sn, ts, 1, bs)
    _ref_step(twin, opt, *b0, 0.1)
    tr.step(*b0)
    obs, win, tsd, tgt = tr._data(*b0)
    loss = torch.empty((), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.NlcError, match="N must be >= 1"):
        tr._launch_step(_i64_ptr(tr._idx(bs)), obs, win, tsd, tgt, 0, _f64_ptr(loss), tr._workspace(bs))
    assert tr._step == 1 and float(tr.state_dict()["state"][0]["step"]) == 1.0
    _ref_step(twin, opt, *b1, 0.1)
    tr.step(*b1)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 2)


def test_model_changes_after_construction_reach_the_kernels(nlc):
    """After NLTrainer(model): load a state dict with other state_std / action_std, set ilt_options and flip
    normalize_time.  loss_and_grad then equals the oracle with the NEW constants (the kernel takes them from the model
    descriptor, which must be re-uploaded), and a step trains on them too."""
    env, h, S, N = "cartpole", 64, 17, 40
    st = _stats(env)
    d = st["d"]
    sd = _sd(env, h, S)
    s0, a0, sn, ts = _data(env, N, 4)
    model = _model(nlc, sd, env, h, S)
    tr = nlc.NLTrainer(model)
    tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), (sn - s0).cuda())  # the old descriptor is in use
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["state_std"] = sd["state_std"] * torch.linspace(0.5, 2.0, d, dtype=torch.float64)
    sd2["action_std"] = torch.tensor([2.5], dtype=torch.float64)
    model.load_state_dict(sd2)
    ilt = {"alpha": 0.02, "tol": 1e-3}
    model.ilt_options = ilt
    model.normalize_time = False
    data = (s0, a0, ts, sn - s0)
    ref_loss, ref_grads = _oracle_loss_grads(sd2, data, S, True, False, ilt)
    loss = tr.loss_and_grad(*(t.cuda() for t in data))
    rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    assert rel <= 1e-12, f"loss rel err {rel:.3e}: the trainer kept the constants of construction time"
    for k, p in model.named_parameters():
        assert_grad_close(k, p.grad, ref_grads[k], 1e-9)
    # one step on the new constants == the grad-mode path + Adam on a twin carrying them
    twin = _model(nlc, sd2, env, h, S)
    twin.ilt_options, twin.normalize_time = ilt, False
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    b = tuple(t.cuda() for t in data)
    ref = _ref_step(twin, opt, *b, 0.1)
    assert abs(float(tr.step(*b)) - ref) <= 1e-12 * abs(ref)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 1)


@pytest.mark.parametrize("flag", ["amsgrad", "maximize"])
def test_load_state_dict_refuses_amsgrad_and_maximize(nlc, flag):
    """The trainer's update is plain Adam: an amsgrad or maximize Adam state is refused, not silently half-taken."""
    env, h, S, bs = "pendulum", 64, 17, 16
    sd = _sd(env, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(env, bs, 4))
    twin = _model(nlc, sd, env, h, S)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4, **{flag: True})
    _ref_step(twin, opt, *_batch(s0, a0, sn, ts, 0, bs), 0.1)
    tr = nlc.NLTrainer(_model(nlc, sd, env, h, S))
    with pytest.raises(ValueError, match=flag):
        tr.load_state_dict(opt.state_dict())
