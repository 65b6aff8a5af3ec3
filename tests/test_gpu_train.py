"""GPU: the fused training step (NLTrainer / nlc_train_step) against autograd through the CPU oracle and against the
reference's training loop on the existing grad-mode path (train_utils.py:388-408)."""

import copy
import warnings

import numpy as np
import pytest
import torch

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
    """loss_and_grad: the loss to 1e-12 relative and every parameter gradient to 1e-9 of that tensor's max |grad|, against
    autograd through oracle.nl_model.nl_forward + ((pred - target)^2).mean() on the CPU."""
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
        _close_to_scale(p.grad, leaves[k].grad, 1e-9, k)


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
