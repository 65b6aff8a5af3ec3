"""GPU: the NODE baseline under the midpoint and rk4 (3/8 rule) fixed-grid solvers -- forward, planner, fused training step,
held-out loss, groups, and a switch of ``model.method`` on live objects -- against the CPU restatement of
tests/node_rk_reference.py (oracle.node_model.ode_func + euler_substeps + the three steps in their stated evaluation order;
torchdiffeq is absent offline: parity unpinned vs upstream).

Tolerances are the project's: forward 1e-9 (test_node_forward_vs_oracle_sizes), planner rtol = atol = 1e-8
(test_mppi_node_dynamics_vs_reference_golden), training loss 1e-12 relative, every gradient block 1e-9 of its own scale floored
at 1e-6 of the tensor's, step() 1e-12, run() 1e-9 over 20 iterations, gradnorm 1e-12, evaluate 1e-12."""

import copy
import ctypes as C

import numpy as np
import pytest
import torch

import node_rk_reference as rk
import test_gpu_train_node as tn
from gpu_common import GOLD, TOL, _batched_vs_singles, _Replay, _state, build_node, load_sd

pytestmark = pytest.mark.gpu

NEW = ("midpoint", "rk4")
P = tn.P
DT = 0.05
DIV = float(torch.tensor(DT, dtype=torch.float32).double() * 8.0)  # the model's time normaliser (a float32 dt widened)


def _node(nlc, sd, H, aug, method, normalize=True, normalize_time=True):
    m = build_node(nlc, sd, H, aug, normalize, normalize_time)
    m.method = method
    return m


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward
# without normalize_time: 1, 3 and 8 sub-steps; 0.15 and 0.4 end exactly on a grid point (8 is the hsub cap)
FWD_TIMES = ((0.03, 1), (0.15, 3), (0.4, 8))
FWD_SHAPES = [(16, (5, 1, 1), 1), (17, (2, 1, 2), 17), (270, (1, 0, 1), 70), (270, (5, 1, 1), 17), (16, (2, 1, 2), 70),
              (17, (1, 0, 1), 1)]


@pytest.mark.parametrize("method", NEW)
@pytest.mark.parametrize("H,dims,N", FWD_SHAPES, ids=[f"H{h}_d{d[0]}a{d[1]}u{d[2]}_N{n}" for h, d, n in FWD_SHAPES])
def test_forward_vs_reference(nlc, method, H, dims, N):
    from oracle import node_model as on

    d, aug, nu = dims
    sd = on.make_synthetic_state_dict(13 + H, d, nu, H, aug, np.linspace(0.7, 2.9, d), [2.5])
    g = torch.Generator().manual_seed(N + H)
    obs = torch.randn(N, d, dtype=torch.float64, generator=g) * 2
    win = (torch.rand(N, 3, nu, dtype=torch.float64, generator=g) * 2 - 1) * 5
    model = _node(nlc, sd, H, aug, method, normalize_time=False)
    for t, nsub in FWD_TIMES:
        assert len(on.euler_substeps(t)) == nsub
        ts = torch.full((N, 1), t, dtype=torch.float64)
        ref = rk.forward(sd, obs, win, ts, method, normalize_time=False)
        with torch.no_grad():
            got = model(obs.cuda(), win.cuda(), ts.cuda()).cpu()
        np.testing.assert_allclose(got.numpy(), ref.numpy(), **TOL)
    # the methods differ by far more than the tolerance: the test tells them apart
    ts = torch.full((N, 1), 0.4, dtype=torch.float64)
    other = rk.forward(sd, obs, win, ts, "euler", normalize_time=False)
    assert float((other - ref).abs().max()) > 1e-6


@pytest.mark.parametrize("H,dims", [(16, (5, 1, 1)), (270, (2, 1, 2))])
def test_constant_slope_all_methods_agree(nlc, H, dims):
    """With 4.weight = 0 the ODE function is the constant 4.bias: every consistent method gives x + t_end * bias, to 1e-13."""
    from oracle import node_model as on

    d, aug, nu = dims
    sd = on.make_synthetic_state_dict(3, d, nu, H, aug, np.linspace(0.7, 2.9, d), [2.5], out_scale=1.0)
    sd[P + "4.weight"] = torch.zeros_like(sd[P + "4.weight"])
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(17, d, dtype=torch.float64, generator=g) * 2
    win = torch.randn(17, 1, nu, dtype=torch.float64, generator=g)
    for t, _ in FWD_TIMES:
        want = obs / sd["state_std"] + t * sd[P + "4.bias"][:d]
        for method in rk.METHODS:
            with torch.no_grad():
                got = _node(nlc, sd, H, aug, method, normalize_time=False)(obs.cuda(), win.cuda(), torch.full((17, 1), t, dtype=torch.float64).cuda()).cpu()
            assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), (method, t)


# ---------------------------------------------------------------------------------------------------------------------
# 2. planner
@pytest.mark.parametrize("method", NEW)
@pytest.mark.parametrize("env", ["cartpole", "pendulum", "acrobot"])
def test_mppi_vs_oracle_mppi_over_three_commands(nlc, env, method):
    """K = 64, T = 8 at the golden file's model: three consecutive commands against oracle.mppi.mppi_command over the CPU
    restatement of the method."""
    from oracle import envs as oenvs
    from oracle import mppi as omppi

    g = np.load(f"{GOLD}/g11_node_{env}.npz")
    sd = load_sd(g, "sd_")
    model = _node(nlc, sd, int(g["H"]), int(g["AUG"]), method)
    K, T, d, nu, A = int(g["K"]), int(g["T"]), int(g["nx"]), int(g["nu"]), float(g["A"])
    assert (K, T) == (64, 8)
    gen = torch.Generator().manual_seed(31)
    raws = [torch.randn(K, T, nu, dtype=torch.float64, generator=gen) for _ in range(3)]
    U0 = torch.randn(T, nu, dtype=torch.float64, generator=gen) * 0.3
    dyn = rk.make_dynamics(sd, method)
    with torch.no_grad():
        p = nlc.MPPIDelay(nlc.NLDynamics(model, 0.05), nlc.EnvCost("oderl-" + env), d, nlc.noise_sigma(nu), num_samples=K,
                          horizon=T, device="cpu", lambda_=1.0, u_min=torch.tensor(-A), u_max=torch.tensor(A), u_scale=A,
                          U_init=U0.clone())
        p.noise_dist = _Replay(*[r.clone() for r in raws])
        U = U0.clone()
        for i in range(3):
            state = _state(nlc, "oderl-" + env, 40 + i)
            ab = (torch.rand(4, nu, dtype=torch.float64, generator=gen) - 0.5) * A
            act = p.command(state, ab)
            ref = omppi.mppi_command(U, state, ab, raws[i], dyn, oenvs.RUNNING_COST["oderl-" + env], d,
                                     torch.inverse(nlc.noise_sigma(nu)), 1.0, A, torch.tensor(-A), torch.tensor(A))
            np.testing.assert_allclose(act.numpy(), ref["action"].numpy(), rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(p.cost_total.numpy(), ref["cost_total"].numpy(), rtol=1e-8, atol=1e-8)
            U = ref["U"].clone()


@pytest.mark.parametrize("method", NEW)
def test_batched_planner_equals_single_planners(nlc, method):
    from oracle import nl_model as onl
    from oracle import node_model as on

    env, d, nu, A = "oderl-acrobot", 6, 2, 5.0
    st = onl.ENV_STATS[env]
    model = _node(nlc, on.make_synthetic_state_dict(3, d, nu, 100, 1, st["state_std"], [A / 2]), 100, 1, method)
    _batched_vs_singles(nlc, lambda: nlc.NLDynamics(model, 0.05), env, E=3, K=100, T=6, n_cmd=2)


# ---------------------------------------------------------------------------------------------------------------------
# 3. training against float64 autograd through the restatement
def _ref_loss_grads(sd, s0, a0, ts, target, method, row_times):
    leaves = {k: (v.clone().requires_grad_() if k in tn.PARAMS else v) for k, v in sd.items()}
    loss = ((rk.forward_rows(leaves, s0, a0, ts, method, row_times=row_times) - target) ** 2).mean()
    loss.backward()
    return loss.detach(), {k: leaves[k].grad for k in tn.PARAMS}


def _ref_loss(sd, s0, a0, ts, target, method, row_times):
    with torch.no_grad():
        return float(((rk.forward_rows(sd, s0, a0, ts, method, row_times=row_times) - target) ** 2).mean())


# (H, N, times): "mixed" = rows of 3, 1 and 40 sub-steps in one tile
LG_CASES = [(270, 1, "fixed"), (17, 16, "mixed"), (270, 17, "mixed"), (17, 37, "mixed")]


@pytest.mark.parametrize("method", NEW)
@pytest.mark.parametrize("row_times", [False, True], ids=["first", "row"])
@pytest.mark.parametrize("H,N,times", LG_CASES, ids=[f"H{c[0]}_N{c[1]}_{c[2]}" for c in LG_CASES])
def test_loss_and_grad_vs_reference_autograd(nlc, method, row_times, H, N, times):
    d, aug, nu = (5, 1, 1) if H == 270 else (2, 1, 2)
    sd, (s0, a0, sn, ts) = tn._setup(H, d, aug, nu, N, mean=True, times=times, seed=7 * d + H)
    target = sn - s0
    ref_loss, ref_grads = _ref_loss_grads(sd, s0, a0, ts, target, method, row_times)
    model = _node(nlc, sd, H, aug, method)
    tr = nlc.NODETrainer(model, row_times=row_times)
    assert tr.fused
    loss = tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), target.cuda())
    rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    print(f"{method}: loss rel err {rel:.3e}")
    assert rel <= 1e-12, f"loss rel err {rel:.3e}"
    worst = max(tn._assert_grad_close(k, p.grad, ref_grads[k], d, aug) for k, p in model.named_parameters())
    print(f"{method}: worst gradient block ratio {worst:.3e}")
    # and not Euler's numbers
    eul, _ = tn._oracle_loss_grads(sd, s0, a0, ts, target, True, True, row_times)
    assert abs(float(eul) - float(ref_loss)) > 1e-9 * abs(float(ref_loss))


@pytest.mark.parametrize("method", NEW)
def test_rows_at_and_past_the_cap(nlc, method):
    """row_times: a row of exactly the method's cap (256 / s sub-steps) trains to the bounds; a member whose batch holds a row
    one sub-step past it gets a NaN loss on the device, and the other member's loss and gradients are bit for bit those of a
    trainer of its own.  The trainer's host check refuses that ts before any launch; the group here is given it unchecked."""
    from oracle import node_model as on

    cap = 256 // rk.STAGES[method]
    t_cap, t_past = cap * 0.05 * DIV, (cap + 0.5) * 0.05 * DIV
    assert len(on.euler_substeps(t_cap / DIV)) == cap and len(on.euler_substeps(t_past / DIV)) == cap + 1
    H, d, aug, nu, N = 17, 2, 1, 2, 3
    # a contractive model: 12.8 / 6.4 / 3.2 time units of an expansive one would leave the float64 range of the bounds
    sd, (s0, a0, sn, _) = tn._setup(H, d, aug, nu, N, mean=True, seed=9, out_scale=0.05)
    target = sn - s0
    ts_ok = torch.tensor([[t_cap], [tn.T3], [tn.T1]], dtype=torch.float64)
    ts_bad = torch.tensor([[tn.T3], [t_past], [tn.T1]], dtype=torch.float64)
    ref_loss, ref_grads = _ref_loss_grads(sd, s0, a0, ts_ok, target, method, True)
    single = nlc.NODETrainer(_node(nlc, sd, H, aug, method), row_times=True)
    assert single.max_substeps() == cap
    loss = single.loss_and_grad(s0.cuda(), a0.cuda(), ts_ok.cuda(), target.cuda())
    assert abs(float(loss) - float(ref_loss)) <= 1e-12 * abs(float(ref_loss))
    for k, p in single.model.named_parameters():
        tn._assert_grad_close(k, p.grad, ref_grads[k], d, aug)
    with pytest.raises(ValueError, match="sub-steps"):
        single.loss_and_grad(s0.cuda(), a0.cuda(), ts_bad.cuda(), target.cuda())
    grp = nlc.NODETrainerGroup([_node(nlc, sd, H, aug, method) for _ in range(2)], row_times=True)
    grp._check_ts = lambda ts: None  # the library's own contract is under test
    st = lambda t: torch.stack([t, t]).cuda()  # noqa: E731
    gl = grp.loss_and_grad(st(s0), st(a0), torch.stack([ts_ok, ts_bad]).cuda(), st(target))
    assert torch.equal(gl[0], loss) and bool(torch.isnan(gl[1]))
    for p, q in zip(grp.models[0].parameters(), single.model.parameters()):
        assert torch.equal(p.grad, q.grad)
    ge = grp.evaluate(st(s0), st(a0), torch.stack([ts_ok, ts_bad]).cuda(), st(target))
    assert bool(torch.isnan(ge[1])) and abs(float(ge[0]) - float(ref_loss)) <= 1e-12 * abs(float(ref_loss))


def _pair(nlc, method, **kw):
    model, twin, data, sd = tn._pair(nlc, **kw)
    model.method = twin.method = method
    return model, twin, data, sd


@pytest.mark.parametrize("method", NEW)
@pytest.mark.parametrize("clip,wd,N", [(0.1, 0.0, 1), (0.1, 1e-2, 16)])
def test_one_step_vs_clip_and_adam(nlc, method, clip, wd, N):
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, method, N=N)
    kw = dict(lr=1e-4, weight_decay=wd)
    tr = nlc.NODETrainer(model, clip_grad_norm=clip, **kw)
    assert tr.fused
    opt = torch.optim.Adam(twin.parameters(), **kw)
    ref_loss, _ = tn._ref_step(twin, opt, s0, a0, ts, sn - s0, clip)
    loss = tr.step(s0, a0, ts, sn - s0)
    assert abs(float(loss) - ref_loss) <= 1e-12 * abs(ref_loss)
    tn._assert_adam_state_equal(model, twin, tr, opt, 1e-12, 1)


@pytest.mark.parametrize("method", NEW)
@pytest.mark.parametrize("bs", [1, 7])
def test_run_follows_the_reference_loop(nlc, method, bs):
    iters = 20
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, method, H=33, N=64, times="random")
    perm = torch.randint(0, 64, (iters * bs,), generator=torch.Generator().manual_seed(1)).cuda()
    tr = nlc.NODETrainer(model, lr=1e-3)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    ref = []
    for i in range(iters):
        ind = perm[i * bs : (i + 1) * bs]
        ref.append(tn._ref_step(twin, opt, s0[ind], a0[ind], ts[ind], sn[ind] - s0[ind], 0.1)[0])
    losses = tr.run(s0, a0, sn, ts, perm, bs)
    tn._close_to_scale(losses, torch.tensor(ref, dtype=torch.float64), 1e-9, "run losses")
    for (k, p), q in zip(model.named_parameters(), twin.parameters()):
        tn._close_to_scale(p, q, 1e-9, k)


@pytest.mark.parametrize("method", NEW)
def test_gradnorm_equals_clip_grad_norm(nlc, method):
    from neurallaplacecontrol_amd.training import _f64_ptr, _i64_ptr

    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, method)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    _, total = tn._ref_step(twin, opt, s0, a0, ts, sn - s0, 0.1)
    assert total > 0.1
    tr = nlc.NODETrainer(model)
    N = s0.shape[0]
    tr._gather()
    loss, gn = torch.empty(1, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
    tgt, tsf = (sn - s0).contiguous(), ts.reshape(-1).contiguous()
    ctx = tr._ctx
    with ctx.stream():
        ctx.check(ctx.lib.nlc_node_train_group_step(
            ctx.h, C.byref(tr._desc()), 1, 0, _f64_ptr(tr._flat), _f64_ptr(tr._m), _f64_ptr(tr._v), 1, _f64_ptr(s0),
            _f64_ptr(a0), _f64_ptr(tsf), _f64_ptr(tgt), _i64_ptr(tr._idx(N)), N, a0.shape[1], _f64_ptr(loss), _f64_ptr(gn),
            _f64_ptr(tr._workspace(N)), 0))
    assert abs(float(gn) - total) <= 1e-12 * total


@pytest.mark.parametrize("method", NEW)
@pytest.mark.parametrize("row_times", [False, True])
def test_evaluate_vs_reference_and_loss_and_grad(nlc, method, row_times):
    H, d, aug, nu, N = 270, 5, 1, 1, 70
    sd, (s0, a0, sn, ts) = tn._setup(H, d, aug, nu, N, mean=True, times="mixed", seed=11)
    target = sn - s0
    tr = nlc.NODETrainer(_node(nlc, sd, H, aug, method), row_times=row_times)
    dev = tuple(t.cuda() for t in (s0, a0, ts, target))
    loss = tr.evaluate(*dev)
    ref = _ref_loss(sd, s0, a0, ts, target, method, row_times)
    assert abs(float(loss) - ref) <= 1e-12 * abs(ref)
    lg = tr.loss_and_grad(*dev)
    assert abs(float(loss) - float(lg)) <= 4e-16 * abs(float(lg)) * N  # the same sums in another tile order
    ind = torch.tensor([5, 3, 3, 69, 17, 0, 64], dtype=torch.int64)
    sub = tr.evaluate(*dev, indices=ind.cuda())
    ref = _ref_loss(sd, s0[ind], a0[ind], ts[ind], target[ind], method, row_times)
    assert abs(float(sub) - ref) <= 1e-12 * abs(ref)


# ---------------------------------------------------------------------------------------------------------------------
# 4. groups
def _tiny(nlc, n, method, **kw):
    models, data = tn._tiny(nlc, n, **kw)
    for m in models:
        m.method = method
    return models, data


@pytest.mark.parametrize("method", NEW)
@pytest.mark.parametrize("M", [2, 5])
def test_group_equals_single_trainers(nlc, method, M):
    N = 37
    models, (s0, a0, sn, ts) = _tiny(nlc, M, method, N=N, times="mixed")
    singles = [nlc.NODETrainer(copy.deepcopy(m), row_times=True) for m in models]
    grp = nlc.NODETrainerGroup(models, row_times=True)
    assert grp.fused
    data = (s0, a0, ts, sn - s0)
    gl = grp.loss_and_grad(*data)
    for i, tr in enumerate(singles):
        assert torch.equal(gl[i], tr.loss_and_grad(*data))
        for p, q in zip(grp.models[i].parameters(), tr.model.parameters()):
            assert torch.equal(p.grad, q.grad)
    for _ in range(2):
        gl = grp.step(*data)
        for i, tr in enumerate(singles):
            assert torch.equal(gl[i], tr.step(*data))
    for i, tr in enumerate(singles):
        for p, q in zip(grp.models[i].parameters(), tr.model.parameters()):
            assert torch.equal(p, q)
    ge = grp.evaluate(*data)
    for i, tr in enumerate(singles):
        assert torch.equal(ge[i], tr.evaluate(*data))


@pytest.mark.parametrize("method", NEW)
def test_run_is_bit_reproducible(nlc, method):
    outs = []
    for _ in range(2):
        model, _, (s0, a0, sn, ts), _ = _pair(nlc, method, H=33, N=64, times="mixed")
        tr = nlc.NODETrainer(model, row_times=True)
        losses = tr.run(s0, a0, sn, ts, torch.arange(64).cuda(), 16)
        outs.append((losses.clone(), [p.detach().clone() for p in model.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    for p, q in zip(outs[0][1], outs[1][1]):
        assert torch.equal(p, q)


def test_group_refuses_members_of_different_methods(nlc):
    models, data = _tiny(nlc, 2, "rk4")
    models[1].method = "midpoint"
    with pytest.raises(ValueError, match="member 1.*method"):
        nlc.NODETrainerGroup(models)
    models[1].method = "rk4"
    grp = nlc.NODETrainerGroup(models)
    models[1].method = "euler"  # and at a later call
    s0, a0, sn, ts = data
    with pytest.raises(ValueError, match="member 1.*method"):
        grp.step(s0, a0, ts, sn - s0)


def test_fit_keep_best_and_freeze_come_through_the_base(nlc):
    """fit with a validation set and patience on an rk4 group: runs, returns its criterion history, restores the best."""
    models, (s0, a0, sn, ts) = _tiny(nlc, 2, "rk4", N=96)
    grp = nlc.NODETrainerGroup(models, lr=[1e-2, 1e-3])
    val = (s0[:32], a0[:32], ts[:32], (sn - s0)[:32])
    out = grp.fit((s0[32:], a0[32:], sn[32:], ts[32:]), val, epochs=1, batch_size=4, eval_every=4, seed=3, patience=2)
    assert bool(torch.isfinite(out["best_loss"]).all())
    assert torch.equal(grp.evaluate(*val), out["best_loss"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. switching model.method on live objects
def test_switching_the_method_on_a_live_trainer_equals_fresh_trainers(nlc):
    (m,), (s0, a0, sn, ts) = _tiny(nlc, 1, "euler", times="mixed")
    w0 = copy.deepcopy(m.state_dict())
    tr = nlc.NODETrainer(m, row_times=True)
    for method in ("euler", "rk4", "euler"):
        m.method = method
        loss = tr.loss_and_grad(s0, a0, ts, sn - s0)
        ev = tr.evaluate(s0, a0, ts, sn - s0)
        (f,), _ = _tiny(nlc, 1, method, times="mixed")
        f.load_state_dict(w0)
        fresh = nlc.NODETrainer(f, row_times=True)
        assert torch.equal(loss, fresh.loss_and_grad(s0, a0, ts, sn - s0)), method
        assert torch.equal(ev, fresh.evaluate(s0, a0, ts, sn - s0)), method
        for p, q in zip(m.parameters(), f.parameters()):
            assert torch.equal(p.grad, q.grad), method
    # the cap follows the method: a time of 100 sub-steps is fine for euler and refused for rk4
    t100 = torch.full_like(ts, 100 * 0.05 * DIV - 1e-6)
    tr.evaluate(s0, a0, t100, sn - s0)
    m.method = "rk4"
    with pytest.raises(ValueError, match="64 rk4 sub-steps"):
        tr.evaluate(s0, a0, t100, sn - s0)


def test_switching_the_method_on_a_live_planner_and_model_equals_fresh_ones(nlc):
    from oracle import nl_model as onl
    from oracle import node_model as on

    env, d, nu, A, K, T = "oderl-cartpole", 5, 1, 3.0, 64, 8
    sd = on.make_synthetic_state_dict(4, d, nu, 64, 1, onl.ENV_STATS[env]["state_std"], [A / 2])
    gen = torch.Generator().manual_seed(8)
    raws = [torch.randn(K, T, nu, dtype=torch.float64, generator=gen) for _ in range(3)]
    U0 = torch.randn(T, nu, dtype=torch.float64, generator=gen) * 0.3
    obs = torch.randn(17, d, dtype=torch.float64, generator=gen)
    win = torch.randn(17, 2, nu, dtype=torch.float64, generator=gen)
    ts = torch.full((17, 1), 0.05, dtype=torch.float64)

    def planner(model, U, draws):
        p = nlc.MPPIDelay(nlc.NLDynamics(model, 0.05), nlc.EnvCost(env), d, nlc.noise_sigma(nu), num_samples=K, horizon=T,
                          device="cpu", lambda_=1.0, u_min=torch.tensor(-A), u_max=torch.tensor(A), u_scale=A, U_init=U)
        p.noise_dist = _Replay(*draws)
        return p

    live = build_node(nlc, sd, 64, 1)
    with torch.no_grad():
        p = planner(live, U0.clone(), [r.clone() for r in raws])
        outs = {}
        for i, method in enumerate(("euler", "rk4", "euler")):
            live.method = method
            U_before = p.U.clone()
            state, ab = _state(nlc, env, 60 + i), (torch.rand(4, nu, dtype=torch.float64, generator=gen) - 0.5) * A
            act = p.command(state, ab)
            fwd = live(obs.cuda(), win.cuda(), ts.cuda())
            fresh = _node(nlc, sd, 64, 1, method)
            q = planner(fresh, U_before, [raws[i].clone()])
            assert torch.equal(act, q.command(state, ab)), method
            assert torch.equal(p.cost_total, q.cost_total), method
            assert torch.equal(fwd, fresh(obs.cuda(), win.cuda(), ts.cuda())), method
            outs[i] = fwd
        assert not torch.equal(outs[0], outs[1])


def test_the_option_refuses_other_values_before_any_launch(nlc):
    from neurallaplacecontrol_amd import _lib

    ctx = _lib.Ctx(0)
    for v in (3, -1, 0.5):
        assert ctx.lib.nlc_set_option(ctx.h, b"node_method", float(v)) == -1  # NLC_ERR_BAD_ARG
    for v in (0, 1, 2, 0):
        assert ctx.lib.nlc_set_option(ctx.h, b"node_method", float(v)) == 0
