"""GPU: the fused training step (NLTrainer / NLTrainerGroup, nlc_train_step) of fixed Talbot (`fixed_tablot`) and Stehfest
models -- the linear-ILT instance of train_fwd_bwd_kernel -- against autograd through the CPU oracle and against the
reference's training loop on the grad-mode path, with the bounds of tests/test_gpu_train.py (the Fourier suite)."""

import copy
import ctypes as C
import warnings

import pytest
import torch
from test_gpu_train import _batch, _close_to_scale, _data, _model, _ref_step, _roundoff_misses, _sd
from train_compare import assert_grad_close

pytestmark = pytest.mark.gpu

LINEAR = [("fixed_tablot", 17), ("stehfest", 8)]


def _trainer_warnings(rec):
    return [w for w in rec if "NLTrainer" in str(w.message)]


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("algo,S", LINEAR)
def test_linear_models_train_fused_without_a_warning(nlc, algo, S):
    """NLTrainer and NLTrainerGroup of fixed_tablot / stehfest models are fused, silently (before the linear instance they
    warned and trained on the grad-mode path)."""
    env, h = "cartpole", 64
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(_model(nlc, _sd(env, h, S), env, h, S, algo=algo))
        grp = nlc.NLTrainerGroup([_model(nlc, _sd(env, h, S, seed=s), env, h, S, algo=algo) for s in (4, 5)])
    assert tr.fused is True and grp.fused is True
    assert not _trainer_warnings(rec)


# ---------------------------------------------------------------------------------------------------------------- 2
# (env, h, algo, S, N, B, encode_obs_time)
LG_CASES = [
    ("cartpole", 64, "fixed_tablot", 8, 16, 4, False),  # O = 2 d S = 80, a multiple of 16
    ("cartpole", 128, "fixed_tablot", 17, 37, 4, False),  # ragged second tile
    ("acrobot", 64, "fixed_tablot", 33, 19, 3, False),
    ("pendulum", 256, "fixed_tablot", 11, 1, 1, False),
    ("pendulum", 64, "stehfest", 2, 16, 1, False),
    ("pendulum", 64, "stehfest", 8, 203, 16, True),
    ("cartpole", 128, "stehfest", 12, 16, 4, False),
    ("cartpole", 64, "stehfest", 16, 2100, 4, False),  # 132 tiles on 128 workgroups: some walk two
]


@pytest.mark.parametrize("env,h,algo,S,N,B,enc", LG_CASES, ids=[f"{c[0]}-h{c[1]}-{c[2]}{c[3]}-N{c[4]}-B{c[5]}" for c in LG_CASES])
def test_loss_and_grad_vs_oracle_autograd(nlc, env, h, algo, S, N, B, enc):
    """loss_and_grad against autograd through oracle.nl_model.nl_forward(..., ilt_algorithm=algo) on the CPU: the loss to 1e-12
    relative, every gradient block (tests/train_compare.py) to 1e-9 of its own scale."""
    from oracle import nl_model as onl

    sd = _sd(env, h, S, enc)
    s0, a0, sn, ts = _data(env, N, B, enc)
    target = sn - s0
    names = [k for k in sd if k.startswith(("action_encoder.", "laplace_rep_func."))]
    leaves = {k: (v.clone().requires_grad_() if k in names else v) for k, v in sd.items()}
    ref_loss = ((onl.nl_forward(leaves, s0, a0, ts, S=S, ilt_algorithm=algo) - target) ** 2).mean()
    ref_loss.backward()
    ref_loss = ref_loss.detach()
    model = _model(nlc, sd, env, h, S, enc, algo=algo)
    tr = nlc.NLTrainer(model)
    assert tr.fused
    loss = tr.loss_and_grad(*_cuda(s0, a0, ts, target))
    assert loss.dim() == 0 and loss.is_cuda
    rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    print(f"loss {float(loss):.6e} rel err {rel:.2e}")
    assert rel <= 1e-12, f"loss rel err {rel:.3e}"
    for k, p in model.named_parameters():
        assert_grad_close(k, p.grad, leaves[k].grad, 1e-9)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("algo,S", LINEAR)
def test_one_step_vs_clip_and_adam(nlc, algo, S):
    """step() == the twin's grad-mode forward + clip_grad_norm_ + torch.optim.Adam: parameters and both moments to 1e-12 of
    each tensor's magnitude."""
    env, h = "cartpole", 128
    sd = _sd(env, h, S)
    s0, a0, sn, ts = _cuda(*_data(env, 16, 4))
    bsd = sn - s0
    model, twin = _model(nlc, sd, env, h, S, algo=algo), _model(nlc, sd, env, h, S, algo=algo)
    tr = nlc.NLTrainer(model, lr=1e-4, clip_grad_norm=0.1)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    ref_loss = _ref_step(twin, opt, s0, a0, ts, bsd, 0.1)
    loss = tr.step(s0, a0, ts, bsd)
    assert tr.fused and abs(float(loss) - ref_loss) <= 1e-12 * abs(ref_loss)
    sd_tr, sd_ref = tr.state_dict(), opt.state_dict()
    named_twin = dict(twin.named_parameters())
    for i, (k, p) in enumerate(model.named_parameters()):
        _close_to_scale(p, named_twin[k], 1e-12, k)
        for key in ("exp_avg", "exp_avg_sq"):
            _close_to_scale(sd_tr["state"][i][key], sd_ref["state"][i][key], 1e-12, f"{k} {key}")
        assert float(sd_tr["state"][i]["step"]) == 1.0


@pytest.mark.parametrize("algo,S", LINEAR)
def test_run_50_iterations_vs_reference_loop(nlc, algo, S):
    """run() over 50 iterations at batch 7 == the reference loop on the grad-mode path: every loss to 1e-9 relative, final
    parameters to 1e-9 of max |p| (elements that miss must have a roundoff-sized gradient, as in the Fourier suite)."""
    env, h, bs, iters = "cartpole", 64, 7, 50
    sd = _sd(env, h, S)
    s0, a0, sn, ts = _cuda(*_data(env, bs * iters + 3, 4))
    perm = torch.randperm(s0.shape[0], generator=torch.Generator().manual_seed(5)).cuda()
    model, twin = _model(nlc, sd, env, h, S, algo=algo), _model(nlc, sd, env, h, S, algo=algo)
    tr = nlc.NLTrainer(model, lr=1e-4, clip_grad_norm=0.1)
    losses = tr.run(s0, a0, sn, ts, perm, batch_size=bs)
    assert tr.fused and losses.shape == (iters,) and losses.is_cuda
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    ref, grads = [], {k: [] for k, _ in twin.named_parameters()}
    for i in range(iters):
        ind = perm[i * bs : i * bs + bs]
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


@pytest.mark.parametrize("algo,S", LINEAR)
def test_train_step_gradnorm_equals_clip_grad_norm(nlc, algo, S):
    """nlc_train_step's gradnorm output equals clip_grad_norm_'s return on loss_and_grad's gradients to 1e-12 relative."""
    env, h, N, B = "pendulum", 128, 40, 4
    s0, a0, sn, ts = _cuda(*_data(env, N, B))
    model = _model(nlc, _sd(env, h, S), env, h, S, algo=algo)
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
    with ctx.stream():
        ctx.check(ctx.lib.nlc_train_step(ctx.h, C.byref(tr._desc()), p(flat), p(m), p(v), 1, p(obs), p(win), p(tsd), p(tgt),
                                         p(idx), N, B, p(loss), p(gnorm), p(ws)))
    got = float(gnorm)
    assert ref > 0 and abs(got - ref) <= 1e-12 * ref, f"gradnorm {got!r} vs clip_grad_norm_ {ref!r}"


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("algo,S", LINEAR)
def test_run_is_bit_reproducible(nlc, algo, S):
    env, h, bs = "acrobot", 64, 16
    sd = _sd(env, h, S)
    s0, a0, sn, ts = _cuda(*_data(env, 12 * bs, 4))
    perm = torch.randperm(s0.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
    out = []
    for _ in range(2):
        model = _model(nlc, sd, env, h, S, algo=algo)
        losses = nlc.NLTrainer(model).run(s0, a0, sn, ts, perm, batch_size=bs)
        out.append((losses.cpu(), [p.detach().cpu().clone() for p in model.parameters()]))
    assert torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_group_of_three_stehfest_members_equals_single_trainers(nlc):
    """M = 3 stehfest S = 8 members on stacked data, N = 37 (three tiles, the last ragged): losses, gradients, and after five
    steps the parameters and optimiser states are torch.equal to three single trainers on deep copies."""
    env, h, S, N = "cartpole", 64, 8, 37
    models = [_model(nlc, _sd(env, h, S, seed=s), env, h, S, algo="stehfest") for s in (1, 2, 3)]
    twins = [copy.deepcopy(m) for m in models]
    sets = [_cuda(*_data(env, N, 4, seed=20 + i)) for i in range(3)]
    batches = [(s0, a0, ts, sn - s0) for s0, a0, sn, ts in sets]
    stacked = tuple(torch.stack(ts) for ts in zip(*batches))
    grp = nlc.NLTrainerGroup(models)
    singles = [nlc.NLTrainer(t) for t in twins]
    assert grp.fused and all(s.fused for s in singles)
    loss = grp.loss_and_grad(*stacked)
    ref = torch.stack([s.loss_and_grad(*b) for s, b in zip(singles, batches)])
    assert loss.shape == (3,) and torch.equal(loss, ref)
    for i, (m, t) in enumerate(zip(models, twins)):
        for (k, p), q in zip(m.named_parameters(), t.parameters()):
            assert torch.equal(p.grad, q.grad), f"member {i} grad {k}"
    for _ in range(5):
        assert torch.equal(grp.step(*stacked), torch.stack([s.step(*b) for s, b in zip(singles, batches)]))
    for i, (m, t) in enumerate(zip(models, twins)):
        for (k, p), q in zip(m.named_parameters(), t.parameters()):
            assert torch.equal(p, q), f"member {i} {k}"
    for i, (sd, s) in enumerate(zip(grp.state_dict(), singles)):
        ref_sd = s.state_dict()
        for j in sd["state"]:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(sd["state"][j][key].cpu(), ref_sd["state"][j][key].cpu()), f"member {i} param {j} {key}"
    assert not torch.equal(loss[0], loss[1])


# ---------------------------------------------------------------------------------------------------------------- 6
def test_switching_the_algorithm_on_a_live_trainer(nlc):
    """model.ilt_algorithm fourier -> fixed_tablot -> fourier on one trainer: every stage is fused, and its loss, gradients
    and step are torch.equal to a fresh trainer's on a deep copy that took over the optimiser state.  Then dehoog: one
    warning, the grad-mode path (== the twin's reference step to 1e-12) on the shared Adam state, and back to fused."""
    from oracle import nl_model as onl
    from test_gpu_train import _stats

    env, h, S, bs = "cartpole", 64, 9, 16
    st = _stats(env)
    sd = onl.make_synthetic_state_dict(3, st["d"], st["nu"], h, S, st["state_std"], [st["act_high"] / 2], tame="dehoog")
    s0, a0, sn, ts = _cuda(*_data(env, 8 * bs, 4))
    model = _model(nlc, sd, env, h, S)
    stage_losses = None
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(model)
        for i, algo in enumerate(("fourier", "fixed_tablot", "fourier")):
            model.ilt_algorithm = algo
            twin = copy.deepcopy(model)
            fresh = nlc.NLTrainer(twin)
            fresh.load_state_dict(tr.state_dict())
            b = _batch(s0, a0, sn, ts, i, bs)
            la, lb = tr.loss_and_grad(*b), fresh.loss_and_grad(*b)
            assert tr.fused and fresh.fused and torch.equal(la, lb), algo
            for (k, p), q in zip(model.named_parameters(), twin.parameters()):
                assert torch.equal(p.grad, q.grad), f"{algo} grad {k}"
            if algo == "fixed_tablot":  # the same weights under the algorithm the trainer was built with give another loss
                other = copy.deepcopy(model)
                other.ilt_algorithm = "fourier"
                stage_losses = (float(la), float(nlc.NLTrainer(other).loss_and_grad(*b)))
            assert torch.equal(tr.step(*b), fresh.step(*b)), algo
            for (k, p), q in zip(model.named_parameters(), twin.parameters()):
                assert torch.equal(p, q), f"{algo} {k}"
    assert not _trainer_warnings(rec)
    # the switch reached the kernels: a descriptor left at fourier would have given the other loss
    assert abs(stage_losses[1] - stage_losses[0]) > 1e-3 * abs(stage_losses[0]), stage_losses
    assert float(tr.state_dict()["state"][0]["step"]) == 3.0
    # dehoog: per-call grad-mode fallback on the trainer's own Adam state
    model.ilt_algorithm = "dehoog"
    twin = copy.deepcopy(model)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    opt.load_state_dict(tr.state_dict())
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = [float(tr.step(*_batch(s0, a0, sn, ts, i, bs))) for i in (3, 4)]
    ref = [_ref_step(twin, opt, *_batch(s0, a0, sn, ts, i, bs), 0.1) for i in (3, 4)]
    assert len(_trainer_warnings(rec)) == 1
    assert all(abs(g - r) <= 1e-12 * abs(r) for g, r in zip(got, ref)), (got, ref)
    assert float(tr.state_dict()["state"][0]["step"]) == 5.0
    named_twin = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        _close_to_scale(p, named_twin[k], 1e-12, k)
    # and back
    model.ilt_algorithm = "fixed_tablot"
    twin = copy.deepcopy(model)
    fresh = nlc.NLTrainer(twin)
    fresh.load_state_dict(tr.state_dict())
    b = _batch(s0, a0, sn, ts, 5, bs)
    assert torch.equal(tr.step(*b), fresh.step(*b)) and tr.fused
    assert float(tr.state_dict()["state"][0]["step"]) == 6.0


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals_reach_no_launch(nlc):
    """A stehfest model at odd S through the C ABI.  nlc_set_model is the only way a descriptor reaches a ctx, and it refuses
    this one with NLC_ERR_UNSUPPORTED (check_ilt) -- so nlc_train_step on that ctx has no model to refuse and answers
    NLC_ERR_STATE; check_train repeats the table check for a descriptor that got past it.  Either way nothing is launched:
    the ctx's profile counts no training kernel and the output buffers keep their bits.  At the Python level the trainer is
    not fused, with one warning."""
    from neurallaplacecontrol_amd import _lib

    env, h, S, N, B = "pendulum", 64, 7, 16, 4
    model = _model(nlc, _sd(env, h, S), env, h, S, algo="stehfest")
    ctx = _lib.Ctx(0)
    ctx.profile(True)
    with pytest.raises(_lib.NlcError) as err:
        model.upload(ctx)
    assert err.value.code == _lib.NLC_ERR_UNSUPPORTED
    s0, a0, sn, ts = _cuda(*_data(env, N, B))
    P = sum(p.numel() for p in model.parameters())
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).contiguous()
    before = flat.clone()
    m, v = torch.zeros(P, dtype=torch.float64, device="cuda"), torch.zeros(P, dtype=torch.float64, device="cuda")
    loss = torch.full((), 123.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.float64, device="cuda")
    idx = torch.arange(N, dtype=torch.int64, device="cuda")
    desc = _lib.TrainDesc(1e-4, 0.9, 0.999, 1e-8, 0.0, 0.1)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with ctx.stream():
        rc = ctx.lib.nlc_train_step(ctx.h, C.byref(desc), p(flat), p(m), p(v), 1, p(s0), p(a0.contiguous()),
                                    p(ts.reshape(-1).contiguous()), p((sn - s0).contiguous()), p(idx), N, B, p(loss), None, p(ws))
    torch.cuda.synchronize()
    assert rc == -5, rc  # NLC_ERR_STATE (include/nlc.h)
    assert not any(k.startswith("train_") for k in ctx.profile_read())
    assert torch.equal(flat, before) and float(loss) == 123.0 and not bool(m.any()) and not bool(v.any())
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(model)
    assert not tr.fused and len(_trainer_warnings(rec)) == 1 and "stehfest" in str(_trainer_warnings(rec)[0].message)


def test_scale_rule_is_fouriers_alone(nlc):
    """A Fourier model at ILT scale 1 is still refused (one warning, not fused); a fixed_tablot model carries its default
    scale 1 and is accepted -- the scale == 2 requirement is the Fourier series' quarter turns."""
    env, h, S = "pendulum", 64, 8
    fourier = _model(nlc, _sd(env, h, S), env, h, S)
    fourier.ilt_options = {"scale": 1.0}
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(fourier)
    assert not tr.fused and len(_trainer_warnings(rec)) == 1 and "scale" in str(_trainer_warnings(rec)[0].message)
    talbot = _model(nlc, _sd(env, h, S), env, h, S, algo="fixed_tablot")
    assert talbot.model_desc().ilt.scale == 1.0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(talbot)
        s0, a0, sn, ts = _cuda(*_data(env, 16, 4))
        loss = tr.loss_and_grad(s0, a0, ts, sn - s0)
    assert tr.fused and not _trainer_warnings(rec) and bool(torch.isfinite(loss))
