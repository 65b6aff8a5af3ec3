"""GPU: the opt-in fused training step of de Hoog NL models (``NLTrainer(model, dehoog="fused")``, ctx option
``train_dehoog``; csrc/kernels_train_dehoog.hip around the de Hoog ILT kernels) against float64 autograd through the CPU
oracle, against the existing grad-mode path, and against itself bit for bit (groups, reruns, live switching).

Models are ``make_synthetic_state_dict(..., tame="dehoog")``: the quotient-difference table is ill-conditioned on random
Laplace terms.  Conditioning is a precondition of every comparison with the CPU reference, checked on all rows: the oracle's
in-place and functional de Hoog forwards agree to 1e-9 (1 + |ref|).

Bounds: the project's 1e-12 relative on the loss and 1e-9 of the block scale on gradients.  A case that misses them is held
to ``train_compare``'s condition-aware bound instead -- ``sens`` = the CPU reference's own response to a relative 1e-15
perturbation of its parameters, factor 200 -- and must then also show that the existing GPU grad-mode path (the model's
``_forward_train`` + ``backward``) is no closer to the reference than a tenth of the fused error."""

import copy
import functools
import warnings

import numpy as np
import pytest
import torch
from gpu_common import dehoog_line_integrate_functional
from train_compare import assert_grad_close, blockwise_errors

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- setup
def _sd(d, h, S, seed=3):
    from oracle import nl_model as onl

    return onl.make_synthetic_state_dict(seed, d, 1, h, S, [1.0] * d, [1.0], tame="dehoog")


def _model(nlc, sd, d, h, S, algo="dehoog", normalize_time=True):
    m = nlc.NeuralLaplaceModel(
        d, 1, d, hidden_units=h, s_recon_terms=S, ilt_algorithm=algo, state_mean=np.zeros(d), state_std=np.ones(d),
        action_mean=np.array([0.0]), action_std=np.array([1.0]), normalize=True, normalize_time=normalize_time).double()
    m.load_state_dict(sd)
    return m.to("cuda")


def _data(d, N, B, seed=17, normalize_time=True):
    """s0 (N, d), a0 (N, B, 1), sn (N, d), ts (N, 1).  Times: 0.1 .. 0.15 as the model uses them without normalize_time
    (around the 0.125 the tamed weights sample their transform at); with it ts = 5e-3 .. 7.5e-3, which the model divides
    by 8 dt = 0.4."""
    g = torch.Generator().manual_seed(seed)
    s0 = torch.randn(N, d, dtype=torch.float64, generator=g)
    a0 = torch.rand(N, B, 1, dtype=torch.float64, generator=g) * 2 - 1
    sn = s0 + torch.randn(N, d, dtype=torch.float64, generator=g) * 0.05
    tn = torch.rand(N, 1, dtype=torch.float64, generator=g) * 0.05 + 0.1
    return s0, a0, sn, tn * (0.05 if normalize_time else 1.0)


def _oracle(sd, data, S, normalize_time, functional, scale=None):
    """Loss and parameter gradients by float64 autograd on the CPU (functional de Hoog), or the in-place oracle's predictions."""
    from oracle import ilt as oilt
    from oracle import nl_model as onl

    s0, a0, sn, ts = data
    if not functional:
        with torch.no_grad():
            return onl.nl_forward(sd, s0, a0, ts, S=S, ilt_algorithm="dehoog", normalize_time=normalize_time).reshape(s0.shape)
    names = [k for k in sd if k.startswith(("action_encoder.", "laplace_rep_func."))]
    leaves = {k: ((v * scale if scale is not None else v.clone()).requires_grad_() if k in names else v) for k, v in sd.items()}
    saved = oilt.LINE_INTEGRATE["dehoog"]
    oilt.LINE_INTEGRATE["dehoog"] = dehoog_line_integrate_functional
    try:
        pred = onl.nl_forward(leaves, s0, a0, ts, S=S, ilt_algorithm="dehoog", normalize_time=normalize_time)
    finally:
        oilt.LINE_INTEGRATE["dehoog"] = saved
    # (nl_forward squeezes: at d = 1 its (N,) against an (N, 1) target would broadcast to (N, N))
    pred = pred.reshape(s0.shape)
    loss = ((pred - (sn - s0)) ** 2).mean()
    loss.backward()
    return float(loss.detach()), {k: leaves[k].grad for k in names}, pred.detach()


@functools.lru_cache(maxsize=None)
def _reference(d, h, S, N, B, normalize_time):
    """One CPU reference per case, shared and left unchanged: state dict, data, loss, gradients, and the precondition."""
    sd = _sd(d, h, S)
    data = _data(d, N, B, normalize_time=normalize_time)
    loss, grads, pred = _oracle(sd, data, S, normalize_time, True)
    inplace = _oracle(sd, data, S, normalize_time, False)
    # the precondition: both CPU forms of the table agree on EVERY row
    gap = (pred - inplace).abs() / (1.0 + inplace.abs())
    assert float(gap.max()) <= 1e-9, f"ill-conditioned case: in-place vs functional oracle differ by {float(gap.max()):.3e}"
    return sd, data, loss, grads


# (d, h, S, N, B, normalize_time): S = 3, 5, 17, 33 are Mq = 1, 2, 8, 16 (both launch-bound classes of the ILT kernels); N = 13
# at d = 5 is 65 ILT rows, one past a 64-row block; N = 17, 37 ragged tiles, 2048 the largest call.
# The 2048-row case is there for the largest grid (128 tiles, 32 blocks of the ILT kernels), so it takes the cheapest model:
# d = 1 and the 5-term table
LG_CASES = [
    (5, 128, 33, 13, 4, True),
    (1, 64, 3, 1, 1, True),
    (3, 64, 5, 17, 16, False),
    (5, 128, 17, 16, 4, True),
    (3, 128, 17, 37, 1, False),
    (5, 64, 5, 37, 16, True),
    (1, 128, 5, 2048, 4, True),
]


def _fused(nlc, models, group=False, **kw):
    """A dehoog="fused" trainer (a group for a list), built with every warning recorded: none may come from the trainer."""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainerGroup(models, dehoog="fused", **kw) if group else nlc.NLTrainer(models, dehoog="fused", **kw)
    assert not [w for w in rec if "Trainer" in str(w.message)], [str(w.message) for w in rec]
    assert tr.fused is True
    return tr


# ---------------------------------------------------------------------------------------------------------------- 1
def test_fused_dehoog_trainer_constructs_without_warning(nlc):
    """Fails without the feature: a de Hoog model gives a fused trainer, and so does a group of 3, with no warning."""
    d, h, S = 3, 64, 5
    _fused(nlc, _model(nlc, _sd(d, h, S), d, h, S))
    _fused(nlc, [_model(nlc, _sd(d, h, S, seed=s), d, h, S) for s in (3, 4, 5)], group=True)
    with pytest.raises(ValueError, match="dehoog"):
        nlc.NLTrainer(_model(nlc, _sd(d, h, S), d, h, S), dehoog="hip")


# ---------------------------------------------------------------------------------------------------------------- 2
def _grad_mode(model, data):
    s0, a0, sn, ts = (t.cuda() for t in data)
    model.zero_grad()
    loss = torch.nn.functional.mse_loss(model(s0, a0, ts).squeeze(), (sn - s0).squeeze())
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}


def _worst_block(grads, ref):
    return max(err / scale for k in ref for _, err, scale in blockwise_errors(k, grads[k], ref[k]))


def _compare(nlc, case, got_loss, got_grads, what):
    """The bounds of the module docstring for one fused result of ``case``; prints the measured figures."""
    d, h, S, N, B, nt = case
    sd, data, ref_loss, ref_grads = _reference(*case)
    rel = abs(got_loss - ref_loss) / abs(ref_loss)
    worst = _worst_block(got_grads, ref_grads)
    print(f"{what} {case}: loss rel err {rel:.3e}, worst gradient block {worst:.3e}")
    strict = rel <= 1e-12
    if strict:
        try:
            for k in ref_grads:
                assert_grad_close(k, got_grads[k], ref_grads[k], 1e-9)
        except AssertionError:
            strict = False
    if strict:
        return
    # condition-aware: the reference's own response to a relative 1e-15 perturbation of its parameters
    p_loss, p_grads, _ = _oracle(sd, data, S, nt, True, scale=1.0 + 1e-15)
    sens = {k: (p_grads[k] - ref_grads[k]).abs() for k in ref_grads}
    gm_loss, gm_grads = _grad_mode(_model(nlc, sd, d, h, S, normalize_time=nt), data)
    gm_rel, gm_worst = abs(gm_loss - ref_loss) / abs(ref_loss), _worst_block(gm_grads, ref_grads)
    print(f"  condition-aware: grad-mode loss rel err {gm_rel:.3e}, worst block {gm_worst:.3e}; "
          f"loss sens {abs(p_loss - ref_loss) / abs(ref_loss):.3e}")
    assert abs(got_loss - ref_loss) <= 1e-12 * abs(ref_loss) + 200.0 * abs(p_loss - ref_loss), f"loss rel err {rel:.3e}"
    for k in ref_grads:
        assert_grad_close(k, got_grads[k], ref_grads[k], 1e-9, sens=sens[k])
    # the grad-mode path runs the same ILT kernels: it must not be much closer than the fused step
    if rel > 1e-12:
        assert gm_rel >= 0.1 * rel, f"grad-mode loss is closer: {gm_rel:.3e} against {rel:.3e}"
    if worst > 1e-9:
        assert gm_worst >= 0.1 * worst, f"grad-mode gradients are closer: {gm_worst:.3e} against {worst:.3e}"


@pytest.mark.parametrize("case", LG_CASES, ids=["-".join(map(str, c)) for c in LG_CASES])
def test_loss_and_grad_vs_oracle_autograd(nlc, case):
    d, h, S, N, B, nt = case
    sd, data, _, _ = _reference(*case)
    s0, a0, sn, ts = data
    model = _model(nlc, sd, d, h, S, normalize_time=nt)
    tr = _fused(nlc, model)
    loss = tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), (sn - s0).cuda())
    assert loss.dim() == 0 and loss.is_cuda
    _compare(nlc, case, float(loss), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}, "loss_and_grad")


# ---------------------------------------------------------------------------------------------------------------- 3
def _ref_step(model, opt, bs0, ba0, bts, bsd, clip):
    opt.zero_grad()
    loss = torch.nn.MSELoss()(model(bs0, ba0, bts).squeeze(), bsd.squeeze())
    loss.backward()
    total = torch.nn.utils.clip_grad_norm_(model.parameters(), clip) if clip > 0 else None
    opt.step()
    return loss.detach(), total


def _twin_divergence(nlc, sd, d, h, S, batches, clip, lr):
    """How far two grad-mode runs drift apart when their initial parameters differ by a relative 1e-15: per tensor, the
    parameters and both moments, the losses, and the first iteration's total gradient norm -- the reference path's own
    conditioning over these iterations."""
    runs = []
    for scale in (None, 1.0 + 1e-15):
        sdp = {k: (v * scale if scale is not None and k.startswith(("action_encoder.", "laplace_rep_func.")) else v)
               for k, v in sd.items()}
        m = _model(nlc, sdp, d, h, S)
        opt = torch.optim.Adam(m.parameters(), lr=lr)
        steps = [_ref_step(m, opt, *b, clip) for b in batches]
        losses, total = [float(x[0]) for x in steps], float(steps[0][1])
        st = opt.state_dict()["state"]
        runs.append((losses, [p.detach().cpu() for p in m.parameters()], [st[i]["exp_avg"].cpu() for i in range(len(st))],
                     [st[i]["exp_avg_sq"].cpu() for i in range(len(st))], total))
    a, b = runs
    return (max(abs(x - y) for x, y in zip(a[0], b[0])),
            [[float((x - y).abs().max()) for x, y in zip(a[j], b[j])] for j in (1, 2, 3)], abs(a[4] - b[4]))


def test_one_step_vs_clip_and_adam(nlc):
    """step() == grad-mode forward + clip_grad_norm_ + torch.optim.Adam on a twin: loss, gradnorm, parameters and both
    moments per tensor to 1e-12 of the tensor's magnitude; what misses gets 200 x the divergence of two grad-mode twins
    whose parameters differ by a relative 1e-15 on top.  gradnorm is the library's output: nlc_train_step called through
    ctypes on a fused de Hoog trainer's ctx (the trainer itself passes no gradnorm pointer), as
    test_gpu_train.py::test_train_step_gradnorm_equals_clip_grad_norm does, against what clip_grad_norm_ returned on the
    grad-mode twin."""
    import ctypes as C

    d, h, S, N, B, clip, lr = 5, 128, 17, 16, 4, 0.1, 1e-4
    sd = _sd(d, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(d, N, B))
    batch = (s0, a0, ts, sn - s0)
    model, twin = _model(nlc, sd, d, h, S), _model(nlc, sd, d, h, S)
    tr = _fused(nlc, model, lr=lr, clip_grad_norm=clip)
    opt = torch.optim.Adam(twin.parameters(), lr=lr)
    ref_loss, ref_total = _ref_step(twin, opt, *batch, clip)
    loss = tr.step(*batch)
    assert tr.fused and tr._step == 1
    # gradnorm: the step entry's own output, on a second fused trainer's ctx and copies of the initial parameters
    probe = _fused(nlc, _model(nlc, sd, d, h, S), lr=lr, clip_grad_norm=clip)
    obs, win, tsd, tgt = probe._data(*batch)
    flat = torch.cat([p.detach().reshape(-1) for p in probe._params]).contiguous()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    out_loss = torch.empty((), dtype=torch.float64, device="cuda")
    gnorm = torch.full((), float("nan"), dtype=torch.float64, device="cuda")
    idx = torch.arange(N, dtype=torch.int64, device="cuda")
    ws = probe._workspace(N)
    ctx = probe._ctx
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with ctx.stream():
        ctx.check(ctx.lib.nlc_train_step(ctx.h, C.byref(probe._desc()), ptr(flat), ptr(m), ptr(v), 1, ptr(obs), ptr(win),
                                         ptr(tsd), ptr(tgt), ptr(idx), N, B, ptr(out_loss), ptr(gnorm), ptr(ws)))
    total = float(gnorm)
    assert torch.equal(out_loss, loss)  # the same step as the trainer's
    assert float(ref_total) > clip, "the test wants a clipping case"
    dloss, (dp, dm, dv), dtotal = _twin_divergence(nlc, sd, d, h, S, [batch], clip, lr)
    print(f"step: loss rel err {abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)):.3e}, "
          f"gradnorm rel err {abs(total - float(ref_total)) / float(ref_total):.3e}")
    assert abs(float(loss) - float(ref_loss)) <= 1e-12 * abs(float(ref_loss)) + 200.0 * dloss
    assert abs(total - float(ref_total)) <= 1e-12 * float(ref_total) + 200.0 * dtotal, f"gradnorm {total!r} vs {float(ref_total)!r}"
    sd_tr, sd_ref = tr.state_dict(), opt.state_dict()
    named_twin = dict(twin.named_parameters())
    worst = 0.0
    for i, (k, p) in enumerate(model.named_parameters()):
        for got, ref, div, what in ((p, named_twin[k], dp[i], k), (sd_tr["state"][i]["exp_avg"], sd_ref["state"][i]["exp_avg"], dm[i], k + " exp_avg"),
                                    (sd_tr["state"][i]["exp_avg_sq"], sd_ref["state"][i]["exp_avg_sq"], dv[i], k + " exp_avg_sq")):
            got, ref = got.detach().cpu(), ref.detach().cpu()
            err, sc = float((got - ref).abs().max()), float(ref.abs().max()) + 1e-300
            worst = max(worst, err / sc)
            assert err <= 1e-12 * sc + 200.0 * div, f"{what}: {err:.3e} > 1e-12 x {sc:.3e} + 200 x {div:.3e}"
        assert float(sd_tr["state"][i]["step"]) == 1.0
    print(f"step: worst parameter / moment error {worst:.3e} of the tensor's magnitude")


# ---------------------------------------------------------------------------------------------------------------- 4
def _run_setup(nlc, d=5, h=128, S=17, bs=7, iters=10, seed=3):
    sd = _sd(d, h, S, seed=seed)
    s0, a0, sn, ts = (t.cuda() for t in _data(d, bs * iters + 3, 4))
    perm = torch.randperm(s0.shape[0], generator=torch.Generator().manual_seed(5)).cuda()
    return sd, (s0, a0, sn, ts), perm


def _params(model):
    return [p.detach().cpu().clone() for p in model.parameters()]


def test_run_equals_a_loop_of_steps_and_tracks_the_grad_mode_loop(nlc):
    d, h, S, bs, iters = 5, 128, 17, 7, 10
    sd, (s0, a0, sn, ts), perm = _run_setup(nlc, d, h, S, bs, iters)
    model, twin, ref = (_model(nlc, sd, d, h, S) for _ in range(3))
    tr = _fused(nlc, model)
    losses = tr.run(s0, a0, sn, ts, perm, batch_size=bs)
    assert losses.shape == (iters,) and losses.is_cuda
    tr2 = _fused(nlc, twin)
    batches = []
    for i in range(iters):
        ind = perm[i * bs:i * bs + bs]
        batches.append((s0[ind], a0[ind], ts[ind], sn[ind] - s0[ind]))
    stepped = torch.stack([tr2.step(*b) for b in batches])
    assert torch.equal(losses, stepped)
    for a, b in zip(_params(model), _params(twin)):
        assert torch.equal(a, b)
    # the grad-mode loop, at the project's 1e-9; what misses gets 200 x the divergence of two grad-mode runs
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    ref_losses = torch.stack([_ref_step(ref, opt, *b, 0.1)[0] for b in batches])
    rel = float(((losses - ref_losses).abs() / ref_losses.abs()).max())
    perr = max(float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300) for a, b in zip(_params(model), _params(ref)))
    print(f"run: worst loss rel err {rel:.3e}, worst parameter err {perr:.3e} of max |p|")
    if rel > 1e-9 or perr > 1e-9:
        dloss, (dp, _, _), _ = _twin_divergence(nlc, sd, d, h, S, batches, 0.1, 1e-4)
        print(f"run: grad-mode twins diverge by {dloss:.3e} (loss), {max(dp):.3e} (parameters)")
        assert float((losses - ref_losses).abs().max()) <= 1e-9 * float(ref_losses.abs().min()) + 200.0 * dloss
        for a, b, div in zip(_params(model), _params(ref), dp):
            assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max()) + 200.0 * div


# ---------------------------------------------------------------------------------------------------------------- 5
def test_two_runs_from_one_state_are_bit_equal(nlc):
    sd, data, perm = _run_setup(nlc, 3, 64, 33)
    out = []
    for _ in range(2):
        model = _model(nlc, sd, 3, 64, 33)
        losses = _fused(nlc, model).run(*data, perm, batch_size=7)
        out.append((losses.cpu(), _params(model)))
    assert torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))


def _state(tr, i=0):
    return tr._flat[i].cpu().clone(), tr._m[i].cpu().clone(), tr._v[i].cpu().clone()


@pytest.mark.parametrize("M,stacked", [(2, False), (5, True)])
def test_group_members_are_bit_equal_to_single_trainers(nlc, M, stacked):
    """Losses, gradients, parameters and moments of every member of a group == its own NLTrainer's: loss_and_grad at N = 37
    (a ragged third tile), then run() at batch 7; a shared dataset, and one stacked per member."""
    d, h, S, bs, iters = 5, 128, 17, 7, 4
    sds = [_sd(d, h, S, seed=10 + i) for i in range(M)]
    sets = [tuple(t.cuda() for t in _data(d, 37, 4, seed=30 + (i if stacked else 0))) for i in range(M)]
    perms = torch.stack([torch.randperm(37, generator=torch.Generator().manual_seed(50 + i)) for i in range(M)]).cuda()
    singles = []
    for i in range(M):
        m = _model(nlc, sds[i], d, h, S)
        tr = _fused(nlc, m)
        s0, a0, sn, ts = sets[i]
        lg = tr.loss_and_grad(s0, a0, ts, sn - s0)
        grads = [p.grad.detach().cpu().clone() for p in m.parameters()]
        losses = tr.run(s0, a0, sn, ts, perms[i, : bs * iters], batch_size=bs)
        singles.append((lg.cpu(), grads, losses.cpu(), _state(tr)))
    models = [_model(nlc, sds[i], d, h, S) for i in range(M)]
    grp = _fused(nlc, models, group=True)
    if stacked:
        s0, a0, sn, ts = (torch.stack([sets[i][j] for i in range(M)]) for j in range(4))
    else:
        s0, a0, sn, ts = sets[0]
    lg = grp.loss_and_grad(s0, a0, ts, sn - s0)
    assert lg.shape == (M,)
    grads = [[p.grad.detach().cpu().clone() for p in m.parameters()] for m in models]
    losses = grp.run(s0, a0, sn, ts, perms[:, : bs * iters], batch_size=bs)
    assert losses.shape == (M, iters)
    for i in range(M):
        assert torch.equal(lg[i].cpu(), singles[i][0])
        assert all(torch.equal(a, b) for a, b in zip(grads[i], singles[i][1]))
        assert torch.equal(losses[i].cpu(), singles[i][2])
        assert all(torch.equal(a, b) for a, b in zip(_state(grp, i), singles[i][3]))


def test_per_member_lr_and_a_frozen_member(nlc):
    """lr=[...] per member: each bit-equal to a single trainer built with its lr; a frozen member's parameter and moment rows
    keep their int64 bit patterns while the others move."""
    d, h, S, bs, M = 3, 64, 5, 7, 3
    lrs = [1e-4, 3e-4, 1e-3]
    sds = [_sd(d, h, S, seed=20 + i) for i in range(M)]
    s0, a0, sn, ts = (t.cuda() for t in _data(d, 30, 4))
    perm = torch.randperm(30, generator=torch.Generator().manual_seed(2)).cuda()[: 3 * bs]
    want = []
    for i in range(M):
        tr = _fused(nlc, _model(nlc, sds[i], d, h, S), lr=lrs[i])
        want.append((tr.run(s0, a0, sn, ts, perm, batch_size=bs).cpu(), _state(tr)))
    grp = _fused(nlc, [_model(nlc, sds[i], d, h, S) for i in range(M)], group=True, lr=lrs)
    losses = grp.run(s0, a0, sn, ts, perm, batch_size=bs)
    for i in range(M):
        assert torch.equal(losses[i].cpu(), want[i][0])
        assert all(torch.equal(a, b) for a, b in zip(_state(grp, i), want[i][1]))
    grp.freeze([False, True, False])
    before = [t.view(torch.int64).clone() for t in (grp._flat[1], grp._m[1], grp._v[1])]
    moved = grp._flat[0].clone()
    more = grp.run(s0, a0, sn, ts, perm, batch_size=bs)
    assert more.shape == (M, 3) and bool(torch.isfinite(more).all())
    for t, b in zip((grp._flat[1], grp._m[1], grp._v[1]), before):
        assert torch.equal(t.view(torch.int64), b)
    assert not torch.equal(grp._flat[0], moved)
    assert grp.active.tolist() == [True, False, True]


# ---------------------------------------------------------------------------------------------------------------- 6
def test_evaluate_equals_the_training_loss_and_the_reference(nlc):
    """evaluate == loss_and_grad's loss on the same rows (1e-13 relative: another summation order of the tile losses, as the
    Fourier suite holds that pair), and agrees with the CPU reference under the module's rule; a group gives (M,)."""
    case = (5, 128, 17, 16, 4, True)
    d, h, S, N, B, nt = case
    sd, data, ref_loss, _ = _reference(*case)
    s0, a0, sn, ts = (t.cuda() for t in data)
    model = _model(nlc, sd, d, h, S)
    tr = _fused(nlc, model)
    before = _params(model)
    ev = tr.evaluate(s0, a0, ts, sn - s0)
    assert ev.dim() == 0 and ev.is_cuda and tr._step == 0
    assert all(torch.equal(a, b) for a, b in zip(before, _params(model)))
    lg = tr.loss_and_grad(s0, a0, ts, sn - s0)
    assert abs(float(ev) - float(lg)) <= 1e-13 * abs(float(lg))
    _compare(nlc, case, float(ev), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}, "evaluate")
    # rows picked by index, without a gather: the same loss as the gathered batch
    pick = torch.tensor([3, 0, 11, 7, 15], device="cuda")
    a = tr.evaluate(s0, a0, ts, sn - s0, indices=pick)
    b = tr.evaluate(s0[pick], a0[pick], ts[pick], (sn - s0)[pick])
    assert torch.equal(a, b)
    grp = _fused(nlc, [_model(nlc, sd, d, h, S), _model(nlc, _sd(d, h, S, seed=9), d, h, S)], group=True)
    evg = grp.evaluate(s0, a0, ts, sn - s0)
    assert evg.shape == (2,) and torch.equal(evg[0], ev)


# ---------------------------------------------------------------------------------------------------------------- 7
def _trainer_warnings(rec):
    return [w for w in rec if "NLTrainer" in str(w.message)]


def test_calls_past_the_limits_take_the_grad_mode_path_once_warned(nlc):
    """N = 2049 and a window of 17: the per-call grad-mode path on the trainer's Adam state, one warning in all, the step
    count moving once per call."""
    d, h, S = 1, 64, 3
    sd = _sd(d, h, S)
    model, twin = _model(nlc, sd, d, h, S), _model(nlc, sd, d, h, S)
    big = tuple(t.cuda() for t in _data(d, 2049, 4))
    long_ = tuple(t.cuda() for t in _data(d, 5, 17))
    small = tuple(t.cuda() for t in _data(d, 16, 4))
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(model, dehoog="fused")
        tr.step(small[0], small[1], small[3], small[2] - small[0])
        assert tr._step == 1
        l1 = tr.step(big[0], big[1], big[3], big[2] - big[0])
        assert tr._step == 2
        l2 = tr.step(long_[0], long_[1], long_[3], long_[2] - long_[0])
        assert tr._step == 3 and tr.fused
        tr.step(small[0], small[1], small[3], small[2] - small[0])
    assert len(_trainer_warnings(rec)) == 1
    _ref_step(twin, opt, small[0], small[1], small[3], small[2] - small[0], 0.1)
    r1, _ = _ref_step(twin, opt, big[0], big[1], big[3], big[2] - big[0], 0.1)
    r2, _ = _ref_step(twin, opt, long_[0], long_[1], long_[3], long_[2] - long_[0], 0.1)
    # the refused calls ran the reference's ops on moments the fused step left: the twin's trajectory to 1e-9
    assert abs(float(l1) - float(r1)) <= 1e-9 * abs(float(r1)) and abs(float(l2) - float(r2)) <= 1e-9 * abs(float(r2))
    assert float(tr.state_dict()["state"][0]["step"]) == 4.0


def test_even_terms_and_an_empty_batch_raise(nlc):
    """An even term count: nlc_set_model takes the model, the step entry refuses it on the host as NLC_ERR_UNSUPPORTED with
    its own message (before it looks at a pointer: the call below passes none), and the trainer's per-call grad-mode path,
    taken with the one warning, then raises from the de Hoog ILT entry, which takes odd counts only.  N = 0 raises too."""
    import ctypes as C

    d, h = 3, 64
    s0, a0, sn, ts = (t.cuda() for t in _data(d, 16, 4))
    tr = _fused(nlc, _model(nlc, _sd(d, h, 4), d, h, 4))
    ctx, null = tr._ctx, C.c_void_p(0)
    rc = ctx.lib.nlc_train_step(ctx.h, C.byref(tr._desc()), null, null, null, 1, null, null, null, null, null, 16, 4, null,
                                null, null)
    assert rc == nlc._lib.NLC_ERR_UNSUPPORTED
    assert "(dehoog): ilt_reconstruction_terms must be odd, 3 .. 33" in ctx.lib.nlc_last_error(ctx.h).decode()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(nlc._lib.NlcError):
            tr.step(s0, a0, ts, sn - s0)
    assert len(_trainer_warnings(rec)) == 1 and "must be odd" in str(_trainer_warnings(rec)[0].message)
    assert tr._step == 0
    tr = _fused(nlc, _model(nlc, _sd(d, h, 5), d, h, 5))
    with pytest.raises(nlc._lib.NlcError):
        tr.step(s0[:0], a0[:0], ts[:0], (sn - s0)[:0])
    assert tr._step == 0


def test_live_switching_on_a_fused_trainer_and_the_default_guard(nlc):
    """fourier -> dehoog -> fourier on a dehoog="fused" trainer: every stage fused, no warning, each torch.equal to a fresh
    trainer on a deep copy that took over the optimiser state.  A default trainer still is not fused and warns once."""
    d, h, S, bs = 3, 64, 5, 7
    sd = _sd(d, h, S)
    s0, a0, sn, ts = (t.cuda() for t in _data(d, 3 * bs, 4))
    perm = torch.arange(3 * bs).cuda()
    model = _model(nlc, sd, d, h, S, algo="fourier")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(model, dehoog="fused")
        for algo in ("fourier", "dehoog", "fourier"):
            model.ilt_algorithm = algo
            fresh_model = copy.deepcopy(model)
            fresh = nlc.NLTrainer(fresh_model, dehoog="fused")
            fresh.load_state_dict(tr.state_dict())
            a = tr.run(s0, a0, sn, ts, perm, batch_size=bs)
            b = fresh.run(s0, a0, sn, ts, perm, batch_size=bs)
            assert tr.fused and fresh.fused
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
            assert all(torch.equal(x, y) for x, y in zip(_params(model), _params(fresh_model)))
    assert not _trainer_warnings(rec)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        plain = nlc.NLTrainer(_model(nlc, sd, d, h, S))
        plain.step(s0[:bs], a0[:bs], ts[:bs], (sn - s0)[:bs])
    assert not plain.fused and len(_trainer_warnings(rec)) == 1


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("M", [1, 2])
def test_keep_best_restore_best_and_fit_against_a_host_loop(nlc, M):
    """fit() on a tiny fused de Hoog trainer (and a group of 2) == a host loop of run, evaluate, .item() and clones, bit for bit."""
    d, h, S, bs, every, epochs = 3, 64, 5, 4, 2, 2
    sds = [_sd(d, h, S, seed=40 + i) for i in range(M)]
    s0, a0, sn, ts = (t.cuda() for t in _data(d, 21, 4))
    val = tuple(t.cuda() for t in _data(d, 9, 4, seed=99))
    val = (val[0], val[1], val[3], val[2] - val[0])

    def build():
        models = [_model(nlc, sd, d, h, S) for sd in sds]
        return models, (_fused(nlc, models, group=True, lr=1e-3) if M > 1 else _fused(nlc, models[0], lr=1e-3))

    models, tr = build()
    out = tr.fit((s0, a0, sn, ts), val, epochs=epochs, batch_size=bs, eval_every=every, seed=7)
    # the host loop
    hmodels, ht = build()
    best = [float("inf")] * M
    best_w = [_params(m) for m in hmodels]
    best_it, done, crits, train = [-1] * M, 0, [], []
    for epoch in range(epochs):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7 + epoch)
        perm = torch.randperm(21, device="cuda", generator=gen)
        for chunk in perm.split(every * bs):
            if chunk.numel() < bs:
                continue
            train.append(ht.run(s0, a0, sn, ts, chunk, bs))
            done += chunk.numel() // bs
            crit = ht.evaluate(*val).reshape(-1)
            crits.append(crit)
            for i in range(M):
                if crit[i].item() < best[i]:
                    best[i], best_it[i], best_w[i] = crit[i].item(), done, _params(hmodels[i])
    assert torch.equal(out["criterion"].reshape(M, -1), torch.stack(crits, dim=-1))
    assert torch.equal(out["train_loss"].reshape(M, -1), torch.cat([t.reshape(M, -1) for t in train], dim=-1))
    assert out["best_loss"].reshape(-1).tolist() == best and out["best_iter"].reshape(-1).tolist() == best_it
    for i in range(M):  # fit restored the best weights
        assert all(torch.equal(a, b) for a, b in zip(_params(models[i]), best_w[i]))
    # keep_best / restore_best by hand: a worse loss keeps the snapshot, restore writes it back
    snap = [_params(m) for m in models]
    improved = tr.keep_best(torch.full((M,), float("inf"), dtype=torch.float64, device="cuda"))
    assert improved.reshape(-1).tolist() == [0] * M
    tr.run(s0, a0, sn, ts, torch.arange(bs).cuda(), bs)
    assert not all(torch.equal(a, b) for a, b in zip(_params(models[0]), snap[0]))
    tr.restore_best()
    for i in range(M):
        assert all(torch.equal(a, b) for a, b in zip(_params(models[i]), snap[i]))
