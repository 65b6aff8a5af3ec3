"""GPU: the fused training step of the NODE baseline (NODETrainer / NODETrainerGroup, nlc_node_train_group_*) against
float64 autograd through the CPU oracle (oracle.node_model.forward + MSE; rows one at a time for row_times=True) and against
the reference's training loop on the model's grad-mode path (train_utils.py:388-408).  Tolerances are docs/training.md's:
loss 1e-12 relative, every gradient block 1e-9 of its own max |grad| (floored at 1e-6 of the tensor's), step() 1e-12 of each
tensor's magnitude, run() 1e-9 over 50 iterations, gradnorm 1e-12.

Blocks: the state / action column blocks of 0.weight, the state / augment row blocks of 4.weight and 4.bias, otherwise the
whole tensor.  No test launches the kernels with a non-positive or over-long time: the clamp is checked on the host
(tests/test_train_node_host.py)."""

import copy
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
from gpu_common import build_node
from train_compare import BLOCK_FLOOR

pytestmark = pytest.mark.gpu

P = "x_ode_func_in_x_and_u.linear_tanh_stack."
PARAMS = [P + f"{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]
DT = 0.05
# raw times whose normalised end (/ 0.4) takes 3, 1 and 40 Euler sub-steps of 0.05
T3, T1, T40 = 0.05, 0.012, 0.788


def _times(kind, N, normalize_time, gen):
    div = DT * 8.0 if normalize_time else 1.0
    if kind == "fixed":  # the reference's fixed grid: 3 sub-steps with normalize_time, 1 without
        return torch.full((N, 1), DT, dtype=torch.float64)
    if kind == "grid":  # ends exactly on grid points k * 0.05 of the normalised time, k = 1 .. 8
        k = torch.arange(N) % 8 + 1
        return (k.to(torch.float64) * 0.05 * div).view(N, 1)
    if kind == "mixed":  # rows of 3, 1 and 40 sub-steps; row 0 takes 3
        assert normalize_time
        return torch.tensor([T3, T1, T40], dtype=torch.float64)[torch.arange(N) % 3].view(N, 1)
    if kind == "random":
        return (torch.rand(N, 1, dtype=torch.float64, generator=gen) * 0.08 + 0.02) * (div / 0.4)
    raise ValueError(kind)


def _setup(H, d, aug, nu, N, normalize=True, normalize_time=True, mean=False, times="fixed", B=3, seed=0, out_scale=0.3):
    from oracle import node_model as on

    rng = np.random.RandomState(seed)
    std = rng.uniform(0.5, 3.0, d)
    sd = on.make_synthetic_state_dict(seed, d, nu, H, aug, list(std), None, DT, out_scale=out_scale)
    sm = rng.uniform(-1.0, 1.0, d) if mean else np.zeros(d)
    sd["state_mean"] = torch.tensor(sm, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + 17)
    s0 = torch.tensor(sm) + torch.randn(N, d, dtype=torch.float64, generator=g) * torch.tensor(std)
    a0 = (torch.rand(N, B, nu, dtype=torch.float64, generator=g) * 2 - 1) * 3.0
    sn = s0 + torch.randn(N, d, dtype=torch.float64, generator=g) * 0.05 * torch.tensor(std)
    return sd, (s0, a0, sn, _times(times, N, normalize_time, g))


def _oracle_pred(sd, s0, a0, ts, normalize, normalize_time, row_times):
    from oracle import node_model as on

    if not row_times:
        return on.forward(sd, s0, a0, ts, normalize, normalize_time)
    # rows that share a time integrate together: the oracle takes ts[0] of what it is given
    out = torch.empty(s0.shape[0], s0.shape[1], dtype=torch.float64)
    flat = ts.reshape(-1)
    for t in flat.unique():
        rows = (flat == t).nonzero().reshape(-1)
        out = out.index_copy(0, rows, on.forward(sd, s0[rows], a0[rows], ts[rows], normalize, normalize_time))
    return out


def _oracle_loss_grads(sd, s0, a0, ts, target, normalize, normalize_time, row_times):
    leaves = {k: (v.clone().requires_grad_() if k in PARAMS else v) for k, v in sd.items()}
    loss = ((_oracle_pred(leaves, s0, a0, ts, normalize, normalize_time, row_times) - target) ** 2).mean()
    loss.backward()
    return loss.detach(), {k: leaves[k].grad for k in PARAMS}


def _oracle_loss(sd, s0, a0, ts, target, normalize=True, normalize_time=True, row_times=False):
    with torch.no_grad():
        return float(((_oracle_pred(sd, s0, a0, ts, normalize, normalize_time, row_times) - target) ** 2).mean())


def _blocks(name, t, d, aug):
    if name == P + "0.weight":
        return [("state", t[:, :d]), ("action", t[:, d + aug :])] + ([("augment", t[:, d : d + aug])] if aug else [])
    if name in (P + "4.weight", P + "4.bias"):
        return [("state", t[:d])] + ([("augment", t[d:])] if aug else [])
    return [("all", t)]


def _assert_grad_close(name, got, ref, d, aug, tol=1e-9):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite gradient"
    tmax = float(ref.abs().max())
    worst = 0.0
    for (label, g), (_, r) in zip(_blocks(name, got, d, aug), _blocks(name, ref, d, aug)):
        scale = max(float(r.abs().max()), BLOCK_FLOOR * tmax) + 1e-300
        err = float((g - r).abs().max())
        worst = max(worst, err / scale)
        print(f"{name}[{label}]: err {err:.3e} scale {scale:.3e} ratio {err / scale:.3e}")
        assert err <= tol * scale, f"{name}[{label}]: max err {err:.3e} > {tol:g} x block scale {scale:.3e}"
    return worst


def _close_to_scale(got, ref, tol, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    sc = float(ref.abs().max()) + 1e-300
    err = float((got - ref).abs().max())
    assert err <= tol * sc, f"{what}: max err {err:.3e} > {tol:g} x {sc:.3e}"


def _ref_step(model, opt, bs0, ba0, bts, bsd, clip):
    """train_utils.py:391-408 on the model's grad-mode path; returns (loss, clip_grad_norm_'s total norm or None)."""
    opt.zero_grad()
    loss = torch.nn.MSELoss()(model(bs0, ba0, bts).squeeze(), bsd.squeeze())
    loss.backward()
    total = float(torch.nn.utils.clip_grad_norm_(model.parameters(), clip)) if clip > 0 else None
    opt.step()
    return loss.item(), total


def _assert_adam_state_equal(model, twin, tr, opt, tol, steps):
    sd_tr, sd_ref = tr.state_dict(), opt.state_dict()
    named_twin = dict(twin.named_parameters())
    for i, (k, p) in enumerate(model.named_parameters()):
        _close_to_scale(p, named_twin[k], tol, k)
        for key in ("exp_avg", "exp_avg_sq"):
            _close_to_scale(sd_tr["state"][i][key], sd_ref["state"][i][key], tol, f"{k} {key}")
        assert float(sd_tr["state"][i]["step"]) == float(sd_ref["state"][i]["step"]) == steps, k


def _pair(nlc, H=270, d=5, aug=1, nu=1, N=16, seed=3, **kw):
    """Model, twin and a device dataset at the reference's own shape; the last layer keeps its initial scale so the clip of
    0.1 is active."""
    kw.setdefault("out_scale", 1.0)
    sd, data = _setup(H, d, aug, nu, N, seed=seed, **kw)
    mk = lambda: build_node(nlc, sd, H, aug)  # noqa: E731
    return mk(), mk(), tuple(t.cuda() for t in data), sd


def _tiny(nlc, n, N=64, H=17, seed=5, times="random"):
    """n small NODEs of one descriptor with different weights, and a device dataset."""
    from oracle import node_model as on

    sd, data = _setup(H, 3, 1, 1, N, seed=seed, times=times, out_scale=1.0)
    models = []
    for i in range(n):
        sdi = dict(sd)
        sdi.update({k: v for k, v in on.make_synthetic_state_dict(seed + 10 * i, 3, 1, H, 1, None, None, DT, 1.0).items()
                    if k in PARAMS})
        models.append(build_node(nlc, sdi, H, 1))
    return models, tuple(t.cuda() for t in data)


# ---------------------------------------------------------------------------------------------------------------------
# 1. loss_and_grad against the oracle
# (H, d, aug, nu, N, normalize, normalize_time, non-zero means, times, row_times)
LG_CASES = [
    (270, 5, 1, 1, 1, True, True, True, "fixed", False),     # the reference's shape and batch: 3 sub-steps
    (270, 5, 1, 1, 16, True, True, False, "fixed", False),   # a full tile
    (272, 6, 2, 2, 17, True, False, True, "fixed", False),   # widest; no normalize_time: 1 sub-step; one row past a tile
    (1, 1, 0, 1, 2, False, False, False, "random", False),   # smallest of everything, raw inputs
    (15, 3, 0, 1, 15, True, True, False, "grid", True),      # ends exactly on grid points, odd H in = 60
    (16, 2, 1, 2, 37, True, True, True, "mixed", True),      # 1, 3 and 40 sub-steps in one tile, ragged third tile
    (17, 5, 1, 1, 37, True, True, False, "mixed", False),    # the same mix under the default: every row follows row 0
    (33, 3, 0, 1, 2100, True, True, False, "fixed", False),  # > 128 tiles: a workgroup walks a ragged second tile
    (270, 5, 1, 1, 37, True, True, True, "mixed", True),     # the reference's width with per-row times (odd H in = 1890)
    (33, 6, 2, 2, 16, True, False, False, "grid", True),     # grid points without normalize_time, in = 10
]


@pytest.mark.parametrize("case", LG_CASES, ids=[f"H{c[0]}_d{c[1]}a{c[2]}u{c[3]}_N{c[4]}_{c[8]}_{'row' if c[9] else 'first'}"
                                                for c in LG_CASES])
def test_loss_and_grad_vs_oracle_autograd(nlc, case):
    H, d, aug, nu, N, normalize, normalize_time, mean, times, row_times = case
    sd, (s0, a0, sn, ts) = _setup(H, d, aug, nu, N, normalize, normalize_time, mean, times, seed=7 * d + H)
    target = sn - s0
    ref_loss, ref_grads = _oracle_loss_grads(sd, s0, a0, ts, target, normalize, normalize_time, row_times)
    model = build_node(nlc, sd, H, aug, normalize, normalize_time)
    tr = nlc.NODETrainer(model, row_times=row_times)
    assert tr.fused
    loss = tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), target.cuda())
    assert loss.dim() == 0 and loss.is_cuda
    rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    print(f"loss rel err {rel:.3e}")
    assert rel <= 1e-12, f"loss rel err {rel:.3e}"
    worst = max(_assert_grad_close(k, p.grad, ref_grads[k], d, aug) for k, p in model.named_parameters())
    print(f"worst gradient block ratio {worst:.3e}")
    assert float(max(g.abs().max() for g in ref_grads.values())) > 0


def test_case_list_covers_the_edges():
    c = LG_CASES
    assert {1, 15, 16, 17, 33, 270, 272} == {x[0] for x in c}
    assert {(5, 1, 1), (3, 0, 1), (2, 1, 2), (6, 2, 2), (1, 0, 1)} == {(x[1], x[2], x[3]) for x in c}
    assert {1, 2, 15, 16, 17, 37, 2100} == {x[4] for x in c}
    assert {"fixed", "grid", "mixed"} <= {x[8] for x in c}
    assert {(True, True), (True, False), (False, False)} <= {(x[5], x[6]) for x in c}
    assert any(x[8] == "mixed" and x[9] for x in c) and any(x[8] == "mixed" and not x[9] for x in c)
    assert {0, 1} == {((x[1] + x[2] + x[3]) * x[0]) % 2 for x in c}  # both parities of H in: 8-byte aligned rows


def test_default_times_follow_row_zero_like_forward_train(nlc):
    """Under the default every row integrates to the first row's time: the loss equals the model's own grad-mode forward +
    MSE (model._forward_train) to 1e-12, and differs from the per-row loss."""
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, H=33, N=37, times="mixed", out_scale=0.3)
    loss = nlc.NODETrainer(model).loss_and_grad(s0, a0, ts, sn - s0)
    ref = torch.nn.functional.mse_loss(twin._forward_train(s0, a0, ts).squeeze(), (sn - s0).squeeze()).detach()
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref))
    rows = nlc.NODETrainer(twin, row_times=True).loss_and_grad(s0, a0, ts, sn - s0)
    assert abs(float(rows) - float(ref)) > 1e-6 * abs(float(ref))


# ---------------------------------------------------------------------------------------------------------------------
# 2. step(), run(), gradnorm against the grad-mode path on a twin
@pytest.mark.parametrize("clip,wd,N", [(0.1, 0.0, 1), (1e6, 0.0, 16), (0.1, 1e-2, 16), (0.0, 0.0, 16)])
def test_one_step_vs_clip_and_adam(nlc, clip, wd, N):
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, N=N)
    kw = dict(lr=1e-4, weight_decay=wd)
    tr = nlc.NODETrainer(model, clip_grad_norm=clip, **kw)
    opt = torch.optim.Adam(twin.parameters(), **kw)
    ref_loss, _ = _ref_step(twin, opt, s0, a0, ts, sn - s0, clip)
    loss = tr.step(s0, a0, ts, sn - s0)
    assert abs(float(loss) - ref_loss) <= 1e-12 * abs(ref_loss)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 1)


@pytest.mark.parametrize("bs", [1, 7])
def test_run_follows_the_reference_loop(nlc, bs):
    """run() over 50 iterations (a permutation with duplicates) against the reference loop on the twin: losses and final
    parameters to 1e-9.  Batch 1 is the reference's NODE batch size (train_utils.py:319-320)."""
    iters = 50
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, H=33, N=64, times="random")
    perm = torch.randint(0, 64, (iters * bs,), generator=torch.Generator().manual_seed(1)).cuda()
    tr = nlc.NODETrainer(model, lr=1e-3)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    ref = []
    for i in range(iters):
        ind = perm[i * bs : (i + 1) * bs]
        ref.append(_ref_step(twin, opt, s0[ind], a0[ind], ts[ind], sn[ind] - s0[ind], 0.1)[0])
    losses = tr.run(s0, a0, sn, ts, perm, bs)
    assert losses.shape == (iters,) and losses.is_cuda
    _close_to_scale(losses, torch.tensor(ref, dtype=torch.float64), 1e-9, "run losses")
    for (k, p), q in zip(model.named_parameters(), twin.parameters()):
        _close_to_scale(p, q, 1e-9, k)


def test_gradnorm_equals_clip_grad_norm_and_the_clip_is_active(nlc):
    from neurallaplacecontrol_amd import _lib
    from neurallaplacecontrol_amd.training import _f64_ptr, _i64_ptr

    model, twin, (s0, a0, sn, ts), _ = _pair(nlc)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    _, total = _ref_step(twin, opt, s0, a0, ts, sn - s0, 0.1)
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
    assert _lib.NLC_ERR_UNSUPPORTED == -4


def test_run_is_bit_reproducible(nlc):
    outs = []
    for _ in range(2):
        model, _, (s0, a0, sn, ts), _ = _pair(nlc, H=33, N=64, times="mixed")
        tr = nlc.NODETrainer(model, row_times=True)
        losses = tr.run(s0, a0, sn, ts, torch.arange(64).cuda(), 16)
        outs.append((losses.clone(), [p.detach().clone() for p in model.parameters()], tr.state_dict()))
    assert torch.equal(outs[0][0], outs[1][0])
    for p, q in zip(outs[0][1], outs[1][1]):
        assert torch.equal(p, q)
    for i in outs[0][2]["state"]:
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(outs[0][2]["state"][i][key], outs[1][2]["state"][i][key])


# ---------------------------------------------------------------------------------------------------------------------
# 3. groups against single trainers built from deep copies, bit for bit
@pytest.mark.parametrize("stacked", [False, True])
@pytest.mark.parametrize("row_times", [False, True])
def test_group_equals_single_trainers(nlc, stacked, row_times):
    M, N = 3, 37
    models, (s0, a0, sn, ts) = _tiny(nlc, M, N=M * N if stacked else N)
    singles = [nlc.NODETrainer(copy.deepcopy(m), row_times=row_times) for m in models]
    grp = nlc.NODETrainerGroup(models, row_times=row_times)
    assert grp.fused
    if stacked:
        data = tuple(t.reshape((M, N) + tuple(t.shape[1:])) for t in (s0, a0, ts, sn - s0))
    else:
        data = (s0, a0, ts, sn - s0)
    mine = lambda i: tuple(t[i] for t in data) if stacked else data  # noqa: E731
    gl = grp.loss_and_grad(*data)
    for i, tr in enumerate(singles):
        assert torch.equal(gl[i], tr.loss_and_grad(*mine(i)))
        for p, q in zip(grp.models[i].parameters(), tr.model.parameters()):
            assert torch.equal(p.grad, q.grad)
    for _ in range(2):
        gl = grp.step(*data)
        for i, tr in enumerate(singles):
            assert torch.equal(gl[i], tr.step(*mine(i)))
    for i, (tr, sdg) in enumerate(zip(singles, grp.state_dict())):
        for p, q in zip(grp.models[i].parameters(), tr.model.parameters()):
            assert torch.equal(p, q)
        sds = tr.state_dict()
        for j in sds["state"]:
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(sdg["state"][j][key], sds["state"][j][key])
    ge = grp.evaluate(*data)
    for i, tr in enumerate(singles):
        assert torch.equal(ge[i], tr.evaluate(*mine(i)))


def test_a_member_does_not_depend_on_the_group_size(nlc):
    models, (s0, a0, sn, ts) = _tiny(nlc, 5, N=64)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(2)).cuda()
    g2 = nlc.NODETrainerGroup([copy.deepcopy(m) for m in models[:2]])
    g5 = nlc.NODETrainerGroup([copy.deepcopy(m) for m in models])
    l2, l5 = g2.run(s0, a0, sn, ts, perm, 16), g5.run(s0, a0, sn, ts, perm, 16)
    assert torch.equal(l2[1], l5[1])
    for p, q in zip(g2.models[1].parameters(), g5.models[1].parameters()):
        assert torch.equal(p, q)


def test_group_refuses_members_of_different_descriptors(nlc):
    models, _ = _tiny(nlc, 2)
    models[1].normalize_time = False
    with pytest.raises(ValueError, match="member 1"):
        nlc.NODETrainerGroup(models)


# ---------------------------------------------------------------------------------------------------------------------
# 4. evaluate
@pytest.mark.parametrize("row_times", [False, True])
def test_evaluate_vs_oracle_and_loss_and_grad(nlc, row_times):
    H, d, aug, nu, N = 270, 5, 1, 1, 203
    sd, (s0, a0, sn, ts) = _setup(H, d, aug, nu, N, mean=True, times="mixed", seed=11)
    target = sn - s0
    tr = nlc.NODETrainer(build_node(nlc, sd, H, aug), row_times=row_times)
    dev = tuple(t.cuda() for t in (s0, a0, ts, target))
    before = [p.detach().clone() for p in tr.model.parameters()]
    loss = tr.evaluate(*dev)
    ref = _oracle_loss(sd, s0, a0, ts, target, row_times=row_times)
    assert loss.dim() == 0 and abs(float(loss) - ref) <= 1e-12 * abs(ref)
    lg = tr.loss_and_grad(*dev)
    assert abs(float(loss) - float(lg)) <= 1e-12 * abs(float(lg))
    ind = torch.tensor([5, 3, 3, 200, 17, 0, 64], dtype=torch.int64)
    sub = tr.evaluate(*dev, indices=ind.cuda())
    ref = _oracle_loss(sd, s0[ind], a0[ind], ts[ind], target[ind], row_times=row_times)
    assert abs(float(sub) - ref) <= 1e-12 * abs(ref)
    for p, q in zip(tr.model.parameters(), before):
        assert torch.equal(p, q)


def test_evaluate_large_n_against_the_oracle_in_chunks(nlc):
    """156 250 rows (the reference's validation share of 1e6 samples at batch 16 granularity), per-row times from the fixed
    grid's three values; the oracle sums the squared errors chunk by chunk."""
    H, d, aug, nu, N = 33, 5, 1, 1, 156250
    sd, (s0, a0, sn, ts) = _setup(H, d, aug, nu, N, times="grid", seed=13, B=1)
    target = sn - s0
    tr = nlc.NODETrainer(build_node(nlc, sd, H, aug), row_times=True)
    loss = tr.evaluate(s0.cuda(), a0.cuda(), ts.cuda(), target.cuda())
    total = 0.0
    with torch.no_grad():
        flat = ts.reshape(-1)
        for t in flat.unique():
            rows = (flat == t).nonzero().reshape(-1)
            pred = _oracle_pred(sd, s0[rows], a0[rows], ts[rows], True, True, False)
            total += float(((pred - target[rows]) ** 2).sum())
    ref = total / (N * d)
    assert abs(float(loss) - ref) <= 1e-12 * abs(ref)


# ---------------------------------------------------------------------------------------------------------------------
# 5. keep_best / restore_best / fit against the host loop, bit for bit
def test_fit_equals_the_host_loop(nlc):
    (m1,), (s0, a0, sn, ts) = _tiny(nlc, 1, N=96)
    m2 = copy.deepcopy(m1)
    val = (s0[:32], a0[:32], ts[:32], (sn - s0)[:32])
    train = (s0[32:], a0[32:], sn[32:], ts[32:])
    tr = nlc.NODETrainer(m1, lr=1e-2)
    out = tr.fit(train, val, epochs=2, batch_size=4, eval_every=5, seed=3)
    ref = nlc.NODETrainer(m2, lr=1e-2)
    best, best_iter, best_w, crits, done = float("inf"), -1, None, [], 0
    for epoch in range(2):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3 + epoch)
        perm = torch.randperm(64, device="cuda", generator=gen)
        for chunk in perm.split(5 * 4):
            if chunk.numel() < 4:
                continue
            ref.run(*train, chunk, 4)
            done += chunk.numel() // 4
            crit = ref.evaluate(*val).item()
            crits.append(crit)
            if crit < best:
                best, best_iter, best_w = crit, done, [p.detach().clone() for p in m2.parameters()]
    assert out["criterion"].cpu().tolist() == crits
    assert float(out["best_loss"]) == best and int(out["best_iter"]) == best_iter
    for p, q in zip(m1.parameters(), best_w):
        assert torch.equal(p, q)
    # the state_dict is the reference's: it loads into a fresh twin
    fresh = copy.deepcopy(m2)
    fresh.load_state_dict(m1.state_dict())


def test_keep_best_and_restore_best_on_crafted_losses(nlc):
    (m,), (s0, a0, sn, ts) = _tiny(nlc, 1)
    tr = nlc.NODETrainer(m)
    w0 = [p.detach().clone() for p in m.parameters()]
    assert int(tr.keep_best(torch.tensor(2.0, device="cuda"))) == 1
    tr.step(s0, a0, ts, sn - s0)
    assert int(tr.keep_best(torch.tensor(3.0, device="cuda"))) == 0
    assert int(tr.keep_best(torch.tensor(float("nan"), device="cuda"))) == 0
    tr.restore_best()
    for p, q in zip(m.parameters(), w0):
        assert torch.equal(p, q)
    assert float(tr.best_loss) == 2.0 and int(tr.best_tag) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. fallback, refusals
@pytest.mark.parametrize("row_times", [False, True])
def test_hidden_300_trains_on_the_grad_mode_path(nlc, row_times):
    """A width nlc_set_node_model refuses: one warning, fused False, the numbers of a hand-written Adam loop (with row_times
    the rows are integrated one at a time)."""
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, H=300, N=6, times="mixed", out_scale=0.3)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tr = nlc.NODETrainer(model, lr=1e-3, row_times=row_times)
        losses = [tr.step(s0, a0, ts, sn - s0) for _ in range(3)]
    assert not tr.fused and len([x for x in w if "grad-mode" in str(x.message)]) == 1
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    for got in losses:
        opt.zero_grad()
        if row_times:
            pred = torch.cat([twin(s0[r : r + 1], a0[r : r + 1], ts[r : r + 1]) for r in range(6)])
        else:
            pred = twin(s0, a0, ts)
        loss = torch.nn.functional.mse_loss(pred.squeeze(), (sn - s0).squeeze())
        loss.backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.1)
        opt.step()
        assert float(got) == float(loss)
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("bad", [0.0, -0.01, float("nan"), 0.4 * 0.05 * 256.5])
def test_bad_times_raise_before_any_launch(nlc, bad):
    """A ts holding 0, a negative time, NaN or a time past 256 sub-steps: ValueError from the trainer's one host read, with
    nothing launched and no step counted."""
    (m,), (s0, a0, sn, ts) = _tiny(nlc, 1)
    tr = nlc.NODETrainer(m, row_times=True)
    ts = ts.clone()
    ts[7] = bad
    for call in (lambda: tr.step(s0, a0, ts, sn - s0), lambda: tr.loss_and_grad(s0, a0, ts, sn - s0),
                 lambda: tr.evaluate(s0, a0, ts, sn - s0), lambda: tr.run(s0, a0, sn, ts, torch.arange(64).cuda(), 16)):
        with pytest.raises(ValueError, match="sub-steps"):
            call()
    # every launch is preceded by the allocation of its workspace: none was made
    assert tr._ws == {} and tr._step == 0


def test_ts_is_read_once_per_tensor(nlc):
    (m,), (s0, a0, sn, ts) = _tiny(nlc, 1)
    tr = nlc.NODETrainer(m)
    tr.step(s0, a0, ts, sn - s0)
    seen = dict(tr._ts_seen)
    tr.run(s0, a0, sn, ts, torch.arange(64).cuda(), 16)
    tr.evaluate(s0, a0, ts, sn - s0)
    assert tr._ts_seen == seen and len(seen) == 1
    ts.mul_(1.0)  # an in-place write moves the version: checked again
    tr.evaluate(s0, a0, ts, sn - s0)
    assert len(tr._ts_seen) == 2


def test_library_refusals_before_any_launch(nlc):
    from neurallaplacecontrol_amd import _lib

    ctx = _lib.Ctx(0)
    z = C.c_void_p(0)
    one = torch.zeros(8, dtype=torch.float64, device="cuda")
    p = C.c_void_p(one.data_ptr())
    assert ctx.lib.nlc_node_train_group_workspace_bytes(ctx.h, 1, 16) == -1
    assert ctx.lib.nlc_node_train_group_loss_grad(ctx.h, 1, 0, p, p, p, p, p, p, 1, 1, p, p, p, 0) == -5  # NLC_ERR_STATE
    assert ctx.lib.nlc_node_train_group_eval(ctx.h, 1, 0, p, p, p, p, p, z, 1, 1, p, p, 0) == -5
    (m,), _ = _tiny(nlc, 1)
    m.upload(ctx)
    assert ctx.lib.nlc_node_train_group_workspace_bytes(ctx.h, 1, 16) > 0
    assert ctx.lib.nlc_node_train_group_workspace_bytes(ctx.h, 1, 16) == ctx.lib.nlc_node_train_group_workspace_bytes(ctx.h, 1, 1)
    assert ctx.lib.nlc_node_train_group_loss_grad(ctx.h, 1, 0, p, p, p, p, p, p, 0, 1, p, p, p, 0) == -2  # N = 0
    assert ctx.lib.nlc_node_train_group_loss_grad(ctx.h, 0, 0, p, p, p, p, p, p, 1, 1, p, p, p, 0) == -2  # M < 1
    assert ctx.lib.nlc_node_train_group_loss_grad(ctx.h, 65536, 0, p, p, p, p, p, p, 1, 1, p, p, p, 0) == -4
    assert ctx.lib.nlc_node_train_group_eval(ctx.h, 65536, 0, p, p, p, p, p, z, 1, 1, p, p, 0) == -4
    assert ctx.lib.nlc_node_train_group_loss_grad(ctx.h, 1, 0, z, p, p, p, p, p, 1, 1, p, p, p, 0) == -1  # NULL
