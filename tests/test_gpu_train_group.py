"""GPU: grouped training (NLTrainerGroup / RNNTrainerGroup, nlc_train_group_* / nlc_rnn_train_group_*): M models of one
descriptor in the same three launches, the member on the grid's second axis.

Every comparison is against single trainers (NLTrainer / RNNTrainer) built from deep copies of the same initial models, in the
same process, and is bit-equal (torch.equal): a member's workgroups execute the same instruction stream on the same operands
in the same reduction order whatever M is, so one differing bit is a wrong stride or a shared slab, not rounding.  Accuracy
against the CPU oracle is pinned by tests/test_gpu_train.py and tests/test_gpu_train_rnn.py for the single trainers."""

import copy
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- helpers
def _nl_model(nlc, seed, d=3, nu=1, h=64, S=3, algo="fourier", state_std=None):
    from oracle import nl_model as onl

    std = [1.0 + 0.5 * i for i in range(d)] if state_std is None else state_std
    sd = onl.make_synthetic_state_dict(seed, d, nu, h, S, std, [1.5] * nu, tame=True)
    m = nlc.NeuralLaplaceModel(d, nu, d, hidden_units=h, s_recon_terms=S, ilt_algorithm=algo, state_mean=np.zeros(d),
                               state_std=np.ones(d), action_mean=np.zeros(nu), action_std=np.ones(nu), normalize=True,
                               normalize_time=True).double()
    m.load_state_dict(sd)
    return m.to("cuda")


def _rnn_model(nlc, seed, cls="DeltaTRNN", d=3, nu=1, H=64):
    from oracle import rnn_model as orn

    std = [1.0 + 0.5 * i for i in range(d)]
    sd = orn.make_synthetic_state_dict(seed, d, nu, H, std, [1.5] * nu, out_scale=1.0, time_input=cls == "DeltaTRNN")
    if cls == "RNN":
        sd.pop("dt", None)  # the reference's RNN has no dt buffer
    kw = dict(hidden_units=H, state_mean=np.zeros(d), state_std=np.ones(d), action_mean=np.zeros(nu), action_std=np.ones(nu),
              normalize=True)
    if cls == "DeltaTRNN":
        kw["normalize_time"] = True
    m = getattr(nlc, cls)(d, nu, **kw).double()
    m.load_state_dict(sd)
    return m.to("cuda")


def _data(N, d=3, nu=1, B=2, seed=17):
    """s0 (N, d), a0 (N, B, nu), sn (N, d), ts (N, 1) on the device."""
    g = torch.Generator().manual_seed(seed)
    std = torch.tensor([1.0 + 0.5 * i for i in range(d)], dtype=torch.float64)
    s0 = torch.randn(N, d, dtype=torch.float64, generator=g) * std
    a0 = (torch.rand(N, B, nu, dtype=torch.float64, generator=g) * 2 - 1) * 3.0
    sn = s0 + torch.randn(N, d, dtype=torch.float64, generator=g) * 0.05 * std
    ts = torch.rand(N, 1, dtype=torch.float64, generator=g) * 0.08 + 0.02
    return tuple(t.cuda() for t in (s0, a0, sn, ts))


def _stack(datasets):
    return tuple(torch.stack(ts) for ts in zip(*datasets))


def _batch(ds):
    s0, a0, sn, ts = ds
    return s0, a0, ts, sn - s0


def _twins(models):
    return [copy.deepcopy(m) for m in models]


def _assert_params_equal(models, twins, what=""):
    for i, (m, t) in enumerate(zip(models, twins)):
        for (k, p), q in zip(m.named_parameters(), t.parameters()):
            assert torch.equal(p, q), f"{what} member {i} {k}"


def _assert_grads_equal(models, twins):
    for i, (m, t) in enumerate(zip(models, twins)):
        for (k, p), q in zip(m.named_parameters(), t.parameters()):
            assert p.grad is not None and torch.equal(p.grad, q.grad), f"member {i} grad {k}"


def _assert_states_equal(sds, singles):
    for i, (sd, tr) in enumerate(zip(sds, singles)):
        ref = tr.state_dict() if hasattr(tr, "state_dict") else tr
        assert sd["state"].keys() == ref["state"].keys()
        for j in sd["state"]:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(sd["state"][j][key].cpu(), ref["state"][j][key].cpu()), f"member {i} param {j} {key}"


def _check_loss_grad_steps(group_cls, single_cls, models, stacked, datasets, steps=5):
    """loss_and_grad, then `steps` step()s: losses, gradients, parameters and both moments equal the singles'."""
    twins = _twins(models)
    grp = group_cls(models)
    singles = [single_cls(t) for t in twins]
    assert grp.fused and all(s.fused for s in singles) and grp.models == models
    gb = _batch(_stack(datasets)) if stacked else _batch(datasets[0])
    sb = [_batch(ds) for ds in datasets] if stacked else [_batch(datasets[0])] * len(models)
    loss = grp.loss_and_grad(*gb)
    ref = torch.stack([s.loss_and_grad(*b) for s, b in zip(singles, sb)])
    assert loss.shape == (len(models),) and torch.equal(loss, ref)
    _assert_grads_equal(models, twins)
    for _ in range(steps):
        loss = grp.step(*gb)
        ref = torch.stack([s.step(*b) for s, b in zip(singles, sb)])
        assert torch.equal(loss, ref)
    _assert_params_equal(models, twins, "after steps")
    _assert_states_equal(grp.state_dict(), singles)
    return grp, singles


def _check_run(group_cls, single_cls, models, ds, perms, bs):
    twins = _twins(models)
    grp = group_cls(models)
    singles = [single_cls(t) for t in twins]
    losses = grp.run(*ds, perms, batch_size=bs)
    ref = torch.stack([s.run(*ds, perms[i], batch_size=bs) for i, s in enumerate(singles)])
    assert losses.shape == (len(models), perms.shape[1] // bs) and losses.is_cuda
    assert torch.equal(losses, ref)
    _assert_params_equal(models, twins, "after run")
    return grp, twins


# ---------------------------------------------------------------------------------------------------------------- 1, 2
def test_nl_stacked_loss_grad_and_steps_equal_singles(nlc):
    """M = 3, N = 37 (three tiles, the last ragged), different seeds and different datasets."""
    models = [_nl_model(nlc, s) for s in (1, 2, 3)]
    _check_loss_grad_steps(nlc.NLTrainerGroup, nlc.NLTrainer, models, True, [_data(37, seed=20 + i) for i in range(3)])


@pytest.mark.parametrize("bs", [7, 16])
def test_nl_shared_dataset_run_equals_singles(nlc, bs):
    """(3, L) permutations with duplicates over one dataset, 20 iterations."""
    ds = _data(50)
    perms = torch.randint(0, 50, (3, 20 * bs), generator=torch.Generator().manual_seed(bs))
    _check_run(nlc.NLTrainerGroup, nlc.NLTrainer, [_nl_model(nlc, s) for s in (1, 2, 3)], ds, perms, bs)


def test_shared_permutation_and_identical_members_give_identical_rows(nlc):
    ds = _data(50)
    models = [_nl_model(nlc, 4) for _ in range(3)]
    losses = nlc.NLTrainerGroup(models).run(*ds, torch.randperm(50, generator=torch.Generator().manual_seed(0)), batch_size=7)
    assert losses.shape == (3, 7)
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2])
    _assert_params_equal(models[1:], [models[0]] * 2)


@pytest.mark.parametrize("family", ["nl", "rnn", "rnn_no_ts"])
def test_run_on_stacked_datasets_equals_singles(nlc, family):
    """run() with a dataset per member (data_row_stride > 0, the [iters][M][bs] index array): 30 rows each, batch 7 (a
    ragged tile), permutations with duplicates.  An RNN takes no ts: the group accepts None as the single trainer does."""
    M, bs = 3, 7
    if family == "nl":
        models, G, S_ = [_nl_model(nlc, s) for s in (1, 2, 3)], nlc.NLTrainerGroup, nlc.NLTrainer
    else:
        cls = "RNN" if family == "rnn_no_ts" else "DeltaTRNN"
        models, G, S_ = [_rnn_model(nlc, s, cls) for s in (1, 2, 3)], nlc.RNNTrainerGroup, nlc.RNNTrainer
    twins = _twins(models)
    sets = [_data(30, seed=40 + i) for i in range(M)]
    s0, a0, sn, ts = _stack(sets)
    perms = torch.randint(0, 30, (M, 6 * bs), generator=torch.Generator().manual_seed(3))
    losses = G(models).run(s0, a0, sn, None if family == "rnn_no_ts" else ts, perms, batch_size=bs)
    ref = torch.stack([S_(t).run(*sets[i], perms[i], batch_size=bs) for i, t in enumerate(twins)])
    assert losses.shape == (M, 6) and torch.equal(losses, ref)
    _assert_params_equal(models, twins, "after a stacked run")
    if family == "rnn_no_ts":  # step() on stacked batches without ts
        b = _batch((s0, a0, sn, ts))
        loss = G(models).step(b[0], b[1], None, b[3])
        ref = torch.stack([S_(t).step(*_batch(sets[i])) for i, t in enumerate(twins)])
        assert torch.equal(loss, ref)
        _assert_params_equal(models, twins, "after a stacked step without ts")


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_tile_walk_inside_a_group(nlc, family):
    """N = 2100: 132 tiles, more than kMaxBlocks = 128 workgroups, so workgroups 0..3 of every member walk two tiles."""
    if family == "nl":
        models, G, S_ = [_nl_model(nlc, s) for s in (1, 2)], nlc.NLTrainerGroup, nlc.NLTrainer
    else:
        models, G, S_ = [_rnn_model(nlc, s) for s in (1, 2)], nlc.RNNTrainerGroup, nlc.RNNTrainer
    twins = _twins(models)
    b = _batch(_data(2100))
    loss = G(models).loss_and_grad(*b)
    ref = torch.stack([S_(t).loss_and_grad(*b) for t in twins])
    assert torch.equal(loss, ref)
    _assert_grads_equal(models, twins)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("cls,H,d,B,M,N", [("DeltaTRNN", 64, 3, 3, 3, 20), ("DeltaTRNN", 160, 5, 4, 2, 16), ("RNN", 64, 3, 2, 2, 20)])
def test_rnn_family_steps_and_run_equal_singles(nlc, cls, H, d, B, M, N):
    mk = lambda: [_rnn_model(nlc, 1 + i, cls, d=d, H=H) for i in range(M)]  # noqa: E731
    _check_loss_grad_steps(nlc.RNNTrainerGroup, nlc.RNNTrainer, mk(), True, [_data(N, d=d, B=B, seed=30 + i) for i in range(M)])
    ds = _data(40, d=d, B=B)
    perms = torch.randint(0, 40, (M, 20 * 7), generator=torch.Generator().manual_seed(H))
    _check_run(nlc.RNNTrainerGroup, nlc.RNNTrainer, mk(), ds, perms, 7)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_more_members_than_compute_units(nlc):
    M = 260
    models = [_nl_model(nlc, 100 + i) for i in range(M)]
    twins = {i: copy.deepcopy(models[i]) for i in (0, 129, 259)}
    b = _batch(_data(16, B=1))
    loss = nlc.NLTrainerGroup(models).step(*b)
    assert loss.shape == (M,) and bool(torch.isfinite(loss).all())
    assert len(set(loss.tolist())) == M, "the members' losses must be pairwise distinct"
    for i, t in twins.items():
        assert torch.equal(nlc.NLTrainer(t).step(*b), loss[i]), i
        _assert_params_equal([models[i]], [t], f"member {i}")


# ---------------------------------------------------------------------------------------------------------------- 6
def test_member_independence(nlc):
    """The same member in a group of 2 and a group of 5, with different neighbours: identical bits."""
    b = _batch(_data(37))
    out = []
    for seeds, pos in (((9, 1), 0), ((2, 3, 9, 4, 5), 2)):
        models = [_nl_model(nlc, s) for s in seeds]
        grp = nlc.NLTrainerGroup(models)
        loss = grp.loss_and_grad(*b)[pos].clone()
        grads = [p.grad.clone() for p in models[pos].parameters()]
        grp.step(*b)
        out.append((loss, grads, [p.detach().clone() for p in models[pos].parameters()]))
    (l2, g2, w2), (l5, g5, w5) = out
    assert torch.equal(l2, l5)
    assert all(torch.equal(a, c) for a, c in zip(g2, g5)) and all(torch.equal(a, c) for a, c in zip(w2, w5))


# ---------------------------------------------------------------------------------------------------------------- 7
def test_optimiser_state_round_trip_and_real_adam_states(nlc):
    b = _batch(_data(20))
    models = [_nl_model(nlc, s) for s in (1, 2)]
    grp = nlc.NLTrainerGroup(models)
    for _ in range(2):
        grp.step(*b)
    sds = grp.state_dict()
    assert isinstance(sds, list) and len(sds) == 2
    grp2 = nlc.NLTrainerGroup(_twins(models))
    grp2.load_state_dict(sds)
    _assert_states_equal(grp2.state_dict(), sds)
    assert torch.equal(grp.step(*b), grp2.step(*b))
    _assert_params_equal(grp.models, grp2.models)

    # states of real torch.optim.Adam objects, then one step: equals the singles
    models = [_nl_model(nlc, s) for s in (3, 4)]
    twins, opts = _twins(models), []
    for m in models:
        opt = torch.optim.Adam(m.parameters(), lr=3e-4, betas=(0.8, 0.99), eps=1e-7)
        for _ in range(2):
            opt.zero_grad()
            torch.nn.functional.mse_loss(m(b[0], b[1], b[2]).squeeze(), b[3].squeeze()).backward()
            opt.step()
        opts.append(opt)
    for m, t in zip(models, twins):
        t.load_state_dict(m.state_dict())
    grp, singles = nlc.NLTrainerGroup(models), [nlc.NLTrainer(t) for t in twins]
    grp.load_state_dict([o.state_dict() for o in opts])
    for s, o in zip(singles, opts):
        s.load_state_dict(o.state_dict())
    assert grp.lr == 3e-4 and grp.betas == (0.8, 0.99)
    assert torch.equal(grp.step(*b), torch.stack([s.step(*b) for s in singles]))
    _assert_params_equal(models, twins)
    _assert_states_equal(grp.state_dict(), singles)


def test_unequal_step_counts_and_amsgrad_are_refused(nlc):
    b = _batch(_data(20))
    models = [_nl_model(nlc, s) for s in (1, 2)]
    one = nlc.NLTrainer(copy.deepcopy(models[0]))
    one.step(*b)
    two = nlc.NLTrainer(copy.deepcopy(models[1]))
    two.step(*b)
    two.step(*b)
    grp = nlc.NLTrainerGroup(models)
    with pytest.raises(ValueError, match="step count"):
        grp.load_state_dict([one.state_dict(), two.state_dict()])
    assert grp.state_dict()[0]["state"] == {}, "a refused list leaves the group's state alone"
    ams = [torch.optim.Adam(m.parameters(), amsgrad=True).state_dict() for m in models]
    with pytest.raises(ValueError, match="amsgrad"):
        grp.load_state_dict(ams)
    lrs = [torch.optim.Adam(m.parameters(), lr=lr).state_dict() for m, lr in zip(models, (1e-3, 1e-4))]
    with pytest.raises(ValueError, match="hyper-parameters"):
        grp.load_state_dict(lrs)


# ---------------------------------------------------------------------------------------------------------------- 8
def test_equality_rule(nlc):
    with pytest.raises(ValueError, match="member 1"):
        nlc.NLTrainerGroup([_nl_model(nlc, 1), _nl_model(nlc, 2, h=128)])
    odd = _nl_model(nlc, 3)
    with torch.no_grad():
        odd.state_std.mul_(2.0)
    with pytest.raises(ValueError, match="member 2.*state_std"):
        nlc.NLTrainerGroup([_nl_model(nlc, 1), _nl_model(nlc, 2), odd])
    with pytest.raises(ValueError, match="member 1.*class"):
        nlc.RNNTrainerGroup([_rnn_model(nlc, 1), _rnn_model(nlc, 2, "RNN")])

    b = _batch(_data(20))
    models = [_nl_model(nlc, s) for s in (1, 2)]
    twins = _twins(models)
    grp = nlc.NLTrainerGroup(models)
    grp.step(*b)
    with torch.no_grad():
        models[1].state_std.mul_(2.0)
    for call in (grp.step, grp.loss_and_grad):
        with pytest.raises(ValueError, match="member 1.*state_std"):
            call(*b)
    # all members changed consistently: the new constants take effect (the singles re-read theirs too)
    with torch.no_grad():
        models[0].state_std.mul_(2.0)
        for t in twins:
            t.state_std.mul_(2.0)
    singles = [nlc.NLTrainer(t) for t in twins]
    for t, m in zip(twins, models):
        t.load_state_dict(m.state_dict())
    before = torch.stack([p.detach().clone() for p in models[0].parameters()][:1])
    assert torch.equal(grp.loss_and_grad(*b), torch.stack([s.loss_and_grad(*b) for s in singles]))
    _assert_grads_equal(models, twins)
    assert torch.equal(before, torch.stack([p.detach() for p in models[0].parameters()][:1])), "loss_and_grad updates nothing"


# ---------------------------------------------------------------------------------------------------------------- 9
def _grad_mode_loop(models, b, steps, **adam):
    out = []
    for m in models:
        opt, mine = torch.optim.Adam(m.parameters(), lr=1e-4, **adam), []
        for _ in range(steps):
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(m(b[0], b[1], b[2]).squeeze(), b[3].squeeze())
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 0.1)
            opt.step()
            mine.append(loss.detach())
        out.append(torch.stack(mine))
    return torch.stack(out)


@pytest.mark.parametrize("family", ["dehoog", "rnn96"])
def test_unsupported_family_falls_back_with_one_warning(nlc, family):
    if family == "dehoog":
        models, G = [_nl_model(nlc, s, algo="dehoog") for s in (1, 2)], nlc.NLTrainerGroup
    else:
        models, G = [_rnn_model(nlc, s, H=96) for s in (1, 2)], nlc.RNNTrainerGroup
    twins = _twins(models)
    b = _batch(_data(12))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        grp = G(models)
        losses = torch.stack([grp.step(*b) for _ in range(2)], dim=1)
    assert len([x for x in w if "grad-mode" in str(x.message)]) == 1
    assert grp.fused is False and losses.shape == (2, 2)
    assert torch.equal(losses, _grad_mode_loop(twins, b, 2))
    _assert_params_equal(models, twins)
    assert len(grp.state_dict()) == 2


def test_refused_call_runs_grad_mode_on_the_shared_state(nlc):
    """B = 17 on a fused group: one warning, the grad-mode path member by member, the step count stays consistent."""
    models = [_nl_model(nlc, s) for s in (1, 2)]
    twins = _twins(models)
    b16, b17 = _batch(_data(12, B=16)), _batch(_data(12, B=17))
    grp, singles = nlc.NLTrainerGroup(models), [nlc.NLTrainer(t) for t in twins]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got, ref = [], []
        for b in (b16, b17, b17, b16):
            got.append(grp.step(*b))
            ref.append(torch.stack([s.step(*b) for s in singles]))
    assert len([x for x in w if "NLTrainerGroup" in str(x.message)]) == 1
    assert grp.fused and torch.equal(torch.stack(got), torch.stack(ref))
    _assert_params_equal(models, twins)
    sds = grp.state_dict()
    assert all(float(sd["state"][0]["step"]) == 4.0 for sd in sds)
    _assert_states_equal(sds, singles)


def test_empty_batch_raises(nlc):
    grp = nlc.NLTrainerGroup([_nl_model(nlc, s) for s in (1, 2)])
    s0, a0, ts, tgt = _batch(_data(4))
    with pytest.raises(nlc._lib.NlcError):
        grp.step(s0[:0], a0[:0], ts[:0], tgt[:0])


def test_abi_refuses_bad_member_counts(nlc):
    """M < 1: NLC_ERR_BAD_SHAPE; M past the grid's y limit: NLC_ERR_UNSUPPORTED; both before any launch."""
    import ctypes as C

    tr = nlc.NLTrainer(_nl_model(nlc, 1))
    obs, win, tsd, tgt = tr._data(*_batch(_data(4)))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ctx, buf = tr._ctx, torch.zeros(tr._flat.numel(), dtype=torch.float64, device="cuda")
    for M, code in ((0, -2), (65536, nlc._lib.NLC_ERR_UNSUPPORTED)):  # include/nlc.h: NLC_ERR_BAD_SHAPE is -2
        rc = ctx.lib.nlc_train_group_loss_grad(ctx.h, M, 0, p(buf), p(obs), p(win), p(tsd), p(tgt), p(tr._idx(4)), 4,
                                               win.shape[1], p(buf), p(buf), p(tr._workspace(4)))
        assert rc == code, (M, rc)
        assert ctx.lib.nlc_train_group_workspace_bytes(ctx.h, M, 4) == -1


# ---------------------------------------------------------------------------------------------------------------- 10
def test_write_back_and_repeatability(nlc):
    ds = _data(50)
    perms = torch.randint(0, 50, (2, 70), generator=torch.Generator().manual_seed(5))
    init = [_nl_model(nlc, s) for s in (1, 2)]
    runs = []
    for _ in range(2):
        models = _twins(init)
        losses = nlc.NLTrainerGroup(models).run(*ds, perms, batch_size=7)
        runs.append((losses, models))
    assert torch.equal(runs[0][0], runs[1][0])
    _assert_params_equal(runs[0][1], runs[1][1], "two runs")
    twins = _twins(init)
    for i, t in enumerate(twins):
        nlc.NLTrainer(t).run(*ds, perms[i], batch_size=7)
    s0, a0, _, ts = ds
    with torch.no_grad():
        for m, t in zip(runs[0][1], twins):
            assert torch.equal(m(s0, a0, ts), t(s0, a0, ts))
