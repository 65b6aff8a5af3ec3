"""GPU: per-member settings and patience of the trainer groups (nlc_*_train_group_step_members, nlc_train_patience) -- a group
with a learning rate, weight decay and clip norm per member against single trainers built with those scalars, bit for bit; a
sequence of equal numbers against the scalar group; frozen rows as int64 bit patterns with NaN-payload sentinels in the
moments; a frozen member whose gradient is NaN; ``fit(patience=)`` against a host loop written here from ``run``,
``evaluate``, ``.item()``, the reference's counter (train_utils.py:439-448) and ``freeze``; the refusals.

Shapes are the smallest the families take, 37 rows (three tiles, the last ragged) and M = 3: NL h = 64, S = 3, d = 3, window 2
(tensors of 96 and of 3 072 elements: shorter and longer than one 1 024-element Adam chunk), RNN H = 64 (192 and 12 288), NODE
H = 17 with (d, aug, nu) = (3, 0, 1) and rows of 1, 2 and 3 Euler sub-steps."""

import copy
import ctypes as C

import numpy as np
import pytest
import torch
from gpu_common import build_node
from test_gpu_train import _gen_model, _gen_setup
from test_gpu_train_node import DT
from test_gpu_train_node import PARAMS as NODE_PARAMS
from test_gpu_train_node import _setup as _node_setup
from test_gpu_train_rnn import _model as _rnn_model
from test_gpu_train_rnn import _setup as _rnn_setup

pytestmark = pytest.mark.gpu

M, N = 3, 37
LR, WD, CLIP = (1e-4, 3e-4, 1e-3), (0.0, 1e-2, 0.0), (0.1, 1.0, 0.0)
SENTINEL = 0x7FF8_0000_0000_0001  # a quiet NaN whose payload is 1 + the element's index
BAD_ARG, BAD_SHAPE, UNSUPPORTED = -1, -2, -4
FAMILIES = ["nl", "nl_talbot", "rnn", "node"]
NAN, INF = float("nan"), float("inf")


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


def _share_buffers(models):
    """A group shares the descriptor: member 0's normalisation buffers for all."""
    sd0 = models[0].state_dict()
    for mdl in models[1:]:
        mdl.load_state_dict({k: (sd0[k] if k in dict(mdl.named_buffers()) else v) for k, v in mdl.state_dict().items()})


def _family(nlc, family, rows=N, seed=40, members=M):
    """(Single, Group, models, (s0, a0, ts, target) on the device, extra constructor arguments)."""
    if family in ("nl", "nl_talbot"):
        algo = "fourier" if family == "nl" else "fixed_tablot"
        models, data = [], None
        for m in range(members):
            sd, dm = _gen_setup(3, 1, False, 64, 3, 2, rows, seed=seed + m)
            models.append(_gen_model(nlc, sd, 3, 1, False, 64, 3, algo=algo))
            data = dm if data is None else data
        _share_buffers(models)
        return nlc.NLTrainer, nlc.NLTrainerGroup, models, _cuda(*data), {}
    if family == "rnn":
        models, data = [], None
        for m in range(members):
            sd, (s0, a0, sn, ts) = _rnn_setup("DeltaTRNN", 3, 1, 64, rows, 2, seed=seed + m)
            models.append(_rnn_model(nlc, "DeltaTRNN", sd, 3, 1, 64))
            data = (s0, a0, ts, sn - s0) if data is None else data
        _share_buffers(models)
        return nlc.RNNTrainer, nlc.RNNTrainerGroup, models, _cuda(*data), {}
    from oracle import node_model as on

    sd, (s0, a0, sn, _) = _node_setup(17, 3, 0, 1, rows, seed=seed, B=2, out_scale=1.0)
    models = []
    for m in range(members):
        sdm = dict(sd)
        sdm.update({k: v for k, v in on.make_synthetic_state_dict(seed + 10 * m, 3, 1, 17, 0, None, None, DT, 1.0).items()
                    if k in NODE_PARAMS})
        models.append(build_node(nlc, sdm, 17, 0))
    # raw times whose normalised end (/ 0.4) takes 3, 1 and 2 Euler sub-steps of 0.05; each row integrates to its own
    ts = torch.tensor([0.05, 0.012, 0.03], dtype=torch.float64)[torch.arange(rows) % 3].view(rows, 1)
    return nlc.NODETrainer, nlc.NODETrainerGroup, models, _cuda(s0, a0, ts, sn - s0), {"row_times": True}


def _singles(Single, models, kw, lr=LR, wd=WD, clip=CLIP):
    pick = lambda v, i: v[i] if isinstance(v, tuple) else v  # noqa: E731
    return [Single(copy.deepcopy(m), lr=pick(lr, i), weight_decay=pick(wd, i), clip_grad_norm=pick(clip, i), **kw)
            for i, m in enumerate(models)]


def _bits(t):
    return t.detach().contiguous().view(torch.int64).clone()


def _assert_member_equals(grp, i, tr, what=""):
    for p, q in zip(grp.models[i].parameters(), tr.model.parameters()):
        assert torch.equal(p, q), (what, i, "params")
    assert torch.equal(grp._m[i], tr._m[0]), (what, i, "exp_avg")
    assert torch.equal(grp._v[i], tr._v[0]), (what, i, "exp_avg_sq")


def _run_args(data, length, seed):
    s0, a0, ts, tgt = data
    perm = torch.randint(0, s0.shape[0], (length,), generator=torch.Generator().manual_seed(seed)).cuda()
    return (s0, a0, s0 + tgt, ts, perm)


# ---------------------------------------------------------------------------------------------------------------------
# 1. a group with per-member settings against single trainers with those scalars
@pytest.mark.parametrize("family", FAMILIES)
def test_members_equal_their_single_trainers(nlc, family):
    """Five step() calls on the 37 rows, then a run() of 8 iterations at batch 7: losses, parameters, exp_avg and exp_avg_sq
    torch.equal.  Member 0 clips at 0.1, member 1 clips at 1.0 and decays, member 2 does neither."""
    Single, Group, models, data, kw = _family(nlc, family)
    singles = _singles(Single, models, kw)
    grp = Group(models, lr=list(LR), weight_decay=WD, clip_grad_norm=np.array(CLIP), **kw)
    assert grp.fused and grp._per_member()
    assert grp.lr == LR and grp.weight_decay == WD and grp.clip_grad_norm == CLIP
    for k in range(5):
        gl = grp.step(*data)
        for i, tr in enumerate(singles):
            assert torch.equal(gl[i], tr.step(*data)), (k, i)
    for i, tr in enumerate(singles):
        _assert_member_equals(grp, i, tr, "after step()")
    run = _run_args(data, 8 * 7, seed=3)
    gl = grp.run(*run, 7)
    assert gl.shape == (M, 8)
    for i, tr in enumerate(singles):
        assert torch.equal(gl[i], tr.run(*run, 7)), i
        _assert_member_equals(grp, i, tr, "after run()")
    assert grp._step == 13 and all(tr._step == 13 for tr in singles)
    # the members' settings did act: the same start under other settings ends elsewhere
    assert not torch.equal(grp._m[0], grp._m[1])
    sds = grp.state_dict()
    assert [sd["param_groups"][0]["lr"] for sd in sds] == list(LR)
    assert [sd["param_groups"][0]["weight_decay"] for sd in sds] == list(WD)
    # assigning takes effect at the next call: a number again, and the group is the scalar group
    grp.lr, grp.weight_decay, grp.clip_grad_norm = 2e-4, 0.0, 0.1
    assert not grp._per_member() and grp.lr == 2e-4
    for tr in singles:
        tr.lr, tr.weight_decay, tr.clip_grad_norm = 2e-4, 0.0, 0.1
    gl = grp.step(*data)
    for i, tr in enumerate(singles):
        assert torch.equal(gl[i], tr.step(*data)), i
        _assert_member_equals(grp, i, tr, "after the scalars came back")


# ---------------------------------------------------------------------------------------------------------------------
# 2. a sequence of equal numbers is the scalar group
@pytest.mark.parametrize("family", FAMILIES)
def test_a_sequence_of_equal_numbers_is_the_scalar_group(nlc, family):
    _, Group, models, data, kw = _family(nlc, family)
    seq = Group([copy.deepcopy(m) for m in models], lr=[1e-4] * M, **kw)
    one = Group(models, lr=1e-4, **kw)
    assert seq._per_member() and not one._per_member()
    for k in range(5):
        assert torch.equal(seq.step(*data), one.step(*data)), k
    for a, b in ((seq._flat, one._flat), (seq._m, one._m), (seq._v, one._v)):
        assert torch.equal(a, b)
    for ma, mb in zip(seq.models, one.models):
        for p, q in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(p, q)


# ---------------------------------------------------------------------------------------------------------------------
# 3. frozen rows are not written
@pytest.mark.parametrize("family", FAMILIES)
def test_frozen_rows_are_not_written(nlc, family):
    Single, Group, models, data, kw = _family(nlc, family)
    singles = _singles(Single, models, kw, lr=1e-3, wd=0.0, clip=0.1)
    grp = Group(models, lr=1e-3, **kw)
    grp.step(*data)
    for tr in singles:
        tr.step(*data)
    assert not grp._per_member() and bool(grp.active.all())
    grp.freeze([False, True, False])
    assert grp._per_member() and grp.active.tolist() == [True, False, True] and grp.active.is_cuda
    P = grp._m.shape[1]
    kept_m = grp._m[1].clone()
    # distinct NaN payloads in the first half of member 1's exp_avg: a rewrite through arithmetic would quiet or merge them
    grp._m[1, : P // 2] = (torch.arange(P // 2, dtype=torch.int64) + SENTINEL).view(torch.float64).cuda()
    before = [_bits(grp._flat[1]), _bits(grp._m[1]), _bits(grp._v[1])]
    for k in range(3):
        gl = grp.step(*data)
        # member 1's loss is still reported, on the weights it was frozen with
        assert torch.equal(gl[1], singles[1].loss_and_grad(*data)), k
        for i in (0, 2):
            assert torch.equal(gl[i], singles[i].step(*data)), (k, i)
    for got, want, what in zip((grp._flat[1], grp._m[1], grp._v[1]), before, ("params", "exp_avg", "exp_avg_sq")):
        assert torch.equal(_bits(got), want), what
    for p, q in zip(grp.models[1].parameters(), singles[1].model.parameters()):
        assert torch.equal(p, q)
    for i in (0, 2):
        _assert_member_equals(grp, i, singles[i], "beside a frozen member")
    steps = [int(sd["state"][0]["step"]) for sd in grp.state_dict()]
    assert steps == [4, 1, 4]  # a frozen member's step is the count it stopped at
    # unfreeze (a device mask): member 1 steps again, with the group's step count
    grp._m[1].copy_(kept_m)
    grp.unfreeze(torch.tensor([False, True, False]).cuda())
    assert bool(grp.active.all())
    singles[1]._step = grp._step
    gl = grp.step(*data)
    for i, tr in enumerate(singles):
        assert torch.equal(gl[i], tr.step(*data)), i
        _assert_member_equals(grp, i, tr, "after unfreeze")
    assert grp._step == 5 and [int(sd["state"][0]["step"]) for sd in grp.state_dict()] == [5, 5, 5]


# ---------------------------------------------------------------------------------------------------------------------
# 4. a frozen member with a NaN gradient does not leak
def test_a_frozen_member_with_nan_times_does_not_leak(nlc):
    """NODE, stacked data: the group's own host check reads the times once, while they are valid; then the frozen member's
    rows of ts become NaN under it (a write through ``.data`` moves no version).  The kernels give such rows a NaN squared
    error: member 1 reports NaN and keeps its rows; the others' bits equal their single trainers'."""
    Single, Group, models, (s0, a0, ts, tgt), kw = _family(nlc, "node", rows=M * N)
    stack = lambda t: t.reshape((M, N) + tuple(t.shape[1:]))  # noqa: E731
    s0, a0, ts, tgt = stack(s0), stack(a0), stack(ts).clone(), stack(tgt)
    singles = _singles(Single, models, kw, lr=1e-3, wd=0.0, clip=0.1)
    grp = Group(models, lr=1e-3, **kw)
    gl = grp.step(s0, a0, ts, tgt)
    for i, tr in enumerate(singles):
        assert torch.equal(gl[i], tr.step(s0[i], a0[i], ts[i].clone(), tgt[i])), i
    grp.freeze(torch.tensor([False, True, False]))
    seen = dict(grp._ts_seen)
    ts.data[1].fill_(NAN)
    before = [_bits(grp._flat[1]), _bits(grp._m[1]), _bits(grp._v[1])]
    for k in range(2):
        gl = grp.step(s0, a0, ts, tgt)
        assert grp._ts_seen == seen  # the host check was the group's own, made once
        assert bool(torch.isnan(gl[1])) and bool(torch.isfinite(gl[[0, 2]]).all())
        for i in (0, 2):
            assert torch.equal(gl[i], singles[i].step(s0[i], a0[i], ts[i].clone(), tgt[i])), (k, i)
    for got, want in zip((grp._flat[1], grp._m[1], grp._v[1]), before):
        assert torch.equal(_bits(got), want)
    for i in (0, 2):
        _assert_member_equals(grp, i, singles[i], "beside a NaN member")
        assert all(bool(torch.isfinite(p).all()) for p in grp.models[i].parameters())
    assert all(bool(torch.isfinite(p).all()) for p in grp.models[1].parameters())


# ---------------------------------------------------------------------------------------------------------------------
# 5. fit with patience against a host loop
FIT_LR = (1e-3, 0.5, 1e-3)
PATIENCE, EPOCHS, BS, EVERY, ROWS, SEED = 1, 4, 4, 2, 40, 5  # 40 rows: 5 slices of 8 indices per epoch, 20 checks


def _host_fit(grp, train, val):
    """The loop a user writes today: the M criteria read on the host at every check, the parameters cloned on improvement,
    the reference's counter (train_utils.py:439-448) per member, ``freeze`` for a member that stops."""
    s0, a0, sn, ts = train
    best, best_iter, best_params = [INF] * M, [-1] * M, [None] * M
    waiting, active, stopped_at = [0] * M, [True] * M, [-1] * M
    done, train_loss, criterion = 0, [], []
    for epoch in range(EPOCHS):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(SEED + epoch)
        perm = torch.randperm(ROWS, device="cuda", generator=gen)
        for chunk in perm.split(EVERY * BS):
            losses = grp.run(s0, a0, sn, ts, chunk, BS)
            done += chunk.numel() // BS
            crit = grp.evaluate(*val)
            for m in range(M):
                if not active[m]:
                    continue  # the reference has left its loop
                c = crit[m].item()
                if c < best[m]:
                    best[m], best_iter[m], waiting[m] = c, done, 0
                    best_params[m] = [p.detach().clone() for p in grp.models[m].parameters()]
                elif waiting[m] > PATIENCE:
                    active[m], stopped_at[m] = False, done
                    grp.freeze([k == m for k in range(M)])
                else:
                    waiting[m] += 1
            train_loss.append(losses)
            criterion.append(crit)
    final = [[p.detach().clone() for p in mdl.parameters()] for mdl in grp.models]
    return torch.cat(train_loss, dim=-1), torch.stack(criterion, dim=-1), best, best_iter, best_params, active, stopped_at, final


def test_fit_with_patience_equals_the_host_loop(nlc):
    """RNN H = 64, M = 3, lr (1e-3, 0.5, 1e-3), 20 checks two iterations apart, patience 1, a validation set of 37 rows.  On
    the MI355X the two members at 1e-3 overfit the 40 training rows after two to five iterations and stop at iterations 8 and
    10; the member at 0.5 starts from a criterion near 65 and keeps finding lower ones, so it stays active to the end."""
    _, Group, models, _, kw = _family(nlc, "rnn")
    _, (s0, a0, sn, ts) = _rnn_setup("DeltaTRNN", 3, 1, 64, ROWS, 2, seed=100)
    train = _cuda(s0, a0, sn, ts)
    _, (v0, va, vn, vt) = _rnn_setup("DeltaTRNN", 3, 1, 64, N, 2, seed=200)
    val = _cuda(v0, va, vt, vn - v0)
    host = Group([copy.deepcopy(m) for m in models], lr=FIT_LR)
    ref_train, ref_crit, best, best_iter, best_params, active, stopped_at, final = _host_fit(host, train, val)
    print("criterion", ref_crit.tolist(), "best_iter", best_iter, "active", active, "stopped_at", stopped_at)
    assert ref_crit.shape == (M, 20)

    grp = Group(models, lr=FIT_LR)
    out = grp.fit(train, val, epochs=EPOCHS, batch_size=BS, eval_every=EVERY, seed=SEED, patience=PATIENCE, restore_best=False)
    assert out["active"].dtype == torch.bool and out["active"].is_cuda and out["stopped_at"].dtype == torch.int64
    assert out["active"].tolist() == active and out["stopped_at"].tolist() == stopped_at
    assert torch.equal(out["active"], grp.active)
    # not vacuous: a member stopped before the last check, and a member stayed active to the end
    assert any(0 < s < 40 for s in stopped_at) and any(active)
    assert all((s == -1) == a for s, a in zip(stopped_at, active))
    assert torch.equal(_bits(out["train_loss"]), _bits(ref_train)) and torch.equal(_bits(out["criterion"]), _bits(ref_crit))
    assert out["best_loss"].tolist() == best and out["best_iter"].tolist() == best_iter
    for m in range(M):
        for p, q in zip(grp.models[m].parameters(), final[m]):
            assert torch.equal(_bits(p), _bits(q)), m
    grp.restore_best()
    for m in range(M):
        for p, q in zip(grp.models[m].parameters(), best_params[m]):
            assert torch.equal(_bits(p), _bits(q)), m
    # patience=None returns what it always has
    plain = Group([copy.deepcopy(m) for m in models], lr=1e-3)
    assert sorted(plain.fit(train, val, batch_size=BS, eval_every=EVERY)) == ["best_iter", "best_loss", "criterion", "train_loss"]
    assert not plain._per_member()


def test_fit_with_patience_on_a_single_trainer(nlc):
    """M = 1 through the same code: an lr of 0.5 stops improving and stops; the weights then stay."""
    Single, _, models, _, _ = _family(nlc, "rnn", members=1)
    _, (s0, a0, sn, ts) = _rnn_setup("DeltaTRNN", 3, 1, 64, ROWS, 2, seed=100)
    train = _cuda(s0, a0, sn, ts)
    tr = Single(models[0], lr=0.5)
    out = tr.fit(train, None, epochs=EPOCHS, batch_size=BS, eval_every=EVERY, seed=SEED, patience=0, restore_best=False)
    print("criterion", out["criterion"].tolist(), "stopped_at", out["stopped_at"].item())
    assert out["active"].shape == () and out["stopped_at"].shape == ()
    stopped = out["stopped_at"].item()
    assert not out["active"].item() and 0 < stopped < 40 and stopped % EVERY == 0
    assert int(tr.state_dict()["state"][0]["step"]) == stopped


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
def test_refusals(nlc):
    from neurallaplacecontrol_amd import _lib

    _, Group, models, data, kw = _family(nlc, "rnn")
    with pytest.raises(ValueError, match="one per member"):
        Group(models, lr=[1e-4, 1e-3])
    with pytest.raises(ValueError, match="Invalid lr"):
        Group(models, lr=[1e-4, -1e-3, 1e-4])
    with pytest.raises(ValueError, match="Invalid weight_decay"):
        Group(models, weight_decay=-1.0)
    grp = Group(models, lr=list(LR))
    grp.step(*data)
    state = [_bits(grp._flat), _bits(grp._m), _bits(grp._v)]

    def unmoved(what):
        torch.cuda.synchronize()
        assert grp._step == 1 and grp.lr == LR, what
        for got, want in zip((grp._flat, grp._m, grp._v), state):
            assert torch.equal(_bits(got), want), what

    with pytest.raises(ValueError):
        grp.lr = [1e-4] * 4
    unmoved("wrong length")
    with pytest.raises(ValueError):
        grp.lr = (1e-4, 1e-4, -1.0)
    unmoved("negative lr")
    with pytest.raises(ValueError):
        grp.freeze([True, False])
    unmoved("mask of the wrong length")

    # the raw entry: a NULL struct, and each of the four arrays NULL in turn
    ctx = grp._ctx
    obs, win, ts, tgt, rows, stride = grp._group_data(*data)
    good = grp._members_arg()
    loss = torch.empty(M, dtype=torch.float64, device="cuda")

    def raw(members):
        with ctx.stream():
            return ctx.lib.nlc_rnn_train_group_step_members(
                ctx.h, C.byref(grp._desc()), M, stride, C.c_void_p(grp._flat.data_ptr()), C.c_void_p(grp._m.data_ptr()),
                C.c_void_p(grp._v.data_ptr()), grp._step + 1, C.c_void_p(obs.data_ptr()), C.c_void_p(win.data_ptr()),
                C.c_void_p(ts.data_ptr()), C.c_void_p(tgt.data_ptr()), C.c_void_p(grp._idx(rows).data_ptr()), rows, win.shape[1],
                C.c_void_p(loss.data_ptr()), None, C.c_void_p(grp._workspace(rows).data_ptr()), members)

    assert raw(None) == BAD_ARG
    unmoved("NULL struct")
    for field, _ in _lib.TrainMembers._fields_:
        bad = _lib.TrainMembers(good.lr_dev, good.wd_dev, good.max_norm_dev, good.active_dev)
        setattr(bad, field, None)
        assert raw(C.byref(bad)) == BAD_ARG, field
        assert ctx.lib.nlc_last_error(ctx.h)
        unmoved(field)

    # nlc_train_patience: no model needed; NULL pointers, M = 0, M = 65536
    bare = _lib.Ctx(0)
    improved = torch.zeros(M, dtype=torch.int32, device="cuda")
    waiting = torch.full((M,), 9, dtype=torch.int64, device="cuda")
    active = torch.ones(M, dtype=torch.int32, device="cuda")
    stopped = torch.full((M,), -1, dtype=torch.int64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def patience(m=M, imp=ptr(improved), w=ptr(waiting), a=ptr(active), s=ptr(stopped), p=1.0):
        with bare.stream():
            return bare.lib.nlc_train_patience(bare.h, m, imp, w, a, s, p, 7)

    assert patience(m=0) == BAD_SHAPE and patience(m=-1) == BAD_SHAPE and patience(m=65536) == UNSUPPORTED
    assert patience(imp=None) == BAD_ARG and patience(w=None) == BAD_ARG and patience(a=None) == BAD_ARG
    assert patience(s=None) == BAD_ARG and patience(p=NAN) == BAD_ARG
    torch.cuda.synchronize()
    assert waiting.tolist() == [9] * M and active.tolist() == [1] * M and stopped.tolist() == [-1] * M
    # and a call that is taken: waiting 9 > 1, nobody improved: every member stops with the tag
    assert patience() == 0
    torch.cuda.synchronize()
    assert active.tolist() == [0] * M and stopped.tolist() == [7] * M and waiting.tolist() == [9] * M
    unmoved("after the patience calls")
