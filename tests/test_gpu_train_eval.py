"""GPU: the held-out loss of the fused trainers (``evaluate`` / nlc_train_group_eval, nlc_rnn_train_group_eval) against the
float64 CPU oracle (oracle.nl_model.nl_forward / oracle.rnn_model + MSE), against the training forward, and for what a
forward-only call must leave alone.  The loss bound is the training loss's: 1e-12 relative (docs/training.md)."""

import copy
import warnings

import pytest
import torch
from test_gpu_train import _gen_model, _gen_setup
from test_gpu_train_rnn import _model as _rnn_model
from test_gpu_train_rnn import _setup as _rnn_setup

pytestmark = pytest.mark.gpu

TOL = 1e-12


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


def _close(got, ref, what=""):
    got, ref = got.detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    err = float(((got - ref).abs() / ref.abs()).max())
    print(f"{what}: rel err {err:.3e}")
    assert err <= TOL, f"{what}: rel err {err:.3e} > {TOL:g}"


def _nl_oracle(sd, data, S, normalize=True, normalize_time=True, algo="fourier", rows=None):
    from oracle import nl_model as onl

    s0, a0, ts, tgt = (t if rows is None else t[rows] for t in data)
    with torch.no_grad():
        pred = onl.nl_forward(sd, s0, a0, ts, S=S, normalize=normalize, normalize_time=normalize_time, ilt_algorithm=algo)
    return ((pred.reshape(tgt.shape) - tgt) ** 2).mean()


def _rnn_oracle(cls, sd, data, normalize=True, normalize_time=True, rows=None):
    from oracle import rnn_model as orn

    s0, a0, sn, ts = (t if rows is None else t[rows] for t in data)
    with torch.no_grad():
        pred = orn.forward(sd, s0, a0, ts, normalize, normalize_time) if cls == "DeltaTRNN" else orn.forward_rnn(sd, s0, a0, normalize)
    return ((pred - (sn - s0)) ** 2).mean()


def _rnn_args(data):
    s0, a0, sn, ts = data
    return s0, a0, ts, sn - s0


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the CPU oracle
# (algo, h, S, d, nu, enc, B, N, normalize, normalize_time, non-zero means)
NL_CASES = [
    ("fourier", 64, 3, 1, 1, False, 1, 1, True, True, False),
    ("fourier", 128, 17, 5, 1, True, 5, 37, True, True, False),  # nin = 2, ragged third tile
    ("fourier", 256, 33, 6, 1, False, 16, 2100, True, True, False),
    ("fixed_tablot", 64, 8, 5, 1, False, 4, 37, True, True, False),
    ("stehfest", 128, 12, 5, 1, False, 4, 37, True, True, False),
    ("fourier", 64, 5, 3, 1, False, 3, 19, False, False, False),
    ("fourier", 64, 5, 3, 2, False, 3, 19, True, True, True),
]


@pytest.mark.parametrize("case", NL_CASES, ids=[f"{c[0]}-h{c[1]}-S{c[2]}-d{c[3]}-B{c[6]}-N{c[7]}-n{int(c[8])}{int(c[10])}" for c in NL_CASES])
def test_nl_evaluate_vs_oracle(nlc, case):
    algo, h, S, d, nu, enc, B, N, normalize, normalize_time, mean = case
    sd, data = _gen_setup(d, nu, enc, h, S, B, N, normalize, normalize_time, mean, seed=h + S)
    ref = _nl_oracle(sd, data, S, normalize, normalize_time, algo)
    tr = nlc.NLTrainer(_gen_model(nlc, sd, d, nu, enc, h, S, normalize, normalize_time, algo=algo))
    loss = tr.evaluate(*_cuda(*data))
    assert loss.shape == () and loss.dtype == torch.float64 and loss.is_cuda
    _close(loss, ref, "NL evaluate vs oracle")


# (class, d, nin, H, N, B)
RNN_CASES = [
    ("DeltaTRNN", 1, 1, 64, 1, 1),
    ("DeltaTRNN", 8, 3, 128, 37, 16),
    ("DeltaTRNN", 5, 1, 160, 4103, 4),
    ("RNN", 8, 1, 64, 37, 16),
    ("RNN", 1, 2, 128, 4103, 1),
    ("RNN", 5, 1, 160, 1, 4),
]


@pytest.mark.parametrize("case", RNN_CASES, ids=[f"{c[0]}-d{c[1]}-nin{c[2]}-H{c[3]}-N{c[4]}-B{c[5]}" for c in RNN_CASES])
def test_rnn_evaluate_vs_oracle(nlc, case):
    cls, d, nin, H, N, B = case
    sd, data = _rnn_setup(cls, d, nin, H, N, B, mean=True, seed=H + N)
    ref = _rnn_oracle(cls, sd, data)
    tr = nlc.RNNTrainer(_rnn_model(nlc, cls, sd, d, nin, H))
    loss = tr.evaluate(*_cuda(*_rnn_args(data)))
    assert loss.shape == () and loss.dtype == torch.float64
    _close(loss, ref, "RNN evaluate vs oracle")


# ---------------------------------------------------------------------------------------------------------------------
# shared fixtures for the rest: one NL and one RNN trainer with a 300-row dataset
def _nl_trainer(nlc, N=300, h=64, S=5, d=3, B=3, seed=11, algo="fourier"):
    sd, data = _gen_setup(d, 1, False, h, S, B, N, seed=seed)
    model = _gen_model(nlc, sd, d, 1, False, h, S, algo=algo)
    return nlc.NLTrainer(model), sd, data


def _rnn_trainer(nlc, cls="DeltaTRNN", N=300, H=64, d=3, B=3, seed=11):
    sd, data = _rnn_setup(cls, d, 1, H, N, B, seed=seed)
    return nlc.RNNTrainer(_rnn_model(nlc, cls, sd, d, 1, H)), sd, data


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_evaluate_agrees_with_the_training_forward(nlc, family):
    if family == "nl":
        tr, _, data = _nl_trainer(nlc, N=37, h=128, S=17, d=5, B=4)
        args = _cuda(*data)
    else:
        tr, _, data = _rnn_trainer(nlc, N=37, H=160, d=5, B=4)
        args = _cuda(*_rnn_args(data))
    ev = tr.evaluate(*args)
    _close(ev, tr.loss_and_grad(*args), "evaluate vs loss_and_grad")


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_indices(nlc, family):
    N = 300
    if family == "nl":
        tr, sd, data = _nl_trainer(nlc, N=N)
        args = _cuda(*data)
    else:
        tr, sd, data = _rnn_trainer(nlc, N=N)
        args = _cuda(*_rnn_args(data))
    assert torch.equal(tr.evaluate(*args), tr.evaluate(*args, indices=torch.arange(N)))
    g = torch.Generator().manual_seed(5)
    rows = torch.cat((torch.randint(0, N // 2, (40,), generator=g), torch.tensor([7, 7, N - 1, 0])))  # duplicates, gaps
    ref = _nl_oracle(sd, data, 5, rows=rows) if family == "nl" else _rnn_oracle("DeltaTRNN", sd, data, rows=rows)
    _close(tr.evaluate(*args, indices=rows.cuda()), ref, "gathered rows vs oracle")


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_deterministic_and_more_tiles_than_workgroups(nlc, family):
    """The grid is at most two workgroups per compute unit (nlc_train_eval.h eval_grid): N = 16 (2 CUs) + 37 rows leave
    workgroups with a second tile, the last tile ragged."""
    N = 16 * 2 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    if family == "nl":
        tr, sd, data = _nl_trainer(nlc, N=N, S=3, d=1, B=1)
        args, ref = _cuda(*data), _nl_oracle(sd, data, 3)
    else:
        tr, sd, data = _rnn_trainer(nlc, N=N, d=1, B=2)
        args, ref = _cuda(*_rnn_args(data)), _rnn_oracle("DeltaTRNN", sd, data)
    a, b = tr.evaluate(*args), tr.evaluate(*args)
    assert torch.equal(a, b)
    _close(a, ref, "walked grid vs oracle")


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_large_n_equals_the_weighted_mean_of_its_chunks(nlc, family):
    """N = 50 000 (3125 tiles) against ten 5 000-row chunks: both sides are evaluate's own, a grid-walk consistency check.
    Worst-case summation bound (3125 + 16 d) 2^-53 = 3.6e-13 < 1e-12."""
    N, C = 50_000, 5_000
    if family == "nl":
        tr, _, data = _nl_trainer(nlc, N=N, h=64, S=3, d=3, B=2)
        args = _cuda(*data)
    else:
        tr, _, data = _rnn_trainer(nlc, N=N, H=64, d=3, B=2)
        args = _cuda(*_rnn_args(data))
    whole = tr.evaluate(*args)
    parts = torch.stack([tr.evaluate(*args, indices=torch.arange(k * C, (k + 1) * C)) for k in range(N // C)])
    _close(whole, parts.mean(), "whole vs chunks")


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_evaluate_has_no_side_effects(nlc, family):
    if family == "nl":
        tr, _, data = _nl_trainer(nlc, N=37)
        args = _cuda(*data)
    else:
        tr, _, data = _rnn_trainer(nlc, N=37)
        args = _cuda(*_rnn_args(data))
    twin = type(tr)(copy.deepcopy(tr.model))  # never evaluates
    tr.step(*args)  # moments and a step count worth keeping
    twin.step(*args)
    tr.model.zero_grad()
    first = next(tr.model.parameters())
    first.grad = torch.ones_like(first)

    def state(t):
        ps = list(t.model.parameters())
        return ([p.detach().clone() for p in ps], [None if p.grad is None else p.grad.clone() for p in ps],
                [p._version for p in ps] + [b._version for b in t.model.buffers()], t._m.clone(), t._v.clone(), t._step)

    before = state(tr)
    tr.evaluate(*args)
    tr.evaluate(*args, indices=torch.arange(5))
    after = state(tr)
    assert all(torch.equal(a, b) for a, b in zip(before[0], after[0]))
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(before[1], after[1]))
    assert before[2] == after[2] and torch.equal(before[3], after[3]) and torch.equal(before[4], after[4])
    assert before[5] == after[5]
    assert torch.equal(tr.step(*args), twin.step(*args))
    for p, q in zip(tr.model.parameters(), twin.model.parameters()):
        assert torch.equal(p, q)


# ---------------------------------------------------------------------------------------------------------------------
# groups
def _group(nlc, family, M, N, stacked, h=64):
    """M members of different weights, their single trainers on deep copies, and a dataset (stacked: (M, N, ...))."""
    models, datas = [], []
    for m in range(M):
        if family == "nl":
            sd, data = _gen_setup(3, 1, False, h, 5, 3, N, seed=20 + m)
            models.append(_gen_model(nlc, sd, 3, 1, False, h, 5))
            datas.append(_cuda(*data))
        else:
            sd, data = _rnn_setup("DeltaTRNN", 3, 1, h, N, 3, seed=20 + m)
            models.append(_rnn_model(nlc, "DeltaTRNN", sd, 3, 1, h))
            datas.append(_cuda(*_rnn_args(data)))
    # a group shares the descriptor: member 0's normalisation buffers for all
    sd0 = models[0].state_dict()
    for mdl in models[1:]:
        mdl.load_state_dict({k: (sd0[k] if k in dict(mdl.named_buffers()) else v) for k, v in mdl.state_dict().items()})
    args = tuple(torch.stack([dm[i] for dm in datas]) for i in range(4)) if stacked else datas[0]
    return models, args, datas


@pytest.mark.parametrize("family", ["nl", "rnn"])
@pytest.mark.parametrize("stacked", [True, False])
def test_group_members_equal_their_single_trainers(nlc, family, stacked):
    Single, Group = (nlc.NLTrainer, nlc.NLTrainerGroup) if family == "nl" else (nlc.RNNTrainer, nlc.RNNTrainerGroup)
    models, args, datas = _group(nlc, family, 3, 37, stacked)
    singles = [Single(copy.deepcopy(m)) for m in models]
    losses = Group(models).evaluate(*args)
    assert losses.shape == (3,)
    for i, tr in enumerate(singles):
        assert torch.equal(losses[i], tr.evaluate(*(datas[i] if stacked else datas[0]))), i
    # (M, N) indices: member i its own rows
    idx = torch.stack([torch.arange(i, i + 20) for i in range(3)]).cuda()
    gl = Group(models).evaluate(*args, indices=idx)
    for i, tr in enumerate(singles):
        assert torch.equal(gl[i], tr.evaluate(*(datas[i] if stacked else datas[0]), indices=idx[i])), i


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_member_bits_do_not_depend_on_the_group_size(nlc, family):
    Group = nlc.NLTrainerGroup if family == "nl" else nlc.RNNTrainerGroup
    models, args, _ = _group(nlc, family, 5, 37, False)
    five = Group(models).evaluate(*args)
    two = Group([copy.deepcopy(models[0]), copy.deepcopy(models[3])]).evaluate(*args)
    assert torch.equal(two[0], five[0]) and torch.equal(two[1], five[3])


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_group_of_260(nlc, family):
    Single, Group = (nlc.NLTrainer, nlc.NLTrainerGroup) if family == "nl" else (nlc.RNNTrainer, nlc.RNNTrainerGroup)
    models, args, _ = _group(nlc, family, 2, 16, False)
    members = [copy.deepcopy(models[i % 2]) for i in range(260)]
    losses = Group(members).evaluate(*args)
    a, b = Single(models[0]).evaluate(*args), Single(models[1]).evaluate(*args)
    assert losses.shape == (260,)
    assert torch.equal(losses[0::2], a.expand(130)) and torch.equal(losses[1::2], b.expand(130))


# ---------------------------------------------------------------------------------------------------------------------
# live switching and fallbacks
def _trainer_warnings(rec):
    return [w for w in rec if "Trainer" in str(w.message)]


def test_switching_the_algorithm_on_a_live_trainer(nlc):
    tr, sd, data = _nl_trainer(nlc, N=37, S=8)
    args = _cuda(*data)
    for algo in ("fixed_tablot", "fourier"):
        tr.model.ilt_algorithm = algo
        fresh = nlc.NLTrainer(_gen_model(nlc, sd, 3, 1, False, 64, 8, algo=algo))
        assert torch.equal(tr.evaluate(*args), fresh.evaluate(*args)), algo


def _fallback_ref(model, args):
    with torch.no_grad():
        return torch.nn.functional.mse_loss(model(*args[:3]).squeeze(), args[3].squeeze())


def test_dehoog_on_a_live_trainer_falls_back_with_one_warning(nlc):
    tr, _, data = _nl_trainer(nlc, N=37, S=5)
    args = _cuda(*data)
    tr.model.ilt_algorithm = "dehoog"
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a, b = tr.evaluate(*args), tr.evaluate(*args)
    assert len(_trainer_warnings(rec)) == 1
    _close(a, _fallback_ref(tr.model, args), "dehoog fallback")
    assert torch.equal(a, b)


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_window_of_17_falls_back_with_one_warning(nlc, family):
    if family == "nl":
        tr, _, data = _nl_trainer(nlc, N=19, B=17)
        args = _cuda(*data)
    else:
        tr, _, data = _rnn_trainer(nlc, N=19, B=17)
        args = _cuda(*_rnn_args(data))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a = tr.evaluate(*args)
        tr.evaluate(*args)
    assert len(_trainer_warnings(rec)) == 1
    _close(a, _fallback_ref(tr.model, args), "window-of-17 fallback")


def test_a_dehoog_trainer_evaluates_through_the_model(nlc):
    sd, data = _gen_setup(3, 1, False, 64, 5, 3, 19, seed=2)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(_gen_model(nlc, sd, 3, 1, False, 64, 5, algo="dehoog"))
    assert not tr.fused
    args = _cuda(*data)
    _close(tr.evaluate(*args), _fallback_ref(tr.model, args), "non-fused trainer")


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_empty_batch_raises(nlc, family):
    if family == "nl":
        tr, _, data = _nl_trainer(nlc, N=4)
        args = _cuda(*data)
    else:
        tr, _, data = _rnn_trainer(nlc, N=4)
        args = _cuda(*_rnn_args(data))
    with pytest.raises(nlc._lib.NlcError):
        tr.evaluate(*(t[:0] for t in args))
    with pytest.raises(nlc._lib.NlcError):
        tr.evaluate(*args, indices=torch.zeros(0, dtype=torch.int64))
