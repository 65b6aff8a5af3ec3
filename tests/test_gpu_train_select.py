"""GPU: snapshot selection of the fused trainers -- the raw entry nlc_train_keep_best against a numpy statement of the rule,
compared as int64 bit patterns (misaligned rows of odd P, guard doubles on both sides, NaN-payload sentinels in the rows that
must stay untouched); ``keep_best`` / ``restore_best`` with crafted losses on single trainers, groups and a non-fused
(de Hoog) trainer; ``fit`` against a host loop written here from ``run``, ``evaluate``, ``.item()`` and cloned parameters."""

import copy
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
from test_gpu_train import _gen_model, _gen_setup
from test_gpu_train_eval import _cuda, _group, _rnn_args
from test_gpu_train_rnn import _model as _rnn_model
from test_gpu_train_rnn import _setup as _rnn_setup

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SENTINEL = 0x7FF8_0000_0000_0001  # a quiet NaN whose payload is 1 + the element's index: every element has bits of its own
BAD_ARG, BAD_SHAPE, UNSUPPORTED = -1, -2, -4


# ---------------------------------------------------------------------------------------------------------------------
# 1. the raw entry
@pytest.fixture(scope="module")
def ctx(nlc):
    return nlc._lib.Ctx(0)


class _Buffers:
    """params and best_params [M][P] inside larger device buffers, ``soff`` / ``doff`` guard doubles in front (an odd
    offset starts row 0 on an odd double) and 4 behind; best pre-filled, guards included, with distinct NaN-payload
    sentinels; best_loss, best_tag, improved (pre-filled with 7)."""

    def __init__(self, M, P, best_loss, soff=4, doff=4, seed=0):
        self.M, self.P, self.soff, self.doff = M, P, soff, doff
        g = torch.Generator().manual_seed(seed)
        self.params = torch.randn(soff + M * P + 4, dtype=torch.float64, generator=g).cuda()
        n = doff + M * P + 4
        self.best = (torch.arange(n, dtype=torch.int64) + SENTINEL).view(torch.float64).cuda()
        self.best_loss = torch.tensor(best_loss, dtype=torch.float64).cuda()
        self.best_tag = torch.full((M,), -1, dtype=torch.int64).cuda()
        self.improved = torch.full((M,), 7, dtype=torch.int32).cuda()

    def bits(self):
        torch.cuda.synchronize()
        return {"params": self.params.view(torch.int64).cpu().numpy().copy(),
                "best": self.best.view(torch.int64).cpu().numpy().copy(),
                "best_loss": self.best_loss.view(torch.int64).cpu().numpy().copy(),
                "best_tag": self.best_tag.cpu().numpy().copy(), "improved": self.improved.cpu().numpy().copy()}

    def call(self, ctx, values, tag, **override):
        """One nlc_train_keep_best with the losses ``values``; ``override`` replaces arguments (M, P, or a pointer by
        name).  Returns the code."""
        self.loss = torch.tensor(values, dtype=torch.float64).cuda()
        ptr = {"loss": self.loss.data_ptr(), "params": self.params.data_ptr() + 8 * self.soff,
               "best_loss": self.best_loss.data_ptr(), "best": self.best.data_ptr() + 8 * self.doff,
               "best_tag": self.best_tag.data_ptr(), "improved": self.improved.data_ptr()}
        M, P = override.pop("M", self.M), override.pop("P", self.P)
        ptr.update(override)
        vp = lambda k: C.c_void_p(ptr[k])  # noqa: E731
        with ctx.stream():
            return ctx.lib.nlc_train_keep_best(ctx.h, M, P, vp("loss"), vp("params"), vp("best_loss"), vp("best"),
                                               vp("best_tag"), tag, vp("improved"))


def _expect(before, M, P, soff, doff, loss, tag):
    """The rule in numpy, on the bit patterns."""
    loss = np.asarray(loss, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        better = loss < before["best_loss"].view(np.float64)
    want = {k: v.copy() for k, v in before.items()}
    src = before["params"][soff : soff + M * P].reshape(M, P)
    dst = want["best"][doff : doff + M * P].reshape(M, P)  # a view: the guards on both sides stay what they were
    dst[better] = src[better]
    want["best_loss"][better] = loss.view(np.int64)[better]
    want["best_tag"][better] = tag
    want["improved"] = better.astype(np.int32)
    return want, better


def _same(got, want, what):
    for k in want:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.flatnonzero(got[k] != want[k])[:8]}"


# best_loss before the call, and two loss patterns: between them improve / equal / worse / NaN / +inf, with improving
# members on even and on odd rows (odd rows of an odd P are the misaligned ones)
BEST0 = [2.0, 2.0, 2.0, 2.0, INF]
PATTERNS = [[1.0, 2.0, 3.0, NAN, INF], [2.0, 1.0, NAN, 0.5, 3.0]]


@pytest.mark.parametrize("P", [1, 2, 1023, 1024, 1025, 4099])
def test_raw_entry_bits(ctx, P):
    M = 5
    for loss in PATTERNS:
        for soff, doff in ((4, 4), (3, 4), (3, 3)):  # rows 16-byte aligned together, never together, both odd
            b = _Buffers(M, P, BEST0, soff, doff, seed=P)
            before = b.bits()
            assert b.call(ctx, loss, 11) == 0
            want, better = _expect(before, M, P, soff, doff, loss, 11)
            assert 0 < better.sum() < M
            _same(b.bits(), want, f"P={P} offsets {soff},{doff} loss {loss}")
            # the same loss again: nothing improves, nothing but `improved` is written
            after = b.bits()
            assert b.call(ctx, loss, 12) == 0
            want2, better2 = _expect(after, M, P, soff, doff, loss, 12)
            assert not better2.any() and np.array_equal(want2["best"], after["best"])
            _same(b.bits(), want2, f"P={P} second call")


@pytest.mark.parametrize("M", [1, 260])
def test_raw_entry_member_counts(ctx, M):
    """P = 33 (odd: every second row misaligned); M = 260 is more members than one commit workgroup's 256 threads."""
    P = 33
    best0 = [BEST0[m % 5] for m in range(M)]
    for pat in PATTERNS:
        loss = [pat[(m + m // 5) % 5] for m in range(M)] if M > 1 else [pat[0 if pat[0] < 2.0 else 1]]
        b = _Buffers(M, P, best0, seed=M)
        before = b.bits()
        assert b.call(ctx, loss, 5) == 0
        want, better = _expect(before, M, P, 4, 4, loss, 5)
        assert better.any()
        _same(b.bits(), want, f"M={M}")


def test_raw_entry_without_the_improved_array(ctx):
    b = _Buffers(5, 33, BEST0)
    before = b.bits()
    assert b.call(ctx, PATTERNS[1], 3, improved=0) == 0
    want, _ = _expect(before, 5, 33, 4, 4, PATTERNS[1], 3)
    want["improved"] = before["improved"]
    _same(b.bits(), want, "improved_dev NULL")


@pytest.mark.parametrize("what,override,code", [
    ("NULL loss", {"loss": 0}, BAD_ARG), ("NULL params", {"params": 0}, BAD_ARG), ("NULL best_loss", {"best_loss": 0}, BAD_ARG),
    ("NULL best_params", {"best": 0}, BAD_ARG), ("NULL best_tag", {"best_tag": 0}, BAD_ARG),
    ("params == best_params", "alias", BAD_ARG), ("M = 0", {"M": 0}, BAD_SHAPE), ("M = -1", {"M": -1}, BAD_SHAPE),
    ("P = 0", {"P": 0}, BAD_SHAPE), ("P = -3", {"P": -3}, BAD_SHAPE), ("M = 65536", {"M": 65536}, UNSUPPORTED)])
def test_raw_entry_refusals_launch_nothing(ctx, what, override, code):
    b = _Buffers(5, 33, BEST0)
    before = b.bits()
    if override == "alias":
        override = {"params": b.best.data_ptr() + 8 * b.doff}
    assert b.call(ctx, [0.0] * 5, 9, **override) == code, what  # a loss every member would improve on
    assert ctx.lib.nlc_last_error(ctx.h)
    _same(b.bits(), before, what)


# ---------------------------------------------------------------------------------------------------------------------
# 2. keep_best / restore_best with crafted losses
def _loss(v):
    return torch.tensor(v, dtype=torch.float64, device="cuda")


def _opt_state(tr):
    sds = tr.state_dict() if isinstance(tr.state_dict(), list) else [tr.state_dict()]
    return [(k, {n: (t.clone() if torch.is_tensor(t) else t) for n, t in st.items()}) for sd in sds for k, st in sorted(sd["state"].items())]


def _state_equal(a, b):
    assert len(a) == len(b) and len(a) > 0
    for (ka, sa), (kb, sb) in zip(a, b):
        assert ka == kb and sa.keys() == sb.keys()
        for n in sa:
            assert torch.equal(torch.as_tensor(sa[n]), torch.as_tensor(sb[n])), (ka, n)


def _trainer_warnings(rec):
    return [w for w in rec if "Trainer" in str(w.message)]


@pytest.mark.parametrize("algo", ["fourier", "dehoog"])
def test_keep_best_and_restore_on_a_tiny_trainer(nlc, algo):
    """Losses 3.0, 2.0, 2.5 with one step() between the calls: the snapshot is the second call's.  ``dehoog``: the non-fused
    trainer, the same rule in torch ops, with the trainer's one warning (at construction); its model has the shape of
    test_gpu_train_eval's de Hoog case (d = 3, S = 5, window 3, 19 rows)."""
    d, S, B, N = (1, 3, 1, 3) if algo == "fourier" else (3, 5, 3, 19)
    sd, data = _gen_setup(d, 1, False, 64, S, B, N, seed=3)
    args = _cuda(*data)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.NLTrainer(_gen_model(nlc, sd, d, 1, False, 64, S, algo=algo))
        assert tr.fused == (algo == "fourier")
        assert tr.best_loss is None and tr.best_tag is None
        with pytest.raises(RuntimeError):
            tr.restore_best()
        flags = []
        for k, v in enumerate([3.0, 2.0, 2.5]):
            tr.step(*args)
            flags.append(tr.keep_best(_loss(v) if k != 1 else _loss([v])))  # 0-dim or (1,)
            if k == 1:
                then = [p.detach().clone() for p in tr.model.parameters()]
                ev_then = tr.evaluate(*args)
        assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
        assert [int(f) for f in flags] == [1, 1, 0]
        assert all(f.dtype == torch.int32 and f.shape == () and f.is_cuda for f in flags)
        assert tr.best_loss.shape == () and tr.best_loss.is_cuda and float(tr.best_loss) == 2.0
        assert tr.best_tag.dtype == torch.int64 and int(tr.best_tag) == 2  # the Adam step count at the second call
        assert any(not torch.equal(p, q) for p, q in zip(tr.model.parameters(), then))  # the third step moved them
        key, state = tr.model._weights_key(), _opt_state(tr)
        tr.restore_best()
        assert all(torch.equal(p, q) for p, q in zip(tr.model.parameters(), then))
        assert tr.model._weights_key() != key
        _state_equal(_opt_state(tr), state)  # moments and step count (3) untouched
        assert int(_opt_state(tr)[0][1]["step"]) == 3
        assert float(tr.best_loss) == 2.0 and int(tr.best_tag) == 2
        assert torch.equal(tr.evaluate(*args), ev_then)
        # an explicit tag, and a NaN after it
        assert int(tr.keep_best(_loss(1.0), tag=40)) == 1 and int(tr.best_tag) == 40
        assert int(tr.keep_best(_loss(NAN))) == 0 and float(tr.best_loss) == 1.0
        with pytest.raises(ValueError):
            tr.keep_best(_loss([1.0, 2.0]))
    assert len(_trainer_warnings(rec)) == (0 if algo == "fourier" else 1)


@pytest.mark.parametrize("family", ["nl", "rnn"])
def test_group_members_equal_their_single_trainers(nlc, family):
    """M = 3, each member's best at a different call: member 0 at the first, 1 at the second, 2 at the third."""
    Single, Group = (nlc.NLTrainer, nlc.NLTrainerGroup) if family == "nl" else (nlc.RNNTrainer, nlc.RNNTrainerGroup)
    models, args, _ = _group(nlc, family, 3, 8, False)
    singles = [Single(copy.deepcopy(m)) for m in models]
    grp = Group(models)
    calls = [[1.0, 5.0, 5.0], [2.0, 1.0, 4.0], [3.0, 2.0, 1.0]]
    for k, row in enumerate(calls):
        grp.step(*args)
        flags = grp.keep_best(_loss(row))
        assert flags.shape == (3,) and flags.dtype == torch.int32
        for i, tr in enumerate(singles):
            tr.step(*args)
            assert torch.equal(tr.keep_best(_loss(row[i])), flags[i]), (k, i)
    assert grp.best_tag.tolist() == [1, 2, 3] and grp.best_loss.tolist() == [1.0, 1.0, 1.0]
    for i, tr in enumerate(singles):
        assert torch.equal(grp._best[i], tr._best[0]), i
        assert torch.equal(grp.best_loss[i], tr.best_loss) and torch.equal(grp.best_tag[i], tr.best_tag), i
    assert not torch.equal(grp._best[0], grp._best[1])
    grp.restore_best()
    for i, tr in enumerate(singles):
        tr.restore_best()
        for p, q in zip(grp.models[i].parameters(), tr.model.parameters()):
            assert torch.equal(p, q), i


# ---------------------------------------------------------------------------------------------------------------------
# 3. fit against a host loop
def _fit_setup(nlc, family, R):
    """A trainer class, a model, ``data(epoch)`` (a fresh dataset per epoch, as the reference regenerates its synthetic one)
    and a validation set."""
    if family == "nl":
        sd, _ = _gen_setup(3, 1, False, 64, 5, 3, R, seed=11)
        model = _gen_model(nlc, sd, 3, 1, False, 64, 5)

        def draw(seed):
            s0, a0, ts, tgt = _cuda(*_gen_setup(3, 1, False, 64, 5, 3, R, seed=seed)[1])
            return s0, a0, s0 + tgt, ts

        return nlc.NLTrainer, model, draw
    sd, _ = _rnn_setup("DeltaTRNN", 3, 1, 64, R, 3, seed=11)
    model = _rnn_model(nlc, "DeltaTRNN", sd, 3, 1, 64)
    return nlc.RNNTrainer, model, lambda seed: _cuda(*_rnn_setup("DeltaTRNN", 3, 1, 64, R, 3, seed=seed)[1])


def _host_fit(tr, data, val, R, epochs, bs, every, seed, step_lr):
    """The loop a user writes today: a host read at every check, the parameters cloned from Python on improvement, the
    rate driven by a real StepLR on a dummy optimiser."""
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=tr.lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=step_lr[0], gamma=step_lr[1])
    best, best_iter, best_params, done, train_loss, criterion = INF, -1, None, 0, [], []
    for epoch in range(epochs):
        s0, a0, sn, ts = data(epoch)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed + epoch)
        perm = torch.randperm(R, device="cuda", generator=gen)
        for chunk in perm.split(every * bs):
            if chunk.numel() < bs:
                continue
            losses = tr.run(s0, a0, sn, ts, chunk, bs)
            done += chunk.numel() // bs
            crit = tr.evaluate(*val) if val is not None else losses.sum(-1)
            if crit.item() < best:
                best, best_iter = crit.item(), done
                best_params = [p.detach().clone() for p in tr.model.parameters()]
            train_loss.append(losses)
            criterion.append(crit)
        opt.step()
        sched.step()
        tr.lr = opt.param_groups[0]["lr"]
    final = [p.detach().clone() for p in tr.model.parameters()]
    return torch.cat(train_loss), torch.stack(criterion), best, best_iter, best_params, final


@pytest.mark.parametrize("family", ["nl", "rnn"])
@pytest.mark.parametrize("with_val", [True, False])
def test_fit_equals_the_host_loop(nlc, family, with_val):
    """Batch 4, eval_every 3, 2 epochs, step_lr (1, 0.5).  42 rows: slices of 12, 12, 12 and 6 indices (3, 3, 3 and 1
    iterations); 38 rows: the last slice has 2 indices, no full batch, and is skipped."""
    R = 42 if with_val else 38
    Trainer, model, draw = _fit_setup(nlc, family, R)
    sets = {e: draw(100 + e) for e in range(2)}
    val = None
    if with_val:
        s0, a0, sn, ts = draw(200)
        val = (s0, a0, ts, sn - s0)
    host = Trainer(copy.deepcopy(model), lr=1e-3)
    ref_train, ref_crit, ref_best, ref_iter, ref_params, ref_final = _host_fit(host, sets.__getitem__, val, R, 2, 4, 3, 5, (1, 0.5))
    assert ref_train.shape == ((20,) if with_val else (18,)) and ref_crit.shape == ((8,) if with_val else (6,))

    seen = []

    def data(epoch):
        seen.append(epoch)
        return sets[epoch]

    tr = Trainer(model, lr=1e-3)
    out = tr.fit(data, val, epochs=2, batch_size=4, eval_every=3, seed=5, step_lr=(1, 0.5), restore_best=False)
    assert seen == [0, 1]
    assert tr.lr == host.lr == 1e-3 * 0.5 * 0.5
    assert torch.equal(out["train_loss"], ref_train) and torch.equal(out["criterion"], ref_crit)
    assert out["best_loss"].item() == ref_best and out["best_iter"].item() == ref_iter
    assert 0 < ref_iter <= ref_train.numel()
    for p, q in zip(tr.model.parameters(), ref_final):
        assert torch.equal(p, q)
    tr.restore_best()
    for p, q in zip(tr.model.parameters(), ref_params):
        assert torch.equal(p, q)

    # a tuple for data, and restore_best at the end (the default): the restored weights are those of its own best check
    tr2 = Trainer(copy.deepcopy(model), lr=1e-3)  # `model` now holds the restored weights: any start will do here
    out2 = tr2.fit(sets[0], val, epochs=1, batch_size=4, eval_every=3, seed=5)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in tr2.model.parameters()]), tr2._best[0])
    assert out2["best_loss"].item() == out2["criterion"].min().item()
