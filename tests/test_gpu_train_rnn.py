"""GPU: the fused training step of the DeltaTRNN / RNN baselines (RNNTrainer / nlc_rnn_train_step) against float64 autograd
through the CPU oracle (oracle.rnn_model) and against the reference's training loop on the grad-mode path
(train_utils.py:388-408).  Tolerances are docs/training.md's: loss 1e-12 relative, gradients 1e-9 of each block's own max
(floored at 1e-6 of the tensor's), steps 1e-12 of each tensor's magnitude, run() 1e-9."""

import copy
import warnings

import numpy as np
import pytest
import torch
from train_compare_rnn import assert_rnn_grad_close

pytestmark = pytest.mark.gpu

PARAMS = ["gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "linear_out.weight", "linear_out.bias"]


def _setup(cls, d, nin, H, N, B, normalize=True, normalize_time=True, mean=False, enc=False, seed=0, out_scale=0.2):
    """Synthetic weights (oracle.rnn_model.make_synthetic_state_dict), normalisation buffers (stds drawn per dim, means
    non-zero if `mean`) and a dataset in the reference's layout, drawn as tests/test_gpu_train.py::_data draws it:
    s0 (N, d), a0 (N, B, nin) (the harness's time channel last if `enc`), sn (N, d), ts (N, 1)."""
    from oracle import rnn_model as orn

    rng = np.random.RandomState(seed)
    std = rng.uniform(0.5, 3.0, d)
    sd = orn.make_synthetic_state_dict(seed, d, nin, H, list(std), None, out_scale=out_scale, time_input=cls == "DeltaTRNN")
    sm = rng.uniform(-1.0, 1.0, d) if mean else np.zeros(d)
    sd["state_mean"] = torch.tensor(sm, dtype=torch.float64)
    sd["action_mean"] = torch.tensor(rng.uniform(-0.5, 0.5, nin) if mean else np.zeros(nin), dtype=torch.float64)
    sd["action_std"] = torch.tensor(rng.uniform(0.5, 2.0, nin), dtype=torch.float64)
    if cls == "RNN":
        del sd["dt"]  # the reference's RNN has no dt buffer
    g = torch.Generator().manual_seed(seed + 17)
    nu = nin - int(enc)
    s0 = torch.tensor(sm) + torch.randn(N, d, dtype=torch.float64, generator=g) * torch.tensor(std)
    a0 = (torch.rand(N, B, nu, dtype=torch.float64, generator=g) * 2 - 1) * 3.0
    if enc:  # the harness's time channel (mppi_with_model.py:110-119)
        tch = torch.flip(torch.arange(B), (0,)).view(1, B, 1).repeat(N, 1, 1).to(torch.float64)
        a0 = torch.cat((a0, tch), dim=2)
    sn = s0 + torch.randn(N, d, dtype=torch.float64, generator=g) * 0.05 * torch.tensor(std)
    ts = torch.rand(N, 1, dtype=torch.float64, generator=g) * 0.08 + 0.02
    return sd, (s0, a0, sn, ts)


def _model(nlc, cls, sd, d, nin, H, normalize=True, normalize_time=True, enc=False):
    kw = dict(hidden_units=H, encode_obs_time=enc, state_mean=np.zeros(d), state_std=np.ones(d), action_mean=np.zeros(nin),
              action_std=np.ones(nin), normalize=normalize)
    if cls == "DeltaTRNN":
        kw["normalize_time"] = normalize_time
    m = getattr(nlc, cls)(d, nin - int(enc), **kw).double()
    m.load_state_dict(sd)
    return m.to("cuda")


def _oracle_loss_grads(cls, sd, s0, a0, ts, target, normalize, normalize_time):
    from oracle import rnn_model as orn

    leaves = {k: (v.clone().requires_grad_() if k in PARAMS else v) for k, v in sd.items()}
    if cls == "DeltaTRNN":
        pred = orn.forward(leaves, s0, a0, ts, normalize, normalize_time)
    else:
        pred = orn.forward_rnn(leaves, s0, a0, normalize)
    loss = ((pred - target) ** 2).mean()
    loss.backward()
    return loss.detach(), {k: leaves[k].grad for k in PARAMS}


def _ref_step(model, opt, bs0, ba0, bts, bsd, clip):
    """train_utils.py:391-408 on the model's grad-mode path; returns (loss, clip_grad_norm_'s total norm or None)."""
    opt.zero_grad()
    pred = model(bs0, ba0, bts)
    loss = torch.nn.MSELoss()(pred.squeeze(), bsd.squeeze())
    loss.backward()
    total = None
    if clip > 0:
        total = float(torch.nn.utils.clip_grad_norm_(model.parameters(), clip))
    opt.step()
    return loss.item(), total


def _close_to_scale(got, ref, tol, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    sc = float(ref.abs().max()) + 1e-300
    err = float((got - ref).abs().max())
    assert err <= tol * sc, f"{what}: max err {err:.3e} > {tol:g} x {sc:.3e}"


def _assert_adam_state_equal(model, twin, tr, opt, tol, steps):
    sd_tr, sd_ref = tr.state_dict(), opt.state_dict()
    named_twin = dict(twin.named_parameters())
    for i, (k, p) in enumerate(model.named_parameters()):
        _close_to_scale(p, named_twin[k], tol, k)
        for key in ("exp_avg", "exp_avg_sq"):
            _close_to_scale(sd_tr["state"][i][key], sd_ref["state"][i][key], tol, f"{k} {key}")
        assert float(sd_tr["state"][i]["step"]) == float(sd_ref["state"][i]["step"]) == steps, k


def _batch(s0, a0, sn, ts, i, bs):
    sl = slice(i * bs, (i + 1) * bs)
    return s0[sl], a0[sl], ts[sl], sn[sl] - s0[sl]


def _pair(nlc, cls="DeltaTRNN", d=5, nin=1, H=160, M=16, B=4, seed=3, **kw):
    """Model, twin and a device dataset at the reference's own shape.  linear_out keeps its initial scale (out_scale 1, an
    untrained model): the total gradient norm is then above the reference's clip of 0.1, so the clip is active
    (test_gradnorm_equals_clip_grad_norm_and_the_clip_is_active)."""
    kw.setdefault("out_scale", 1.0)
    sd, data = _setup(cls, d, nin, H, M, B, seed=seed, **kw)
    mk = lambda: _model(nlc, cls, sd, d, nin, H)  # noqa: E731
    return mk(), mk(), tuple(t.cuda() for t in data), sd


# ---------------------------------------------------------------------------------------------------------------------
# 1. loss_and_grad against the oracle
# (class, d, nin, H, N, B, normalize, normalize_time, non-zero means, encode_obs_time)
LG_CASES = [
    ("DeltaTRNN", 5, 1, 160, 16, 4, True, True, True, False),     # the reference's own shape
    ("DeltaTRNN", 3, 1, 64, 1, 1, True, True, False, False),      # one row, one step
    ("DeltaTRNN", 6, 2, 128, 203, 16, True, False, False, False), # longest window, ragged tile, raw-input branch
    ("RNN", 8, 3, 160, 17, 7, True, None, True, False),           # largest d and nin, one row past a tile, odd window
    ("RNN", 1, 1, 64, 33, 2, False, None, False, False),          # smallest d, raw branch
    ("DeltaTRNN", 5, 1, 160, 4103, 4, True, True, False, False),  # > 128 tiles: second and third tiles, the last ragged
    ("DeltaTRNN", 5, 1, 128, 16, 4, False, False, False, False),
    ("DeltaTRNN", 5, 2, 160, 16, 4, True, True, True, True),      # encode_obs_time: time channel in the window
]


@pytest.mark.parametrize("case", LG_CASES, ids=[f"{c[0]}_d{c[1]}_nin{c[2]}_H{c[3]}_N{c[4]}_B{c[5]}" for c in LG_CASES])
def test_loss_and_grad_vs_oracle_autograd(nlc, case):
    """The loss to 1e-12 relative and every gradient block (tests/train_compare_rnn.py) to 1e-9 of its own max against
    float64 autograd through oracle.rnn_model on the CPU.  With one row and one step h_0 = 0 makes weight_hh's reference
    gradient exactly zero, and the kernel's must be exactly zero too."""
    cls, d, nin, H, N, B, normalize, normalize_time, mean, enc = case
    sd, (s0, a0, sn, ts) = _setup(cls, d, nin, H, N, B, normalize, normalize_time, mean, enc, seed=7 * d + H + B)
    target = sn - s0
    ref_loss, ref_grads = _oracle_loss_grads(cls, sd, s0, a0, ts, target, normalize, normalize_time)
    model = _model(nlc, cls, sd, d, nin, H, normalize, normalize_time, enc)
    tr = nlc.RNNTrainer(model)
    assert tr.fused
    loss = tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), target.cuda())
    assert loss.dim() == 0 and loss.is_cuda
    rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    print(f"loss rel err {rel:.3e}")
    assert rel <= 1e-12, f"loss rel err {rel:.3e}"
    if B == 1:
        assert not bool(ref_grads["gru.weight_hh_l0"].any())
        assert not bool(dict(model.named_parameters())["gru.weight_hh_l0"].grad.any()), "weight_hh gradient is not exactly 0"
    for k, p in model.named_parameters():
        if B == 1 and k == "gru.weight_hh_l0":
            continue
        assert_rnn_grad_close(k, p.grad, ref_grads[k], H, d, 1e-9, report=print)


def test_case_list_covers_the_edges():
    c = LG_CASES
    assert {64, 128, 160} == {x[3] for x in c}
    assert {1, 8} <= {x[1] for x in c} and {1, 2, 3} == {x[2] for x in c}
    assert {1, 16} <= {x[5] for x in c}
    ns = {x[4] for x in c}
    assert any(n < 16 for n in ns) and any(n % 16 == 1 and n > 16 for n in ns) and any(n > 2048 for n in ns)
    assert {"DeltaTRNN", "RNN"} == {x[0] for x in c}
    dt = {(x[6], x[7]) for x in c if x[0] == "DeltaTRNN"}
    assert {(True, True), (True, False), (False, False)} <= dt  # the three legal DeltaTRNN branches
    assert {True, False} == {x[6] for x in c if x[0] == "RNN"}
    assert sum(1 for x in c if x[8]) >= 2  # non-zero means, non-unit stds
    assert any(x[9] for x in c)


# ---------------------------------------------------------------------------------------------------------------------
# 2. step() against the grad-mode path on a twin
def _one_step(nlc, cls, clip, wd, **adam):
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, cls, nin=1)
    kw = dict(lr=1e-4, weight_decay=wd, **adam)
    tr = nlc.RNNTrainer(model, clip_grad_norm=clip, **kw)
    opt = torch.optim.Adam(twin.parameters(), **kw)
    ref_loss, _ = _ref_step(twin, opt, s0, a0, ts, sn - s0, clip)
    loss = tr.step(s0, a0, ts, sn - s0)
    assert abs(float(loss) - ref_loss) <= 1e-12 * abs(ref_loss)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 1)


@pytest.mark.parametrize("cls", ["DeltaTRNN", "RNN"])
@pytest.mark.parametrize("clip,wd", [(0.1, 0.0), (1e6, 0.0), (0.1, 1e-2), (0.0, 0.0)])
def test_one_step_vs_clip_and_adam(nlc, cls, clip, wd):
    """step() == the grad-mode forward + clip_grad_norm_(clip) + torch.optim.Adam on a twin: parameters, exp_avg and
    exp_avg_sq to 1e-12 of each tensor's magnitude (clip active, inactive, off, and with weight decay)."""
    _one_step(nlc, cls, clip, wd)


def test_steps_with_non_default_adam_hyperparameters(nlc):
    """5 step()s with betas (0.3, 0.95) -- torch.lerp's other branch --, eps 1e-3 and weight decay 1e-2."""
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, M=80)
    kw = dict(lr=1e-3, betas=(0.3, 0.95), eps=1e-3, weight_decay=1e-2)
    tr = nlc.RNNTrainer(model, clip_grad_norm=0.1, **kw)
    opt = torch.optim.Adam(twin.parameters(), **kw)
    for i in range(5):
        b = _batch(s0, a0, sn, ts, i, 16)
        ref, _ = _ref_step(twin, opt, *b, 0.1)
        assert abs(float(tr.step(*b)) - ref) <= 1e-12 * abs(ref)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 5)


def test_gradnorm_equals_clip_grad_norm_and_the_clip_is_active(nlc):
    """nlc_rnn_train_step's gradnorm output equals clip_grad_norm_'s return value on the twin to 1e-12 relative; at the test
    shape the total norm is above 0.1 (the clip = 0.1 cases clip) and below 1e6 (that case does not)."""
    import ctypes as C

    model, twin, (s0, a0, sn, ts), _ = _pair(nlc)
    tr = nlc.RNNTrainer(model)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    _, ref = _ref_step(twin, opt, s0, a0, ts, sn - s0, 0.1)
    assert 0.1 < ref < 1e6
    obs, win, tsd, tgt = tr._data(s0, a0, ts, sn - s0)
    N = obs.shape[0]
    flat = torch.cat([p.detach().reshape(-1) for p in tr._params]).contiguous()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    loss = torch.empty((), dtype=torch.float64, device="cuda")
    gnorm = torch.full((), float("nan"), dtype=torch.float64, device="cuda")
    idx = torch.arange(N, dtype=torch.int64, device="cuda")
    ctx = tr._ctx
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with ctx.stream():
        ctx.check(ctx.lib.nlc_rnn_train_step(ctx.h, C.byref(tr._desc()), p(flat), p(m), p(v), 1, p(obs), p(win), p(tsd),
                                             p(tgt), p(idx), N, win.shape[1], p(loss), p(gnorm), p(tr._workspace(N))))
    assert abs(float(gnorm) - ref) <= 1e-12 * ref, f"gradnorm {float(gnorm)!r} vs clip_grad_norm_ {ref!r}"


# ---------------------------------------------------------------------------------------------------------------------
# 3. run() against the reference loop
def _roundoff_misses(got, ref, grads_ref, tol, what):
    """As tests/test_gpu_train.py: parameters within tol of max |p|; an element that misses must belong to a gradient that
    is roundoff-sized (below 1e-12 of its tensor's max |g|) at some iteration."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    sc = float(ref.abs().max()) + 1e-300
    bad = (got - ref).abs() > tol * sc
    if not bool(bad.any()):
        return
    tiny = torch.zeros_like(bad)
    for g in grads_ref:
        tiny |= g.abs() <= 1e-12 * (float(g.abs().max()) + 1e-300)
    assert bool(tiny[bad].all()), f"{what}: {int(bad.sum())} elements miss {tol:g} x {sc:.3e} without a roundoff-sized gradient"


def _run_vs_loop(nlc, cls, M, perm, bs, B=4, lr=1e-4):
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, cls, M=M, B=B)
    tr = nlc.RNNTrainer(model, lr=lr, clip_grad_norm=0.1)
    losses = tr.run(s0, a0, sn, ts, perm.cuda(), batch_size=bs)
    iters = perm.numel() // bs
    assert losses.shape == (iters,) and losses.is_cuda
    opt = torch.optim.Adam(twin.parameters(), lr=lr)
    ref, grads = [], {k: [] for k, _ in twin.named_parameters()}
    for i in range(iters):
        ind = perm[i * bs : (i + 1) * bs].cuda()
        ref.append(_ref_step(twin, opt, s0[ind], a0[ind], ts[ind], sn[ind] - s0[ind], 0.1)[0])
        for k, p in twin.named_parameters():
            grads[k].append(p.grad.detach().cpu().clone())
    ref = torch.tensor(ref, dtype=torch.float64)
    rel = float(((losses.cpu() - ref).abs() / ref.abs()).max())
    print(f"run loss rel err {rel:.3e}")
    assert rel <= 1e-9, f"loss rel err {rel:.3e}"
    named_twin = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        _roundoff_misses(p, named_twin[k], grads[k], 1e-9, k)
    assert float(tr.state_dict()["state"][0]["step"]) == iters


def test_run_200_iterations_vs_reference_loop(nlc):
    M = 16 * 200 + 5
    _run_vs_loop(nlc, "DeltaTRNN", M, torch.randperm(M, generator=torch.Generator().manual_seed(5)), 16)


@pytest.mark.parametrize("which", ["duplicates_subset", "bs7", "bs20", "bs2100"])
def test_run_permutations_and_batch_sizes_vs_reference_loop(nlc, which):
    """A permutation with duplicates (an unsorted strict subset of the rows), batch sizes 7 and 20, and a few iterations of
    2100 rows (132 tiles, more than the 128 workgroups)."""
    g = np.random.RandomState(9)
    M, perm, bs = {
        "duplicates_subset": (300, torch.as_tensor(g.randint(0, 300, size=16 * 12)), 16),
        "bs7": (7 * 15 + 3, torch.randperm(7 * 15 + 3, generator=torch.Generator().manual_seed(3)), 7),
        "bs20": (20 * 10 + 5, torch.randperm(20 * 10 + 5, generator=torch.Generator().manual_seed(4)), 20),
        "bs2100": (3 * 2100 + 13, torch.randperm(3 * 2100 + 13, generator=torch.Generator().manual_seed(5)), 2100),
    }[which]
    if which == "duplicates_subset":
        assert len(set(perm.tolist())) < perm.numel() and len(set(perm.tolist())) < M
    _run_vs_loop(nlc, "RNN" if which == "bs7" else "DeltaTRNN", M, perm, bs, B=3, lr=1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# 4. reproducibility
def test_run_is_bit_reproducible(nlc):
    sd, data = _setup("DeltaTRNN", 5, 1, 160, 40 * 16, 4, seed=3)
    s0, a0, sn, ts = (t.cuda() for t in data)
    perm = torch.randperm(s0.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
    out = []
    for _ in range(2):
        model = _model(nlc, "DeltaTRNN", sd, 5, 1, 160)
        losses = nlc.RNNTrainer(model).run(s0, a0, sn, ts, perm, batch_size=16)
        out.append((losses.cpu(), [p.detach().cpu().clone() for p in model.parameters()]))
    assert torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 5. integration
def test_optimizer_state_round_trips_with_adam(nlc):
    """5 fused steps, state_dict() into torch.optim.Adam, 5 reference steps == 10 fused steps; and the way back."""
    sd, data = _setup("DeltaTRNN", 5, 1, 64, 160, 4, seed=3)
    s0, a0, sn, ts = (t.cuda() for t in data)
    batches = [_batch(s0, a0, sn, ts, i, 16) for i in range(10)]
    mk = lambda sd_=sd: _model(nlc, "DeltaTRNN", sd_, 5, 1, 64)  # noqa: E731
    full = mk()
    tr_full = nlc.RNNTrainer(full)
    for b in batches:
        tr_full.step(*b)
    mixed = mk()
    tr = nlc.RNNTrainer(mixed)
    for b in batches[:5]:
        tr.step(*b)
    opt = torch.optim.Adam(mixed.parameters(), lr=1e-4)
    opt.load_state_dict(tr.state_dict())
    for b in batches[5:]:
        _ref_step(mixed, opt, *b, 0.1)
    named = dict(mixed.named_parameters())
    for k, p in full.named_parameters():
        _close_to_scale(named[k], p, 1e-9, k)
    ref = mk()
    opt2 = torch.optim.Adam(ref.parameters(), lr=1e-4)
    for b in batches[:5]:
        _ref_step(ref, opt2, *b, 0.1)
    back = mk({k: v.detach().cpu() for k, v in ref.state_dict().items()})
    tr2 = nlc.RNNTrainer(back)
    tr2.load_state_dict(opt2.state_dict())
    for b in batches[5:]:
        _ref_step(ref, opt2, *b, 0.1)
        tr2.step(*b)
    named = dict(back.named_parameters())
    for k, p in ref.named_parameters():
        _close_to_scale(named[k], p, 1e-9, k)


def test_lr_change_between_calls(nlc):
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, H=64, M=32)
    tr = nlc.RNNTrainer(model)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for i in range(2):
        b = _batch(s0, a0, sn, ts, i, 16)
        _ref_step(twin, opt, *b, 0.1)
        sched.step()
        tr.step(*b)
        tr.lr = opt.param_groups[0]["lr"]
    named = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        _close_to_scale(p, named[k], 1e-12, k)


def test_model_changes_after_construction_reach_the_kernels(nlc):
    """model.load_state_dict with another state_std / action_std after RNNTrainer(model): loss_and_grad equals the oracle
    with the NEW constants."""
    d, H, N = 5, 128, 40
    sd, (s0, a0, sn, ts) = _setup("DeltaTRNN", d, 1, H, N, 4, seed=2)
    model = _model(nlc, "DeltaTRNN", sd, d, 1, H)
    tr = nlc.RNNTrainer(model)
    tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), (sn - s0).cuda())  # the old descriptor is in use
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["state_std"] = sd["state_std"] * torch.linspace(0.5, 2.0, d, dtype=torch.float64)
    sd2["action_std"] = torch.tensor([2.5], dtype=torch.float64)
    model.load_state_dict(sd2)
    ref_loss, ref_grads = _oracle_loss_grads("DeltaTRNN", sd2, s0, a0, ts, sn - s0, True, True)
    loss = tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), (sn - s0).cuda())
    rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    assert rel <= 1e-12, f"loss rel err {rel:.3e}: the trainer kept the constants of construction time"
    for k, p in model.named_parameters():
        assert_rnn_grad_close(k, p.grad, ref_grads[k], H, d, 1e-9)


def test_trained_weights_reach_forward_and_planner(nlc):
    """After step(): model(...) under no_grad (the HIP inference path) and MPPIDelay.command() on a planner built BEFORE
    training equal the same calls on a model freshly built from model.state_dict() to 1e-12."""
    d, nu, H, A = 5, 1, 160, 3.0
    sd, data = _setup("DeltaTRNN", d, nu, H, 64, 4, seed=3)
    s0, a0, sn, ts = (t.cuda() for t in data)
    model = _model(nlc, "DeltaTRNN", sd, d, nu, H)

    def planner(m, U0, raw):
        mppi = nlc.MPPIDelay(nlc.NLDynamics(m, 0.05), nlc.EnvCost("oderl-cartpole"), d, nlc.noise_sigma(nu), 256, 10, "cpu",
                             lambda_=1.0, u_min=torch.tensor(-A), u_max=torch.tensor(A), u_scale=A, U_init=U0.clone())
        mppi.noise_dist = type("Replay", (), {"sample": staticmethod(lambda shape: raw)})()
        return mppi

    gen = torch.Generator().manual_seed(0)
    raw = torch.randn(256, 10, nu, dtype=torch.float64, generator=gen)
    U0 = torch.randn(10, nu, dtype=torch.float64, generator=gen) * 0.1
    state, ab = nlc.initial_state("oderl-cartpole"), torch.zeros(4, nu, dtype=torch.float64)
    early = planner(model, U0, raw)
    before = early.command(state, ab)
    tr = nlc.RNNTrainer(model, lr=1e-2)
    for i in range(4):
        tr.step(*_batch(s0, a0, sn, ts, i, 16))
    fresh = _model(nlc, "DeltaTRNN", {k: v.detach().cpu() for k, v in model.state_dict().items()}, d, nu, H)
    with torch.no_grad():
        y, y_ref = model(s0, a0, ts), fresh(s0, a0, ts)
    np.testing.assert_allclose(y.cpu().numpy(), y_ref.cpu().numpy(), rtol=1e-12, atol=1e-14)
    early.U = U0.clone()
    after = early.command(state, ab)
    ref = planner(fresh, U0, raw).command(state, ab)
    np.testing.assert_allclose(after.cpu().numpy(), ref.cpu().numpy(), rtol=1e-12, atol=1e-14)
    assert not torch.equal(after.cpu(), before.cpu())


# ---------------------------------------------------------------------------------------------------------------------
# 6. fallbacks
def test_fallback_width_warns_once_and_matches_reference_loop(nlc):
    """hidden_units=96 (nlc_set_rnn_model refuses it): one warning at construction, fused False, run() + step() equal the
    reference loop on a twin, step count included."""
    sd, data = _setup("DeltaTRNN", 5, 1, 96, 5 * 16, 4, seed=4)
    s0, a0, sn, ts = (t.cuda() for t in data)
    model, twin = _model(nlc, "DeltaTRNN", sd, 5, 1, 96), _model(nlc, "DeltaTRNN", sd, 5, 1, 96)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.RNNTrainer(model)
        losses = tr.run(s0, a0, sn, ts, torch.arange(s0.shape[0]).cuda(), batch_size=16)
        tr.step(*_batch(s0, a0, sn, ts, 0, 16))
    assert len([w for w in rec if "RNNTrainer" in str(w.message)]) == 1 and not tr.fused
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    ref = [_ref_step(twin, opt, *_batch(s0, a0, sn, ts, i, 16), 0.1)[0] for i in range(5)]
    _ref_step(twin, opt, *_batch(s0, a0, sn, ts, 0, 16), 0.1)
    np.testing.assert_allclose(losses.cpu().numpy(), ref, rtol=1e-12)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 6)


def test_window_of_17_falls_back_and_shares_the_adam_state(nlc):
    """B = 17 (the kernels take 1..16): one warning per trainer, and an alternating B = 17 / B = 4 sequence on one trainer
    keeps one Adam state -- parameters, moments and the step count equal a twin on torch.optim.Adam."""
    sd, data = _setup("DeltaTRNN", 5, 1, 64, 6 * 16, 17, seed=5)
    s0, a0, sn, ts = (t.cuda() for t in data)
    model, twin = _model(nlc, "DeltaTRNN", sd, 5, 1, 64), _model(nlc, "DeltaTRNN", sd, 5, 1, 64)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr = nlc.RNNTrainer(model, lr=1e-3)
        assert tr.fused
        for i, B in enumerate((17, 4, 17, 4, 4, 17)):
            s0b, a0b, tsb, bsd = _batch(s0, a0, sn, ts, i, 16)
            a0b = a0b[:, -B:].contiguous()
            ref, _ = _ref_step(twin, opt, s0b, a0b, tsb, bsd, 0.1)
            loss = tr.step(s0b, a0b, tsb, bsd)
            assert abs(float(loss) - ref) <= 1e-12 * abs(ref), (i, B)
    assert len([w for w in rec if "RNNTrainer" in str(w.message)]) == 1
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 6)


def test_refused_call_leaves_the_step_count_and_empty_batch_raises(nlc):
    from neurallaplacecontrol_amd import _lib
    from neurallaplacecontrol_amd.training import _f64_ptr, _i64_ptr

    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, H=64, M=32)
    tr = nlc.RNNTrainer(model)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    b0, b1 = _batch(s0, a0, sn, ts, 0, 16), _batch(s0, a0, sn, ts, 1, 16)
    _ref_step(twin, opt, *b0, 0.1)
    tr.step(*b0)
    obs, win, tsd, tgt = tr._data(*b0)
    loss = torch.empty((), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.NlcError, match="N must be >= 1"):
        tr._launch_step(_i64_ptr(tr._idx(16)), obs, win, tsd, tgt, 0, _f64_ptr(loss), tr._workspace(16))
    assert tr._step == 1 and float(tr.state_dict()["state"][0]["step"]) == 1.0
    with pytest.raises(_lib.NlcError):
        tr.step(s0[:0], a0[:0], ts[:0], (sn - s0)[:0])
    assert tr._step == 1
    _ref_step(twin, opt, *b1, 0.1)
    tr.step(*b1)
    _assert_adam_state_equal(model, twin, tr, opt, 1e-12, 2)


@pytest.mark.parametrize("flag", ["amsgrad", "maximize"])
def test_load_state_dict_refuses_amsgrad_and_maximize(nlc, flag):
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, H=64)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4, **{flag: True})
    _ref_step(twin, opt, s0, a0, ts, sn - s0, 0.1)
    with pytest.raises(ValueError, match=flag):
        nlc.RNNTrainer(model).load_state_dict(opt.state_dict())


def test_trainer_rejects_float32_host_and_undefined_branch_models(nlc):
    model = _pair(nlc, H=64)[0]
    with pytest.raises(NotImplementedError, match="float64"):
        nlc.RNNTrainer(copy.deepcopy(model).float())
    with pytest.raises(RuntimeError, match="GPU"):
        nlc.RNNTrainer(copy.deepcopy(model).cpu())
    sd, _ = _setup("DeltaTRNN", 5, 1, 64, 16, 4)
    with pytest.raises(NameError):
        nlc.RNNTrainer(_model(nlc, "DeltaTRNN", sd, 5, 1, 64, normalize=False, normalize_time=True))


def test_rnn_accepts_and_ignores_ts(nlc):
    """RNN ignores ts, but the reference's loop still passes it: any ts (even of another length) gives the same step."""
    model, twin, (s0, a0, sn, ts), _ = _pair(nlc, "RNN", H=64)
    la = nlc.RNNTrainer(model).step(s0, a0, ts, sn - s0)
    lb = nlc.RNNTrainer(twin).step(s0, a0, torch.full((3,), 7.0, device="cuda", dtype=torch.float64), sn - s0)
    assert torch.equal(la, lb)
    for a, b in zip(model.parameters(), twin.parameters()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 7. NLTrainer still works (the full guard is tests/test_gpu_train.py)
def test_nl_trainer_still_runs(nlc):
    from oracle import nl_model as onl

    d, nu, h, S = 5, 1, 64, 17
    sd = onl.make_synthetic_state_dict(3, d, nu, h, S, [1.0] * d, [1.5], tame=True)
    m = nlc.NeuralLaplaceModel(d, nu, d, hidden_units=h, s_recon_terms=S, ilt_algorithm="fourier", state_mean=np.zeros(d),
                               state_std=np.ones(d), action_mean=np.array([0]), action_std=np.array([1.0]), normalize=True,
                               normalize_time=True).double()
    m.load_state_dict(sd)
    m = m.to("cuda")
    g = torch.Generator().manual_seed(0)
    s0 = torch.randn(16, d, dtype=torch.float64, generator=g)
    a0 = torch.rand(16, 4, nu, dtype=torch.float64, generator=g) * 2 - 1
    ts = torch.rand(16, 1, dtype=torch.float64, generator=g) * 0.08 + 0.02
    tgt = torch.randn(16, d, dtype=torch.float64, generator=g) * 0.05
    tr = nlc.NLTrainer(m)
    assert tr.fused and isinstance(tr, nlc.NLTrainer) and not isinstance(tr, nlc.RNNTrainer)
    leaves = {k: (v.clone().requires_grad_() if k.startswith(("action_encoder.", "laplace_rep_func.")) else v)
              for k, v in sd.items()}
    ref = ((onl.nl_forward(leaves, s0, a0, ts, S=S) - tgt) ** 2).mean()
    loss = tr.loss_and_grad(s0.cuda(), a0.cuda(), ts.cuda(), tgt.cuda())
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
