"""GPU: planner option ``gru_prefix`` (include/nlc.h, csrc/nlc_gru_prefix.h) -- windows of the MPPI history whose first consumed
actions are clipped at u_min / u_max start the GRU encoder from a table of precomputed states.  Only whole GRU steps are
skipped and the steps that run are the encoder's own step body, so every test compares ``gru_prefix = 1`` against
``gru_prefix = 0`` on the same inputs, seed and command counter with ``torch.equal``: latents, states, costs, action and U.
``gru_coop = 0`` sends the small launches to the wave-per-tile kernel, ``rollout_variant = 2`` to the two-launch body."""

import numpy as np
import pytest
import torch

from gpu_common import build_model

pytestmark = [pytest.mark.gpu, pytest.mark.fp64_bit_identity]

ENV = "oderl-cartpole"


@pytest.fixture(scope="module")
def model(nlc):
    from oracle import nl_model as onl

    st = onl.ENV_STATS[ENV]
    sd = onl.make_synthetic_state_dict(5, st["d"], st["nu"], 128, 17, st["state_std"], [st["act_high"] / 2], tame=True)
    return build_model(nlc, sd)


def _planner(nlc, model, K, T, prefix, E=1, u_min=-3.0, u_max=3.0, u_scale=3.0, sigma=1.0, U0=0.0, u_init=0.0, noise_rng="philox", **opts):
    from neurallaplacecontrol_amd.planners.mppi_batch import BatchedMPPIDelay

    options = {"rollout_variant": 2, "gru_coop": 0, "gru_prefix": prefix, **opts}
    kw = dict(lambda_=1.0, u_min=torch.tensor(u_min), u_max=torch.tensor(u_max), u_scale=u_scale, noise_rng=noise_rng, seed=21,
              u_init=torch.tensor([u_init], dtype=torch.float64), planner_options=options)
    sig = nlc.noise_sigma(1) * sigma ** 2
    U_init = torch.full((T, 1) if E == 1 else (E, T, 1), U0, dtype=torch.float64)
    if E == 1:
        return nlc.MPPIDelay(nlc.NLDynamics(model, 0.05), nlc.EnvCost(ENV), 5, sig, K, T, "cuda", U_init=U_init, **kw)
    return BatchedMPPIDelay(nlc.NLDynamics(model, 0.05), nlc.EnvCost(ENV), 5, sig, E, K, T, "cuda", U_init=U_init, **kw)


def _restate_histogram(perturbed, B, u_max, u_min, u_scale):
    """Windows by prefix length (tests/test_gru_prefix_host.py restate, counted)."""
    p = perturbed.reshape(-1, perturbed.shape[-2]).cpu().numpy()
    bits = p.view(np.uint64)
    hi, lo = ((np.array([b], np.float64) / np.float64(u_scale)).view(np.uint64)[0] for b in (u_max, u_min))
    hist = [0] * 5
    for k in range(p.shape[0]):
        for t in range(p.shape[1]):
            n = 0
            for s in range(min(B, 4)):
                i = t + B - 1 - s
                if i < B - 1 or bits[k, i - (B - 1)] not in (hi, lo):
                    break
                n = s + 1
            hist[n] += 1
    return hist


def _run(p, state, ab, n_cmd=2):
    """n_cmd closed-loop-like commands; everything the command leaves behind, and the prefix stats of each."""
    out, stats = [], []
    ab = ab.clone()
    for _ in range(n_cmd):
        with torch.no_grad():
            act = p.command(state, ab)
        torch.cuda.synchronize()
        stats.append((p.gru_prefix, p.perturbed_action.clone()))
        out.append((act.cpu().clone(), p.gru_latents.clone(), p.states.clone(), p.cost_total.clone(), p.U.cpu().clone()))
        ab = torch.roll(ab, -1, -2)
        ab[..., -1, :] = act.cpu().reshape(ab[..., -1, :].shape)
    return out, stats


def _same(a, b, what):
    for step, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("action", "latents", "states", "cost_total", "U"), x, y):
            assert u.shape == v.shape and torch.equal(u, v), (what, step, name)


def _inputs(nlc, E, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    if E == 1:
        return nlc.initial_state(ENV, g), (torch.rand(B, 1, generator=g, dtype=torch.float64) * 2 - 1) * 3.0
    return (torch.stack([nlc.initial_state(ENV, g) for _ in range(E)]),
            (torch.rand(E, B, 1, generator=g, dtype=torch.float64) * 2 - 1) * 3.0)


# U (and the u_init shifted in behind it) three sigma above the bound: 99.9 % clip at u_max; tiny sigma: nothing clips;
# u_min == u_max: every window is whole
CLASSES = {"one_sigma": {}, "one_side": dict(U0=4.0, u_init=4.0), "none": dict(sigma=1e-3), "all": dict(u_min=1.5, u_max=1.5)}


@pytest.mark.parametrize("K,T,B,E", [(48, 7, 4, 1), (16, 2, 4, 1), (64, 12, 5, 1), (32, 6, 4, 2)])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_bit_equal_and_histogram(nlc, model, K, T, B, E, cls):
    """Shapes: 336 windows (ragged against 16), every window touching the action buffer (T = 2 < B - 1 + 1), B = 5 (the table
    ends at four steps, a fifth always runs), two batched episodes.  The histogram sums to the window count, equals the
    Python restatement on the command's own perturbed actions, and the class the inputs aim at is the one that fills."""
    kw = CLASSES[cls]
    state, ab = _inputs(nlc, E, B)
    on, off = _planner(nlc, model, K, T, 1, E, **kw), _planner(nlc, model, K, T, 0, E, **kw)
    a, sa = _run(on, state, ab)
    b, sb = _run(off, state, ab)
    _same(a, b, (K, T, B, E, cls))
    for (used, hist), pert in sa:
        assert used and sum(hist) == E * K * T
        assert hist == _restate_histogram(pert, B, kw.get("u_max", 3.0), kw.get("u_min", -3.0), 3.0), (hist, cls)
    assert all(not used and not any(hist) for (used, hist), _ in sb)
    hist = sa[0][0][1]
    if cls == "none":
        assert hist[0] == E * K * T
    if cls == "all":  # window t holds min(t + 1, B) perturbed elements
        want = [0] * 5
        for t in range(T):
            want[min(t + 1, B, 4)] += E * K
        assert hist == want
    if cls == "one_side":
        assert (sa[0][1] == 1.0).double().mean() > 0.9 and hist[0] < 0.1 * E * K * T
    if cls == "one_sigma":
        assert all(h > 0 for h in hist[:min(T, 4) + 1])


def test_hand_set_perturbed_histogram(nlc, model):
    """noise_rng = "torch" with a replayed draw and U = 0: perturbed = clip(u_scale eps) / u_scale is set by hand -- runs of
    clipped actions of every length and sign pattern, asymmetric bounds, u_max != u_scale."""
    K, T, B, u_max, u_min, u_scale = 32, 9, 4, 2.0, -1.0, 4.0
    rng = np.random.default_rng(0)
    eps = rng.uniform(-0.2, 0.45, (K, T))                          # inside the bounds (-0.25, 0.5) ...
    eps[rng.random((K, T)) < 0.6] = 9.0                            # ... or far outside
    eps[rng.random((K, T)) < 0.3] *= -1.0
    eps[0], eps[1], eps[2, ::2] = 9.0, -9.0, 0.5                   # whole rows clipped; exactly on the bound counts too
    raw = torch.as_tensor(eps, dtype=torch.float64).reshape(K, T, 1)
    state, ab = _inputs(nlc, 1, B)
    ab[2] = u_max                                                  # a buffer entry equal to a bound must not count
    res = []
    for prefix in (1, 0):
        p = _planner(nlc, model, K, T, prefix, u_min=u_min, u_max=u_max, u_scale=u_scale, noise_rng="torch")
        p.noise_dist = type("Replay", (), {"sample": staticmethod(lambda shape: raw.clone())})()
        res.append(_run(p, state, ab, n_cmd=1))
    _same(res[0][0], res[1][0], "hand-set")
    (used, hist), pert = res[0][1][0]
    assert used and hist == _restate_histogram(pert, B, u_max, u_min, u_scale) and sum(hist) == K * T
    assert min(hist) > 0
    want = torch.clamp(raw * u_scale, u_min, u_max) / u_scale
    assert torch.equal(pert.cpu(), want)


def test_table_rebuilt_for_new_bounds_and_weights(nlc):
    """Plan, move u_max / u_min, plan again; plan, load other weights, plan again: the second command equals the one a fresh
    planner (with and without the table) gives at the same command counter."""
    from oracle import nl_model as onl

    K, T, B = 48, 7, 4
    st = onl.ENV_STATS[ENV]
    sd = lambda seed: onl.make_synthetic_state_dict(seed, st["d"], st["nu"], 128, 17, st["state_std"],  # noqa: E731
                                                    [st["act_high"] / 2], tame=True)
    state, ab = _inputs(nlc, 1, B)
    zeros = torch.zeros(T, 1, dtype=torch.float64)

    def second_command_of_fresh(m, prefix, **kw):
        q = _planner(nlc, m, K, T, prefix, **kw)
        q._commands = 1
        return _run(q, state, ab, n_cmd=1)

    m = build_model(nlc, sd(5))
    p = _planner(nlc, m, K, T, 1)
    _run(p, state, ab, n_cmd=1)
    p.u_max, p.u_min = torch.tensor(2.0, device=p.u_max.device), torch.tensor(-2.5, device=p.u_min.device)
    p._buf = None  # a new descriptor at the next command (nlc_mppi_configure)
    p.U = zeros
    moved, stats = _run(p, state, ab, n_cmd=1)
    assert stats[0][0][0]
    for prefix in (1, 0):
        _same(moved, second_command_of_fresh(m, prefix, u_max=2.0, u_min=-2.5)[0], ("moved bounds", prefix))

    p = _planner(nlc, m, K, T, 1)
    first, _ = _run(p, state, ab, n_cmd=1)
    m.load_state_dict(sd(6))  # the planner follows its model's weights (nlc_set_model, then nlc_mppi_configure)
    p.U = zeros
    reloaded, stats = _run(p, state, ab, n_cmd=1)
    assert stats[0][0][0] and not torch.equal(first[0][1], reloaded[0][1])
    other = build_model(nlc, sd(6))
    for prefix in (1, 0):
        _same(reloaded, second_command_of_fresh(other, prefix)[0], ("other weights", prefix))


def test_non_finite_action_buffer_entry(nlc, model):
    """A NaN in action_buffer row 2 (history element 1) reaches the windows t = 0, 1 of every sample and no others: NaN
    latents there, finite latents elsewhere, with and without the table."""
    K, T, B = 48, 7, 4
    state, ab = _inputs(nlc, 1, B)
    ab[2] = float("nan")
    lat = []
    for prefix in (1, 0):
        p = _planner(nlc, model, K, T, prefix, U0=2.5)
        with torch.no_grad():
            p.command(state, ab)
        torch.cuda.synchronize()
        lat.append(p.gru_latents.clone())
        assert p.gru_prefix[0] == bool(prefix)
    assert torch.isnan(lat[0][:, :2]).all() and torch.isfinite(lat[0][:, 2:]).all()
    assert torch.equal(torch.isnan(lat[0]), torch.isnan(lat[1]))
    assert torch.equal(torch.nan_to_num(lat[0]), torch.nan_to_num(lat[1]))


def test_out_of_scope(nlc, model):
    """gru_prefix = 1 where the table cannot serve is the documented error (NLC_ERR_UNSUPPORTED); auto falls back silently."""
    from oracle import nl_model as onl
    from neurallaplacecontrol_amd import _lib

    state, ab = _inputs(nlc, 1, 4)
    for opts in (dict(gru_gemm=1), dict(gru_coop=1), dict(rollout_variant=3)):
        with pytest.raises(_lib.NlcError) as err:
            _planner(nlc, model, 48, 7, 1, **opts).command(state, ab)
        assert err.value.code == _lib.NLC_ERR_UNSUPPORTED and "gru_prefix" in str(err.value)
        p = _planner(nlc, model, 48, 7, -1, **opts)
        p.command(state, ab)
        assert p.gru_prefix == (False, [0] * 5)
    auto = _planner(nlc, model, 48, 7, -1)
    auto.command(state, ab)
    assert auto.gru_prefix[0]
    # acrobot: two action dimensions
    st = onl.ENV_STATS["oderl-acrobot"]
    d, nu, A = st["d"], st["nu"], st["act_high"]
    m2 = build_model(nlc, onl.make_synthetic_state_dict(3, d, nu, 128, 17, st["state_std"], [A / 2], tame=True))
    s2 = nlc.initial_state("oderl-acrobot", torch.Generator().manual_seed(2))
    for prefix in (1, -1):
        p = nlc.MPPIDelay(nlc.NLDynamics(m2, 0.05), nlc.EnvCost("oderl-acrobot"), d, nlc.noise_sigma(nu), 48, 7, "cuda",
                          lambda_=1.0, u_min=torch.tensor(-A), u_max=torch.tensor(A), u_scale=A, noise_rng="philox", seed=4,
                          U_init=torch.zeros(7, nu, dtype=torch.float64),
                          planner_options={"rollout_variant": 2, "gru_coop": 0, "gru_prefix": prefix})
        if prefix == 1:
            with pytest.raises(_lib.NlcError) as err:
                p.command(s2, torch.zeros(4, nu, dtype=torch.float64))
            assert err.value.code == _lib.NLC_ERR_UNSUPPORTED and "gru_prefix" in str(err.value)
        else:
            p.command(s2, torch.zeros(4, nu, dtype=torch.float64))
            assert p.gru_prefix == (False, [0] * 5)
