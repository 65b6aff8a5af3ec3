"""GPU: a table-started encoder tile takes its first step's hidden-side products (W_hh0 H0, W_hh1 H1 on top of their start
values) from the "gru_prefix" table (csrc/nlc_gru_prefix.h, csrc/nlc_gru_tile.h).  The step body sums the hidden side first in
every chain, so the table holds the full kernel's own accumulators and the latents stay byte-equal between the list launch,
the full wave-per-tile kernel and the cooperative body; against the oracle's GRU they hold the encoder tests' tolerance.

The perturbed actions are set by hand (``noise_rng = "torch"`` with a replayed draw, U = 0): perturbed = clip(u_scale eps) /
u_scale, bounds 2 and -1 at u_scale 4.  One case (three planners, one command each) is computed once and shared."""

import numpy as np
import pytest
import torch

from gpu_common import TOL, build_model

pytestmark = pytest.mark.gpu

ENV = "oderl-cartpole"
U_MAX, U_MIN, U_SCALE = 2.0, -1.0, 4.0

# (K, T, B, hidden_units, E): K = 16 / 48 / 272 with T = 1 / 5 -- 16 windows (one tile over all lists), 240 and 1 360 (lists
# that end in partial tiles, more than one workgroup); B = 2 (only length 1 starts a tile, and its step is the last one) and 4;
# GRU width 64, and 32 / 128 once each; two batched episodes
CASES = [(16, 1, 2, 128, 1), (48, 5, 2, 128, 1), (48, 5, 4, 128, 1), (272, 1, 4, 128, 1), (272, 5, 4, 128, 1),
         (48, 5, 4, 64, 1), (48, 5, 4, 256, 1), (16, 5, 4, 128, 2), (272, 5, 2, 128, 2)]


def _sd(h, seed=5):
    from oracle import nl_model as onl

    st = onl.ENV_STATS[ENV]
    return onl.make_synthetic_state_dict(seed, st["d"], st["nu"], h, 17, st["state_std"], [st["act_high"] / 2], tame=True)


_models = {}


def _model(nlc, h):
    if h not in _models:
        sd = _sd(h)
        _models[h] = (sd, build_model(nlc, sd))
    return _models[h]


def _planner(nlc, model, K, T, E=1, u_min=U_MIN, u_max=U_MAX, u_scale=U_SCALE, noise_rng="torch", U0=0.0, **opts):
    from neurallaplacecontrol_amd.planners.mppi_batch import BatchedMPPIDelay

    options = {"rollout_variant": 2, "gru_coop": 0, "gru_prefix": 0, **opts}
    kw = dict(lambda_=1.0, u_min=torch.tensor(u_min), u_max=torch.tensor(u_max), u_scale=u_scale, noise_rng=noise_rng, seed=21,
              u_init=torch.tensor([U0], dtype=torch.float64), planner_options=options)
    U_init = torch.full((T, 1) if E == 1 else (E, T, 1), U0, dtype=torch.float64)
    if E == 1:
        return nlc.MPPIDelay(nlc.NLDynamics(model, 0.05), nlc.EnvCost(ENV), 5, nlc.noise_sigma(1), K, T, "cuda", U_init=U_init, **kw)
    return BatchedMPPIDelay(nlc.NLDynamics(model, 0.05), nlc.EnvCost(ENV), 5, nlc.noise_sigma(1), E, K, T, "cuda", U_init=U_init, **kw)


def _inputs(nlc, E, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    if E == 1:
        return nlc.initial_state(ENV, g), (torch.rand(B, 1, generator=g, dtype=torch.float64) * 2 - 1) * 3.0
    return (torch.stack([nlc.initial_state(ENV, g) for _ in range(E)]),
            (torch.rand(E, B, 1, generator=g, dtype=torch.float64) * 2 - 1) * 3.0)


def _hand_eps(E, K, T):
    """Draws inside the bounds' images (-0.25, 0.5) or far outside, both signs; rows set by hand: wholly clipped at either
    bound, a clipped action directly followed by an unclipped one (both ways round), alternating bounds, exactly on a bound."""
    rng = np.random.default_rng(1000 * K + 10 * T + E)
    eps = rng.uniform(-0.2, 0.45, (E * K, T))
    eps[rng.random((E * K, T)) < 0.6] = 9.0
    eps[rng.random((E * K, T)) < 0.3] *= -1.0
    for e in range(E):
        rows = eps[e * K:(e + 1) * K]
        rows[0], rows[1] = 9.0, -9.0
        rows[2, 0::2], rows[2, 1::2] = 9.0, 0.125
        rows[3, 0::2], rows[3, 1::2] = -0.125, -9.0
        rows[4, 0::2], rows[4, 1::2] = 9.0, -9.0
        rows[5] = 0.5                                             # exactly u_max / u_scale: counts as clipped
        rows[6], rows[7] = 0.125, -0.125                          # nothing clipped
    return torch.as_tensor(eps, dtype=torch.float64).reshape((K, T, 1) if E == 1 else (E, K, T, 1))


def _command(p, state, ab, raw=None):
    if raw is not None:
        p.noise_dist = type("Replay", (), {"sample": staticmethod(lambda shape: raw.clone())})()
    with torch.no_grad():
        act = p.command(state, ab)
    torch.cuda.synchronize()
    used, hist = p.gru_prefix
    tiles = int(p.ctx.get_stat("gru_prefix_table_tiles"))
    out = dict(action=act.cpu().clone(), latents=p.gru_latents.clone(), states=p.states.clone(), cost=p.cost_total.clone(),
               U=p.U.cpu().clone(), perturbed=p.perturbed_action.clone())
    return out, used, hist, tiles


def _want_tiles(hist, B):
    return sum(-(-hist[n] // 16) for n in range(1, min(B, 5)))


_cases = {}


def _case(nlc, K, T, B, h, E):
    key = (K, T, B, h, E)
    if key not in _cases:
        sd, model = _model(nlc, h)
        state, ab = _inputs(nlc, E, B)
        raw = _hand_eps(E, K, T)
        res = {}
        for name, opts in (("table", dict(gru_prefix=1)), ("full", dict(gru_prefix=0)), ("coop", dict(gru_prefix=0, gru_coop=1))):
            res[name] = _command(_planner(nlc, model, K, T, E, **opts), state, ab, raw)
        _cases[key] = (sd, ab, raw, res)
    return _cases[key]


@pytest.mark.parametrize("K,T,B,h,E", CASES)
def test_table_products_bit_equal_to_full_kernel(nlc, K, T, B, h, E):
    """The list launch against the full kernel on the same perturbed actions: latents byte-equal (and with them states, costs,
    action and U).  Every list that can exist at this (T, B) holds windows -- a window at t reaches min(t + 1, B) perturbed
    actions -- and the stat says how many tiles took their products from the table: every tile of the lists 1 .. B - 1."""
    _, _, raw, res = _case(nlc, K, T, B, h, E)
    (a, used, hist, tiles), (b, used_b, hist_b, tiles_b) = res["table"], res["full"]
    assert torch.equal(a["perturbed"].cpu().reshape(raw.shape), torch.clamp(raw * U_SCALE, U_MIN, U_MAX) / U_SCALE)
    for name in a:
        assert a[name].shape == b[name].shape and torch.equal(a[name], b[name]), name
    assert used and sum(hist) == E * K * T
    assert all(hist[n] > 0 for n in range(min(T, B, 4) + 1)), hist
    assert not any(hist[min(T, B, 4) + 1:])
    assert tiles == _want_tiles(hist, B) and tiles > 0
    assert not used_b and tiles_b == 0 and not any(hist_b)


@pytest.mark.parametrize("K,T,B,h,E", CASES)
def test_cooperative_body_bit_equal_on_the_same_windows(nlc, K, T, B, h, E):
    """The cooperative body (one tile per workgroup, a gate chunk per wavefront) encodes the same windows to the same bytes as
    the wave-per-tile kernel and as the list launch: all three run one accumulation order."""
    _, _, _, res = _case(nlc, K, T, B, h, E)
    coop = res["coop"][0]
    for other in ("full", "table"):
        assert torch.equal(coop["latents"], res[other][0]["latents"]), other
        assert torch.equal(coop["states"], res[other][0]["states"]), other


@pytest.mark.parametrize("h,B", [(128, 2), (128, 4), (64, 4), (256, 4)])
def test_encode_windows_cooperative_against_wave_per_tile(nlc, h, B):
    """The stand-alone encode of an explicit window tensor: N = 16 / 48 / 272 windows, both kernels forced through the option."""
    _, model = _model(nlc, h)
    ctx = model.hip_ctx(torch.device("cuda:0"))
    g = torch.Generator().manual_seed(100 * h + B)
    try:
        for N in (16, 48, 272):
            win = ((torch.rand(N, B, 1, dtype=torch.float64, generator=g) * 2 - 1) * 3.0).cuda()
            outs = []
            for coop in (0, 1):
                ctx.set_option("gru_coop", coop)
                with torch.no_grad():
                    outs.append(model.encode_actions(win).clone())
            assert torch.equal(outs[0], outs[1]), (h, N, B)
    finally:
        ctx.set_option("gru_coop", -1)


@pytest.mark.parametrize("K,T,B,h,E", CASES)
def test_latents_against_the_oracle_gru(nlc, K, T, B, h, E):
    """The list launch's latents against oracle.nl_model's GRU on the windows of the history [action_buffer[1:]; u_scale
    perturbed], at the tolerance of the encoder tests (tests/gpu_common.py TOL)."""
    from oracle import nl_model as onl

    sd, ab, _, res = _case(nlc, K, T, B, h, E)
    out = res["table"][0]
    pert = out["perturbed"].cpu().reshape(E, K, T)
    abuf = ab.reshape(E, B)
    hist = torch.cat((abuf[:, None, 1:].expand(E, K, B - 1), U_SCALE * pert), dim=2)      # (E, K, B - 1 + T)
    win = hist.unfold(2, B, 1).reshape(E * K * T, B, 1)                                   # window (k, t) = hist[t : t + B]
    want = onl.gru_encoder(sd, (win - sd["action_mean"]) / sd["action_std"]).reshape(E * K, T, 2)
    np.testing.assert_allclose(out["latents"].cpu().reshape(E * K, T, 2).numpy(), want.numpy(), **TOL)


def test_products_rebuilt_for_new_bounds_and_weights(nlc):
    """Plan, move the bounds, plan again; plan, load other weights, plan again: the second command's tiles still start from
    the table, and everything it leaves equals what a fresh planner without the table gives at the same command counter --
    the products are those of the new table."""
    K, T, B = 48, 5, 4
    state, ab = _inputs(nlc, 1, B)
    zeros = torch.zeros(T, 1, dtype=torch.float64)
    philox = dict(noise_rng="philox", u_max=3.0, u_min=-3.0, u_scale=3.0)

    def fresh_second_command(m, **kw):
        q = _planner(nlc, m, K, T, gru_prefix=0, **{**philox, **kw})
        q._commands = 1
        return _command(q, state, ab)[0]

    def same(a, b, what):
        for name in a:
            assert torch.equal(a[name], b[name]), (what, name)

    m = build_model(nlc, _sd(128, 5))
    p = _planner(nlc, m, K, T, gru_prefix=1, **philox)
    _command(p, state, ab)
    p.u_max, p.u_min = torch.tensor(2.0, device=p.u_max.device), torch.tensor(-2.5, device=p.u_min.device)
    p._buf = None  # a new descriptor at the next command (nlc_mppi_configure)
    p.U = zeros
    moved, used, hist, tiles = _command(p, state, ab)
    assert used and tiles == _want_tiles(hist, B) and tiles > 0
    same(moved, fresh_second_command(m, u_max=2.0, u_min=-2.5), "moved bounds")

    p = _planner(nlc, m, K, T, gru_prefix=1, **philox)
    first = _command(p, state, ab)[0]
    m.load_state_dict(_sd(128, 6))  # the planner follows its model's weights (nlc_set_model, then nlc_mppi_configure)
    p.U = zeros
    reloaded, used, hist, tiles = _command(p, state, ab)
    assert used and tiles == _want_tiles(hist, B) and tiles > 0
    assert not torch.equal(first["latents"], reloaded["latents"])
    same(reloaded, fresh_second_command(build_model(nlc, _sd(128, 6))), "other weights")


@pytest.mark.parametrize("row", [2, 3])
def test_non_finite_action_buffer_entry(nlc, row):
    """A NaN in action_buffer row `row` is history element row - 1 and reaches the windows t < row of every sample, no others:
    NaN latents there -- also where the step that consumes it is a table-started tile's first (row 3, window t = 0 with its
    one perturbed action clipped) -- and finite latents, the full kernel's bytes, elsewhere.  A skipped step consumes a
    bound's image and never the action buffer."""
    K, T, B = 48, 5, 4
    _, model = _model(nlc, 128)
    state, ab = _inputs(nlc, 1, B)
    ab[row] = float("nan")
    lat = []
    for prefix in (1, 0):
        p = _planner(nlc, model, K, T, gru_prefix=prefix, noise_rng="philox", u_max=3.0, u_min=-3.0, u_scale=3.0, U0=2.5)
        _, used, hist, tiles = _command(p, state, ab)
        lat.append(p.gru_latents.clone())
        assert used == bool(prefix) and (tiles > 0) == bool(prefix)
        if prefix:
            assert hist[1] > 0 and hist[2] > 0
    assert torch.isnan(lat[0][:, :row]).all() and torch.isfinite(lat[0][:, row:]).all()
    assert torch.equal(torch.isnan(lat[0]), torch.isnan(lat[1]))
    assert torch.equal(torch.nan_to_num(lat[0]), torch.nan_to_num(lat[1]))
