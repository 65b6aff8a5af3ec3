"""GPU tests of the importance-weighting step of command() (run with ``-m gpu`` on an MI355X): weight_tile / weight_chunk /
weight_rank / weight_final / merge_kernel against the plain one-level formula in np.longdouble, on prescribed costs and
prescribed noise chosen for the boundaries of the three-level fold.  Cases, reference and the derived bound:
tests/mppi_weight_cases.py (its CPU twin: tests/test_mppi_weights_host.py).

Costs and noise reach the kernels through the public planner on its callables path: dynamics ``lambda s, a: s``, a running
cost that returns the prescribed (K,) vector on the first call of a command and zeros afterwards, U = 0, u_scale = 1, no
bounds, a replayed noise draw.  With U = 0 the perturbation cost is exactly 0, so cost_total IS the prescribed vector and
noise IS the replayed draw, bit for bit -- asserted first in every test.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import mppi_weight_cases as mw
from gpu_common import _Replay

pytestmark = pytest.mark.gpu

def _planner(nlc, case, k_offset=0, K_local=None):
    """An MPPIDelay on the callables path that plans on `case`'s costs and noise (its slice [k_offset, k_offset + K_local))."""
    K, T, nu = case.K, case.T, case.nu
    K_local = K if K_local is None else K_local
    cost = torch.from_numpy(case.cost[k_offset:k_offset + K_local].copy()).cuda()
    calls = [0]

    def running_cost(state, u):
        first = calls[0] % T == 0
        calls[0] += 1
        return cost if first else torch.zeros_like(cost)

    p = nlc.MPPIDelay(lambda s, a: s, running_cost, 1, nlc.noise_sigma(nu), K, T, "cpu", lambda_=case.lam, u_scale=1,
                      U_init=torch.zeros(T, nu, dtype=torch.float64), planner_options={"recognise_closures": 0})
    p.K_local, p.k_offset = K_local, k_offset  # (a shard: phase 1 stand-alone, the merge by hand -- see _sharded)
    p.noise_dist = _Replay(torch.from_numpy(case.noise.copy()))
    return p


def _command(nlc, case, **kw):
    p = _planner(nlc, case, **kw)
    action = p.command(torch.zeros(1, dtype=torch.float64), torch.zeros(1, case.nu, dtype=torch.float64))
    torch.cuda.synchronize()
    lo, hi = p.k_offset, p.k_offset + p.K_local
    assert p.rollout_body == "callables"
    assert np.array_equal(p.cost_total.numpy(), case.cost[lo:hi], equal_nan=True), "cost_total is not the prescribed vector"
    assert np.array_equal(p.noise.numpy(), case.noise[lo:hi]), "noise is not the replayed draw"
    return p, action


def _check(case, p, action, ref=None):
    """cost_total_non_zero, omega, U and the action of a whole-population planner within the derived bound."""
    ref = mw.reference(case) if ref is None else ref
    U = p.U.numpy()
    assert np.array_equal(action.numpy().reshape(-1), U[0].reshape(-1)), "action != U[0] * u_scale"
    r = mw.check(case, ref, p.cost_total_non_zero.numpy(), p.omega.numpy(), U, "kernels")
    print(f"{case}: error / bound = {r:.4f}")  # (the largest over the file is quoted in DESIGN.md)
    return r


# ------------------------------------------------------------------ a. wide spread
@pytest.mark.parametrize("K,T,nu", mw.SHAPES)
def test_wide_spread_of_costs(nlc, K, T, nu):
    """x_k over [0, 730] tile by tile, lambda in {1e-3, 0.7, 50}, c0 in {0, -1e6, 1e9}: every level of the fold rescales by
    factors down to e^-700, and the largest weights of most tiles underflow at the next level."""
    for lam in mw.LAMBDAS:
        for c0 in mw.C0S:
            case = mw.wide_spread(K, T, nu, lam, c0)
            _check(case, *_command(nlc, case))


# ------------------------------------------------------------------ b. ties
@pytest.mark.parametrize("K", [1000, 4097])
def test_ties_are_exact(nlc, K):
    case = mw.ties(K)
    p, action = _command(nlc, case)
    assert np.all(p.cost_total_non_zero.numpy() == 1.0)
    assert np.all(p.omega.numpy() == 1.0 / K)
    _check(case, p, action)  # U against the mean of the noise, within the bound


# ------------------------------------------------------------------ c. one survivor
@pytest.mark.parametrize("K,kstar", mw.SURVIVORS)
def test_one_survivor_is_one_hot(nlc, K, kstar):
    """Every other weight underflows to exactly 0 at both levels: omega is one-hot and U is the winner's noise, bit for bit."""
    case = mw.one_survivor(K, kstar)
    p, action = _command(nlc, case)
    hot = np.zeros(K)
    hot[kstar] = 1.0
    assert np.array_equal(p.omega.numpy(), hot)
    assert p.cost_total_non_zero.numpy()[kstar] == 1.0
    assert np.array_equal(p.U.numpy(), case.noise[kstar])
    assert np.array_equal(action.numpy().reshape(-1), case.noise[kstar][0])


# ------------------------------------------------------------------ d. padding lanes
@pytest.mark.parametrize("K", [1000, 17])
@pytest.mark.parametrize("sign", [1, -1])
def test_padding_lanes_do_not_reach_the_tile_minimum(nlc, K, sign):
    case = mw.padding(K, sign)
    p, action = _command(nlc, case)
    assert p.cost_total_non_zero.numpy()[np.argmin(case.cost)] == 1.0
    _check(case, p, action)


# ------------------------------------------------------------------ e. +inf costs
@pytest.mark.parametrize("case", mw.inf_cases(), ids=repr)
def test_inf_costs_weigh_zero(nlc, case):
    """A whole tile / half a tile / a whole chunk / all but one sample / all chunks but the last at +inf: weight 0 for those
    samples, everything else as if they were absent, a finite action."""
    p, action = _command(nlc, case)
    assert bool(torch.isfinite(action).all()) and bool(torch.isfinite(p.U).all())
    gone = np.isinf(case.cost)
    assert np.all(p.omega.numpy()[gone] == 0.0) and np.all(p.cost_total_non_zero.numpy()[gone] == 0.0)
    _check(case, p, action)
    keep = ~gone
    sub = mw.Case("without", case.cost[keep], case.noise[keep], case.lam)
    ref_sub = mw.reference(sub)
    mw.check(sub, ref_sub, p.cost_total_non_zero.numpy()[keep], p.omega.numpy()[keep], p.U.numpy(), "as if absent")


# ------------------------------------------------------------------ f. the same through the rollout's own cost
def _cartpole_inf_setup(nlc):
    from oracle import envs as oenvs
    from oracle import mppi as omppi

    env, K, T, A = "oderl-cartpole", 64, 5, 3.0
    g = torch.Generator().manual_seed(5)
    states = torch.stack([nlc.initial_state(env, g) for _ in range(K)])
    states_inf = states.clone()
    states_inf[32:48, 0] = 1e200  # the cart position: (x + sin)^2 overflows to +inf in the running cost
    raw = torch.randn(K, T, 1, dtype=torch.float64, generator=g)
    U0 = torch.randn(T, 1, dtype=torch.float64, generator=g) * 0.2
    ab = torch.randn(4, 1, dtype=torch.float64, generator=g)
    sig = nlc.noise_sigma(1)
    ts = torch.full((K, 1), 0.05, dtype=torch.float64)

    def oracle(st):
        return omppi.mppi_command(U0.clone(), st, ab, raw.clone(), lambda s, w: oenvs.ORACLE_DYNAMICS[env](s, w, ts, 1),
                                  oenvs.RUNNING_COST[env], 5, torch.inverse(sig), 0.9, A, torch.tensor(-A), torch.tensor(A))

    kw = dict(lambda_=0.9, u_min=torch.tensor(-A), u_max=torch.tensor(A), u_scale=A)
    return env, K, T, states, states_inf, raw, U0, ab, sig, oracle, kw


def _assert_matches_oracle(out, action, U, omega, cost_total):
    ct = out["cost_total"]
    assert bool(torch.isinf(ct[32:48]).all()) and bool((ct[32:48] > 0).all()) and not bool(torch.isnan(ct).any())
    assert bool(torch.isfinite(out["action"]).all())
    assert torch.equal(torch.isinf(cost_total), torch.isinf(ct)) and not bool(torch.isnan(cost_total).any())
    fin = torch.isfinite(ct)
    np.testing.assert_allclose(cost_total[fin].numpy(), ct[fin].numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(action.numpy(), out["action"].numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(U.numpy(), out["U"].numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(omega.numpy(), out["omega"].numpy(), rtol=1e-9, atol=1e-9)
    assert bool((omega[32:48] == 0).all())


def test_inf_tile_from_the_rollouts_own_cost(nlc):
    """OracleDynamics + EnvCost, K = 64, T = 5, cart position 1e200 for samples 32..47: the rollout kernel itself writes +inf
    (not NaN) costs for one whole tile; the oracle's plain formula gives them weight 0 and a finite action."""
    env, K, T, states, states_inf, raw, U0, ab, sig, oracle, kw = _cartpole_inf_setup(nlc)
    out = oracle(states_inf)
    p = nlc.MPPIDelay(nlc.OracleDynamics(env, 0.05, 1), nlc.EnvCost(env), 5, sig, K, T, "cpu", U_init=U0.clone(), **kw)
    p.noise_dist = _Replay(raw.clone())
    action = p.command(states_inf, ab)
    torch.cuda.synchronize()
    _assert_matches_oracle(out, action, p.U, p.omega, p.cost_total)


def test_inf_tile_in_one_episode_of_a_batched_planner(nlc):
    """E = 3, only episode 1 holds the +inf tile: episodes 0 and 2 equal single planners bit for bit, episode 1 the oracle."""
    from neurallaplacecontrol_amd.planners.mppi_batch import BatchedMPPIDelay

    env, K, T, states, states_inf, raw, U0, ab, sig, oracle, kw = _cartpole_inf_setup(nlc)
    E = 3
    st = torch.stack([states, states_inf, states])
    bat = BatchedMPPIDelay(nlc.OracleDynamics(env, 0.05, 1), nlc.EnvCost(env), 5, sig, E, K, T, "cpu",
                           U_init=U0.clone().expand(E, T, 1).contiguous(), **kw)
    bat.noise_dist = _Replay(raw.clone().expand(E, K, T, 1).contiguous())
    act = bat.command(st, ab.expand(E, 4, 1).contiguous())
    torch.cuda.synchronize()
    single = nlc.MPPIDelay(nlc.OracleDynamics(env, 0.05, 1), nlc.EnvCost(env), 5, sig, K, T, "cpu", U_init=U0.clone(), **kw)
    single.noise_dist = _Replay(raw.clone())
    a1 = single.command(states, ab)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a1).all())
    for e in (0, 2):
        assert torch.equal(act[e], a1) and torch.equal(bat.U[e], single.U) and torch.equal(bat.omega[e], single.omega)
        assert torch.equal(bat.cost_total[e], single.cost_total)
    _assert_matches_oracle(oracle(states_inf), act[1], bat.U[1], bat.omega[1], bat.cost_total[1])


# ------------------------------------------------------------------ g. shard merge
@pytest.mark.parametrize("G,case", mw.shard_cases(), ids=lambda v: repr(v))
def test_shard_merge_equals_one_planner(nlc, G, case):
    """G shard planners' partials merged through nlc_mppi_finish, as test_mppi_two_shards_merge_equals_single does: one
    shard's beta_g > 800 lambda above the others (scale exactly 0), one shard entirely +inf, one shard holding the only
    finite sample, and an ordinary population.  Every rank's U, action and omega equal the one-planner result, and both
    the one-level reference, within the bound."""
    from neurallaplacecontrol_amd import _lib

    ref = mw.reference(case)
    full, a_full = _command(nlc, case)
    _check(case, full, a_full, ref)
    Kl = case.K // G
    shards = []
    for r in range(G):
        p, _ = _command(nlc, case, k_offset=r * Kl, K_local=Kl)  # fills partials (and a local-only update, overwritten next)
        shards.append(p)
    gathered = torch.stack([s._partials for s in shards]).contiguous()
    omega, w = [], []
    for r, p in enumerate(shards):
        p.U = torch.zeros(case.T, case.nu, dtype=torch.float64)  # U after the shift, before the update
        act = torch.empty(case.nu, dtype=torch.float64)
        p.ctx.check(p.ctx.lib.nlc_mppi_finish(p.ctx.h, _lib.ptr(gathered), G, r, C.byref(p._buf), _lib.ptr(act)))
        torch.cuda.synchronize()
        U = p.U.numpy()
        assert np.array_equal(act.numpy(), U[0])
        rank_r = mw.check(case, ref, np.concatenate([np.asarray(ref["w"][:r * Kl], dtype=np.float64), p.cost_total_non_zero.numpy(),
                                                      np.asarray(ref["w"][(r + 1) * Kl:], dtype=np.float64)]),
                          np.concatenate([np.asarray(ref["omega"][:r * Kl], dtype=np.float64), p.omega.numpy(),
                                          np.asarray(ref["omega"][(r + 1) * Kl:], dtype=np.float64)]), U, f"rank {r} of {G}")
        print(f"{case} rank {r}: error / bound = {rank_r:.4f}")
        if r:
            assert np.array_equal(U, shards[0].U.numpy()), "the ranks' U differ"
        omega.append(p.omega.numpy())
        w.append(p.cost_total_non_zero.numpy())
    # the shards' omega and cost_total_non_zero together, against the one planner within twice the bound (both are inside it)
    rel, cap, dUb = mw.bounds(case, ref)
    big = np.isfinite(rel)
    for got, one, want in ((np.concatenate(omega), full.omega.numpy(), ref["omega"]),
                           (np.concatenate(w), full.cost_total_non_zero.numpy(), ref["w"])):
        assert np.all(np.abs(got - one)[big] <= 2 * (want[big] * rel[big]))
    assert np.all(np.abs(shards[0].U.numpy() - full.U.numpy()) <= 2 * dUb.astype(np.float64))


# ------------------------------------------------------------------ h. poisoned costs stay visible
@pytest.mark.parametrize("case", mw.poisoned_cases(), ids=repr)
def test_poisoned_costs_give_a_nan_action(nlc, case):
    """A NaN cost, a -inf cost, all costs +inf: the reference's action is NaN; so are the action and U here."""
    assert np.all(np.isnan(mw.reference(case)["dU"].astype(np.float64)))
    p, action = _command(nlc, case)
    assert bool(torch.isnan(action).all()) and bool(torch.isnan(p.U).all())

