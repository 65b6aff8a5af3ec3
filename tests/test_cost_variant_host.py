"""CPU: the cartpole running cost's state_constraint / change_goal branches (mppi_with_model.py:146-162 -> ctcartpole.py:
311-329) -- ``EnvCost``'s torch formula, the kernels' element math (csrc/nlc_cost.h) built with g++, and the closure
recogniser's proposals -- against ``oracle.envs.cartpole_cost_variant``."""

import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from test_host_logic import _harness_style_closures

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = {"default": {}, "constraint": dict(state_constraint=True), "goal": dict(change_goal=True),
            "goal_flipped": dict(change_goal=True, change_goal_flipped=True)}
BITS = {"default": 0, "constraint": 1, "goal": 2, "goal_flipped": 6}


def _observations(n=1000, seed=0):
    """Cartpole raw states [x, xdot, theta, thetadot] whose tip error e0 = x + sin(theta) - goal covers [-3, 3] for every goal
    (x in [-4, 4]), with the corners put in by hand; and the actions."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.rand(n, 4, dtype=torch.float64, generator=g)
    raw = (raw - 0.5) * torch.tensor([8.0, 6.0, 4 * np.pi, 10.0], dtype=torch.float64)
    raw[0] = torch.tensor([3.0, 0.0, 0.0, 0.0])   # e0 = 3 at goal 0: the wall term is exp(37)
    raw[1] = torch.tensor([-3.0, 0.0, 0.0, 0.0])  # e0 = -3: exp(-23), lost against e0^2
    raw[2] = torch.tensor([0.0, 0.0, 0.0, 0.0])   # e0 = 0: the term is exp(7), about 1 100
    u = (torch.rand(n, 1, dtype=torch.float64, generator=g) - 0.5) * 6.0
    return raw, u


def _trig(raw):
    return torch.stack((raw[:, 0], raw[:, 1], torch.cos(raw[:, 2]), torch.sin(raw[:, 2]), raw[:, 3]), dim=1)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_envcost_variants_vs_oracle(variant):
    """EnvCost(..., variant)(state, action) is the oracle's restatement of the env class, on the trig observation and on the
    raw 4-dim state (whose cos / sin torch computes the same on both sides): rtol 1e-12."""
    import neurallaplacecontrol_amd as nlc
    from oracle import envs as oenvs

    kw = VARIANTS[variant]
    raw, u = _observations()
    obs = _trig(raw)
    ref = oenvs.cartpole_cost_variant(**kw)(obs, u)
    e0 = obs[:, 0] + obs[:, 3]
    assert float(e0.min()) < -3.0 and float(e0.max()) > 3.0 and bool(torch.isfinite(ref).all())
    for env, st in (("oderl-cartpole", obs), ("oderl-cartpole-notrig", raw)):
        cost = nlc.EnvCost(env, **kw)
        assert cost.variant == BITS[variant]
        np.testing.assert_allclose(cost(st, u).numpy(), ref.numpy(), rtol=1e-12, atol=0, err_msg=env)
    if variant == "default":
        assert torch.equal(nlc.EnvCost("oderl-cartpole")(obs, u), oenvs.cartpole_cost(obs, u))


def test_envcost_variant_rules():
    """A variant on pendulum or acrobot is a ValueError; state_constraint wins over change_goal, as the closure's if / elif;
    change_goal_flipped can be assigned at any time."""
    import neurallaplacecontrol_amd as nlc

    for env in ("oderl-pendulum", "oderl-acrobot"):
        for kw in (dict(state_constraint=True), dict(change_goal=True), dict(change_goal=True, change_goal_flipped=True)):
            with pytest.raises(ValueError):
                nlc.EnvCost(env, **kw)
        assert nlc.EnvCost(env).variant == 0
    raw, u = _observations(64, 1)
    obs = _trig(raw)
    both = nlc.EnvCost("oderl-cartpole", state_constraint=True, change_goal=True, change_goal_flipped=True)
    assert both.variant == 1
    assert torch.equal(both(obs, u), nlc.EnvCost("oderl-cartpole", state_constraint=True)(obs, u))
    c = nlc.EnvCost("oderl-cartpole", change_goal=True)
    before = c(obs, u)
    c.change_goal_flipped = True
    assert c.variant == 6 and torch.equal(c(obs, u), nlc.EnvCost("oderl-cartpole", change_goal=True, change_goal_flipped=True)(obs, u))
    assert not torch.equal(before, c(obs, u))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("costhost") / "libcost_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "cost_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.nlc_c_cartpole_state_reward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    lib.nlc_c_cartpole_goal_x.argtypes = [ctypes.c_int]
    lib.nlc_c_cartpole_goal_x.restype = ctypes.c_double
    return lib


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_state_reward_vs_oracle(lib, variant):
    """csrc/nlc_cost.h as the kernels compile it: goal and state reward of every variant.  The oracle's cost with zero
    velocities and a zero action is -state_reward exactly, so the comparison sees that function alone.  Without the wall term
    the two sides do the same products and sums (equal bits); with it libm's exp and torch's may differ in the last place of a
    term that dominates the sum: rtol 4 x 2^-52."""
    from oracle import envs as oenvs

    kw = VARIANTS[variant]
    assert [lib.nlc_c_cartpole_goal_x(b) for b in (0, 1, 2, 6, 3, 7, 4)] == [0.0, 0.0, -2.0, 2.0, 0.0, 0.0, 0.0]
    raw, _ = _observations()
    obs = _trig(raw)
    obs[:, 1] = 0.0
    obs[:, 4] = 0.0
    goal = lib.nlc_c_cartpole_goal_x(BITS[variant])
    e = np.ascontiguousarray(torch.stack((obs[:, 0] + obs[:, 3] - goal, obs[:, 2] - 1.0), dim=1).numpy())
    got = np.empty(len(e))
    lib.nlc_c_cartpole_state_reward(e.ctypes.data, BITS[variant], got.ctypes.data, len(e))
    ref = -oenvs.cartpole_cost_variant(**kw)(obs, torch.zeros(len(e), 1, dtype=torch.float64)).numpy()
    if "state_constraint" in kw:
        np.testing.assert_allclose(got, ref, rtol=4 * 2.0**-52, atol=0)
    else:
        assert np.array_equal(got, ref)
    # past exp's range the reward is -inf (the cost +inf, which the importance weights fold as zero), never NaN
    far = np.array([[80.0, 0.0], [-80.0, 0.0]])
    out = np.empty(2)
    lib.nlc_c_cartpole_state_reward(far.ctypes.data, 1, out.ctypes.data, 2)
    assert out[0] == -np.inf and out[1] == -6400.0


class CTCartpole:  # stand-in with the two methods the closure calls (class name as in envs/oderl/envs/ctcartpole.py)
    def diff_obs_reward_(self, s, exp_reward=False, **kw):
        return -s.pow(2).sum(-1)

    def diff_ac_reward_(self, a):
        return -0.01 * a.pow(2).sum(-1)


def test_candidate_cost_proposes_the_variants():
    """The planner's question (variants=True): a literal closure with state_constraint / change_goal among its free variables
    gets the EnvCost with those flags, the default closure the plain EnvCost; the one-argument form still answers only for
    the default branch."""
    import neurallaplacecontrol_amd as nlc
    from neurallaplacecontrol_amd import _recognise as R

    ts = torch.full((8, 1), 0.05, dtype=torch.float64)
    for kw, want in ((dict(), (False, False)), (dict(state_constraint=True), (True, False)), (dict(change_goal=True), (False, True)),
                     (dict(state_constraint=True, change_goal=True), (True, False))):
        _, cost = _harness_style_closures(None, CTCartpole(), ts, **kw)
        cc = R.candidate_cost(cost, variants=True)
        assert isinstance(cc, nlc.EnvCost) and cc.env_name == "oderl-cartpole", kw
        assert (cc.state_constraint, cc.change_goal, cc.change_goal_flipped) == want + (False,), kw
        if any(kw.values()):
            assert R.candidate_cost(cost) is None
        else:
            assert R.candidate_cost(cost).variant == 0

    class CTPendulum(CTCartpole):
        pass

    _, cost = _harness_style_closures(None, CTPendulum(), ts, state_constraint=True)
    assert R.candidate_cost(cost, variants=True) is None  # that env class has no such branch
