"""GPU: one nlc_ctx through a sequence of model uploads (nlc_set_model / nlc_set_rnn_model / nlc_set_node_model).  A setter
replaces the family's whole group at once: the next forward is the new model's to the bit, a model uploaded again gives its
first result to the bit, what was derived from the old weights (the constant-time forward's folded bias, the planner's
configuration) is dropped for the setter's own family only, and a descriptor the library refuses late leaves the ctx as it
was.  Everything runs at the C level on a ctx of the test's own (the Python models keep a ctx each and hide the planner's
re-configuration)."""

import ctypes as C

import numpy as np
import pytest
import torch

from gpu_common import build_model, build_node, build_rnn

pytestmark = pytest.mark.gpu

N, B, D, NU, A = 16, 4, 5, 1, 3.0  # rows, window, and the cartpole's dims: every planner here has its cost
NLC_ERR_UNSUPPORTED, NLC_ERR_STATE = -4, -5


def _nl(nlc, seed, h, S, algo, env="oderl-cartpole"):
    from oracle import nl_model as onl

    st = onl.ENV_STATS[env]
    sd = onl.make_synthetic_state_dict(seed, st["d"], st["nu"], h, S, st["state_std"], [st["act_high"] / 2], tame=True)
    return build_model(nlc, sd, S=S, algo=algo)


def _rnn(nlc, seed, hidden):
    from oracle import nl_model as onl
    from oracle import rnn_model as orn

    return build_rnn(nlc, orn.make_synthetic_state_dict(seed, D, NU, hidden, onl.ENV_STATS["oderl-cartpole"]["state_std"], [A / 2]),
                     hidden)


def _node(nlc, seed, hidden):
    from oracle import nl_model as onl
    from oracle import node_model as ono

    return build_node(nlc, ono.make_synthetic_state_dict(seed, D, NU, hidden, 1, onl.ENV_STATS["oderl-cartpole"]["state_std"],
                                                         [A / 2]), hidden, 1)


@pytest.fixture(scope="module")
def rows():
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(N, D, dtype=torch.float64, generator=g).cuda()
    win = (torch.randn(N, B, NU, dtype=torch.float64, generator=g) * 0.7).cuda()
    ts = (torch.rand(N, 1, dtype=torch.float64, generator=g) * 0.2 + 0.02).cuda()
    return obs, win, ts


def _nl_forward(ctx, rows, const_t=None):
    from neurallaplacecontrol_amd import _lib

    obs, win, ts = rows
    ws = torch.empty(ctx.lib.nlc_model_workspace_bytes(ctx.h, N) // 8, dtype=torch.float64, device="cuda")
    out = torch.empty((N, D), dtype=torch.float64, device="cuda")
    if const_t is None:
        ctx.launch(ctx.lib.nlc_model_forward, _lib.ptr(obs), _lib.ptr(win), _lib.ptr(ts), N, B, _lib.ptr(out), _lib.ptr(ws))
    else:
        ctx.launch(ctx.lib.nlc_model_forward_const_t, _lib.ptr(obs), _lib.ptr(win), const_t, N, B, _lib.ptr(out), _lib.ptr(ws))
    torch.cuda.synchronize()
    return out


def _rnn_forward(ctx, rows):
    from neurallaplacecontrol_amd import _lib

    obs, win, ts = rows
    out, ws = (torch.empty((N, D), dtype=torch.float64, device="cuda") for _ in range(2))
    ctx.launch(ctx.lib.nlc_rnn_forward, _lib.ptr(obs), _lib.ptr(win), _lib.ptr(ts.reshape(-1).contiguous()), N, B, _lib.ptr(out),
               _lib.ptr(ws))
    torch.cuda.synchronize()
    return out


def _node_forward(ctx, rows):
    from neurallaplacecontrol_amd import _lib

    obs, win, _ = rows
    out = torch.empty((N, D), dtype=torch.float64, device="cuda")
    ctx.launch(ctx.lib.nlc_node_forward, _lib.ptr(obs), _lib.ptr(win[:, -1, :].contiguous()), 0.05, N, _lib.ptr(out))
    torch.cuda.synchronize()
    return out


class _Planner:
    """nlc_mppi_configure for one kind of dynamics and the buffers of a command; ``rollout`` returns the library's status."""

    K, T = 64, 3

    def __init__(self, ctx, dynamics):
        self.ctx, self.dynamics, self.commands = ctx, dynamics, 0
        self.configure()

    def configure(self):
        from neurallaplacecontrol_amd import _lib

        ctx, K, T = self.ctx, self.K, self.T
        d = _lib.MppiDesc()
        d.K = d.K_global = K
        d.T, d.nu, d.d, d.B, d.E = T, NU, D, B, 1
        d.lambda_, d.u_scale, d.has_bounds, d.u_per_command = 1.0, A, 1, 1
        d.u_min[0], d.u_max[0] = -A, A
        d.noise_sigma[0] = d.noise_sigma_inv[0] = d.noise_chol[0] = 1.0
        d.dynamics, d.env, d.ts_pred = self.dynamics, _lib.ENV_IDS["oderl-cartpole"], 0.05
        with ctx.stream():
            ctx.check(ctx.lib.nlc_mppi_configure(ctx.h, C.byref(d)))
        mk = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
        self.t = dict(noise=mk(K, T, NU), perturbed=mk(K, T, NU), states=mk(K, T, D), actions=mk(K, T, NU), cost_total=mk(K),
                      cost_nz=mk(K), omega=mk(K), partials=mk(2 + T * NU), action=mk(NU),
                      workspace=mk(ctx.lib.nlc_mppi_workspace_bytes(ctx.h) // 8))
        self.buf = _lib.MppiBuffers(**{k: v.data_ptr() for k, v in self.t.items()})

    def rollout(self):
        from neurallaplacecontrol_amd import _lib

        state = torch.tensor([0.1, 0.0, 0.9, 0.3, 0.2], dtype=torch.float64)
        abuf = torch.zeros(B, NU, dtype=torch.float64)
        with self.ctx.stream():
            rc = self.ctx.lib.nlc_mppi_rollout(self.ctx.h, _lib.ptr(state), 0, _lib.ptr(abuf), C.byref(self.buf), 1, 7, self.commands)
        torch.cuda.synchronize()
        self.commands += rc == 0
        return rc


def test_nl_model_swap_on_one_ctx(nlc, rows):
    from neurallaplacecontrol_amd import _lib

    obs, win, ts = rows
    mA = _nl(nlc, 31, 128, 17, "fourier")
    others = [_nl(nlc, 32, 64, 8, "stehfest"), _nl(nlc, 33, 128, 17, "dehoog")]
    ctx = _lib.Ctx(0)
    mA.upload(ctx)
    outA = _nl_forward(ctx, rows)
    with torch.no_grad():
        assert torch.equal(outA, mA(obs, win, ts))
    plan = _Planner(ctx, _lib.DYN_NL)
    assert plan.rollout() == 0
    for m in others + [mA]:
        m.upload(ctx)
        assert plan.rollout() == NLC_ERR_STATE  # configured against the previous weights
        out = _nl_forward(ctx, rows)
        with torch.no_grad():
            assert torch.equal(out, m(obs, win, ts))  # the model's own ctx, which never held another model
        plan.configure()
        assert plan.rollout() == 0
    assert torch.equal(out, outA)


def test_folded_bias_follows_a_swap(nlc, rows):
    """Two models of one shape, one query time: the second upload's constant-time forward is the second model's (fwd_tn is
    dropped with the first model), to the bit what a ctx that only ever held the second model gives, and agrees with the
    general kernel on a constant ts column as tests/test_gpu_model.py::test_model_forward_constant_time_path compares
    the two kernels."""
    from neurallaplacecontrol_amd import _lib

    obs, win, _ = rows
    m1, m2 = _nl(nlc, 41, 128, 17, "fourier"), _nl(nlc, 42, 128, 17, "fourier")
    ctx = _lib.Ctx(0)
    m1.upload(ctx)
    c1 = _nl_forward(ctx, rows, const_t=0.05)
    m2.upload(ctx)
    c2 = _nl_forward(ctx, rows, const_t=0.05)
    assert not torch.equal(c1, c2)
    with torch.no_grad():
        assert torch.equal(c1, m1(obs, win, 0.05)) and torch.equal(c2, m2(obs, win, 0.05))
    general = _nl_forward(ctx, (obs, win, torch.full((N, 1), 0.05, dtype=torch.float64, device="cuda")))
    np.testing.assert_allclose(c2.cpu().numpy(), general.cpu().numpy(), rtol=1e-11, atol=1e-13)


def test_baseline_swaps_and_whose_planner_they_invalidate(nlc, rows):
    from neurallaplacecontrol_amd import _lib

    obs, win, ts = rows
    ctx = _lib.Ctx(0)
    _nl(nlc, 31, 128, 17, "fourier").upload(ctx)
    plan = _Planner(ctx, _lib.DYN_NL)

    rnns = [_rnn(nlc, 51, 64), _rnn(nlc, 52, 160), _rnn(nlc, 51, 64)]
    outs = []
    for m in rnns:
        m.upload(ctx)
        outs.append(_rnn_forward(ctx, rows))
        with torch.no_grad():
            assert torch.equal(outs[-1], m(obs, win, ts))
        assert plan.rollout() == 0  # an RNN upload leaves a planner with NL dynamics alone
    assert torch.equal(outs[0], outs[2]) and outs[0].shape == outs[1].shape and not torch.equal(outs[0], outs[1])

    nodes = [_node(nlc, 61, 64), _node(nlc, 62, 270), _node(nlc, 61, 64)]
    nodes[0].upload(ctx)
    plan = _Planner(ctx, _lib.DYN_DTRNN)
    assert plan.rollout() == 0
    outs = []
    for m in nodes:
        m.upload(ctx)
        outs.append(_node_forward(ctx, rows))
        with torch.no_grad():
            assert torch.equal(outs[-1], m(obs, win, torch.full((N, 1), 0.05, dtype=torch.float64, device="cuda")))
        assert plan.rollout() == 0  # a NODE upload leaves a planner with RNN dynamics alone
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])

    rnns[0].upload(ctx)
    assert plan.rollout() == NLC_ERR_STATE  # its own family's planner: re-configure
    plan.configure()
    assert plan.rollout() == 0
    plan = _Planner(ctx, _lib.DYN_NODE)
    assert plan.rollout() == 0
    nodes[1].upload(ctx)
    assert plan.rollout() == NLC_ERR_STATE
    plan.configure()
    assert plan.rollout() == 0


def _ilt_tiles_needed(d, S):  # csrc/nlc_pack.h
    groups = (d * ((S + 1) // 2) + 3) // 4 + (d * (S // 2) + 3) // 4
    return (groups + 1) // 2


def test_late_refusal_leaves_the_ctx_intact(nlc, rows):
    """state_dim 6 with 34 terms: the smallest term count whose layer-3 slots need more than the 25 output tiles the kernels
    are instantiated for (33 terms need exactly 25) -- nlc_set_model refuses it after it has packed the weights."""
    from neurallaplacecontrol_amd import _lib

    S_BAD = 34
    assert _ilt_tiles_needed(6, S_BAD) > 25 and all(_ilt_tiles_needed(6, S) <= 25 for S in range(1, S_BAD))
    mA = _nl(nlc, 31, 128, 17, "fourier")
    bad = _nl(nlc, 71, 128, S_BAD, "fourier", env="oderl-acrobot")
    ctx = _lib.Ctx(0)
    mA.upload(ctx)
    outA = _nl_forward(ctx, rows)
    c_before = _nl_forward(ctx, rows, const_t=0.05)
    plan = _Planner(ctx, _lib.DYN_NL)
    assert plan.rollout() == 0
    nt3 = ctx.get_stat("model_nt3")
    with pytest.raises(_lib.NlcError, match="too large for the fused kernel") as err:
        bad.upload(ctx)
    assert err.value.code == NLC_ERR_UNSUPPORTED
    assert ctx.get_stat("model_nt3") == nt3 > 0
    assert plan.rollout() == 0  # the planner configured before the call still runs
    assert torch.equal(_nl_forward(ctx, rows), outA)
    assert torch.equal(_nl_forward(ctx, rows, const_t=0.05), c_before)
