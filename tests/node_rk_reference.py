"""CPU reference of the NODE baseline under the three fixed-grid solvers (test infrastructure for tests/test_node_rk_host.py
and tests/test_gpu_node_rk.py): ``oracle.node_model.ode_func`` and ``euler_substeps`` with torchdiffeq's fixed-grid ``euler``,
``midpoint`` and ``rk4`` steps restated in the evaluation order docs/training.md gives (rk4 is the 3/8 rule).
torchdiffeq is absent offline: **parity unpinned vs upstream**, like ``oracle.node_model.odeint_euler``."""

import torch

from oracle import node_model as on

METHODS = ("euler", "midpoint", "rk4")
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
OPTION = {"euler": 0, "midpoint": 1, "rk4": 2}  # nlc_set_option(ctx, "node_method", .)


def rk_step(method, f, y, h):
    """One sub-step of width ``h`` from ``y``; ``f`` ignores t."""
    if method == "euler":
        return y + h * f(y)
    if method == "midpoint":
        k1 = f(y)
        k2 = f(y + (h / 2) * k1)
        return y + h * k2
    if method == "rk4":
        k1 = f(y)
        k2 = f(y + h * k1 / 3)
        k3 = f(y + h * (k2 - k1 / 3))
        k4 = f(y + h * (k1 - k2 + k3))
        return y + (k1 + 3 * (k2 + k3) + k4) * h / 8
    raise NotImplementedError(method)


def integrate(method, f, y, t_end, step_size=0.05):
    for h in on.euler_substeps(float(t_end), step_size):
        y = rk_step(method, f, y, h)
    return y


def forward(sd, obs, window, ts_pred, method="euler", normalize=True, normalize_time=True, step_size=0.05):
    """``oracle.node_model.forward`` with ``method``: every row integrates to ``ts_pred[0]``."""
    obs = obs.to(torch.float64)
    d = obs.shape[1]
    aug = sd[on_key("4.weight")].shape[0] - d
    x = (obs - sd["state_mean"]) / sd["state_std"] if normalize else obs
    ts = ts_pred.to(torch.float64)
    if normalize_time:
        ts = ts / (sd["dt"] * 8.0)
    if aug > 0:
        x = torch.cat([x, torch.zeros(obs.shape[0], aug, dtype=torch.float64)], 1)
    window = window.to(torch.float64)
    if window.dim() == 2:
        window = window.unsqueeze(1)
    u = window[:, -1, :]
    out = integrate(method, lambda y: on.ode_func(sd, y, u), x, float(ts.reshape(-1)[0]), step_size)
    return out[:, : out.shape[-1] - aug]


def on_key(tail):
    return "x_ode_func_in_x_and_u.linear_tanh_stack." + tail


def forward_rows(sd, obs, window, ts_pred, method, normalize=True, normalize_time=True, row_times=False):
    """``row_times``: each row to its own time (rows that share a time integrate together)."""
    if not row_times:
        return forward(sd, obs, window, ts_pred, method, normalize, normalize_time)
    out = torch.empty(obs.shape[0], obs.shape[1], dtype=torch.float64)
    flat = ts_pred.reshape(-1)
    for t in flat.unique():
        rows = (flat == t).nonzero().reshape(-1)
        out = out.index_copy(0, rows, forward(sd, obs[rows], window[rows], ts_pred[rows], method, normalize, normalize_time))
    return out


def make_dynamics(sd, method, dt=0.05, normalize=True, normalize_time=True):
    """Harness closure (mppi_with_model.py:103-122) for the oracle MPPI."""

    def dynamics(state, window):
        ts = torch.full((state.shape[0], 1), dt, dtype=torch.float64)
        return state + forward(sd, state, window, ts, method, normalize, normalize_time)

    return dynamics
