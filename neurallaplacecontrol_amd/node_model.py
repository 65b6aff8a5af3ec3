"""MI355X twin of the reference's NODE baseline, ``train_utils.NODE`` / ``xOdeFuncInXAndU``
(``train_utils.py:637-738``; factory ``get_node_model`` ``:101-125``; ``node_hidden_units=270``,
``node_augment_dim=1``, ``node_method="euler"``: ``config.py:40-42``): same constructor arguments, sub-module names and
``state_dict`` keys (``x_ode_func_in_x_and_u.linear_tanh_stack.{0,2,4}.*``, buffers ``state_mean state_std
action_mean action_std dt``), so checkpoints written by the reference load unchanged.

``forward`` is one HIP launch (``nlc_node_forward``): the ODE function's three layers on FP64 matrix cores inside the
fixed-grid solver's loop; behind ``NLDynamics`` the planner runs it inside the horizon loop (``NLC_DYN_NODE``).
``torchdiffeq.odeint(method=..., options={"step_size": 0.05})`` is restated (grid ``k * step_size``, last point =
the end time) for the three fixed-grid solvers used with a ``step_size``: ``method="euler"`` (the default,
``--node_method``), ``"midpoint"`` and ``"rk4"`` -- torchdiffeq's fixed-grid ``rk4`` is the 3/8 rule, not the classic
tableau.  Grid and solvers alike: **parity unpinned vs upstream torchdiffeq**, which is absent offline.  Any other
``method`` raises ``NotImplementedError``.  The tableaus are ``csrc/nlc_node_rk.h``'s (``RK_TABLEAUS`` here restates them
for the grad-mode path); the method reaches the library as the ctx option ``node_method`` with every upload of the
descriptor (``sync_to``), and ``model.method`` may be reassigned: planners and trainers pick the change up at their next call.  The
HIP path is inference-only and float64; in grad mode ``forward`` is the same op sequence in torch ops on PyTorch-ROCm
(trainable).

The plumbing every mirror shares (normalisation buffers and constants, ``upload`` / ``hip_ctx``, the guards) is
``_weights.HipModelMirror``; NODE uses the state half of the constants only.
"""

import math

import torch
import torch.nn as nn

from . import _lib
from ._weights import HipModelMirror
from .laplace import compute_device


class xOdeFuncInXAndU(nn.Module):  # noqa: N801  (reference class name, train_utils.py:637)
    def __init__(self, state_dim=4, action_dim=1, nhidden=50, augment_dim=0):
        super().__init__()
        self.linear_tanh_stack = nn.Sequential(
            nn.Linear(state_dim + action_dim + augment_dim, nhidden),
            nn.Tanh(),
            nn.Linear(nhidden, nhidden),
            nn.Tanh(),
            nn.Linear(nhidden, state_dim + augment_dim),
        )
        for m in self.linear_tanh_stack.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
        self.state_dim, self.action_dim, self.augment_dim = state_dim, action_dim, augment_dim
        self.u = None

    def update_u(self, u):
        self.u = u

    def forward(self, t, x):  # stand-alone use goes through PyTorch-ROCm; NODE.forward uses the HIP kernel
        return self.linear_tanh_stack(torch.cat((x, self.u), 1))


# method -> (ctx option "node_method", a_ij rows below the diagonal, b_i): csrc/nlc_node_rk.h.  One sub-step of width h:
# Y_i = y + h sum_j a_ij k_j, k_i = f(Y_i), y' = y + h sum_i b_i k_i
RK_TABLEAUS = {
    "euler": (0, ((),), (1.0,)),
    "midpoint": (1, ((), (0.5,)), (0.0, 1.0)),
    "rk4": (2, ((), (1.0 / 3.0,), (-1.0 / 3.0, 1.0), (1.0, -1.0, 1.0)), (0.125, 0.375, 0.375, 0.125)),
}


class NODE(HipModelMirror, nn.Module):
    _dyn_id = _lib.DYN_NODE
    _BLOB_KEYS = [f"x_ode_func_in_x_and_u.linear_tanh_stack.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    _blob_size_symbol, _set_model_symbol = "nlc_node_blob_size", "nlc_set_node_model"
    step_size = 0.05  # options={"step_size": 0.05} (train_utils.py:722)

    def __init__(
        self,
        state_dim,
        action_dim,
        latent_dim,
        hidden_units=64,
        encode_obs_time=False,
        state_mean=None,
        state_std=None,
        action_mean=None,
        action_std=None,
        normalize=False,
        normalize_time=False,
        method="euler",
        augment_dim=0,
        action_high=1.0,
        dt=0.05,
    ):
        super().__init__()
        self._tableau(method)
        self.x_ode_func_in_x_and_u = xOdeFuncInXAndU(
            state_dim=state_dim, action_dim=action_dim, augment_dim=augment_dim, nhidden=hidden_units
        )
        self.method = method
        self.state_dim, self.hidden_units = state_dim, hidden_units
        self.augment_dim = augment_dim
        self.action_dim = action_dim
        self.action_high = action_high
        self.normalize = normalize
        self.encode_obs_time = encode_obs_time
        self.normalize_time = normalize_time
        self._register_norm_buffers(state_mean, state_std, action_mean, action_std, dt)

    @classmethod
    def from_reference(cls, ref):
        """Twin of a loaded reference ``NODE`` (same hyper-parameters, buffers and weights, on its device)."""
        f = ref.x_ode_func_in_x_and_u
        return cls(
            f.state_dim, f.action_dim, f.state_dim, hidden_units=f.linear_tanh_stack[0].out_features,
            encode_obs_time=ref.encode_obs_time, state_mean=[0.0] * f.state_dim, state_std=[1.0] * f.state_dim,
            action_mean=[0], action_std=[1.0], normalize=ref.normalize, normalize_time=ref.normalize_time,
            method=ref.method, augment_dim=ref.augment_dim, action_high=ref.action_high,
        )._take_over(ref)

    @staticmethod
    def _tableau(method):
        if method not in RK_TABLEAUS:
            raise NotImplementedError(f"NODE integrates with the fixed-grid solvers {sorted(RK_TABLEAUS)} only "
                                      f"(config.py:40 node_method='euler'); got method={method!r}")
        return RK_TABLEAUS[method]

    @property
    def stages(self):
        """ODE-function evaluations per sub-step of ``method``."""
        return len(self._tableau(self.method)[2])

    # ------------------------------------------------------------------ HIP plumbing
    _weights_key_names = ("normalize", "normalize_time", "step_size", "method")

    def _weights_key_extra(self):
        return (self.normalize, self.normalize_time, self.step_size, self.method)

    def _ctx_options(self):
        """The solver travels beside the descriptor (``nlc_node_desc`` keeps its size): ctx option ``node_method``."""
        return {"node_method": self._tableau(self.method)[0]}

    def model_desc(self):
        d = self.state_dim
        desc = _lib.NodeDesc()
        desc.d, desc.nu, desc.hidden, desc.augment_dim = d, self.action_dim, self.hidden_units, self.augment_dim
        self._fill_norm_constants(desc, d, None, self.normalize)  # the ODE function takes the newest action raw
        desc.time_div = self._time_div()  # normalize_time counts with or without normalize
        desc.step_size = float(self.step_size)
        return desc

    def _forward_train(self, in_batch_obs, in_batch_action, ts_pred):
        """Grad-mode forward for training: the reference's op sequence (``train_utils.py:696-724``) with the restated
        fixed-grid ``odeint`` (``method``'s tableau) in torch ops on PyTorch-ROCm; the HIP kernels serve inference /
        planning and the fused trainers."""
        dev = self._train_device()
        obs, act = in_batch_obs.to(dev), in_batch_action.to(dev)
        desc = self.model_desc()
        sm, ss = self._norm_tensors(desc, obs.dtype, dev)
        x = (obs - sm) / ss
        if self.augment_dim > 0:
            x = torch.cat([x, torch.zeros(obs.shape[0], self.augment_dim, dtype=obs.dtype, device=dev)], 1)
        if act.dim() == 2:
            act = act.unsqueeze(1)
        self.x_ode_func_in_x_and_u.update_u(act[:, -1, :])
        t_end = float(torch.as_tensor(ts_pred).reshape(-1)[0]) / desc.time_div
        niters = int(math.ceil(t_end / self.step_size + 1))
        grid = [k * self.step_size for k in range(niters)]
        grid[-1] = t_end
        _, a, b = self._tableau(self.method)
        f = self.x_ode_func_in_x_and_u
        for k in range(niters - 1):
            h = grid[k + 1] - grid[k]
            if len(b) == 1:
                x = x + h * f(None, x)
                continue
            ks = []
            for row in a:
                ks.append(f(None, x + h * sum(aij * kj for aij, kj in zip(row, ks)) if row else x))
            x = x + h * sum(bi * ki for bi, ki in zip(b, ks))
        return x[:, : x.shape[-1] - self.augment_dim].to(in_batch_obs.device)

    def forward(self, in_batch_obs, in_batch_action, ts_pred):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._forward_train(in_batch_obs, in_batch_action, ts_pred)
        self._no_grad_only()
        out_device = in_batch_obs.device
        dev = compute_device(in_batch_obs, in_batch_action, next(self.parameters()))
        ctx = self.hip_ctx(dev)
        obs = in_batch_obs.detach().to(dev, torch.float64).contiguous()
        act = in_batch_action.detach().to(dev, torch.float64)
        if act.dim() == 2:  # train_utils.py:712-713
            act = act.unsqueeze(1)
        act = act[:, -1, :].contiguous()  # the newest action of the window, raw (:715)
        N, d = obs.shape
        t0 = float(torch.as_tensor(ts_pred).detach().reshape(-1)[0])  # every row integrates to ts_pred[0] (:719)
        out = torch.empty((N, d), dtype=torch.float64, device=dev)
        ctx.launch(ctx.lib.nlc_node_forward, _lib.ptr(obs), _lib.ptr(act), t0, N, _lib.ptr(out))
        return out.to(out_device)
