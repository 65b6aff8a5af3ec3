"""MI355X twin of the reference's Delta-t RNN baseline, ``train_utils.DeltaTRNN`` (``train_utils.py:589-631``;
factory ``get_delta_t_rnn_model`` ``:56-74``, ``rnn_hidden_units=160`` ``config.py:43``): same constructor
arguments, sub-module names and ``state_dict`` keys (``gru.*``, ``linear_out.*``, buffers ``state_mean state_std
action_mean action_std dt``), so checkpoints written by the reference load unchanged.

The plain ``RNN`` baseline (``train_utils.py:550-586``: the same GRU, ``linear_out`` over ``[h | obs]``, no time input,
the un-normalised branch tied to ``normalize``) shares the kernels (``nlc_rnn_desc.time_input = 0``).

``forward`` runs as two HIP launches behind ``nlc_rnn_forward`` (GRU on FP64 matrix cores + hidden part of
``linear_out``; then the state/time part); behind ``NLDynamics`` the planner hoists the GRU out of the horizon loop
(``NLC_DYN_DTRNN``).  The HIP path is inference-only and float64, as the harness uses it
(``mppi_with_model.py:101,319``); in grad mode ``forward`` is the same op sequence on PyTorch-ROCm (trainable).

One constructor body, ``model_desc`` and forward serve both classes through two class-level switches (``_time_input``,
``_normalised_by``); the plumbing every mirror shares (normalisation buffers and constants, ``upload`` / ``hip_ctx``, the
guards) is ``_weights.HipModelMirror``.
"""

import torch
import torch.nn as nn

from . import _lib
from ._weights import HipModelMirror
from .laplace import compute_device


class DeltaTRNN(HipModelMirror, nn.Module):
    _dyn_id = _lib.DYN_DTRNN
    _BLOB_KEYS = ["gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "linear_out.weight",
                  "linear_out.bias"]
    _blob_size_symbol, _set_model_symbol = "nlc_rnn_blob_size", "nlc_set_rnn_model"
    _time_input = 1  # linear_out sees [h | obs | delta t] and the GRU the time stamps of encode_obs_time; RNN: neither
    _normalised_by = "normalize_time"  # the flag that selects the normalised branch (train_utils.py:618-626)

    def __init__(
        self,
        state_dim,
        action_dim,
        hidden_units=64,
        encode_obs_time=False,
        state_mean=None,
        state_std=None,
        action_mean=None,
        action_std=None,
        normalize=False,
        normalize_time=False,
        dt=0.05,
    ):
        super().__init__()
        self.encode_obs_time = encode_obs_time
        self.state_dim, self.action_dim, self.hidden_units = state_dim, action_dim, hidden_units
        self.gru = nn.GRU(self._nin(), hidden_units, batch_first=True)
        self.linear_out = nn.Linear(hidden_units + state_dim + self._time_input, state_dim)
        self.normalize = normalize
        self.normalize_time = normalize_time
        self._register_norm_buffers(state_mean, state_std, action_mean, action_std, dt)

    def _nin(self):
        """GRU input width.  The reference's RNN ignores ``encode_obs_time`` when sizing the GRU (train_utils.py:550-586)."""
        return self.action_dim + (1 if self.encode_obs_time and self._time_input else 0)

    @classmethod
    def from_reference(cls, ref):
        """Twin of a loaded reference ``DeltaTRNN`` (same hyper-parameters, buffers and weights, on its device)."""
        d = ref.linear_out.out_features
        enc = bool(ref.encode_obs_time)
        return cls(
            d, ref.gru.input_size - int(enc), hidden_units=ref.gru.hidden_size, encode_obs_time=enc,
            state_mean=[0.0] * d, state_std=[1.0] * d, action_mean=[0], action_std=[1.0],
            normalize=ref.normalize, normalize_time=ref.normalize_time,
        )._take_over(ref)

    # ------------------------------------------------------------------ HIP plumbing
    def _weights_key_extra(self):
        return (self.normalize, self.normalize_time)

    def model_desc(self):
        """Resolve the reference's branch structure.  DeltaTRNN (train_utils.py:618-626): the raw-input ``else`` belongs to
        ``if self.normalize_time``; normalize=False with normalize_time=True leaves ``batch_obs`` undefined there.  RNN
        (:550-586): ``normalize`` alone decides, and there is no time to normalise."""
        desc = _lib.RnnDesc()
        desc.d, desc.nin, desc.hidden, desc.time_input = self.state_dim, self._nin(), self.hidden_units, self._time_input
        if self._time_input and self.normalize_time and not self.normalize:
            raise NameError("DeltaTRNN(normalize=False, normalize_time=True): the reference's forward fails "
                            "(batch_obs is undefined, train_utils.py:618-631)")
        self._fill_norm_constants(desc, desc.d, desc.nin, getattr(self, self._normalised_by))
        desc.time_div = self._time_div() if self._time_input else 1.0
        return desc

    def _forward_train(self, in_batch_obs, in_batch_action, ts_pred):
        """Grad-mode forward for training (``train_utils.py:388-407``): the reference's op sequence (``:618-631``) on
        PyTorch-ROCm modules; the HIP kernels serve inference / planning."""
        dev = self._train_device()
        obs, act = in_batch_obs.to(dev), in_batch_action.to(dev)
        desc = self.model_desc()  # resolves (and rejects) the reference's normalisation branches
        sm, ss, am, a_s = self._norm_tensors(desc, obs.dtype, dev)
        out, _ = self.gru((act - am) / a_s)
        feats = [out[:, -1, :], (obs - sm) / ss]
        if desc.time_input:
            feats.append(torch.as_tensor(ts_pred).to(dev, obs.dtype).reshape(obs.shape[0], 1) / desc.time_div)
        return self.linear_out(torch.cat(feats, dim=1)).to(in_batch_obs.device)

    def forward(self, in_batch_obs, in_batch_action, ts_pred):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._forward_train(in_batch_obs, in_batch_action, ts_pred)
        self._no_grad_only()
        out_device = in_batch_obs.device
        dev = compute_device(in_batch_obs, in_batch_action, next(self.parameters()))
        ctx = self.hip_ctx(dev)
        obs = in_batch_obs.detach().to(dev, torch.float64).contiguous()
        win = in_batch_action.detach().to(dev, torch.float64).contiguous()
        N, d = obs.shape
        ts = torch.as_tensor(ts_pred).detach().to(dev, torch.float64).reshape(-1).contiguous()
        if ts.numel() != N:
            raise ValueError("ts_pred must hold one prediction time per row (the reference concatenates it per row)")
        out = torch.empty((N, d), dtype=torch.float64, device=dev)
        ws = torch.empty((N, d), dtype=torch.float64, device=dev)
        ctx.launch(ctx.lib.nlc_rnn_forward, _lib.ptr(obs), _lib.ptr(win), _lib.ptr(ts), N, win.shape[1], _lib.ptr(out),
                   _lib.ptr(ws))
        return out.to(out_device)


class RNN(DeltaTRNN):
    """Twin of ``train_utils.RNN`` (``:550-586``): ``linear_out(cat(gru(actions)[:, -1], obs))``; ``ts_pred`` is
    ignored; ``normalize=False`` selects raw observations and actions / 3."""

    _NORM_BUFFERS = DeltaTRNN._NORM_BUFFERS[:4]  # the reference's RNN has no dt buffer
    _time_input = 0
    _normalised_by = "normalize"

    def __init__(self, state_dim, action_dim, hidden_units=64, encode_obs_time=False, state_mean=None, state_std=None,
                 action_mean=None, action_std=None, normalize=False):
        super().__init__(state_dim, action_dim, hidden_units, encode_obs_time, state_mean, state_std, action_mean, action_std,
                         normalize)  # normalize_time stays False: time_div 1

    @classmethod
    def from_reference(cls, ref):
        d = ref.linear_out.out_features
        return cls(d, ref.gru.input_size, hidden_units=ref.gru.hidden_size, encode_obs_time=bool(ref.encode_obs_time),
                   state_mean=[0.0] * d, state_std=[1.0] * d, action_mean=[0], action_std=[1.0],
                   normalize=ref.normalize)._take_over(ref)

    def forward(self, in_batch_obs, in_batch_action, _):
        ts = torch.zeros(in_batch_obs.shape[0], dtype=torch.float64)  # unused by the model (time_input = 0)
        return super().forward(in_batch_obs, in_batch_action, ts)
