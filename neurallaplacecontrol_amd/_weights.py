"""What the nn.Module mirrors of the reference models (NL model, Delta-t RNN / RNN, NODE) share on the way to an ``nlc_ctx``.

``WeightsKeyMixin`` -- change detection for the weights a mirror has uploaded.  A planner asks ``weights_key(model)`` once per
``command()`` (``MPPIDelay._ensure_configured``) and re-uploads (``nlc_set_model``) when the key differs from the one it
uploaded at.  The key is ``(data_ptr, _version)`` of every parameter and buffer:

* an in-place write (``p.mul_(2)`` under ``no_grad``, an optimizer step, ``load_state_dict``) bumps ``_version``;
* a replaced tensor (``lin.weight = nn.Parameter(...)``, ``model.state_std = t``, ``.to()/.double()/.cuda()``) is a new
  registration: torch's global parameter / buffer registration hooks bump a process-wide epoch here, and the cached
  tensor list is re-collected when the epoch moved (so the per-command cost stays a 20-tuple build, ~4 us);
* NOT detectable: a write through ``p.data`` (``p.data.mul_(2)``) -- ``.data`` is an alias with its own version counter.
  Call ``model.mark_weights_dirty()`` after such a write.

``HipModelMirror`` -- the HIP plumbing on top of it, written once: the normalisation buffers and the tail of
``from_reference``, the normalisation constants of a model descriptor (and back, as device tensors), ``upload(ctx)`` /
``hip_ctx(device)``, and the float64 / no-grad / model-on-the-GPU guards.  A mirror declares ``_BLOB_KEYS``, its two library
symbols and ``_dyn_id``, and keeps ``model_desc()``: which of the reference's normalisation branches it is in.
"""

import ctypes as C

import torch
import torch.nn.modules.module as _tm

from . import _lib
from .laplace import compute_device

_EPOCH = [0]


def _bump(*_args):
    _EPOCH[0] += 1
    return None


_tm.register_module_parameter_registration_hook(_bump)
_tm.register_module_buffer_registration_hook(_bump)
_tm.register_module_module_registration_hook(_bump)


class WeightsKeyMixin:
    """``_weights_key()`` / ``mark_weights_dirty()`` for the nn.Module mirrors (NL model, Delta-t RNN / RNN, NODE)."""

    _wk_epoch = -1
    _wk_tensors = None
    _wk_dirty = 0

    def _weights_key_extra(self):
        return ()

    def _apply(self, fn, *args, **kwargs):
        # .float().double() / .half().double() / .to(...) re-allocate through `param.data = fn(param.data)`: the Parameter
        # object and its version counter survive and the caching allocator may hand back the very block just freed, so
        # (data_ptr, _version) can stay equal although the values were rounded.  Conversions are rare: bump.
        self._wk_dirty += 1
        return super()._apply(fn, *args, **kwargs)

    def mark_weights_dirty(self):
        """Force the next planner command / forward to re-upload the weights (needed after a ``.data`` write)."""
        self._wk_dirty += 1

    def _weights_key(self):
        if self._wk_tensors is None or self._wk_epoch != _EPOCH[0]:
            self._wk_tensors = [p for p in self.parameters()] + [b for b in self.buffers()]
            self._wk_epoch = _EPOCH[0]
        return tuple([(t.data_ptr(), t._version) for t in self._wk_tensors]) + (self._wk_dirty,) + tuple(self._weights_key_extra())


def _f64(t):
    return t.detach().to("cpu", torch.float64).reshape(-1)


class HipModelMirror(WeightsKeyMixin):
    """Base of the four mirrors (mixed in before ``nn.Module``).  Each class declares:"""

    _BLOB_KEYS = ()  # state_dict keys in the order of the weight blob its set call expects (include/nlc.h)
    _blob_size_symbol = _set_model_symbol = None  # nlc_*_blob_size(desc) and nlc_set_*model(ctx, desc, blob, n)
    _dyn_id = None  # rollout the fused planner selects for NLDynamics(model, dt)
    _NORM_BUFFERS = ("state_mean", "state_std", "action_mean", "action_std", "dt")  # the reference's, in its order

    # ------------------------------------------------------------------ construction
    def _register_norm_buffers(self, state_mean, state_std, action_mean, action_std, dt=None):
        """The buffers ``_NORM_BUFFERS`` names (RNN's list ends before ``dt``), with the reference's dtypes (w_nl.py:111-115,
        train_utils.py:613-617): ``torch.tensor(dt)`` is FLOAT32, so after ``.double()`` the time normaliser is float32(0.05)
        widened; an ``action_mean`` built from ``np.array([0] * nu)`` is int64.  Also: no ctx yet, nothing uploaded."""
        for name, value in zip(self._NORM_BUFFERS, (state_mean, state_std, action_mean, action_std, dt)):
            self.register_buffer(name, torch.tensor(value))
        self._ctx = self._uploaded_key = None

    def _take_over(self, ref):
        """Tail of ``from_reference``: ``ref``'s device and dtype, its buffers (dtypes included), weights and mode."""
        first = next(ref.parameters())
        m = self.to(device=first.device, dtype=first.dtype)
        for name in self._NORM_BUFFERS:
            m.register_buffer(name, getattr(ref, name).detach().clone())
        m.load_state_dict(ref.state_dict())
        m.train(ref.training)
        return m

    # ------------------------------------------------------------------ normalisation constants
    def _fill_norm_constants(self, desc, d, nin, normalised):
        """``state_mean / state_std`` (d entries) and, unless ``nin`` is None (NODE), ``action_mean / action_std`` (nin entries,
        a scalar buffer broadcast) of any model descriptor.  Normalised: the buffers; raw inputs: mean 0, std 1 and the
        reference's ``actions / 3``."""
        if normalised:
            sm, ss = _f64(self.state_mean), _f64(self.state_std)
            fits = sm.numel() == d and ss.numel() == d
            if nin is None:
                if not fits:
                    raise ValueError("normalisation buffers do not match state_dim")
            else:
                am, a_s = (t.expand(nin) if t.numel() == 1 else t for t in (_f64(self.action_mean), _f64(self.action_std)))
                if not fits or am.numel() != nin or a_s.numel() != nin:
                    raise ValueError("normalisation buffers do not broadcast against the model's input dims")
        else:
            sm, ss, am, a_s = [0.0] * d, [1.0] * d, [0.0] * (nin or 0), [3.0] * (nin or 0)
        for i in range(d):
            desc.state_mean[i], desc.state_std[i] = float(sm[i]), float(ss[i])
        for i in range(nin or 0):
            desc.action_mean[i], desc.action_std[i] = float(am[i]), float(a_s[i])

    def _time_div(self):
        """What the model divides a prediction time by under ``normalize_time`` (``dt * 8``), else 1."""
        return float(_f64(self.dt)[0] * 8.0) if self.normalize_time else 1.0

    @staticmethod
    def _norm_tensors(desc, dtype, device):
        """A descriptor's constants back as device tensors: ``(state_mean, state_std)`` and, where it carries them,
        ``(..., action_mean, action_std)``."""
        mk = lambda a, n: torch.tensor(list(a)[:n], dtype=dtype, device=device)  # noqa: E731
        out = (mk(desc.state_mean, desc.d), mk(desc.state_std, desc.d))
        if hasattr(desc, "action_mean"):
            out += (mk(desc.action_mean, desc.nin), mk(desc.action_std, desc.nin))
        return out

    # ------------------------------------------------------------------ weights into a ctx
    def _require_float64(self):
        if any(p.dtype != torch.float64 for p in self.parameters()):
            raise NotImplementedError(
                "the HIP path computes in float64 only: call model.double() first (reference: mppi_with_model.py:101)"
            )

    def upload(self, ctx):
        """Pack the current weights into ``ctx`` (the class's ``nlc_set_*model``); returns the key they were taken at.
        Planners keep their own ctx (planner state lives there) and call this when the key changes."""
        self._require_float64()
        key = self._weights_key()
        sd = self.state_dict()
        blob = torch.cat([_f64(sd[k]) for k in self._BLOB_KEYS]).contiguous()
        desc = self.model_desc()
        n = getattr(ctx.lib, self._blob_size_symbol)(C.byref(desc))
        if n != blob.numel():
            raise ValueError(f"weight blob has {blob.numel()} doubles, library expects {n}")
        ctx.check(getattr(ctx.lib, self._set_model_symbol)(ctx.h, C.byref(desc), _lib.ptr(blob), blob.numel()))
        return key

    def _ctx_options(self):
        """``nlc_set_option`` settings that belong to the model's descriptor without being part of its struct (NODE: the
        solver).  ``sync_to`` sets them with every upload."""
        return {}

    def sync_to(self, ctx):
        """``upload(ctx)`` after the model's ctx options: what the model's own ctx, planners and trainers call."""
        for name, value in self._ctx_options().items():
            ctx.set_option(name, value)
        return self.upload(ctx)

    def hip_ctx(self, device=None):
        """The model's own ``nlc_ctx`` (its forward's) with its current weights uploaded."""
        dev = compute_device(next(self.parameters())) if device is None else torch.device(device)
        if self._ctx is None or self._ctx.device_index != dev.index:
            self._ctx = _lib.Ctx(dev.index)
            self._uploaded_key = None
        if self._weights_key() != self._uploaded_key:
            self._uploaded_key = self.sync_to(self._ctx)
        return self._ctx

    # ------------------------------------------------------------------ guards
    def _no_grad_only(self):
        if torch.is_grad_enabled():
            raise NotImplementedError(
                f"neurallaplacecontrol_amd.{type(self).__name__} is inference-only on the HIP path: "
                "wrap the call in torch.no_grad() (as the reference harness does, mppi_with_model.py:319)"
            )

    def _train_device(self, dev=None, mod=None):
        """The GPU the parameters of ``mod`` (default: the model) live on, for a grad-mode forward: there is no CPU path in
        this package, training included.  ``dev``: the device the forward computes on, which they must be on."""
        have = next((self if mod is None else mod).parameters()).device
        if have.type != "cuda" or (dev is not None and have != dev):
            raise RuntimeError("training forward: move the model to the GPU first (model.to('cuda'))")
        return have
