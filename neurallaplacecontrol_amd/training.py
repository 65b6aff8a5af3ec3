"""Fused training step of ``NeuralLaplaceModel`` (``NLTrainer``) and of the ``DeltaTRNN`` / ``RNN`` baselines
(``RNNTrainer``): the reference's training iteration (``train_utils.py:388-408``) --

    pred_sd = model(bs0, ba0, bts); loss = nn.MSELoss()(pred_sd.squeeze(), bsd.squeeze())
    loss.backward(); torch.nn.utils.clip_grad_norm_(model.parameters(), clip); optimizer.step()   # Adam

-- as three HIP launches (``nlc_train_step`` / ``nlc_rnn_train_step``, ``include/nlc.h``): forward + backward of a 16-row tile per workgroup,
a fixed-order reduction of the tile gradients, clip + Adam.  No host synchronisation inside, so ``run()`` walks a whole
permutation with the weights, Adam moments and per-iteration losses on the device.

Models the kernels do not take (de Hoog / fixed Talbot / Stehfest, widths other than 64 / 128 / 256, ...) train through
the reference's op sequence -- the model's grad-mode forward + ``clip_grad_norm_`` + ``torch.optim.Adam`` -- from
construction on, with one warning.  A fused trainer sends a single call the library refuses (a window longer than 16, a
model setting changed to one the kernels do not take) through the same op sequence, on the trainer's own Adam state, also
with one warning.

What does not depend on the model -- the flat parameter buffer and its views, the workspace cache, the re-upload of a changed
model descriptor, the grad-mode fallbacks on the shared Adam state, ``run()`` and the optimiser state -- is ``_FusedTrainer``;
a trainer class names its three library entries and says which models it takes.
"""

import ctypes as C
import warnings

import torch

from . import _lib
from .laplace import compute_device


def _i64_ptr(t, offset=0):
    assert t.dtype == torch.int64 and t.is_contiguous()
    return C.c_void_p(t.data_ptr() + 8 * offset)


def _f64_ptr(t, offset=0):
    if t is None:
        return C.c_void_p(0)
    assert t.dtype == torch.float64 and t.is_contiguous()
    return C.c_void_p(t.data_ptr() + 8 * offset)


class _FusedTrainer:
    """``tr = Trainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1)``

    * ``tr.loss_and_grad(bs0, ba0, bts, bsd)`` -- loss (0-dim device tensor) and ``p.grad`` of every parameter;
    * ``tr.step(bs0, ba0, bts, bsd)`` -- one reference iteration (loss, backward, clip, Adam); the loss BEFORE the update;
    * ``tr.run(s0, a0, sn, ts, permutation, batch_size=16)`` -- every full batch of ``permutation`` (``bsd = sn - s0``) on the
      device, one loss per iteration;
    * ``tr.state_dict()`` / ``tr.load_state_dict(sd)`` -- ``torch.optim.Adam``'s format.

    ``tr.lr`` may change between calls (what a ``StepLR`` would do).  After ``step()`` / ``run()`` the model's parameters
    hold the new weights, written in place (their ``_version`` moves, so ``model.forward`` and planners re-upload).  The
    model's buffers and settings (normalisation constants, ``normalize`` / ``normalize_time``, ``ilt_options``) are
    re-read before every call: a change after construction (``model.load_state_dict(checkpoint)``, say) takes effect."""

    _entries = None  # the library's (workspace_bytes, loss_grad, step) of the model family
    _reads_ts = True  # False: the model ignores ts_pred, and the kernels get no ts pointer (a property where it varies)

    def _unsupported(self, model):
        """Why no fused kernels exist for ``model`` whatever its shape (None: ask the library)."""
        return None

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1):
        params = list(model.parameters())
        model._require_float64()
        if not params[0].is_cuda:
            raise RuntimeError("training: move the model to the GPU first (model.to('cuda'))")
        self.model = model
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.clip_grad_norm = float(weight_decay), float(clip_grad_norm)
        self._dev = compute_device(params[0])
        named = dict(model.named_parameters())
        self._params = [named[k] for k in model._BLOB_KEYS]  # blob order (= model.parameters() order)
        self._sizes = [p.numel() for p in self._params]
        self._fallback = None
        self._name = type(self).__name__
        why = self._unsupported(model)
        if why is None:
            self._ctx = _lib.Ctx(self._dev.index)
            self._model_key = None
            why = self._sync_model()
        if why is not None:
            warnings.warn(f"{self._name}: {why} -- this model trains through its grad-mode forward + clip_grad_norm_ + "
                          "torch.optim.Adam instead of the fused HIP step", stacklevel=2)
            self._fallback = torch.optim.Adam(params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
            return
        P = sum(self._sizes)
        self._flat = torch.empty(P, dtype=torch.float64, device=self._dev)
        self._m = torch.zeros(P, dtype=torch.float64, device=self._dev)
        self._v = torch.zeros(P, dtype=torch.float64, device=self._dev)
        self._step = 0
        self._ws = {}
        self._arange = {}
        self._warned = False

    @property
    def fused(self):
        """True when the fused HIP step runs (False: the fallback's torch optimiser)."""
        return self._fallback is None

    # ------------------------------------------------------------------ plumbing
    def _model_state_key(self):
        """What the kernels read from the model descriptor besides the weights: the buffers (normalisation, dt) and the
        settings of ``_weights_key_extra()``.  Not the parameters: the trainer's own write-back moves their versions, and
        the kernels read the weights from ``_flat`` on every call."""
        m = self.model
        return (tuple((id(b), b.data_ptr(), b._version) for b in m.buffers()), m._wk_dirty, tuple(m._weights_key_extra()))

    def _sync_model(self):
        """Re-upload the model descriptor if the buffers or settings changed since the last upload.  Returns None when the
        descriptor in the ctx is current, else the library's reason for refusing the new one (the fused kernels must not
        run then: the ctx still holds the old constants)."""
        key = self._model_state_key()
        if self._model_key is not None and self._model_key[0] == key:
            return self._model_key[1]
        why = None
        try:
            self.model.upload(self._ctx)
        except _lib.NlcError as err:
            if err.code != _lib.NLC_ERR_UNSUPPORTED:
                raise
            why = str(err)
        self._model_key = (key, why)
        return why

    def _host_path(self, why):
        """A call the fused kernels do not take: warn once per trainer."""
        if not self._warned:
            self._warned = True
            warnings.warn(f"{self._name}: {why} -- calls the library refuses run the grad-mode forward + clip_grad_norm_ + "
                          "torch.optim.Adam on the trainer's optimiser state instead of the fused HIP step", stacklevel=3)

    def _views(self, flat):
        out, o = [], 0
        for p, n in zip(self._params, self._sizes):
            out.append(flat[o : o + n].view_as(p))
            o += n
        return out

    def _gather(self):
        torch.cat([p.detach().reshape(-1) for p in self._params], out=self._flat)

    def _scatter(self):
        with torch.no_grad():
            for p, v in zip(self._params, self._views(self._flat)):
                p.copy_(v)

    def _workspace(self, N):
        ws = self._ws.get(N)
        if ws is None:
            n = getattr(self._ctx.lib, self._entries[0])(self._ctx.h, N)
            if n < 0:
                raise _lib.NlcError(n, self._entries[0])
            ws = self._ws[N] = torch.empty((n + 7) // 8, dtype=torch.float64, device=self._dev)
        return ws

    def _desc(self):
        return _lib.TrainDesc(self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.clip_grad_norm)

    def _data(self, s0, a0, ts, target):
        f64 = lambda t: torch.as_tensor(t).detach().to(self._dev, torch.float64).contiguous()  # noqa: E731
        obs, win, tgt = f64(s0), f64(a0), f64(target)
        ts = f64(ts).reshape(-1) if self._reads_ts else None
        if win.dim() == 2:
            win = win.unsqueeze(1)
        N = obs.shape[0]
        if (ts is not None and ts.numel() != N) or tgt.numel() != obs.numel() or win.shape[0] != N:
            raise ValueError("training batch: s0 (N, d), a0 (N, B, nin), ts (N,) or (N, 1), target (N, d)")
        return obs, win, ts, tgt.reshape(obs.shape)

    def _idx(self, N):
        idx = self._arange.get(N)
        if idx is None:
            idx = self._arange[N] = torch.arange(N, dtype=torch.int64, device=self._dev)
        return idx

    def _ref_loss(self, bs0, ba0, bts, bsd):
        pred = self.model(bs0, ba0, bts)
        return torch.nn.functional.mse_loss(pred.squeeze(), bsd.squeeze())

    # ------------------------------------------------------------------ API
    def loss_and_grad(self, bs0, ba0, bts, bsd):
        """Loss of the batch and ``p.grad`` of every parameter (train_utils.py:391-402); no update."""
        why = None if not self.fused else self._sync_model()
        if not self.fused or why is not None:
            if why is not None:
                self._host_path(why)
            return self._host_loss_and_grad(bs0, ba0, bts, bsd)
        obs, win, ts, tgt = self._data(bs0, ba0, bts, bsd)
        N = obs.shape[0]
        self._gather()
        grad = torch.empty_like(self._flat)
        loss = torch.empty((), dtype=torch.float64, device=self._dev)
        ctx = self._ctx
        with ctx.stream():
            rc = getattr(ctx.lib, self._entries[1])(
                ctx.h, _f64_ptr(self._flat), _f64_ptr(obs), _f64_ptr(win), _f64_ptr(ts), _f64_ptr(tgt), _i64_ptr(self._idx(N)),
                N, win.shape[1], _f64_ptr(grad), _f64_ptr(loss), _f64_ptr(self._workspace(N)))
        why = self._refused(rc)
        if why is not None:
            self._host_path(why)
            return self._host_loss_and_grad(bs0, ba0, bts, bsd)
        for p, g in zip(self._params, self._views(grad)):
            p.grad = g
        return loss

    def step(self, bs0, ba0, bts, bsd):
        """One iteration of the reference's loop (train_utils.py:391-404); returns the loss before the update."""
        if not self.fused:
            return self._fallback_step(bs0, ba0, bts, bsd)
        why = self._sync_model()
        if why is not None:
            return self._host_steps(why, [(bs0, ba0, bts, bsd)])[0]
        obs, win, ts, tgt = self._data(bs0, ba0, bts, bsd)
        N = obs.shape[0]
        self._gather()
        loss = torch.empty((), dtype=torch.float64, device=self._dev)
        ctx = self._ctx
        with ctx.stream():
            try:
                self._launch_step(_i64_ptr(self._idx(N)), obs, win, ts, tgt, N, _f64_ptr(loss), self._workspace(N))
            except _lib.NlcError as err:
                if err.code != _lib.NLC_ERR_UNSUPPORTED:
                    raise
                return self._host_steps(str(err), [(bs0, ba0, bts, bsd)])[0]
        self._scatter()
        return loss

    def _launch_step(self, idx_ptr, obs, win, ts, tgt, N, loss_ptr, ws, desc=None):
        """One ``nlc_train_step`` / ``nlc_rnn_train_step``; the Adam step count moves only once the library has accepted the call (it checks
        everything on the host before the first launch)."""
        ctx = self._ctx
        ctx.check(getattr(ctx.lib, self._entries[2])(
            ctx.h, C.byref(desc if desc is not None else self._desc()), _f64_ptr(self._flat), _f64_ptr(self._m),
            _f64_ptr(self._v), self._step + 1, _f64_ptr(obs), _f64_ptr(win), _f64_ptr(ts), _f64_ptr(tgt), idx_ptr, N,
            win.shape[1], loss_ptr, None, _f64_ptr(ws)))
        self._step += 1

    def _refused(self, rc):
        """None if the library took the call, its reason if it refused the shape (NLC_ERR_UNSUPPORTED); raises otherwise."""
        if rc == _lib.NLC_ERR_UNSUPPORTED:
            return (self._ctx.lib.nlc_last_error(self._ctx.h) or b"").decode()
        self._ctx.check(rc)
        return None

    def _host_loss_and_grad(self, bs0, ba0, bts, bsd):
        self.model.zero_grad()
        loss = self._ref_loss(bs0, ba0, bts, bsd)
        loss.backward()
        return loss.detach()

    def _host_steps(self, why, batches):
        """Iterations the fused kernels refused, on the grad-mode path with a transient torch.optim.Adam that starts from
        the trainer's step count and moments and hands them back: the trainer keeps one optimiser state."""
        self._host_path(why)
        opt = self._adam()
        self._export_state(opt)
        out = [self._fallback_step(*b, opt=opt) for b in batches]
        st = opt.state.get(self._params[0])
        if st is not None:
            with torch.no_grad():
                for p, m, v in zip(self._params, self._views(self._m), self._views(self._v)):
                    m.copy_(opt.state[p]["exp_avg"])
                    v.copy_(opt.state[p]["exp_avg_sq"])
            self._step = int(st["step"])
        return out

    def _fallback_step(self, bs0, ba0, bts, bsd, opt=None):
        opt = self._fallback if opt is None else opt
        for grp in opt.param_groups:
            grp["lr"] = self.lr
        opt.zero_grad()
        loss = self._ref_loss(bs0, ba0, bts, bsd)
        loss.backward()
        if self.clip_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.clip_grad_norm)
        opt.step()
        return loss.detach()

    def run(self, s0, a0, sn, ts, permutation, batch_size=16):
        """Every full batch of ``permutation`` (train_utils.py:388-408 with ``bsd = bsn - bs0``): returns the (iters,) losses
        on the device.  Fused: the dataset stays where it is, each iteration is one ``nlc_train_step`` on its slice of the
        permutation, nothing crosses to the host until the end."""
        bs = int(batch_size)
        iters = int(permutation.shape[0]) // bs

        def host(why=None):
            s0_, a0_, sn_, ts_ = (torch.as_tensor(t).to(self._dev) for t in (s0, a0, sn, ts))
            perm = torch.as_tensor(permutation).to(self._dev)
            batches = []
            for i in range(iters):
                ind = perm[i * bs : i * bs + bs]
                batches.append((s0_[ind], a0_[ind], ts_[ind], sn_[ind] - s0_[ind]))
            out = [self._fallback_step(*b) for b in batches] if why is None else self._host_steps(why, batches)
            return torch.stack(out) if out else torch.empty(0, dtype=torch.float64, device=self._dev)

        if not self.fused:
            return host()
        why = self._sync_model() if iters > 0 else None
        if why is not None:
            return host(why)
        obs, win, tsd, sn_d = self._data(s0, a0, ts, sn)
        tgt = sn_d - obs
        perm = torch.as_tensor(permutation).to(self._dev, torch.int64).contiguous()
        losses = torch.empty(iters, dtype=torch.float64, device=self._dev)
        if iters == 0:
            return losses
        ws = self._workspace(bs)
        self._gather()
        desc = self._desc()
        ctx = self._ctx
        with ctx.stream():
            for i in range(iters):
                try:
                    self._launch_step(_i64_ptr(perm, i * bs), obs, win, tsd, tgt, bs, _f64_ptr(losses, i), ws, desc)
                except _lib.NlcError as err:
                    # the library checks the shape on the host before any launch, and the shape is the same for every
                    # iteration: only the first can be refused, with nothing launched
                    if err.code != _lib.NLC_ERR_UNSUPPORTED or i > 0:
                        raise
                    return host(str(err))
        self._scatter()
        return losses

    # ------------------------------------------------------------------ optimiser state
    def _adam(self):
        return torch.optim.Adam(self.model.parameters(), lr=self.lr, betas=self.betas, eps=self.eps,
                                weight_decay=self.weight_decay)

    def _export_state(self, opt):
        """The trainer's step count and moments as ``opt.state`` (copies)."""
        if self._step > 0:
            sdt = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
            for p, m, v in zip(self._params, self._views(self._m), self._views(self._v)):
                opt.state[p] = {"step": torch.tensor(float(self._step), dtype=sdt), "exp_avg": m.clone(),
                                "exp_avg_sq": v.clone()}

    def state_dict(self):
        """``torch.optim.Adam(model.parameters(), ...).state_dict()`` of the same optimiser state."""
        if not self.fused:
            return self._fallback.state_dict()
        opt = self._adam()
        self._export_state(opt)
        return opt.state_dict()

    def load_state_dict(self, sd):
        """Take over a ``torch.optim.Adam`` state (hyper-parameters of its first group, step and moments).  An
        ``amsgrad`` or ``maximize`` state is refused: the trainer's update has neither."""
        for grp in sd.get("param_groups", []):
            for flag in ("amsgrad", "maximize"):
                if grp.get(flag):
                    raise ValueError(f"{self._name}.load_state_dict: an Adam state with {flag}=True is not supported "
                                     "(the trainer runs plain Adam)")
        if not self.fused:
            self._fallback.load_state_dict(sd)
            grp = self._fallback.param_groups[0]
            self.lr = float(grp["lr"])
            return
        opt = self._adam()
        opt.load_state_dict(sd)
        grp = opt.param_groups[0]
        self.lr, self.betas, self.eps = float(grp["lr"]), tuple(float(b) for b in grp["betas"]), float(grp["eps"])
        self.weight_decay = float(grp["weight_decay"])
        steps = {int(opt.state[p]["step"]) for p in self._params if p in opt.state}
        if len(steps) > 1:
            raise ValueError(f"{self._name} keeps one Adam step count for all parameters")
        self._step = steps.pop() if steps else 0
        with torch.no_grad():
            for p, m, v in zip(self._params, self._views(self._m), self._views(self._v)):
                st = opt.state.get(p)
                m.copy_(st["exp_avg"] if st else torch.zeros_like(m))
                v.copy_(st["exp_avg_sq"] if st else torch.zeros_like(v))


class NLTrainer(_FusedTrainer):
    """``tr = NLTrainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1)`` for a
    ``NeuralLaplaceModel``; the fused step takes Fourier models (``nlc_train_step``)."""

    _entries = ("nlc_train_workspace_bytes", "nlc_train_loss_grad", "nlc_train_step")

    def _unsupported(self, model):
        if model.ilt_algorithm != "fourier":
            return f"ilt_algorithm {model.ilt_algorithm!r} has no fused training kernels (fourier only)"
        return None


class RNNTrainer(_FusedTrainer):
    """``tr = RNNTrainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1)`` for a
    ``DeltaTRNN`` or an ``RNN`` (``nlc_rnn_train_step``): the methods and semantics of ``NLTrainer``.  An ``RNN`` ignores
    ``ts`` as its forward does; the reference's loop still passes it, so every method accepts it."""

    _entries = ("nlc_rnn_train_workspace_bytes", "nlc_rnn_train_loss_grad", "nlc_rnn_train_step")

    @property
    def _reads_ts(self):
        return bool(self.model._time_input)
