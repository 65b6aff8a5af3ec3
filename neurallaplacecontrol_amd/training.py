"""Fused training step of ``NeuralLaplaceModel`` (``NLTrainer``), of the ``DeltaTRNN`` / ``RNN`` baselines
(``RNNTrainer``) and of the ``NODE`` baseline (``NODETrainer``): the reference's training iteration (``train_utils.py:388-408``) --

    pred_sd = model(bs0, ba0, bts); loss = nn.MSELoss()(pred_sd.squeeze(), bsd.squeeze())
    loss.backward(); torch.nn.utils.clip_grad_norm_(model.parameters(), clip); optimizer.step()   # Adam

-- as three HIP launches (``nlc_train_step`` / ``nlc_rnn_train_step``, ``include/nlc.h``): forward + backward of a 16-row tile per workgroup,
a fixed-order reduction of the tile gradients, clip + Adam.  No host synchronisation inside, so ``run()`` walks a whole
permutation with the weights, Adam moments and per-iteration losses on the device.

Models the kernels do not take (de Hoog unless the trainer was built with ``dehoog="fused"``, widths other than 64 / 128 /
256, ...) train through
the reference's op sequence -- the model's grad-mode forward + ``clip_grad_norm_`` + ``torch.optim.Adam`` -- from
construction on, with one warning.  A fused trainer sends a single call the library refuses (a window longer than 16, a
model setting changed to one the kernels do not take) through the same op sequence, on the trainer's own Adam state, also
with one warning.

What does not depend on the model -- the flat parameter buffer and its views, the workspace cache, the re-upload of a changed
model descriptor, the grad-mode fallbacks on the shared Adam state, ``run()`` and the optimiser state -- is ``_FusedTrainer``;
a trainer class names its three library entries and says which models it takes.

``NLTrainerGroup`` / ``RNNTrainerGroup`` train M models of one descriptor -- the reference's ``run_exp_multi.py:105-110``
trains one model per (env, delay, model_name), times seeds, and for a fixed env and family those share the architecture and
the normalisation constants -- in the same three launches, the member on the grid's second axis
(``nlc_train_group_step`` / ``nlc_rnn_train_group_step``).  ``_FusedTrainer`` is written over a list of members: a single
trainer is the group of one, and the group classes only change what a call takes (stacked data, ``(M, L)`` permutations) and
returns (``(M,)`` losses, a list of optimiser states).  A member's results are bit-identical to its single trainer's.

A group's ``lr``, ``weight_decay`` and ``clip_grad_norm`` may be sequences of M numbers (the reference's sweeps, ``config.py``
``sweep_mode``), members can be frozen (``freeze`` / ``unfreeze``), and ``fit(patience=)`` freezes each member when it stops
improving (``train_utils.py:315-317``, ``:439-448``): the step is then ``nlc_*_train_group_step_members``, whose Adam launch
reads the settings and an ``active`` flag per member from device arrays; a group of scalar settings calls what it always has.
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


def step_lr_after_epoch(lr, epochs_done, step_size, gamma):
    """The learning rate after ``torch.optim.lr_scheduler.StepLR(opt, step_size, gamma).step()`` has brought the epoch count
    to ``epochs_done``, from the rate before it: a chained multiply when the count reaches a multiple of ``step_size``
    (StepLR's recursive form), not ``lr0 * gamma ** k``."""
    return lr * gamma if epochs_done > 0 and epochs_done % int(step_size) == 0 else lr


class _FusedTrainer:
    """``tr = Trainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1)``

    * ``tr.loss_and_grad(bs0, ba0, bts, bsd)`` -- loss (0-dim device tensor) and ``p.grad`` of every parameter;
    * ``tr.step(bs0, ba0, bts, bsd)`` -- one reference iteration (loss, backward, clip, Adam); the loss BEFORE the update;
    * ``tr.run(s0, a0, sn, ts, permutation, batch_size=16)`` -- every full batch of ``permutation`` (``bsd = sn - s0``) on the
      device, one loss per iteration;
    * ``tr.evaluate(s0, a0, ts, target, indices=None)`` -- the held-out loss (overlay.py:112-115): forward and MSE only, on
      the current weights; touches no gradient, moment or parameter;
    * ``tr.keep_best(loss, tag=None)`` / ``tr.restore_best()`` -- the reference's save-on-improvement (train_utils.py:439-448)
      on the device: the current weights become the snapshot of every member whose ``loss`` is below its ``tr.best_loss``
      (``tr.best_tag``: the step count then), with no host read; ``restore_best`` writes the snapshot back;
    * ``tr.fit(data, val=None, epochs=1, batch_size=16, eval_every=1000, ...)`` -- the reference's epoch loop
      (train_utils.py:345-468) from ``run``, ``evaluate``, ``keep_best`` and a ``StepLR`` schedule, nothing read inside;
    * ``tr.state_dict()`` / ``tr.load_state_dict(sd)`` -- ``torch.optim.Adam``'s format.

    ``tr.lr`` may change between calls (what a ``StepLR`` would do).  After ``step()`` / ``run()`` the model's parameters
    hold the new weights, written in place (their ``_version`` moves, so ``model.forward`` and planners re-upload).  The
    model's buffers and settings (normalisation constants, ``normalize`` / ``normalize_time``, ``ilt_options``) are
    re-read before every call: a change after construction (``model.load_state_dict(checkpoint)``, say) takes effect.

    Internally a trainer holds ``self.models`` (one member here, M in a group class): parameters, moments and gradients are
    ``(M, P)`` buffers, losses ``(M,)``, and every library call is the group entry with its M."""

    _entries = None  # the library's group (workspace_bytes, loss_grad, step) of the model family
    _eval_entries = None  # its (eval_workspace_bytes, eval): the forward-only held-out loss
    _reads_ts = True  # False: the model ignores ts_pred, and the kernels get no ts pointer (a property where it varies)
    _grouped = False  # True: calls take / return the leading M (the group classes)

    def _unsupported(self, model):
        """Why no fused kernels exist for ``model`` whatever its shape (None: ask the library)."""
        return None

    def _extra_args(self):
        """What the family's entries take after the workspace pointer (NODE: ``row_times``)."""
        return ()

    def _setup_ctx(self):
        """Options of the trainer's fresh ctx (``NLTrainer(dehoog="fused")`` sets one)."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1):
        self._init([model], lr, betas, eps, weight_decay, clip_grad_norm)

    def _init(self, models, lr, betas, eps, weight_decay, clip_grad_norm):
        self._name = type(self).__name__
        self.models = list(models)
        if not self.models:
            raise ValueError(f"{self._name}: needs at least one model")
        self.model = model = self.models[0]  # the member whose descriptor the ctx holds
        self._M = len(self.models)
        self._members_key = None
        self._check_members()
        for mdl in self.models:
            mdl._require_float64()
            if not next(mdl.parameters()).is_cuda:
                raise RuntimeError("training: move the model to the GPU first (model.to('cuda'))")
        self._hyper, self._members_dirty, self._mem = {}, True, None
        self.lr, self.betas, self.eps = lr, (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.clip_grad_norm = weight_decay, clip_grad_norm
        self._dev = compute_device(next(model.parameters()))
        # per-member state (a group's freeze / unfreeze, fit's patience): the flags the _members step reads, the Adam step
        # count at which a member was frozen (-1: active), and the patience counter's waiting / stopped_at
        self._active = torch.ones(self._M, dtype=torch.int32, device=self._dev)
        self._frozen_step = torch.full((self._M,), -1, dtype=torch.int64, device=self._dev)
        self._waiting = torch.zeros(self._M, dtype=torch.int64, device=self._dev)
        self._stopped_at = torch.full((self._M,), -1, dtype=torch.int64, device=self._dev)
        self._frozen_any = False  # True from the first freeze on: the group then calls the _members entries
        # blob order (= model.parameters() order), per member
        self._mparams = [[dict(mdl.named_parameters())[k] for k in mdl._BLOB_KEYS] for mdl in self.models]
        self._params = self._mparams[0]
        self._sizes = [p.numel() for p in self._params]
        self._best = self._best_loss = self._best_tag = None  # keep_best's snapshot (M, P), its losses and tags (M,)
        self._fallback = None
        why = self._unsupported(model)
        if why is None:
            self._ctx = _lib.Ctx(self._dev.index)
            self._setup_ctx()
            self._model_key = None
            why = self._sync_model()
        if why is not None:
            warnings.warn(f"{self._name}: {why} -- this model trains through its grad-mode forward + clip_grad_norm_ + "
                          "torch.optim.Adam instead of the fused HIP step", stacklevel=3)
            self._fallback = [self._adam(i) for i in range(self._M)]
            return
        M, P = self._M, sum(self._sizes)
        self._flat = torch.empty(M, P, dtype=torch.float64, device=self._dev)
        self._m = torch.zeros(M, P, dtype=torch.float64, device=self._dev)
        self._v = torch.zeros(M, P, dtype=torch.float64, device=self._dev)
        self._step = 0
        self._ws = {}
        self._arange = {}
        self._warned = False

    @property
    def fused(self):
        """True when the fused HIP step runs (False: the fallback's torch optimiser)."""
        return self._fallback is None

    # ------------------------------------------------------------------ settings: one number, or one per member of a group
    def _set_hyper(self, name, value):
        """A single trainer takes a number; a group a number or a sequence of M numbers (kept as a tuple).  A group refuses a
        negative ``lr`` / ``weight_decay`` as ``torch.optim.Adam`` does."""
        if self._grouped and not isinstance(value, (int, float)) and hasattr(value, "__len__") and not (
                torch.is_tensor(value) and value.dim() == 0):
            value = tuple(float(x) for x in value)
            if len(value) != self._M:
                raise ValueError(f"{self._name}: {name} must be a number or a sequence of {self._M} numbers, one per member "
                                 f"(got {len(value)})")
            each = value
        else:
            value = float(value)
            each = (value,)
        if self._grouped and name != "clip_grad_norm" and not all(0.0 <= x for x in each):
            raise ValueError(f"{self._name}: Invalid {name} value: {value}")
        self._hyper[name] = value
        self._members_dirty = True

    lr = property(lambda self: self._hyper["lr"], lambda self, v: self._set_hyper("lr", v))
    weight_decay = property(lambda self: self._hyper["weight_decay"], lambda self, v: self._set_hyper("weight_decay", v))
    clip_grad_norm = property(lambda self: self._hyper["clip_grad_norm"], lambda self, v: self._set_hyper("clip_grad_norm", v))

    def _of(self, name, i):
        """Member ``i``'s value of a setting."""
        v = self._hyper[name]
        return v[i] if isinstance(v, tuple) else v

    def _per_member(self):
        """True once a setting is a sequence or a member has been frozen: the step is then the library's ``_members`` entry,
        which reads the settings and the flags from device arrays.  Otherwise the step is the entry it has always been."""
        return self._frozen_any or any(isinstance(v, tuple) for v in self._hyper.values())

    def _members_arg(self):
        """``nlc_train_members`` of the group; the three setting arrays are uploaded again only after one was assigned."""
        if self._members_dirty or self._mem is None:
            up = lambda k: torch.tensor([self._of(k, i) for i in range(self._M)], dtype=torch.float64, device=self._dev)  # noqa: E731
            self._mem_arrays = (up("lr"), up("weight_decay"), up("clip_grad_norm"))
            self._mem = _lib.TrainMembers(*(t.data_ptr() for t in self._mem_arrays), self._active.data_ptr())
            self._members_dirty = False
        return self._mem

    def _mask(self, mask):
        mask = torch.as_tensor(mask).to(self._dev).reshape(-1) != 0
        if mask.numel() != self._M:
            raise ValueError(f"{self._name}: a member mask holds {self._M} values")
        return mask

    def _freeze(self, mask):
        mask = self._mask(mask)
        newly = mask & (self._active != 0)
        self._frozen_step.copy_(torch.where(newly, torch.full_like(self._frozen_step, self._step_count()), self._frozen_step))
        self._active.masked_fill_(mask, 0)
        self._frozen_any = True

    def _unfreeze(self, mask):
        mask = self._mask(mask)
        self._active.masked_fill_(mask, 1)
        self._frozen_step.masked_fill_(mask, -1)
        self._stopped_at.masked_fill_(mask, -1)
        self._waiting.masked_fill_(mask, 0)

    def _frozen_host(self):
        """Which members are frozen, read on the host (only the paths that synchronise anyway use it)."""
        return [a == 0 for a in self._active.tolist()] if self._frozen_any else [False] * self._M

    # ------------------------------------------------------------------ plumbing
    def _model_state_key(self, model=None):
        """What the kernels read from the model descriptor besides the weights: the buffers (normalisation, dt) and the
        settings of ``_weights_key_extra()``.  Not the parameters: the trainer's own write-back moves their versions, and
        the kernels read the weights from ``_flat`` on every call."""
        m = self.model if model is None else model
        return (tuple((id(b), b.data_ptr(), b._version) for b in m.buffers()), m._wk_dirty, tuple(m._weights_key_extra()))

    @staticmethod
    def _first_difference(a, b):
        """The first thing the descriptor holds in which model ``b`` differs from ``a`` (None: they agree)."""
        if type(a) is not type(b):
            return f"class ({type(b).__name__} against {type(a).__name__})"
        pa = {k: tuple(p.shape) for k, p in a.named_parameters()}
        pb = {k: tuple(p.shape) for k, p in b.named_parameters()}
        for k in pa:
            if pa[k] != pb.get(k):
                return f"the shape of {k} ({pb.get(k)} against {pa[k]})"
        if len(pb) != len(pa):
            return "its set of parameters"
        ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
        for k in ba:
            if k not in bb or ba[k].shape != bb[k].shape or not torch.equal(ba[k].detach().cpu(), bb[k].detach().cpu()):
                return f"buffer {k}"
        if len(bb) != len(ba):
            return "its set of buffers"
        ea, eb = tuple(a._weights_key_extra()), tuple(b._weights_key_extra())
        if ea != eb:
            # a mirror that names its settings (NODE: the solver ``method`` among them) has the first differing one named
            names = getattr(a, "_weights_key_names", ())
            which = next((i for i, (x, y) in enumerate(zip(ea, eb)) if x != y), None)
            if which is not None and which < len(names):
                return f"its settings (_weights_key_extra()): {names[which]} ({eb[which]!r} against {ea[which]!r})"
            return "its settings (_weights_key_extra())"
        return None

    def _check_members(self):
        """The equality rule of a group: every member agrees with member 0 on all the descriptor holds (class, shapes,
        buffers by value, ``_weights_key_extra()``), else ValueError naming the first member and field that differ.  Run at
        construction and before every call; the by-value comparison is redone only when some member's buffers or settings
        have moved since the last one."""
        if self._M == 1:
            return
        key = tuple(self._model_state_key(m) for m in self.models)
        if key == self._members_key:
            return
        for i, mdl in enumerate(self.models[1:], 1):
            field = self._first_difference(self.models[0], mdl)
            if field is not None:
                raise ValueError(f"{self._name}: member {i} differs from member 0 in {field}; a group trains models of one "
                                 "descriptor (class, shapes, buffers, settings)")
        self._members_key = key

    def _sync_model(self):
        """Re-upload the model descriptor if the buffers or settings changed since the last upload.  Returns None when the
        descriptor in the ctx is current, else the library's reason for refusing the new one (the fused kernels must not
        run then: the ctx still holds the old constants)."""
        self._check_members()
        key = self._model_state_key()
        if self._model_key is not None and self._model_key[0] == key:
            return self._model_key[1]
        why = None
        try:
            self.model.sync_to(self._ctx)
        except _lib.NlcError as err:
            if err.code != _lib.NLC_ERR_UNSUPPORTED:
                raise
            why = str(err)
        self._model_key = (key, why)
        self._descriptor_changed()
        return why

    def _descriptor_changed(self):
        """After a re-upload of the model descriptor (``NLTrainer(dehoog="fused")`` drops its workspace cache here)."""

    def _host_path(self, why):
        """A call the fused kernels do not take: warn once per trainer."""
        if not self._warned:
            self._warned = True
            warnings.warn(f"{self._name}: {why} -- calls the library refuses run the grad-mode forward + clip_grad_norm_ + "
                          "torch.optim.Adam on the trainer's optimiser state instead of the fused HIP step", stacklevel=3)

    def _views(self, flat, i=0):
        """Member ``i``'s row of an ``(M, P)`` buffer as views shaped like its parameters."""
        out, o = [], 0
        for p, n in zip(self._mparams[i], self._sizes):
            out.append(flat[i, o : o + n].view_as(p))
            o += n
        return out

    def _gather(self):
        torch.cat([p.detach().reshape(-1) for ps in self._mparams for p in ps], out=self._flat.view(-1))

    def _scatter(self):
        with torch.no_grad():
            for i, ps in enumerate(self._mparams):
                for p, v in zip(ps, self._views(self._flat, i)):
                    p.copy_(v)

    def _workspace(self, N, entry=None):
        """The device workspace of an N-row call, sized by the library's ``entry`` (the training step's unless given) and
        kept for the next call of that size."""
        entry = self._entries[0] if entry is None else entry
        ws = self._ws.get((entry, N))
        if ws is None:
            n = getattr(self._ctx.lib, entry)(self._ctx.h, self._M, N)
            if n < 0:
                raise _lib.NlcError(n, entry)
            ws = self._ws[entry, N] = torch.empty((n + 7) // 8, dtype=torch.float64, device=self._dev)
        return ws

    def _why_host(self):
        """Whether the next call runs the fused kernels: None if so; else why not -- "" for a trainer that has had none
        since construction (it warned then), or the library's reason for refusing the model's current descriptor, which
        the caller hands to ``_host_path`` / ``_host_steps``."""
        return self._sync_model() if self.fused else ""

    def _desc(self):
        # (with per-member settings the library reads lr, weight decay and clip norm from _members_arg(), not from here)
        return _lib.TrainDesc(self._of("lr", 0), self.betas[0], self.betas[1], self.eps, self._of("weight_decay", 0),
                              self._of("clip_grad_norm", 0))

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

    def _stacked(self, s0):
        """True when the data carry a leading M (``s0`` is (M, N, d)): member m reads its own rows."""
        stacked = torch.as_tensor(s0).dim() == 3
        if stacked and not self._grouped:
            raise ValueError(f"{self._name}: s0 must be (N, d)")
        if stacked and torch.as_tensor(s0).shape[0] != self._M:
            raise ValueError(f"{self._name}: stacked data must lead with the group's {self._M} members")
        return stacked

    def _group_data(self, s0, a0, ts, target):
        """``_data`` of a shared (2-D ``s0``) or stacked (3-D: the members' rows back to back) batch or dataset; also the
        rows per member and the library's data_row_stride (0: shared)."""
        if not self._stacked(s0):
            obs, win, tsd, tgt = self._data(s0, a0, ts, target)
            return obs, win, tsd, tgt, obs.shape[0], 0
        rows = torch.as_tensor(s0).shape[1]

        def flat(t):  # (M, rows, ...) -> (M rows, ...); a model that ignores ts may get none
            if t is None:
                return None
            t = torch.as_tensor(t)
            return t.reshape((self._M * rows,) + tuple(t.shape[2:]))

        obs, win, tsd, tgt = self._data(flat(s0), flat(a0), flat(ts) if self._reads_ts else None, flat(target))
        return obs, win, tsd, tgt, rows, rows

    def _member_data(self, i, stacked, *tensors):
        return tuple(torch.as_tensor(t)[i] if stacked and t is not None else t for t in tensors)

    def _idx(self, N):
        """``(M, N)``: every member takes rows 0 .. N - 1 (of the shared batch, or of its own rows of a stacked one)."""
        idx = self._arange.get(N)
        if idx is None:
            idx = torch.arange(N, dtype=torch.int64, device=self._dev).repeat(self._M, 1).contiguous()
            self._arange[N] = idx
        return idx

    def _out(self, t):
        """An ``(M, ...)`` result as the class returns it: a single trainer drops the member axis."""
        return t if self._grouped else t[0]

    def _ref_loss(self, bs0, ba0, bts, bsd, i=0):
        pred = self.models[i](bs0, ba0, bts)
        return torch.nn.functional.mse_loss(pred.squeeze(), bsd.squeeze())

    # ------------------------------------------------------------------ API
    def loss_and_grad(self, bs0, ba0, bts, bsd):
        """Loss of the batch and ``p.grad`` of every parameter (train_utils.py:391-402); no update."""
        why = self._why_host()
        if why is not None:
            if self.fused:
                self._host_path(why)
            return self._host_loss_and_grad(bs0, ba0, bts, bsd)
        obs, win, ts, tgt, N, rows = self._group_data(bs0, ba0, bts, bsd)
        self._gather()
        grad = torch.empty_like(self._flat)
        loss = torch.empty(self._M, dtype=torch.float64, device=self._dev)
        ctx = self._ctx
        with ctx.stream():
            rc = getattr(ctx.lib, self._entries[1])(
                ctx.h, self._M, rows, _f64_ptr(self._flat), _f64_ptr(obs), _f64_ptr(win), _f64_ptr(ts), _f64_ptr(tgt),
                _i64_ptr(self._idx(N)), N, win.shape[1], _f64_ptr(grad), _f64_ptr(loss), _f64_ptr(self._workspace(N)),
                *self._extra_args())
        why = self._refused(rc)
        if why is not None:
            self._host_path(why)
            return self._host_loss_and_grad(bs0, ba0, bts, bsd)
        for i, ps in enumerate(self._mparams):
            for p, g in zip(ps, self._views(grad, i)):
                p.grad = g
        return self._out(loss)

    def evaluate(self, s0, a0, ts, target, indices=None):
        """The held-out loss of the reference's validation (overlay.py:112-115, :175-177: ``model(s0, a0, ts)``, then the
        MSE against ``target = sn - s0``) on the model's current weights: a 0-dim float64 device tensor, ``(M,)`` for a
        group.  ``indices`` picks rows of the dataset -- ``(N,)``, or ``(M, N)`` in a group -- without a gather copy;
        None takes every row.  Forward only (``nlc_train_group_eval``): no ``p.grad``, no write-back, no moments, no step
        count, no host synchronisation.  A call the fused kernels do not take runs the model's ``no_grad`` forward +
        ``mse_loss`` instead, under the trainer's one warning."""
        why = self._why_host()
        if why is not None:
            if self.fused:
                self._host_path(why)
            return self._host_evaluate(s0, a0, ts, target, indices)
        obs, win, tsd, tgt, rows, stride = self._group_data(s0, a0, ts, target)
        M = self._M
        if indices is None:
            idx, N = None, rows
        else:
            idx = torch.as_tensor(indices).to(self._dev, torch.int64)
            if idx.dim() == 1:
                idx = idx.unsqueeze(0).expand(M, -1)
            elif not (self._grouped and idx.dim() == 2 and idx.shape[0] == M):
                raise ValueError(f"{self._name}.evaluate: indices must be (N,)" + (f" or ({M}, N)" if self._grouped else ""))
            idx, N = idx.contiguous(), int(idx.shape[1])
        ws = self._workspace(N, self._eval_entries[0])
        self._gather()
        loss = torch.empty(M, dtype=torch.float64, device=self._dev)
        ctx = self._ctx
        with ctx.stream():
            rc = getattr(ctx.lib, self._eval_entries[1])(
                ctx.h, M, stride, _f64_ptr(self._flat), _f64_ptr(obs), _f64_ptr(win), _f64_ptr(tsd), _f64_ptr(tgt),
                C.c_void_p(0) if idx is None else _i64_ptr(idx), N, win.shape[1], _f64_ptr(loss), _f64_ptr(ws),
                *self._extra_args())
        why = self._refused(rc)
        if why is not None:
            self._host_path(why)
            return self._host_evaluate(s0, a0, ts, target, indices)
        return self._out(loss)

    def _host_evaluate(self, s0, a0, ts, target, indices):
        self._check_members()
        stacked = self._stacked(s0)
        ind = None if indices is None else torch.as_tensor(indices).to(self._dev, torch.int64)
        out = []
        with torch.no_grad():
            for i in range(self._M):
                data = [torch.as_tensor(t).to(self._dev) for t in self._member_data(i, stacked, s0, a0, ts, target)]
                if ind is not None:
                    mine = ind if ind.dim() == 1 else ind[i]
                    data = [t[mine] for t in data]
                out.append(self._ref_loss(*data, i=i).detach())
        return self._out(torch.stack(out))

    def step(self, bs0, ba0, bts, bsd):
        """One iteration of the reference's loop (train_utils.py:391-404); returns the loss before the update."""
        stacked = self._stacked(bs0)
        batches = lambda: [[self._member_data(i, stacked, bs0, ba0, bts, bsd)] for i in range(self._M)]  # noqa: E731
        why = self._why_host()
        if why is not None:
            if self.fused:
                return self._out(self._host_steps(why, batches())[:, 0])
            self._check_members()
            return self._out(torch.stack([self._fallback_step(*b[0], i=i) for i, b in enumerate(batches())]))
        obs, win, ts, tgt, N, rows = self._group_data(bs0, ba0, bts, bsd)
        self._gather()
        loss = torch.empty(self._M, dtype=torch.float64, device=self._dev)
        ctx = self._ctx
        with ctx.stream():
            try:
                self._launch_step(_i64_ptr(self._idx(N)), obs, win, ts, tgt, N, _f64_ptr(loss), self._workspace(N), rows=rows)
            except _lib.NlcError as err:
                if err.code != _lib.NLC_ERR_UNSUPPORTED:
                    raise
                return self._out(self._host_steps(str(err), batches())[:, 0])
        self._scatter()
        return self._out(loss)

    def _launch_step(self, idx_ptr, obs, win, ts, tgt, N, loss_ptr, ws, desc=None, rows=0):
        """One ``nlc_train_group_step`` / ``nlc_rnn_train_group_step`` (idx ``[M][N]``, loss ``[M]``, ``rows`` the
        data_row_stride); the Adam step count moves only once the library has accepted the call (it checks everything on
        the host before the first launch).  With per-member settings or a frozen member it is the ``_members`` entry of the
        same signature plus the group's ``nlc_train_members``."""
        ctx = self._ctx
        entry, more = self._entries[2], ()
        if self._per_member():
            entry, more = entry + "_members", (C.byref(self._members_arg()),)
        ctx.check(getattr(ctx.lib, entry)(
            ctx.h, C.byref(desc if desc is not None else self._desc()), self._M, rows, _f64_ptr(self._flat),
            _f64_ptr(self._m), _f64_ptr(self._v), self._step + 1, _f64_ptr(obs), _f64_ptr(win), _f64_ptr(ts), _f64_ptr(tgt),
            idx_ptr, N, win.shape[1], loss_ptr, None, _f64_ptr(ws), *self._extra_args(), *more))
        self._step += 1

    def _refused(self, rc):
        """None if the library took the call, its reason if it refused the shape (NLC_ERR_UNSUPPORTED); raises otherwise."""
        if rc == _lib.NLC_ERR_UNSUPPORTED:
            return (self._ctx.lib.nlc_last_error(self._ctx.h) or b"").decode()
        self._ctx.check(rc)
        return None

    def _host_loss_and_grad(self, bs0, ba0, bts, bsd):
        self._check_members()
        stacked = self._stacked(bs0)
        out = []
        for i, mdl in enumerate(self.models):
            mdl.zero_grad()
            loss = self._ref_loss(*self._member_data(i, stacked, bs0, ba0, bts, bsd), i=i)
            loss.backward()
            out.append(loss.detach())
        return self._out(torch.stack(out))

    def _host_steps(self, why, batches):
        """Iterations the fused kernels refused (``batches[i]``: member i's), on the grad-mode path member by member with a
        transient torch.optim.Adam that starts from the trainer's step count and the member's moments and hands them back:
        the trainer keeps one optimiser state.  Returns the ``(M, iterations)`` losses."""
        self._host_path(why)
        out, step, frozen = [], self._step, self._frozen_host()
        for i, mine in enumerate(batches):
            if frozen[i]:  # skipped: its losses on the weights it stopped with, no optimiser
                out.append([self._frozen_loss(*b, i=i) for b in mine])
                continue
            opt = self._adam(i)
            self._export_state(opt, i)
            out.append([self._fallback_step(*b, opt=opt, i=i) for b in mine])
            st = opt.state.get(self._mparams[i][0])
            if st is not None:
                with torch.no_grad():
                    for p, m, v in zip(self._mparams[i], self._views(self._m, i), self._views(self._v, i)):
                        m.copy_(opt.state[p]["exp_avg"])
                        v.copy_(opt.state[p]["exp_avg_sq"])
                step = int(st["step"])
        self._step = step  # every active member made the same number of steps from the same count
        if not out[0]:
            return torch.empty(self._M, 0, dtype=torch.float64, device=self._dev)
        return torch.stack([torch.stack(o) for o in out])

    def _fallback_step(self, bs0, ba0, bts, bsd, opt=None, i=0):
        if opt is None:  # a non-fused trainer's own optimiser: a frozen member is skipped (this path synchronises anyway)
            if self._frozen_any and int(self._active[i]) == 0:
                return self._frozen_loss(bs0, ba0, bts, bsd, i=i)
            opt = self._fallback[i]
        for grp in opt.param_groups:
            grp["lr"] = self._of("lr", i)
        opt.zero_grad()
        loss = self._ref_loss(bs0, ba0, bts, bsd, i=i)
        loss.backward()
        clip = self._of("clip_grad_norm", i)
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(self.models[i].parameters(), clip)
        opt.step()
        return loss.detach()

    def _frozen_loss(self, bs0, ba0, bts, bsd, i=0):
        """What a frozen member reports on the grad-mode path: the loss on its weights, no gradient, no update."""
        with torch.no_grad():
            return self._ref_loss(bs0, ba0, bts, bsd, i=i).detach()

    def run(self, s0, a0, sn, ts, permutation, batch_size=16):
        """Every full batch of ``permutation`` (train_utils.py:388-408 with ``bsd = bsn - bs0``): returns the (iters,) losses
        on the device.  Fused: the dataset stays where it is, each iteration is one ``nlc_train_group_step`` on its slice of
        the permutation, nothing crosses to the host until the end."""
        bs = int(batch_size)
        M = self._M
        perm = torch.as_tensor(permutation).to(self._dev, torch.int64)
        if perm.dim() == 1:
            perm = perm.unsqueeze(0).expand(M, -1)  # one permutation for every member
        elif not (self._grouped and perm.dim() == 2 and perm.shape[0] == M):
            raise ValueError(f"{self._name}.run: permutation must be (L,)" + (f" or ({M}, L)" if self._grouped else ""))
        iters = int(perm.shape[1]) // bs
        stacked = self._stacked(s0)

        def host(why=None):
            batches = []
            for i in range(M):
                s0_, a0_, sn_, ts_ = (torch.as_tensor(t).to(self._dev) for t in self._member_data(i, stacked, s0, a0, sn, ts))
                mine = []
                for k in range(iters):
                    ind = perm[i, k * bs : k * bs + bs]
                    mine.append((s0_[ind], a0_[ind], ts_[ind], sn_[ind] - s0_[ind]))
                batches.append(mine)
            if why is not None:
                return self._out(self._host_steps(why, batches))
            self._check_members()
            if iters == 0:
                return self._out(torch.empty(M, 0, dtype=torch.float64, device=self._dev))
            return self._out(torch.stack([torch.stack([self._fallback_step(*b, i=i) for b in mine])
                                          for i, mine in enumerate(batches)]))

        if not self.fused:
            return host()
        why = self._sync_model() if iters > 0 else None
        if why is not None:
            return host(why)
        if iters == 0:
            return self._out(torch.empty(M, 0, dtype=torch.float64, device=self._dev))
        obs, win, tsd, sn_d, _, rows = self._group_data(s0, a0, ts, sn)
        tgt = sn_d - obs
        # iteration k's index array [M][bs]: member m's slice k of its permutation
        idx = perm[:, : iters * bs].reshape(M, iters, bs).transpose(0, 1).contiguous()
        losses = torch.empty(iters, M, dtype=torch.float64, device=self._dev)
        ws = self._workspace(bs)
        self._gather()
        desc = self._desc()
        ctx = self._ctx
        with ctx.stream():
            for i in range(iters):
                try:
                    self._launch_step(_i64_ptr(idx, i * M * bs), obs, win, tsd, tgt, bs, _f64_ptr(losses, i * M), ws, desc,
                                      rows=rows)
                except _lib.NlcError as err:
                    # the library checks the shape on the host before any launch, and the shape is the same for every
                    # iteration: only the first can be refused, with nothing launched
                    if err.code != _lib.NLC_ERR_UNSUPPORTED or i > 0:
                        raise
                    return host(str(err))
        self._scatter()
        return self._out(losses.t().contiguous())

    # ------------------------------------------------------------------ the best weights
    @property
    def best_loss(self):
        """The lowest loss ``keep_best`` has seen, per member: a float64 device tensor shaped like the trainer's losses
        (+inf until a loss beat it; None before the first ``keep_best``)."""
        return None if self._best is None else self._out(self._best_loss)

    @property
    def best_tag(self):
        """The ``tag`` of the ``keep_best`` call that took the snapshot (int64, shaped like ``best_loss``; -1: none yet)."""
        return None if self._best is None else self._out(self._best_tag)

    def _step_count(self):
        """Adam steps taken so far (one count for all parameters and members)."""
        if self.fused:
            return self._step
        st = self._fallback[0].state.get(self._mparams[0][0])
        return int(st["step"]) if st else 0

    def keep_best(self, loss, tag=None):
        """The reference's save-on-improvement (train_utils.py:439-448) without a host read: member m's current parameters
        become its snapshot iff ``loss[m] < best_loss[m]`` (strict; a NaN never improves), and then ``best_loss[m] = loss[m]``
        and ``best_tag[m] = tag``.  ``loss`` is a device tensor, 0-dim or (1,) for a single trainer and (M,) for a group --
        what ``evaluate()`` returned, or a sum of ``run()``'s losses; ``tag`` defaults to the Adam step count.  Returns the
        ``improved`` flags (int32, shaped like ``loss``).  The first call starts the snapshot from the current parameters
        with ``best_loss`` +inf and ``best_tag`` -1, so ``restore_best`` is defined from then on.  Fused:
        ``nlc_train_keep_best``, two launches on the trainer's stream; a non-fused trainer applies the same rule with
        ``torch.where`` on a flat copy."""
        M, P = self._M, sum(self._sizes)
        loss = torch.as_tensor(loss).detach().to(self._dev, torch.float64).reshape(-1).contiguous()
        if loss.numel() != M:
            raise ValueError(f"{self._name}.keep_best: loss must hold {M} value" + ("s, one per member" if M > 1 else ""))
        tag = self._step_count() if tag is None else int(tag)
        first = self._best is None
        if self.fused:
            self._gather()
            flat = self._flat
        else:
            flat = torch.cat([p.detach().reshape(-1) for ps in self._mparams for p in ps]).view(M, P)
        if first:
            self._best = flat.clone()
            self._best_loss = torch.full((M,), float("inf"), dtype=torch.float64, device=self._dev)
            self._best_tag = torch.full((M,), -1, dtype=torch.int64, device=self._dev)
        if not self.fused:
            better = loss < self._best_loss
            self._best.copy_(torch.where(better[:, None], flat, self._best))
            self._best_loss.copy_(torch.where(better, loss, self._best_loss))
            self._best_tag.copy_(torch.where(better, torch.full_like(self._best_tag, tag), self._best_tag))
            return self._out(better.to(torch.int32))
        improved = torch.empty(M, dtype=torch.int32, device=self._dev)
        ctx = self._ctx
        with ctx.stream():  # the stream the loss was written on
            ctx.check(ctx.lib.nlc_train_keep_best(
                ctx.h, M, P, _f64_ptr(loss), _f64_ptr(flat), _f64_ptr(self._best_loss), _f64_ptr(self._best),
                _i64_ptr(self._best_tag), tag, C.c_void_p(improved.data_ptr())))
        return self._out(improved)

    def restore_best(self):
        """Write the snapshot back into the models' parameters, in place (their ``_version`` moves, so ``model.forward`` and
        planners re-upload).  The Adam moments, the step count, ``best_loss`` and ``best_tag`` stay as they are."""
        if self._best is None:
            raise RuntimeError(f"{self._name}.restore_best: keep_best has not been called")
        with torch.no_grad():
            for i, ps in enumerate(self._mparams):
                for p, v in zip(ps, self._views(self._best, i)):
                    p.copy_(v)

    def _patience(self, improved, patience, tag):
        """The reference's waiting / patience counter (train_utils.py:439-448) after a ``keep_best``, without a host read: an
        active member that improved waits from 0 again; one that did not and has ``waiting > patience`` is frozen, with
        ``stopped_at = tag``; else its ``waiting`` grows by one.  Fused: ``nlc_train_patience``, one launch; a non-fused
        trainer applies the same rule in torch ops."""
        improved = improved.reshape(-1).contiguous()
        if self.fused:
            ctx = self._ctx
            with ctx.stream():
                ctx.check(ctx.lib.nlc_train_patience(
                    ctx.h, self._M, C.c_void_p(improved.data_ptr()), _i64_ptr(self._waiting),
                    C.c_void_p(self._active.data_ptr()), _i64_ptr(self._stopped_at), float(patience), int(tag)))
        else:
            live, better = self._active != 0, improved != 0
            stop = live & ~better & (self._waiting.to(torch.float64) > float(patience))
            self._waiting.copy_(torch.where(live & better, torch.zeros_like(self._waiting),
                                            torch.where(live & ~better & ~stop, self._waiting + 1, self._waiting)))
            self._stopped_at.masked_fill_(stop, int(tag))
            self._active.masked_fill_(stop, 0)
        newly = (self._active == 0) & (self._frozen_step < 0)
        self._frozen_step.copy_(torch.where(newly, torch.full_like(self._frozen_step, self._step_count()), self._frozen_step))

    def fit(self, data, val=None, *, epochs=1, batch_size=16, eval_every=1000, seed=0, step_lr=None, restore_best=True,
            patience=None):
        """The reference's epoch loop (train_utils.py:345-468) with nothing read on the host inside.

        ``data`` is ``(s0, a0, sn, ts)`` or a callable ``epoch -> (s0, a0, sn, ts)`` (the reference regenerates the
        synthetic dataset every epoch, :353-370).  Each epoch draws ``torch.randperm(R)`` on the device from a generator
        seeded ``seed + epoch`` (one permutation for all members) and walks it in slices of ``eval_every * batch_size``
        indices: ``run()`` on the slice, then the criterion -- ``evaluate(*val)`` with ``val = (s0, a0, ts, target)``, else
        the slice's summed training losses (the reference's ``cum_loss``, :440) -- then ``keep_best(criterion,
        tag=iterations so far)``.  A last slice without a full batch is skipped.  ``step_lr = (step_size, gamma)`` moves
        ``tr.lr`` after every epoch as ``torch.optim.lr_scheduler.StepLR.step()`` would.  At the end the best weights are
        restored unless ``restore_best`` is False.

        ``patience=None`` (the reference's is ``inf``) stops nobody.  With a number, every check runs the reference's
        counter after ``keep_best`` (``nlc_train_patience``): a member whose criterion has not improved for more than
        ``patience`` checks in a row is frozen from then on -- the loop runs to the end, the Adam update skips the member, and
        its criterion no longer reaches ``keep_best`` (the reference's ``break``).  Its forward and backward still run, so
        ``train_loss`` and ``criterion`` go on reporting it.  The waiting counts start from 0 at every call.

        Returns device tensors: ``train_loss`` (iters,) / (M, iters), ``criterion`` (checks,) / (M, checks), ``best_loss``
        and ``best_iter`` (the iteration count at the best check); with ``patience`` also ``active`` (bool) and ``stopped_at``
        (the iteration count of the check that stopped the member, -1: none)."""
        bs, every = int(batch_size), int(eval_every)
        if bs < 1 or every < 1:
            raise ValueError(f"{self._name}.fit: batch_size and eval_every must be >= 1")
        if patience is not None:
            patience = float(patience)
            if patience != patience or patience < 0:
                raise ValueError(f"{self._name}.fit: patience must be None or a number >= 0 (inf: nobody stops)")
            self._waiting.zero_()
            self._frozen_any = True  # members may stop at any check from here on, and no host read will tell
        train_loss, criterion, done = [], [], 0
        for epoch in range(int(epochs)):
            s0, a0, sn, ts = data(epoch) if callable(data) else data
            gen = torch.Generator(device=self._dev)
            gen.manual_seed(int(seed) + epoch)
            perm = torch.randperm(int(torch.as_tensor(s0).shape[-2]), device=self._dev, generator=gen)
            for chunk in perm.split(every * bs):
                if chunk.numel() < bs:
                    continue
                losses = self.run(s0, a0, sn, ts, chunk, bs)
                done += chunk.numel() // bs
                crit = self.evaluate(*val) if val is not None else losses.sum(-1)
                if patience is None:
                    self.keep_best(crit, tag=done)
                else:  # a stopped member is no longer checked: +inf never improves
                    live = self._active != 0
                    improved = self.keep_best(torch.where(live, crit.reshape(-1), torch.full_like(crit.reshape(-1), float("inf"))),
                                              tag=done)
                    self._patience(improved, patience, done)
                train_loss.append(losses)
                criterion.append(crit)
            if step_lr is not None:
                lr = self.lr
                self.lr = ([step_lr_after_epoch(x, epoch + 1, *step_lr) for x in lr] if isinstance(lr, tuple)
                           else step_lr_after_epoch(lr, epoch + 1, *step_lr))
        if not criterion:
            raise ValueError(f"{self._name}.fit: no epoch held a full batch")
        if restore_best:
            self.restore_best()
        out = {"train_loss": torch.cat(train_loss, dim=-1), "criterion": torch.stack(criterion, dim=-1),
               "best_loss": self.best_loss.clone(), "best_iter": self.best_tag.clone()}
        if patience is not None:
            out["active"], out["stopped_at"] = self._out(self._active != 0), self._out(self._stopped_at.clone())
        return out

    # ------------------------------------------------------------------ optimiser state
    def _adam(self, i=0):
        return torch.optim.Adam(self.models[i].parameters(), lr=self._of("lr", i), betas=self.betas, eps=self.eps,
                                weight_decay=self._of("weight_decay", i))

    def _export_state(self, opt, i=0, step=None):
        """The trainer's step count (``step``: a frozen member's own) and member ``i``'s moments as ``opt.state`` (copies)."""
        step = self._step if step is None else step
        if step > 0:
            sdt = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
            for p, m, v in zip(self._mparams[i], self._views(self._m, i), self._views(self._v, i)):
                opt.state[p] = {"step": torch.tensor(float(step), dtype=sdt), "exp_avg": m.clone(),
                                "exp_avg_sq": v.clone()}

    def _state_dicts(self):
        if not self.fused:
            return [opt.state_dict() for opt in self._fallback]
        # a frozen member's step is the count it stopped at (one device read, only once a member has been frozen)
        at = self._frozen_step.tolist() if self._frozen_any else [-1] * self._M
        out = []
        for i in range(self._M):
            opt = self._adam(i)
            self._export_state(opt, i, at[i] if at[i] >= 0 else None)
            out.append(opt.state_dict())
        return out

    def state_dict(self):
        """``torch.optim.Adam(model.parameters(), ...).state_dict()`` of the same optimiser state."""
        return self._state_dicts()[0]

    def load_state_dict(self, sd):
        """Take over a ``torch.optim.Adam`` state (hyper-parameters of its first group, step and moments).  An
        ``amsgrad`` or ``maximize`` state is refused: the trainer's update has neither."""
        self._load_state_dicts([sd])

    def _load_state_dicts(self, sds):
        """One state per member; nothing of the trainer changes unless all of them can be taken."""
        if len(sds) != self._M:
            raise ValueError(f"{self._name}.load_state_dict: {len(sds)} states for {self._M} members")
        for sd in sds:
            for grp in sd.get("param_groups", []):
                for flag in ("amsgrad", "maximize"):
                    if grp.get(flag):
                        raise ValueError(f"{self._name}.load_state_dict: an Adam state with {flag}=True is not supported "
                                         "(the trainer runs plain Adam)")
        opts = [self._adam(i) for i in range(self._M)]
        # a group that already has per-member settings takes states whose lr or weight decay differ between members, and a
        # frozen member's own step count; a group of uniform settings keeps one of each, as it always has
        per_member, frozen = self._per_member(), self._frozen_host()
        hypers, shared, steps, own = [], set(), set(), []
        for i, (opt, sd) in enumerate(zip(opts, sds)):
            opt.load_state_dict(sd)
            grp = opt.param_groups[0]
            hypers.append((float(grp["lr"]), float(grp["weight_decay"])))
            shared.add((tuple(float(b) for b in grp["betas"]), float(grp["eps"])))
            mine = {int(opt.state[p]["step"]) for p in self._mparams[i] if p in opt.state} or {0}
            own.append(mine)
            if len(mine) > 1 or not frozen[i]:
                steps |= mine
        if len(steps) > 1:
            raise ValueError(f"{self._name} keeps one Adam step count for all parameters" +
                             (" of all members" if self._grouped else "") + (" that are not frozen" if any(frozen) else ""))
        if len(shared) > 1 or (len(set(hypers)) > 1 and not per_member):
            raise ValueError(f"{self._name}.load_state_dict: the members' Adam hyper-parameters differ (one lr, betas, eps "
                             "and weight_decay for the group" +
                             ("; a group with per-member settings takes its own lr and weight_decay per member)"
                              if self._grouped else ")"))
        (self.betas, self.eps), = shared
        for k, name in enumerate(("lr", "weight_decay")):
            vals = [h[k] for h in hypers]
            setattr(self, name, vals[0] if len(set(vals)) == 1 and not isinstance(self._hyper[name], tuple) else vals)
        if not self.fused:
            self._fallback = opts
            return
        if steps:
            self._step = steps.pop()
        if any(frozen):
            self._frozen_step.copy_(torch.tensor([next(iter(s)) if f else -1 for s, f in zip(own, frozen)], dtype=torch.int64))
        with torch.no_grad():
            for i, opt in enumerate(opts):
                for p, m, v in zip(self._mparams[i], self._views(self._m, i), self._views(self._v, i)):
                    st = opt.state.get(p)
                    m.copy_(st["exp_avg"] if st else torch.zeros_like(m))
                    v.copy_(st["exp_avg_sq"] if st else torch.zeros_like(v))


class _Group:
    """What a group class changes in ``_FusedTrainer``: the constructor takes the members, calls take stacked data and
    ``(M, L)`` permutations and return the leading M, the optimiser state is a list of M."""

    _grouped = True

    def __init__(self, models, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1):
        self._init(models, lr, betas, eps, weight_decay, clip_grad_norm)

    @property
    def active(self):
        """Which members the Adam update still moves: a bool device tensor ``(M,)`` (all True until ``freeze`` or ``fit``'s
        patience stopped one)."""
        return self._active != 0

    def freeze(self, mask):
        """Stop updating the members ``mask`` marks (``(M,)`` bools, on the host or the device; no host read).  A frozen
        member's parameters and Adam moments are not written again; its forward and backward still run, so its losses are
        still reported.  From the first call on the group steps through the library's ``_members`` entries."""
        self._freeze(mask)

    def unfreeze(self, mask):
        """Let the members ``mask`` marks step again, with the group's step count; their patience counters start over."""
        self._unfreeze(mask)

    def state_dict(self):
        """A list of M ``torch.optim.Adam`` state dicts, one per member, each with the member's own ``lr`` and
        ``weight_decay``; a frozen member's ``step`` is the count it stopped at (read from the device)."""
        return self._state_dicts()

    def load_state_dict(self, sds):
        """A list of M ``torch.optim.Adam`` states; ValueError when the betas, eps or the step counts of the members that are
        not frozen differ (the group keeps one of each) or one has ``amsgrad`` / ``maximize``.  A group that has per-member
        settings takes each state's own ``lr`` and ``weight_decay``; a group of uniform settings refuses states whose ``lr``
        or ``weight_decay`` differ, as it always has."""
        self._load_state_dicts(list(sds))


class NLTrainer(_FusedTrainer):
    """``tr = NLTrainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1)`` for a
    ``NeuralLaplaceModel``; the fused step takes Fourier, fixed Talbot and Stehfest models (``nlc_train_group_step``,
    M = 1).  ``model.ilt_algorithm`` may change on a live trainer: among those three the next call runs the other kernel
    instance; set to ``"dehoog"`` the calls take the per-call grad-mode path on the trainer's Adam state.

    ``dehoog="grad"`` (the default) is that behaviour: a de Hoog model trains through its grad-mode forward, with one
    warning.  ``dehoog="fused"`` sets the ctx option ``train_dehoog``: a de Hoog model (odd ``s_recon_terms`` 3 .. 33) then
    takes the fused step as the other algorithms do -- the step's forward half, the de Hoog ILT kernels, the loss, their
    backward and the step's backward half (``csrc/nlc_train_dehoog.h``) -- at up to 2048 rows per call; a larger call runs the
    per-call grad-mode path.  Switching ``model.ilt_algorithm`` to or from ``"dehoog"`` on such a trainer takes effect at the
    next call, without a warning."""

    _entries = ("nlc_train_group_workspace_bytes", "nlc_train_group_loss_grad", "nlc_train_group_step")
    _eval_entries = ("nlc_train_group_eval_workspace_bytes", "nlc_train_group_eval")
    _dehoog = "grad"

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1, dehoog="grad"):
        self._dehoog = self._dehoog_mode(dehoog)
        self._init([model], lr, betas, eps, weight_decay, clip_grad_norm)

    def _dehoog_mode(self, dehoog):
        if dehoog not in ("grad", "fused"):
            raise ValueError(f"{type(self).__name__}: dehoog must be 'grad' or 'fused' (got {dehoog!r})")
        return dehoog

    def _setup_ctx(self):
        if self._dehoog == "fused":
            self._ctx.set_option("train_dehoog", 1)

    def _descriptor_changed(self):
        # with the option set a workspace's size depends on the descriptor's ILT algorithm, which may be switched on a live
        # trainer: the cached workspaces (keyed by entry and N) are those of the previous descriptor
        if self._dehoog == "fused":
            self._ws = {}

    def _unsupported(self, model):
        fused = ("fourier", "fixed_tablot", "stehfest") + (("dehoog",) if self._dehoog == "fused" else ())
        if model.ilt_algorithm not in fused:
            return (f"ilt_algorithm {model.ilt_algorithm!r} has no fused training kernels (fourier, fixed_tablot and "
                    "stehfest have)")
        return None


class RNNTrainer(_FusedTrainer):
    """``tr = RNNTrainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1)`` for a
    ``DeltaTRNN`` or an ``RNN`` (``nlc_rnn_train_group_step``, M = 1): the methods and semantics of ``NLTrainer``.  An
    ``RNN`` ignores ``ts`` as its forward does; the reference's loop still passes it, so every method accepts it."""

    _entries = ("nlc_rnn_train_group_workspace_bytes", "nlc_rnn_train_group_loss_grad", "nlc_rnn_train_group_step")
    _eval_entries = ("nlc_rnn_train_group_eval_workspace_bytes", "nlc_rnn_train_group_eval")

    @property
    def _reads_ts(self):
        return bool(self.model._time_input)


class NODETrainer(_FusedTrainer):
    """``tr = NODETrainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1,
    row_times=False)`` for a ``NODE`` (``nlc_node_train_group_step``, M = 1): the methods and semantics of ``NLTrainer``.
    The loss is the reference loop's: the MSE of the model's output (the integrated normalised state) against ``bsd``.

    ``row_times=False`` is the reference's time semantics: every row of a batch integrates to the time of the batch's FIRST
    row (``train_utils.py:719``; what ``model.forward`` does), which is why the reference trains NODE at batch size 1.
    ``row_times=True`` integrates each row to its own time; on the grad-mode fallback that loops the rows one by one.

    A row takes at most ``MAX_SUBSTEPS`` evaluations of the ODE function: that many Euler sub-steps, half as many midpoint
    and a quarter as many rk4 sub-steps (``max_substeps()``).  The first call with a given ``ts`` tensor reads it once on the
    host and raises ``ValueError`` if a time is not positive or needs more; after that the tensor is not read again (a changed
    ``model.method`` reads it again)."""

    _entries = ("nlc_node_train_group_workspace_bytes", "nlc_node_train_group_loss_grad", "nlc_node_train_group_step")
    _eval_entries = ("nlc_node_train_group_eval_workspace_bytes", "nlc_node_train_group_eval")
    MAX_SUBSTEPS = 256  # csrc/nlc_train_node.h kNodeTrainMaxSub

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1, row_times=False):
        self.row_times = bool(row_times)
        self._ts_seen = {}
        self._init([model], lr, betas, eps, weight_decay, clip_grad_norm)

    def max_substeps(self):
        """Sub-steps a row may take under the model's current ``method`` (csrc/nlc_train_node.h node_train_max_sub)."""
        return self.MAX_SUBSTEPS // self.model.stages

    def _extra_args(self):
        return (int(self.row_times),)

    def _check_ts(self, ts):
        """One host read per dataset tensor: every time positive and within ``MAX_SUBSTEPS`` sub-steps of the model's grid
        (torchdiffeq's ``ceil(t / step_size + 1)`` points), else ValueError -- before any launch."""
        ts = torch.as_tensor(ts)
        key = (ts.data_ptr(), ts._version, ts.numel(), self._model_key[0], self.model.method)
        if key in self._ts_seen:
            return
        t_end = ts.detach().to(torch.float64).reshape(-1) / self.model._time_div()
        cap = self.max_substeps()
        ok = (t_end > 0) & (torch.ceil(t_end / float(self.model.step_size) + 1.0) <= cap + 1)
        if not bool(ok.all()):
            raise ValueError(f"{self._name}: every prediction time must be positive and need at most {cap} "
                             f"{self.model.method} sub-steps of {self.model.step_size} (after normalize_time); ts holds one that does not")
        if len(self._ts_seen) >= 64:
            self._ts_seen.clear()
        self._ts_seen[key] = True

    def _group_data(self, s0, a0, ts, target):
        self._check_ts(ts)
        out = super()._group_data(s0, a0, ts, target)
        if out[1].shape[2] != self.model.action_dim:
            raise ValueError(f"{self._name}: a0 must be (N, B, {self.model.action_dim}) or (N, {self.model.action_dim})")
        return out

    def _ref_loss(self, bs0, ba0, bts, bsd, i=0):
        if not self.row_times:
            return super()._ref_loss(bs0, ba0, bts, bsd, i)
        # _forward_train integrates a batch to its first row's time: one row at a time
        mdl, bts = self.models[i], torch.as_tensor(bts).reshape(-1, 1)
        pred = torch.cat([mdl(bs0[r : r + 1], ba0[r : r + 1], bts[r : r + 1]) for r in range(bs0.shape[0])])
        return torch.nn.functional.mse_loss(pred.squeeze(), bsd.squeeze())


class NLTrainerGroup(_Group, NLTrainer):
    """``grp = NLTrainerGroup(models, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1)``: M
    ``NeuralLaplaceModel`` s of one descriptor (run_exp_multi.py:105-110: the delays and seeds of one env) trained by the
    same three launches, each member bit-identical to its own ``NLTrainer``.

    * ``grp.loss_and_grad(bs0, ba0, bts, bsd)`` / ``grp.step(...)`` -- ``(M,)`` losses; a 2-D ``bs0`` (N, d) is one batch
      shared by the members, a 3-D one (M, N, d) gives each its own (the others then lead with M too);
    * ``grp.run(s0, a0, sn, ts, permutations, batch_size=16)`` -- ``(M, iters)`` losses; ``permutations`` (M, L), or (L,) to
      share; the datasets shared or stacked by the same rule;
    * ``grp.state_dict()`` / ``grp.load_state_dict(list)`` -- a list of M ``torch.optim.Adam`` states;
    * ``grp.lr``, ``grp.weight_decay``, ``grp.clip_grad_norm`` -- a number, or a sequence of M numbers (a sweep: member m
      trains with its own, bit-identical to a single trainer built with them); they return what was set, and assigning
      either form takes effect at the next call.  A wrong length, or a negative ``lr`` / ``weight_decay``: ValueError;
    * ``grp.active``, ``grp.freeze(mask)``, ``grp.unfreeze(mask)`` -- members the Adam update skips; ``fit(...,
      patience=k)`` freezes each member when it stops improving;
    * ``grp.fused``, ``grp.models``.

    The members must agree on all the descriptor holds (class, shapes, buffers by value, settings), at construction and at
    every call: ValueError names the first member and field that differ.  One betas, eps and step count.  With numbers for
    all three settings and no frozen member the group calls ``nlc_train_group_step`` as it always has; otherwise
    ``nlc_train_group_step_members``, which reads the settings and the flags from device arrays.

    ``dehoog="fused"`` as for ``NLTrainer``: the M de Hoog members share every launch, the two ILT launches as one batch of
    ``M x rows`` points."""

    def __init__(self, models, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1, dehoog="grad"):
        self._dehoog = self._dehoog_mode(dehoog)
        self._init(models, lr, betas, eps, weight_decay, clip_grad_norm)


class RNNTrainerGroup(_Group, RNNTrainer):
    """``grp = RNNTrainerGroup(models, ...)``: M ``DeltaTRNN`` s or M ``RNN`` s of one descriptor; the methods and
    semantics of ``NLTrainerGroup``."""


class NODETrainerGroup(_Group, NODETrainer):
    """``grp = NODETrainerGroup(models, ..., row_times=False)``: M ``NODE`` s of one descriptor; the methods and semantics of
    ``NLTrainerGroup``.  ``row_times`` is the group's: one value for all members, like the optimiser's hyper-parameters."""

    def __init__(self, models, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.1, row_times=False):
        self.row_times = bool(row_times)
        self._ts_seen = {}
        self._init(models, lr, betas, eps, weight_decay, clip_grad_norm)
