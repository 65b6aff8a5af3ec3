"""The HIP plumbing the four model mirrors share (NeuralLaplaceModel, DeltaTRNN, RNN, NODE), driven on the host through their
public surface -- ``model_desc()``, ``upload(ctx)``, ``state_dict()`` -- against a stub ctx: no library is loaded and no GPU is
touched.  Every expected value is spelled out here from the reference's rules (normalised: the buffers, a scalar action
constant broadcast to the GRU input width; raw inputs: mean 0, std 1, action std 3, ``time_div`` 1; ``time_div`` under
``normalize_time``: float32(0.05) widened, times 8), not computed by the code under test."""

import ctypes as C

import numpy as np
import pytest
import torch

from neurallaplacecontrol_amd import NeuralLaplaceModel, _lib
from neurallaplacecontrol_amd.node_model import NODE
from neurallaplacecontrol_amd.rnn_model import RNN, DeltaTRNN

D, NU, H = 3, 2, 64
SM, SS = [0.1, -0.2, 0.3], [1.5, 2.5, 0.5]
TIME_DIV = 0.4000000059604645  # float(torch.tensor(0.05)) * 8
BROADCAST_ERROR = "normalisation buffers do not broadcast against the model's input dims"

NL_KEYS = (
    [f"action_encoder.gru.{w}_l{layer}" for layer in (0, 1) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    + ["action_encoder.linear_out.weight", "action_encoder.linear_out.bias"]
    + [f"laplace_rep_func.linear_tanh_stack.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
)
RNN_KEYS = ["gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "linear_out.weight", "linear_out.bias"]
NODE_KEYS = [f"x_ode_func_in_x_and_u.linear_tanh_stack.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
BUFFERS = ["state_mean", "state_std", "action_mean", "action_std", "dt"]
BUFFER_DTYPES = {"state_mean": torch.float64, "state_std": torch.float64, "action_mean": torch.int64,
                 "action_std": torch.float64, "dt": torch.float32}


def _norm(am, a_s, sm=SM, ss=SS):
    return dict(state_mean=np.array(sm), state_std=np.array(ss), action_mean=np.array(am), action_std=np.array(a_s))


def _nl(normalize, normalize_time, encode_obs_time=False, am=(0,), a_s=(1.0,), d=D, nu=NU, double=True, **kw):
    model = NeuralLaplaceModel(d, nu, d, hidden_units=H, s_recon_terms=17, ilt_algorithm="fourier", encode_obs_time=encode_obs_time,
                               normalize=normalize, normalize_time=normalize_time, **{**_norm(am, a_s), **kw})
    return model.double() if double else model


def _dtrnn(normalize, normalize_time, encode_obs_time=False, am=(0,), a_s=(1.0,), double=True, **kw):
    model = DeltaTRNN(D, NU, H, encode_obs_time=encode_obs_time, normalize=normalize, normalize_time=normalize_time,
                      **{**_norm(am, a_s), **kw})
    return model.double() if double else model


def _rnn(normalize, normalize_time=False, encode_obs_time=False, am=(0,), a_s=(1.0,), double=True, **kw):
    assert not normalize_time  # the class has no such argument
    model = RNN(D, NU, H, encode_obs_time=encode_obs_time, normalize=normalize, **{**_norm(am, a_s), **kw})
    return model.double() if double else model


def _node(normalize, normalize_time, encode_obs_time=False, am=(0,), a_s=(1.0,), augment_dim=1, double=True, **kw):
    model = NODE(D, NU, D, hidden_units=H, encode_obs_time=encode_obs_time, normalize=normalize, normalize_time=normalize_time,
                 augment_dim=augment_dim, **{**_norm(am, a_s), **kw})
    return model.double() if double else model


def _fields(s):
    """A ctypes structure as a dict (arrays as lists, nested structures as dicts)."""
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        out[name] = _fields(v) if isinstance(v, C.Structure) else (list(v) if isinstance(v, C.Array) else v)
    return out


def _pad(values, n):
    return [float(v) for v in values] + [0.0] * (n - len(values))


def _constants(sm, ss, am=None, a_s=None):
    out = dict(state_mean=_pad(sm, 8), state_std=_pad(ss, 8))
    if am is not None:
        out.update(action_mean=_pad(am, 3), action_std=_pad(a_s, 3))
    return out


FOURIER_17 = dict(algo=0, terms=17, alpha=1.0e-3, tol=10.0 * 1.0e-3, scale=2.0)


class _StubLib:
    """Records (symbol, args); a ``*_blob_size`` query answers the parameter count, every other call 0.  What a
    ``nlc_set_*model`` call points at (descriptor, blob) is copied while the call runs."""

    def __init__(self, nparams):
        self.nparams, self.calls, self.desc_bytes, self.blob = nparams, [], None, None

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name.endswith("_blob_size"):
                return self.nparams
            if name.startswith("nlc_set_"):
                _, desc, blob, n = args
                self.desc_bytes = bytes(desc._obj)
                self.blob = list((C.c_double * n).from_address(blob.value))
            return 0

        return fn


class _StubCtx:
    def __init__(self, nparams):
        self.lib, self.h = _StubLib(nparams), C.c_void_p(0x1234)

    def check(self, rc):
        assert rc == 0


# (factory, descriptor type, its size, blob-size symbol, set symbol, blob keys, has a dt buffer)
FAMILIES = {
    "nl": (_nl, _lib.ModelDesc, 232, "nlc_model_blob_size", "nlc_set_model", NL_KEYS, True),
    "dtrnn": (_dtrnn, _lib.RnnDesc, 200, "nlc_rnn_blob_size", "nlc_set_rnn_model", RNN_KEYS, True),
    "rnn": (_rnn, _lib.RnnDesc, 200, "nlc_rnn_blob_size", "nlc_set_rnn_model", RNN_KEYS, False),
    "node": (_node, _lib.NodeDesc, 160, "nlc_node_blob_size", "nlc_set_node_model", NODE_KEYS, True),
}

# action constants as the constructors get them, and what the descriptor must hold for a GRU input width of nin
SCALAR = dict(am=(1,), a_s=(0.5,))
PER_DIM = dict(am=(1, -2), a_s=(0.5, 2.0))


def _expected_actions(kind, nin):
    if kind is SCALAR:
        return [1.0] * nin, [0.5] * nin
    return [1.0, -2.0], [0.5, 2.0]


def _raw(nin):
    return [0.0] * D, [1.0] * D, [0.0] * nin, [3.0] * nin


# family -> [(normalize, normalize_time, normalised constants?, time_div)]: every branch the class has
BRANCHES = {
    "nl": [(True, True, True, TIME_DIV), (True, False, True, 1.0), (False, False, False, 1.0), (False, True, False, 1.0)],
    "dtrnn": [(True, True, True, TIME_DIV), (True, False, False, 1.0), (False, False, False, 1.0)],
    "rnn": [(True, False, True, 1.0), (False, False, False, 1.0)],
}


@pytest.mark.parametrize("kind", [SCALAR, PER_DIM], ids=["scalar", "per_dim"])
@pytest.mark.parametrize("family,branch", [(f, b) for f, bs in BRANCHES.items() for b in bs])
def test_descriptor_of_the_gru_models_in_every_normalisation_branch(family, branch, kind):
    make, desc_type, size = FAMILIES[family][:3]
    normalize, normalize_time, normalised, time_div = branch
    enc = kind is SCALAR  # the scalar constants also against the wider input of encode_obs_time
    model = make(normalize, normalize_time, encode_obs_time=enc, **kind)
    nin = NU if family == "rnn" else NU + int(enc)  # the reference's RNN ignores encode_obs_time when sizing the GRU
    gru = model.action_encoder.gru if family == "nl" else model.gru
    assert gru.input_size == nin
    desc = model.model_desc()
    assert type(desc) is desc_type and C.sizeof(desc) == size
    sm, ss, am, a_s = (SM, SS) + _expected_actions(kind, nin) if normalised else _raw(nin)
    want = dict(d=D, nin=nin, time_div=time_div, **_constants(sm, ss, am, a_s))
    if family == "nl":
        want.update(h=H, ilt=FOURIER_17)
    else:
        want.update(hidden=H, time_input=1 if family == "dtrnn" else 0)
    assert _fields(desc) == want


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("normalize_time", [True, False])
def test_descriptor_of_node_takes_state_and_time_normalisation_independently(normalize, normalize_time):
    desc = _node(normalize, normalize_time, **PER_DIM).model_desc()
    assert type(desc) is _lib.NodeDesc and C.sizeof(desc) == 160
    sm, ss = (SM, SS) if normalize else ([0.0] * D, [1.0] * D)
    assert _fields(desc) == dict(d=D, nu=NU, hidden=H, augment_dim=1, time_div=TIME_DIV if normalize_time else 1.0,
                                 step_size=0.05, **_constants(sm, ss))


def test_delta_t_rnn_rejects_the_branch_the_reference_cannot_run():
    with pytest.raises(NameError, match="batch_obs is undefined"):
        _dtrnn(False, True).model_desc()


@pytest.mark.parametrize("family,branch", [("nl", (True, False)), ("dtrnn", (True, True)), ("rnn", (True, False))])
@pytest.mark.parametrize("bad", [dict(state_mean=np.zeros(2)), dict(state_std=np.ones(4)), dict(action_mean=np.array([0, 0, 0])),
                                 dict(action_std=np.ones(3))], ids=lambda b: next(iter(b)))
def test_buffers_that_do_not_broadcast_are_refused(family, branch, bad):
    model = FAMILIES[family][0](*branch, **bad)
    with pytest.raises(ValueError) as err:
        model.model_desc()
    assert str(err.value) == BROADCAST_ERROR


@pytest.mark.parametrize("bad", [dict(state_mean=np.zeros(2)), dict(state_std=np.ones(4))], ids=lambda b: next(iter(b)))
def test_node_buffers_that_do_not_match_state_dim_are_refused(bad):
    with pytest.raises(ValueError) as err:
        _node(True, False, **bad).model_desc()
    assert str(err.value) == "normalisation buffers do not match state_dim"


@pytest.mark.parametrize("shape", [dict(d=9), dict(nu=3, encode_obs_time=True)], ids=["state_dim_9", "gru_input_4"])
def test_nl_shape_beyond_the_descriptor_arrays_is_unsupported(shape):
    d = shape.get("d", D)
    model = _nl(True, True, state_mean=np.zeros(d), state_std=np.ones(d), **shape)
    with pytest.raises(_lib.NlcError) as err:
        model.model_desc()
    assert err.value.code == _lib.NLC_ERR_UNSUPPORTED


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_upload_packs_the_blob_in_key_order_through_the_family_s_two_symbols(family):
    make, _, size, blob_size, set_model, keys, _ = FAMILIES[family]
    model = make(True, family in ("nl", "dtrnn"), **PER_DIM)
    nparams = sum(p.numel() for p in model.parameters())
    ctx = _StubCtx(nparams)
    key_before = model._weights_key()
    key = model.upload(ctx)
    assert key == key_before == model._weights_key()
    (first, first_args), (second, second_args) = ctx.lib.calls  # two library calls, in this order
    assert (first, second) == (blob_size, set_model)
    assert len(first_args) == 1 and bytes(first_args[0]._obj) == bytes(model.model_desc())
    assert second_args[0] is ctx.h and second_args[3] == nparams
    assert ctx.lib.desc_bytes == bytes(model.model_desc()) and len(ctx.lib.desc_bytes) == size
    sd = model.state_dict()
    want = torch.cat([sd[k].reshape(-1) for k in keys])
    assert len(ctx.lib.blob) == nparams == want.numel()
    assert ctx.lib.blob == want.tolist()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_upload_refuses_a_blob_of_another_size_than_the_library_expects(family):
    model = FAMILIES[family][0](False, False)
    nparams = sum(p.numel() for p in model.parameters())
    ctx = _StubCtx(nparams + 1)
    with pytest.raises(ValueError) as err:
        model.upload(ctx)
    assert str(err.value) == f"weight blob has {nparams} doubles, library expects {nparams + 1}"
    assert [name for name, _ in ctx.lib.calls] == [FAMILIES[family][3]]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_upload_refuses_a_float32_model_before_any_library_call(family):
    model = FAMILIES[family][0](False, False).float()
    ctx = _StubCtx(0)
    with pytest.raises(NotImplementedError, match="the HIP path computes in float64 only: call model.double\\(\\) first"):
        model.upload(ctx)
    assert ctx.lib.calls == []


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_state_dict_keys_order_and_buffer_dtypes_are_the_reference_s(family):
    make, keys, has_dt = FAMILIES[family][0], FAMILIES[family][5], FAMILIES[family][6]
    model = make(False, False, double=False)  # as constructed: the reference's checkpoints are written from such a model
    buffers = BUFFERS if has_dt else BUFFERS[:4]
    # buffers are registered after the sub-modules, but state_dict() lists a module's own buffers before its children's entries
    assert list(model.state_dict()) == buffers + keys
    assert [name for name, _ in model.named_buffers()] == buffers
    assert {name: b.dtype for name, b in model.named_buffers()} == {name: BUFFER_DTYPES[name] for name in buffers}
    assert not hasattr(model, "dt") or has_dt
    fresh = make(True, False, state_mean=np.zeros(D), state_std=np.ones(D))
    fresh.load_state_dict(model.state_dict())  # a checkpoint loads: same keys, shapes and dtypes
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), model.state_dict().values()))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_forward_in_grad_mode_with_nothing_to_train_is_refused(family):
    model = FAMILIES[family][0](False, False).requires_grad_(False)
    with pytest.raises(NotImplementedError, match="is inference-only on the HIP path"):
        model(torch.zeros(4, D, dtype=torch.float64), torch.zeros(4, 4, NU, dtype=torch.float64), torch.full((4, 1), 0.05))


@pytest.mark.parametrize("family", ["dtrnn", "rnn", "node"])
def test_training_forward_of_a_model_on_the_host_is_refused(family):
    model = FAMILIES[family][0](False, False)
    with pytest.raises(RuntimeError) as err:
        model(torch.zeros(4, D, dtype=torch.float64), torch.zeros(4, 4, NU, dtype=torch.float64), torch.full((4, 1), 0.05))
    assert str(err.value) == "training forward: move the model to the GPU first (model.to('cuda'))"
