"""CPU: the shape functions of the DeltaTRNN / RNN training step (csrc/nlc_train.h), built with g++, against the models'
own parameters; and the three ABI entries in the header and the binding."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ENTRIES = ["nlc_rnn_train_workspace_bytes", "nlc_rnn_train_loss_grad", "nlc_rnn_train_step"]
SHAPES = [(d, nin, H) for d in (1, 5, 8) for nin in (1, 3) for H in (64, 128, 160)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("trainrnnhost") / "libtrain_rnn_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "train_rnn_host.cpp")])
    return ctypes.CDLL(str(out))


def _plan(lib, d, nin, H, time_input):
    n = lib.nlc_t_tensors() + 1
    off, cstart = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    lib.nlc_t_rnn_plan.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    lib.nlc_t_rnn_plan(d, nin, H, time_input, off.ctypes.data, cstart.ctypes.data)
    return off, cstart


def _model(cls, d, nin, H):
    import neurallaplacecontrol_amd as nlc

    return getattr(nlc, cls)(d, nin, hidden_units=H, state_mean=[0.0] * d, state_std=[1.0] * d, action_mean=[0.0],
                             action_std=[1.0], normalize=True)


@pytest.mark.parametrize("cls,time_input", [("DeltaTRNN", 1), ("RNN", 0)])
def test_rnn_blob_offsets_match_the_models_parameters(lib, cls, time_input):
    """rnn_blob_offsets == the cumulative numel() of the model's parameters in _BLOB_KEYS order; the table is padded with
    empty tensors up to the reduce / Adam kernels' tensor count, and its end is nlc_rnn_blob_size's formula."""
    for d, nin, H in SHAPES:
        m = _model(cls, d, nin, H)
        named = dict(m.named_parameters())
        assert list(named) == list(m._BLOB_KEYS)
        sizes = [named[k].numel() for k in m._BLOB_KEYS]
        off, _ = _plan(lib, d, nin, H, time_input)
        assert list(np.diff(off[:7])) == sizes, (cls, d, nin, H)
        assert (off[6:] == off[6]).all()
        assert off[-1] == 3 * H * nin + 3 * H * H + 6 * H + d * (H + d + time_input) + d


@pytest.mark.parametrize("time_input", [1, 0])
def test_no_chunk_straddles_two_tensors(lib, time_input):
    """The chunk a reduce / Adam workgroup b takes, found as train_reduce_kernel finds it (the last tensor t with
    cstart[t] <= b among the first kTensors), lies inside tensor t; the chunks tile the blob exactly once."""
    T, chunk = lib.nlc_t_tensors(), lib.nlc_t_chunk()
    for d, nin, H in SHAPES:
        off, cstart = _plan(lib, d, nin, H, time_input)
        covered = np.zeros(off[-1], dtype=np.int32)
        for b in range(cstart[T]):
            t = 0
            while t + 1 < T and cstart[t + 1] <= b:
                t += 1
            e0 = off[t] + (b - cstart[t]) * chunk
            e1 = min(e0 + chunk, off[t + 1])
            assert off[t] <= e0 < e1 <= off[t + 1], (d, nin, H, b, t)
            covered[e0:e1] += 1
        assert (covered == 1).all(), (d, nin, H)


def test_rnn_act_layout_aligned_disjoint_and_within_the_longest_windows_slab(lib):
    """The workgroup's slab: arrays on 8-double boundaries, disjoint at the extents the kernel indexes, inside total(B), and
    total(B) <= total(16) (the workspace is sized for the longest window)."""
    f = lib.nlc_t_rnn_act_layout
    f.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    out = np.zeros(6, dtype=np.int64)
    for nin in (1, 2, 3):
        for H in (64, 128, 160):
            f(nin, H, 16, out.ctypes.data)
            total16 = int(out[5])
            for B in range(1, 17):
                f(nin, H, B, out.ctypes.data)
                ext = [B * 16 * nin, (B + 1) * 16 * H, B * 16 * 4 * H, B * 16 * 3 * H, B * 16 * 3 * H]
                spans = sorted((int(out[i]), int(out[i]) + ext[i]) for i in range(5))
                assert all(o % 8 == 0 for o, _ in spans) and spans[0][0] == 0
                assert all(e0 <= o1 for (_, e0), (o1, _) in zip(spans, spans[1:]))
                assert spans[-1][1] <= int(out[5]) <= total16


def test_header_declares_and_binding_names_the_entries():
    from neurallaplacecontrol_amd import _lib

    hdr = open(os.path.join(REPO, "include", "nlc.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(\s*nlc_ctx\s*\*", hdr), name
        assert name in _lib.SYMBOLS
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 11


def test_rnn_trainer_is_exported():
    import neurallaplacecontrol_amd as nlc

    assert "RNNTrainer" in nlc.__all__ and issubclass(nlc.RNNTrainer, object) and nlc.RNNTrainer is not nlc.NLTrainer
