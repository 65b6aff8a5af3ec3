"""CPU: the host side of per-member settings and patience -- ``patience_step`` of csrc/nlc_train_members.h built with g++
against a Python restatement of the reference's counter (train_utils.py:439-448), the per-member step size ``-(lr / bc1)``
against Python's with ``==``, the four entries in the header, the binding's symbol list and the built library, and what the
group classes accept.  The helper has a main() and is also built stand-alone under AddressSanitizer / UBSan and run."""

import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HELPER = os.path.join(HERE, "helpers", "train_members_host.cpp")
ENTRIES = ["nlc_train_group_step_members", "nlc_rnn_train_group_step_members", "nlc_node_train_group_step_members",
           "nlc_train_patience"]
PARENT_ABI = 18
INF = float("inf")


def _header():
    return open(os.path.join(REPO, "include", "nlc.h")).read()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("trainmembershost") / "libtrain_members_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), HELPER])
    lib = ctypes.CDLL(str(out))
    vp = ctypes.c_void_p
    lib.nlc_t_patience_run.argtypes = [vp, ctypes.c_long, ctypes.c_double, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                       vp, vp, vp]
    lib.nlc_t_step_size.argtypes = [vp, vp, ctypes.c_double, vp, ctypes.c_long]
    return lib


def _reference(improved, patience):
    """train_utils.py:439-448 for one model: ``(waiting, active, stopped_at)`` after every check; check k has tag k + 1.
    The reference leaves its loop at ``break``: from then on nothing moves."""
    waiting, active, stopped, out = 0, 1, -1, []
    for k, better in enumerate(improved):
        if active:
            if better:  # cum_loss < best_loss
                waiting = 0
            elif waiting > patience:
                active, stopped = 0, k + 1  # break
            else:
                waiting += 1
        out.append((waiting, active, stopped))
    return out


def _run(lib, improved, patience, waiting=0, active=1, stopped=-1):
    n = len(improved)
    imp = np.asarray(improved, dtype=np.int32)
    w, a, s = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int64)
    lib.nlc_t_patience_run(imp.ctypes.data, n, patience, waiting, active, stopped, w.ctypes.data, a.ctypes.data, s.ctypes.data)
    return list(zip(w.tolist(), a.tolist(), s.tolist()))


def _sequences():
    rng = random.Random(7)
    seqs = [[1] * 12, [0] * 12, [1, 0] * 6, [1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]]
    seqs += [[int(rng.random() < p) for _ in range(24)] for p in (0.2, 0.5, 0.8) for _ in range(5)]
    return seqs


@pytest.mark.parametrize("patience", [0, 1, 3, INF])
def test_patience_step_follows_the_reference(lib, patience):
    stopped_some = False
    for seq in _sequences():
        got, want = _run(lib, seq, float(patience)), _reference(seq, patience)
        assert got == want, (patience, seq)
        stopped_some |= want[-1][1] == 0
    assert stopped_some == (patience != INF)
    # the strict comparison: patience p stops at the (p + 2)-th check in a row without improvement
    if patience != INF:
        assert _run(lib, [0] * 8, float(patience))[-1] == (patience + 1, 0, patience + 2)


def test_inf_never_stops(lib):
    out = _run(lib, [0] * 5000, INF)
    assert out[-1] == (5000, 1, -1) and all(a == 1 for _, a, _ in out)


def test_a_frozen_member_is_left_alone(lib):
    for seq in _sequences():
        assert _run(lib, seq, 0.0, waiting=3, active=0, stopped=17) == [(3, 0, 17)] * len(seq)


def test_step_size_equals_python(lib):
    """-(lr / bc1) in the g++ build against Python's ``(lr / bc1) * -1`` of the single trainer's host side, ``==``, for 1 000
    random (lr, step) pairs: an IEEE division and a sign flip on both sides."""
    rng = random.Random(11)
    lr = np.array([10.0 ** rng.uniform(-6, 0) for _ in range(1000)], dtype=np.float64)
    step = np.array([int(10.0 ** rng.uniform(0, 5)) for _ in range(1000)], dtype=np.int64)
    out = np.zeros(1000, dtype=np.float64)
    lib.nlc_t_step_size(lr.ctypes.data, step.ctypes.data, 0.9, out.ctypes.data, 1000)
    for i in range(1000):
        bc1 = 1.0 - 0.9 ** float(step[i])
        assert out[i] == (float(lr[i]) / bc1) * -1.0 == -(float(lr[i]) / bc1), (i, lr[i], step[i])
    assert step.min() == 1 and step.max() > 10000


def test_header_declares_the_entries_and_cites_the_reference():
    hdr = _header()
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(\s*nlc_ctx\s*\*\s*ctx\s*,", hdr)
        assert m, f"{name}(nlc_ctx* ctx, ...) is not declared in include/nlc.h"
        before = hdr[: m.start()]
        assert "train_utils.py:" in before[before.rindex("/*") :], name
    assert re.search(r"}\s*nlc_train_members\s*;", hdr)
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", hdr).group(1)) > PARENT_ABI


def test_binding_lists_and_library_exports_the_entries():
    from neurallaplacecontrol_amd import _lib

    so = _lib.LIB_PATH
    if not os.path.exists(so):
        pytest.fail(f"{so} is not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(so)
    for name in ENTRIES:
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), f"libnlc_hip.so does not export {name}"
    assert lib.nlc_abi_version() > PARENT_ABI
    assert ctypes.sizeof(_lib.TrainMembers) == 32


def test_group_classes_have_the_interface():
    import neurallaplacecontrol_amd as nlc

    for name in ("NLTrainerGroup", "RNNTrainerGroup", "NODETrainerGroup"):
        cls = getattr(nlc, name)
        assert isinstance(cls.active, property), name
        for prop in ("lr", "weight_decay", "clip_grad_norm"):
            assert isinstance(getattr(cls, prop), property), (name, prop)
        assert callable(cls.freeze) and callable(cls.unfreeze), name


def test_the_existing_kernel_units_do_not_include_the_new_header():
    csrc = os.path.join(REPO, "neurallaplacecontrol_amd", "csrc")
    for name in ("nlc_train.h", "nlc_train_dev.h", "nlc_train_eval.h", "nlc_train_node.h", "nlc_train_select.h",
                 "kernels_train.hip", "kernels_train_rnn.hip", "kernels_train_node.hip", "kernels_train_eval.hip",
                 "kernels_train_select.hip"):
        assert "nlc_train_members.h" not in open(os.path.join(csrc, name)).read(), name


def test_helper_stand_alone_under_sanitizers(tmp_path):
    """The helper with its own main(): the patience kernel's loop on the host over exact-size heap blocks at member counts
    around a workgroup's 256 threads, and the step-size expression, under ASan + UBSan."""
    exe = tmp_path / "train_members_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), HELPER])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok"), res.stdout + res.stderr
