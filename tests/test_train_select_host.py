"""CPU: the host side of snapshot selection (``keep_best`` / nlc_train_keep_best) -- the rule of csrc/nlc_train_select.h built
with g++ (less, equal, greater, NaN on either side, +/-inf on either side, -0.0 against 0.0) and its copy plan; the entry in
the header, the binding's symbol list and the built library; the methods on the four trainer classes; and ``fit``'s
``step_lr`` arithmetic against ``torch.optim.lr_scheduler.StepLR``.  The helper has a main() and is also built stand-alone
under AddressSanitizer / UBSan and run."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HELPER = os.path.join(HERE, "helpers", "train_select_host.cpp")
ENTRY = "nlc_train_keep_best"
PARENT_ABI = 16


def _header():
    return open(os.path.join(REPO, "include", "nlc.h")).read()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("trainselecthost") / "libtrain_select_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), HELPER])
    lib = ctypes.CDLL(str(out))
    lib.nlc_t_improves.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    lib.nlc_t_select_chunks.argtypes = [ctypes.c_int64]
    lib.nlc_t_select_chunks.restype = ctypes.c_int64
    lib.nlc_t_select_span.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
    return lib


NAN, INF = float("nan"), float("inf")
# (loss, best, improves)
RULE = [
    (1.0, 2.0, 1),  # less
    (2.0, 2.0, 0),  # equal: the earlier snapshot stays
    (3.0, 2.0, 0),  # greater
    (np.nextafter(2.0, 0.0), 2.0, 1),  # one ulp below
    (NAN, 2.0, 0),  # a NaN loss never improves
    (NAN, INF, 0),
    (1.0, NAN, 0),  # a NaN best is never replaced
    (NAN, NAN, 0),
    (INF, INF, 0),  # best starts at +inf: +inf does not beat it
    (1e308, INF, 1),
    (-INF, INF, 1),  # -inf does, once
    (-INF, -INF, 0),
    (INF, -INF, 0),
    (INF, 1.0, 0),
    (-INF, 1.0, 1),
    (1.0, -INF, 0),
    (-0.0, 0.0, 0),  # the zeros compare equal
    (0.0, -0.0, 0),
    (-5e-324, 0.0, 1),  # the largest negative subnormal is below both
    (-5e-324, -0.0, 1),
]


def test_rule(lib):
    loss = np.array([r[0] for r in RULE], dtype=np.float64)
    best = np.array([r[1] for r in RULE], dtype=np.float64)
    out = np.full(len(RULE), -1, dtype=np.int32)
    lib.nlc_t_improves(loss.ctypes.data, best.ctypes.data, out.ctypes.data, len(RULE))
    assert out.tolist() == [r[2] for r in RULE]
    with np.errstate(invalid="ignore"):
        assert out.tolist() == (loss < best).astype(np.int32).tolist()  # numpy's statement of it, as the GPU test uses


def test_chunks(lib):
    c = lib.nlc_t_select_chunks
    assert [c(P) for P in (1, 2047, 2048, 2049, 4096, 4097)] == [1, 1, 1, 2, 2, 3]
    assert c(2**40) == 2**29  # int64 throughout


@pytest.mark.parametrize("n", [1, 2, 3, 4, 1023, 1024, 1025, 2048])
def test_span_covers_the_chunk_with_aligned_pairs(lib, n):
    out = np.zeros(3, dtype=np.int64)
    for s in (4096, 4104):
        for d in (8192, 8200):
            lib.nlc_t_select_span(s, d, n, out.ctypes.data)
            head, pairs, tail = (int(v) for v in out)
            assert head >= 0 and pairs >= 0 and tail >= 0 and head + 2 * pairs + tail == n
            if pairs:
                assert (s + 8 * head) % 16 == 0 and (d + 8 * head) % 16 == 0
            if (s - d) % 16:
                assert pairs == 0  # the rows never reach a 16-byte boundary together
            else:
                assert head == (s % 16) // 8 and tail <= 1  # all but the ends go as 16-byte accesses


def test_header_declares_the_entry_and_cites_the_reference():
    hdr = _header()
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(\s*nlc_ctx\s*\*\s*ctx\s*,", hdr)
    assert m, f"{ENTRY}(nlc_ctx* ctx, ...) is not declared in include/nlc.h"
    before = hdr[: m.start()]
    comment = before[before.rindex("/*") :]
    assert "train_utils.py:439-448" in comment and ":491" in comment


def test_abi_version_moved():
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", _header()).group(1)) > PARENT_ABI


def test_binding_lists_and_library_exports_the_entry():
    from neurallaplacecontrol_amd import _lib

    assert ENTRY in _lib.SYMBOLS
    so = _lib.LIB_PATH
    if not os.path.exists(so):
        pytest.fail(f"{so} is not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(so)
    assert hasattr(lib, ENTRY), f"libnlc_hip.so does not export {ENTRY}"
    assert lib.nlc_abi_version() > PARENT_ABI


def test_every_trainer_class_has_the_methods():
    import neurallaplacecontrol_amd as nlc

    for name in ("NLTrainer", "RNNTrainer", "NLTrainerGroup", "RNNTrainerGroup"):
        cls = getattr(nlc, name)
        for meth in ("keep_best", "restore_best", "fit"):
            assert callable(getattr(cls, meth, None)), (name, meth)
        assert isinstance(cls.best_loss, property) and isinstance(cls.best_tag, property), name


def test_the_training_headers_do_not_include_the_selection_header():
    csrc = os.path.join(REPO, "neurallaplacecontrol_amd", "csrc")
    for name in ("nlc_train.h", "nlc_train_dev.h", "nlc_train_eval.h", "kernels_train.hip", "kernels_train_rnn.hip",
                 "kernels_train_eval.hip"):
        assert "nlc_train_select.h" not in open(os.path.join(csrc, name)).read(), name


@pytest.mark.parametrize("step_size,gamma", [(2, 0.5), (3, 0.1)])
def test_step_lr_equals_torch_steplr(step_size, gamma):
    """fit's ``step_lr`` over 7 epochs against StepLR on a dummy CPU optimiser: ``==`` after every epoch (the chained
    multiply, which lr0 * gamma ** k does not reproduce: 1e-4 * 0.1 * 0.1 != 1e-4 * 0.1 ** 2 in float64)."""
    from neurallaplacecontrol_amd.training import step_lr_after_epoch

    lr0 = 1e-4
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr0)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=step_size, gamma=gamma)
    lr = lr0
    for epoch in range(7):
        opt.step()
        sched.step()
        lr = step_lr_after_epoch(lr, epoch + 1, step_size, gamma)
        assert lr == opt.param_groups[0]["lr"], (epoch, lr, opt.param_groups[0]["lr"])
    assert lr < lr0


def test_helper_stand_alone_under_sanitizers(tmp_path):
    """The helper with its own main(): the kernels' copy loops on the host over exact-size heap blocks, every row length
    and both row parities, under ASan + UBSan."""
    exe = tmp_path / "train_select_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), HELPER])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok"), res.stdout + res.stderr
