"""CPU: csrc/nlc_devbuf.h built with g++ (tests/helpers/devbuf_host.cpp) -- the owner of the host side's device and pinned
allocations over a counting malloc policy, and the two weight folds of a model upload against NumPy loops in the same
order, compared with ``==``.  The helper has a main() and is also built stand-alone under AddressSanitizer / UBSan and run:
there a "setter" with the model setters' commit rule fails each of its allocations in turn."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HELPER = os.path.join(HERE, "helpers", "devbuf_host.cpp")
ERR = 2  # the counting policy's status for a failed allocation


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("devbufhost") / "libdevbuf_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), HELPER])
    lib = ctypes.CDLL(str(out))
    vp, lg = ctypes.c_void_p, ctypes.c_long
    for name, res, args in [
        ("buf_new", vp, []), ("buf_delete", None, [vp]), ("buf_hold", ctypes.c_int, [vp, lg]),
        ("buf_grow", ctypes.c_int, [vp, lg]), ("buf_reset", None, [vp]), ("buf_size", lg, [vp]), ("buf_get", vp, [vp]),
        ("buf_move", None, [vp, vp]), ("buf_move_new", vp, [vp]), ("fail_at", None, [lg]), ("counts", None, [vp]),
        ("fold_b1", None, [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]),
        ("fold_input_bias", None, [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]),
    ]:
        f = getattr(lib, "nlc_t_" + name)
        f.restype, f.argtypes = res, args
    return lib


def _counts(lib):
    out = np.zeros(3, dtype=np.int64)
    lib.nlc_t_counts(out.ctypes.data)
    return dict(zip(("live", "allocs", "frees"), (int(v) for v in out)))


def test_buf_owns_one_block(lib):
    c0 = _counts(lib)
    b = lib.nlc_t_buf_new()
    assert lib.nlc_t_buf_get(b) is None and lib.nlc_t_buf_size(b) == 0

    # hold: exactly n, the old block freed exactly once
    assert lib.nlc_t_buf_hold(b, 5) == 0 and lib.nlc_t_buf_size(b) == 5
    assert lib.nlc_t_buf_hold(b, 9) == 0 and lib.nlc_t_buf_size(b) == 9
    c = _counts(lib)
    assert (c["allocs"] - c0["allocs"], c["frees"] - c0["frees"], c["live"] - c0["live"]) == (2, 1, 1)

    # grow: nothing while n <= size(), else size() is the new n
    p = lib.nlc_t_buf_get(b)
    assert lib.nlc_t_buf_grow(b, 9) == 0 and lib.nlc_t_buf_grow(b, 1) == 0
    assert lib.nlc_t_buf_get(b) == p and lib.nlc_t_buf_size(b) == 9 and _counts(lib) == c
    assert lib.nlc_t_buf_grow(b, 10) == 0 and lib.nlc_t_buf_size(b) == 10
    c = _counts(lib)
    assert (c["allocs"] - c0["allocs"], c["frees"] - c0["frees"], c["live"] - c0["live"]) == (3, 2, 1)

    # a move leaves the source empty and frees nothing; a move onto a buffer frees that buffer's block
    p = lib.nlc_t_buf_get(b)
    m = lib.nlc_t_buf_move_new(b)
    assert lib.nlc_t_buf_get(b) is None and lib.nlc_t_buf_size(b) == 0
    assert lib.nlc_t_buf_get(m) == p and lib.nlc_t_buf_size(m) == 10 and _counts(lib) == c
    assert lib.nlc_t_buf_hold(b, 3) == 0
    lib.nlc_t_buf_move(b, m)
    assert lib.nlc_t_buf_get(m) is None and lib.nlc_t_buf_get(b) == p and lib.nlc_t_buf_size(b) == 10
    c = _counts(lib)
    assert (c["allocs"] - c0["allocs"], c["frees"] - c0["frees"], c["live"] - c0["live"]) == (4, 3, 1)

    # reset is idempotent
    lib.nlc_t_buf_reset(b)
    lib.nlc_t_buf_reset(b)
    assert lib.nlc_t_buf_get(b) is None and lib.nlc_t_buf_size(b) == 0
    assert _counts(lib)["frees"] - c0["frees"] == 4

    # a failing alloc leaves the buffer empty and reports the policy's status
    assert lib.nlc_t_buf_hold(b, 4) == 0
    for op in (lib.nlc_t_buf_hold, lib.nlc_t_buf_grow):
        lib.nlc_t_fail_at(0)
        assert op(b, 6) == ERR
        assert lib.nlc_t_buf_get(b) is None and lib.nlc_t_buf_size(b) == 0
    assert lib.nlc_t_buf_grow(b, 6) == 0 and lib.nlc_t_buf_size(b) == 6

    lib.nlc_t_buf_delete(b)
    lib.nlc_t_buf_delete(m)
    c = _counts(lib)
    assert c["live"] == c0["live"] == 0 and c["allocs"] - c0["allocs"] == c["frees"] - c0["frees"]


@pytest.mark.parametrize("h,S", [(64, 3), (256, 33)])
def test_fold_b1_keeps_its_bits(lib, h, S):
    rng = np.random.default_rng(h + S)
    W1s, b1, sph = rng.standard_normal((h, 2 * S)), rng.standard_normal(h), rng.uniform(-1.6, 1.6, 2 * S)
    out = np.zeros(h)
    lib.nlc_t_fold_b1(W1s.ctypes.data, b1.ctypes.data, h, S, sph.ctypes.data, out.ctypes.data)
    ref = np.zeros(h)
    for r in range(h):
        acc = b1[r]  # one accumulator seeded with the bias, j ascending
        for j in range(2 * S):
            acc = acc + W1s[r, j] * sph[j]
        ref[r] = acc
    assert (out == ref).all()


@pytest.mark.parametrize("g,nin", [(32, 1), (160, 3)])
def test_fold_input_bias(lib, g, nin):
    rows = 3 * g
    rng = np.random.default_rng(rows + nin)
    Wih, bih, bhh = rng.standard_normal((rows, nin)), rng.standard_normal(rows), rng.standard_normal(rows)
    out = np.full((rows, 4), np.nan)
    lib.nlc_t_fold_input_bias(Wih.ctypes.data, bih.ctypes.data, bhh.ctypes.data, rows, nin, 2 * g, out.ctypes.data)
    ref = np.zeros((rows, 4))
    ref[:, :nin] = Wih
    ref[:, 3] = bih
    ref[: 2 * g, 3] = bih[: 2 * g] + bhh[: 2 * g]  # r and z gates: both biases; n gate: the input side's only
    assert (out == ref).all()


def test_helper_stand_alone_under_sanitizers(tmp_path):
    """The helper with its own main(): the buffer's life, then a setter that builds a local group of three buffers and
    commits it by a move -- every allocation failing in turn leaves the ctx's group untouched and leaks nothing, and a
    successful one frees the old group's blocks once.  Under ASan + UBSan (double frees, leaks at exit)."""
    exe = tmp_path / "devbuf_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), HELPER])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok"), res.stdout + res.stderr
