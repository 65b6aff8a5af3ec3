"""CPU: the host side of the fused de Hoog training step -- the workspace layout of csrc/nlc_train_dehoog.h built with g++
(as tests/test_train_eval_host.py builds the evaluation layouts), the option in the header and the trainer's keyword.  The
helper has a main() and is also built stand-alone under AddressSanitizer / UBSan and run."""

import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HELPER = os.path.join(HERE, "helpers", "train_dehoog_host.cpp")
FIELDS = ("rows", "theta", "phi", "gtheta", "gphi", "pred", "gx", "t", "scratch", "scratch_bytes", "total")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("traindehooghost") / "libtrain_dehoog_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), HELPER])
    lib = ctypes.CDLL(str(out))
    lib.nlc_t_dehoog_ws_layout.argtypes = [ctypes.c_int, ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    lib.nlc_t_dehoog_member_total.argtypes = [ctypes.c_int64] + [ctypes.c_int] * 4
    lib.nlc_t_dehoog_member_total.restype = ctypes.c_int64
    lib.nlc_t_dehoog_tape_entries.argtypes = [ctypes.c_int]
    lib.nlc_t_dehoog_tape_entries.restype = ctypes.c_int64
    lib.nlc_t_dehoog_scratch_bytes.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.nlc_t_dehoog_scratch_bytes.restype = ctypes.c_int64
    return lib


def _layout(lib, M, N, d, h, S, nin=1):
    out = (ctypes.c_int64 * len(FIELDS))()
    lib.nlc_t_dehoog_ws_layout(M, N, d, nin, h, S, out)
    return dict(zip(FIELDS, out))


def _tape_entries(Mq):
    """The value tape of ilt_dehoog_bwd_kernel<Mq>, counted column by column as kernels_dehoog_bwd.hip describes it: q column
    r holds 2 (Mq - r) + 2 entries, an even e column 2 (Mq - r) + 1, an odd one its first entry only, A and B 2 Mq + 1 each."""
    q = sum(2 * (Mq - r) + 2 for r in range(1, Mq + 1))
    e = sum(2 * (Mq - r) + 1 if r % 2 == 0 else 1 for r in range(1, Mq + 1))
    return q + e + 2 * (2 * Mq + 1)


def _ilt_scratch_bytes(rows, d, S):
    """ilt_dehoog_bwd_scratch_bytes(rows, d, S): a slab of 64 rows x 16 bytes per entry for each workgroup of its grid."""
    grid = min((rows * d + 63) // 64, 2048 if (S - 1) // 2 <= 8 else 1024)
    return grid * _tape_entries((S - 1) // 2) * 64 * 16


def test_tape_entries_match_the_kernel_s_layout(lib):
    assert _tape_entries(16) == 466 and _tape_entries(1) == 9  # the kernel's static_asserts
    for Mq in range(1, 17):
        assert lib.nlc_t_dehoog_tape_entries(Mq) == _tape_entries(Mq)


CASES = [(M, N, d, h, S) for M in (1, 2, 5, 64) for N in (1, 13, 16, 17, 37, 2048) for d, h, S in
         ((1, 64, 3), (3, 128, 5), (5, 128, 17), (5, 64, 33), (8, 256, 33))]


@pytest.mark.parametrize("M,N,d,h,S", CASES)
def test_regions_are_aligned_disjoint_and_m_copies(lib, M, N, d, h, S):
    w = _layout(lib, M, N, d, h, S)
    rows = -(-N // 16) * 16
    assert w["rows"] == rows
    mt = lib.nlc_t_dehoog_member_total(N, d, 1, h, S)
    assert mt % 32 == 0
    sizes = {"theta": M * rows * d * S, "phi": M * rows * d * S, "gtheta": M * rows * d * S, "gphi": M * rows * d * S,
             "pred": M * rows * d, "gx": M * rows * d, "t": M * rows, "scratch": -(-w["scratch_bytes"] // 8)}
    # the members' shared regions come first, M copies of one member's; then the ILT arrays in order, each 256-byte aligned,
    # none overlapping the next, all inside the total
    end = M * mt
    for name in ("theta", "phi", "gtheta", "gphi", "pred", "gx", "t", "scratch"):
        assert w[name] % 32 == 0, name
        assert w[name] >= end, name
        end = w[name] + sizes[name]
    assert end <= w["total"] and w["total"] % 32 == 0
    # M members back to back inside an ILT array: M copies of the single layout's array
    # (member m's slice starts m * per doubles into the array), and nothing but the 256-byte round-up between two arrays
    order = ("theta", "phi", "gtheta", "gphi", "pred", "gx", "t", "scratch")
    per = {"theta": rows * d * S, "phi": rows * d * S, "gtheta": rows * d * S, "gphi": rows * d * S, "pred": rows * d,
           "gx": rows * d, "t": rows}
    for name, nxt in zip(order, order[1:]):
        assert w[nxt] - w[name] == -(-(M * per[name]) // 32) * 32, name
    assert w["theta"] == M * mt
    # the tape is what the ILT launcher asks for at M * rows points
    assert w["scratch_bytes"] == _ilt_scratch_bytes(M * rows, d, S)
    assert lib.nlc_t_dehoog_scratch_bytes(M * rows * d, S) == w["scratch_bytes"]


def test_sizes_are_monotone_in_n_up_to_2048_and_capped_beyond(lib):
    for d, h, S in ((3, 128, 5), (5, 128, 33)):
        last = 0
        for N in range(1, 2049, 7):
            tot = _layout(lib, 3, N, d, h, S)["total"]
            assert tot >= last
            last = tot
        assert _layout(lib, 3, 2048, d, h, S)["rows"] == 2048
        # (a larger N is refused by the entries; the layout stays defined, at the largest grid)
        assert _layout(lib, 3, 2049, d, h, S)["rows"] == 2048


def test_a_pure_function_of_its_arguments(lib):
    assert _layout(lib, 5, 37, 5, 128, 17) == _layout(lib, 5, 37, 5, 128, 17)
    assert _layout(lib, 5, 37, 5, 128, 17) == _layout(lib, 5, 48, 5, 128, 17)  # the same tiles


def test_option_is_documented_and_the_keyword_is_checked():
    header = open(os.path.join(REPO, "include", "nlc.h")).read()
    assert '"train_dehoog"' in header
    ctx_src = open(os.path.join(REPO, "neurallaplacecontrol_amd", "csrc", "abi_ctx.hip")).read()
    assert 'n == "train_dehoog"' in ctx_src
    import inspect

    import neurallaplacecontrol_amd as nlc

    for cls in (nlc.NLTrainer, nlc.NLTrainerGroup):
        assert inspect.signature(cls.__init__).parameters["dehoog"].default == "grad"
    tr = nlc.NLTrainer.__new__(nlc.NLTrainer)
    assert tr._dehoog_mode("fused") == "fused" and tr._dehoog_mode("grad") == "grad"
    with pytest.raises(ValueError, match="dehoog"):
        tr._dehoog_mode("hip")
    for cls in (nlc.RNNTrainer, nlc.NODETrainer):
        assert "dehoog" not in inspect.signature(cls.__init__).parameters


def test_gpu_cases_cover_the_issue_edges():
    """The case table of tests/test_gpu_train_dehoog.py keeps the shapes it was built for (a guard against editing them away)."""
    from test_gpu_train_dehoog import LG_CASES

    assert {c[2] for c in LG_CASES} == {3, 5, 17, 33} and {c[0] for c in LG_CASES} == {1, 3, 5}
    assert {c[1] for c in LG_CASES} == {64, 128} and {c[4] for c in LG_CASES} == {1, 4, 16}
    assert {c[3] for c in LG_CASES} == {1, 13, 16, 17, 37, 2048} and {c[5] for c in LG_CASES} == {True, False}


def test_helper_stand_alone_under_sanitizers(tmp_path):
    """The layout helper with its own main(): every accepted shape, under ASan + UBSan."""
    exe = tmp_path / "train_dehoog_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), HELPER])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok"), res.stdout + res.stderr
