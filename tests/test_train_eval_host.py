"""CPU: the host side of the held-out loss -- the eight nlc_*train*_eval entries in the header, the binding's symbol list and
the built library; ``evaluate`` on the four trainer classes; and the layouts of csrc/nlc_train_eval.h (the tile-loss
workspace, the grid rule, a workgroup's LDS partition), built with g++ as tests/test_train_group_host.py builds
train_ws_layout.  The helper has a main() and is also built stand-alone under AddressSanitizer / UBSan and run."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HELPER = os.path.join(HERE, "helpers", "train_eval_host.cpp")
ENTRIES = [f"nlc_{fam}train_{grp}eval{what}" for fam in ("", "rnn_") for grp in ("group_", "") for what in ("_workspace_bytes", "")]
PARENT_ABI = 15


def _header():
    return open(os.path.join(REPO, "include", "nlc.h")).read()


def test_there_are_eight_entries():
    assert len(set(ENTRIES)) == 8


@pytest.mark.parametrize("name", ENTRIES)
def test_header_declares_the_entry_and_cites_the_reference(name):
    hdr = _header()
    m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(\s*nlc_ctx\s*\*\s*ctx\s*,", hdr)
    assert m, f"{name}(nlc_ctx* ctx, ...) is not declared in include/nlc.h"
    assert (m.group(1) == "int64_t") == name.endswith("workspace_bytes")
    before = hdr[: m.start()]
    comment = before[before.rindex("/*") :]
    assert "overlay.py:112-115" in comment and ":175-177" in comment, name


def test_abi_version_moved():
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", _header()).group(1)) > PARENT_ABI


def test_binding_lists_and_library_exports_the_entries():
    from neurallaplacecontrol_amd import _lib

    for name in ENTRIES:
        assert name in _lib.SYMBOLS, name
    so = _lib.LIB_PATH
    if not os.path.exists(so):
        pytest.fail(f"{so} is not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(so)
    for name in ENTRIES:
        assert hasattr(lib, name), f"libnlc_hip.so does not export {name}"
    assert lib.nlc_abi_version() > PARENT_ABI


def test_every_trainer_class_has_evaluate():
    import neurallaplacecontrol_amd as nlc

    for name in ("NLTrainer", "RNNTrainer", "NLTrainerGroup", "RNNTrainerGroup"):
        cls = getattr(nlc, name)
        assert callable(getattr(cls, "evaluate", None)), name
        assert cls._eval_entries[0] in ENTRIES and cls._eval_entries[1] in ENTRIES, name


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("trainevalhost") / "libtrain_eval_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), HELPER])
    lib = ctypes.CDLL(str(out))
    lib.nlc_t_eval_ws_layout.argtypes = [ctypes.c_int64, ctypes.c_void_p]
    lib.nlc_t_eval_grid.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.nlc_t_eval_lds_layout.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    lib.nlc_t_rnn_eval_lds_bytes.restype = ctypes.c_int64
    return lib


@pytest.mark.parametrize("N", [1, 16, 17, 4103, 156_250])
def test_workspace_regions(lib, N):
    out = np.zeros(3, dtype=np.int64)
    lib.nlc_t_eval_ws_layout(N, out.ctypes.data)
    ntiles, tile_loss, total = (int(v) for v in out)
    assert ntiles == -(-N // 16)
    assert (total * 8) % 256 == 0 and total >= ntiles and total - ntiles < 32
    for M in (1, 2, 5):
        spans = [(m * total + tile_loss, m * total + tile_loss + ntiles) for m in range(M)]
        assert all((a * 8) % 256 == 0 for a, _ in spans)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "members' tile losses overlap"
        assert spans[-1][1] <= M * total


def test_grid_rule(lib):
    g = lib.nlc_t_eval_grid
    assert g(1, 256, 2, 1) == 1 and g(300, 256, 2, 1) == 300  # a workgroup per tile while the chip has room
    assert g(9766, 256, 2, 1) == 512 and g(9766, 256, 1, 1) == 256  # not the training step's cap of 128
    assert g(9766, 256, 2, 3) == 170 and g(9766, 256, 2, 64) == 8  # the members share the chip
    assert g(1, 256, 2, 65535) == 1 and g(100, 256, 2, 65535) == 1


def test_row_stride_rule(lib):
    for n in range(1, 600):
        ld = lib.nlc_t_eval_ld(n)
        assert n <= ld <= n + 4 and ld % 4 == 2
        # 16 rows start on 16 different bank quads (64 banks of 4 bytes)
        assert len({(r * ld * 2) % 64 // 4 for r in range(16)}) == 16


@pytest.mark.parametrize("d,nin,h,S,B", [(1, 1, 64, 3, 1), (5, 2, 128, 17, 5), (6, 1, 256, 33, 16), (8, 3, 256, 129, 16), (5, 1, 64, 8, 4)])
def test_lds_partition(lib, d, nin, h, S, B):
    out = np.zeros(18, dtype=np.int64)
    lib.nlc_t_eval_lds_layout(d, nin, h, S, B, out.ctypes.data)
    names = ("X", "a0", "tn", "tgt", "sq", "h0", "h1", "G", "a1", "a2", "u", "total", "ldg", "ldG", "ldK", "ldh", "ldu", "dc")
    L = dict(zip(names, (int(v) for v in out)))
    g, K0 = h // 2, 2 * S + d + 2
    assert L["total"] * 8 <= 160 * 1024
    assert 1 <= L["dc"] <= d and L["ldu"] >= 2 * L["dc"] * S
    assert L["ldg"] >= g and L["ldG"] >= 4 * g and L["ldK"] >= K0 and L["ldh"] >= h
    size = {"X": B * 16 * nin, "a0": 16 * L["ldK"], "tn": 16, "tgt": 16 * d, "sq": 16 * d, "h0": 16 * L["ldg"], "h1": 16 * L["ldg"],
            "G": 16 * L["ldG"], "a1": 16 * L["ldh"], "a2": 16 * L["ldh"], "u": 16 * L["ldu"]}
    # the arrays live together in two phases: the encoder's and the MLP's share what the per-tile inputs leave
    for phase in (("X", "a0", "tn", "tgt", "sq", "h0", "h1", "G"), ("X", "a0", "tn", "tgt", "sq", "a1", "a2", "u")):
        spans = sorted((L[k], L[k] + size[k]) for k in phase)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), phase
        assert spans[-1][1] <= L["total"]
    if (d, S, h) != (8, 129, 256):
        assert L["dc"] == d


def test_rnn_lds_fits(lib):
    for H in (64, 128, 160):
        assert 16 * (4 * H + 4) * 8 < lib.nlc_t_rnn_eval_lds_bytes(H) <= 160 * 1024


def test_helper_stand_alone_under_sanitizers(tmp_path):
    """The layout helper with its own main(): every accepted shape's LDS partition, under ASan + UBSan."""
    exe = tmp_path / "train_eval_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), HELPER])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok"), res.stdout + res.stderr
