"""CPU: the host side of grouped training -- the six nlc_train_group_* / nlc_rnn_train_group_* entries in the header, the
binding's symbol list and the built library; the package's exports; and the per-member workspace partition of
csrc/nlc_train.h (train_ws_layout), built with g++ as tests/test_train_host.py builds the element math."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ENTRIES = [f"nlc_{fam}train_group_{what}" for fam in ("", "rnn_") for what in ("workspace_bytes", "loss_grad", "step")]


def _header():
    return open(os.path.join(REPO, "include", "nlc.h")).read()


@pytest.mark.parametrize("name", ENTRIES)
def test_header_declares_the_entry_with_the_ctx_first(name):
    m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(\s*nlc_ctx\s*\*\s*ctx\s*,", _header())
    assert m, f"{name}(nlc_ctx* ctx, ...) is not declared in include/nlc.h"
    assert (m.group(1) == "int64_t") == name.endswith("workspace_bytes")


def test_header_cites_the_reference_for_every_entry():
    hdr = _header()
    for name in ENTRIES:
        before = hdr[: hdr.index(name + "(")]
        comment = before[before.rindex("/*") :]
        assert "train_utils.py:3" in comment and "run_exp_multi.py:105-110" in comment, name


def test_abi_version_is_at_least_12():
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", _header()).group(1)) >= 12


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
    assert lib.nlc_abi_version() >= 12


def test_package_exports_the_group_trainers():
    import neurallaplacecontrol_amd as nlc

    for name in ("NLTrainerGroup", "RNNTrainerGroup"):
        assert name in nlc.__all__ and hasattr(nlc, name)
    assert issubclass(nlc.NLTrainerGroup, nlc.NLTrainer) and issubclass(nlc.RNNTrainerGroup, nlc.RNNTrainer)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("traingrouphost") / "libtrain_group_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "train_group_host.cpp")])
    return ctypes.CDLL(str(out))


def _layout(lib, rnn, d, nin, h, S, N):
    out = np.zeros(10, dtype=np.int64)
    lib.nlc_t_member_layout.argtypes = [ctypes.c_int] * 5 + [ctypes.c_int64, ctypes.c_void_p]
    lib.nlc_t_member_layout(rnn, d, nin, h, S, N, out.ctypes.data)
    names = ("partial", "tile_loss", "act", "grad", "sq", "total", "nblk", "P", "A", "chunks")
    return dict(zip(names, (int(v) for v in out)))


def _parent_ws_doubles(nblk, P, A, chunks):
    """The single-model workspace size as the library computed it before groups existed: five arrays, each rounded up to 32
    doubles."""
    al = lambda n: (n + 31) // 32 * 32  # noqa: E731
    return al(nblk * P) + al(nblk) + al(nblk * A) + al(P) + al(chunks)


@pytest.mark.parametrize("rnn,d,nin,h,S", [(0, 3, 1, 64, 3), (0, 5, 1, 128, 17), (0, 6, 2, 256, 33), (1, 3, 1, 64, 0), (1, 5, 1, 160, 0)])
@pytest.mark.parametrize("N", [1, 16, 17, 37, 2048, 2100])
def test_member_regions_are_disjoint_aligned_and_m1_is_todays_layout(lib, rnn, d, nin, h, S, N):
    L = _layout(lib, rnn, d, nin, h, S, N)
    assert L["nblk"] == min((N + 15) // 16, 128)
    sizes = {"partial": L["nblk"] * L["P"], "tile_loss": L["nblk"], "act": L["nblk"] * L["A"], "grad": L["P"], "sq": L["chunks"]}
    assert L["total"] == _parent_ws_doubles(L["nblk"], L["P"], L["A"], L["chunks"]), "M = 1 must reproduce the single layout"
    for M in (1, 2, 5):
        spans = []
        for m in range(M):
            base = m * L["total"]
            assert (base * 8) % 256 == 0
            for k, n in sizes.items():
                assert ((base + L[k]) * 8) % 256 == 0, (m, k)
                spans.append((base + L[k], base + L[k] + n))
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] <= M * L["total"]
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "arrays of the members overlap"
