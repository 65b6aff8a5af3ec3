"""CPU: the tiling of the Fourier ILT kernels (csrc/nlc_ilt_tile.h), built with g++: the stream kernels' block tile for every
term count the ABI accepts against the launchers' formulas (restated here in Python), the row-per-lane kernels' tile geometry
and launch shape for every term count they have an instance of, and the table of which launches the row kernels take."""

import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "helpers", "ilt_tile_host.cpp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("ilttile") / "libilt_tile_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", str(out), SRC])
    lib = ctypes.CDLL(str(out))
    lib.nlc_t_rows_grid.restype = ctypes.c_long
    return lib


def _stream(lib, S, backward):
    out = (ctypes.c_long * 4)()
    lib.nlc_t_stream(S, backward, out)
    return dict(zip(["rpp", "iters", "rows", "lds"], list(out)))


def test_max_terms_is_the_abi_limit(lib):
    assert lib.nlc_t_max_terms() == 129  # check_ilt: "ilt terms out of range [1,129]"


@pytest.mark.parametrize("backward", [0, 1])
def test_stream_tiling_equals_the_launcher_formulas(lib, backward):
    """launch_ilt_fourier / launch_ilt_fourier_bwd as they computed the block tile themselves.  No term count is left
    without a tile: iters >= 8 everywhere (the launchers once answered hipErrorInvalidValue below that, and their callers kept
    a fallback kernel for it)."""
    for S in range(1, 130):
        t = _stream(lib, S, backward)
        rpp = min(256 // S, 32)
        if backward:
            iters = 256 // rpp // 8 * 8
            lds = rpp * iters * 8
        else:
            iters = min(256, 7680 // (S | 1)) // rpp // 8 * 8
            lds = rpp * iters * (S | 1) * 8
        assert t == dict(rpp=rpp, iters=iters, rows=rpp * iters, lds=lds), S
        assert t["iters"] % 8 == 0 and t["iters"] >= 8, S
        assert t["rpp"] * 8 <= 256 and t["rpp"] * S <= 256, S
        assert t["rows"] <= 256, S
        assert t["lds"] <= 60 * 1024, S
    # the shapes whose comments and tests quote these numbers
    assert _stream(lib, 17, 0)["iters"] == 16 and _stream(lib, 16, 0)["iters"] == 16
    assert (_stream(lib, 86, 0)["iters"], _stream(lib, 86, 0)["rows"]) == (40, 80)
    assert (_stream(lib, 129, 0)["iters"], _stream(lib, 129, 0)["rows"]) == (56, 56)
    assert _stream(lib, 1, 0)["iters"] == 8


_ROWS = ["TILE", "SLOT", "NLD", "REM", "LPT", "depth", "fwd_per_cu", "bwd_per_cu", "fwd_lds", "bwd_lds"]


@pytest.mark.parametrize("S", list(range(3, 34, 2)))
def test_row_tile_geometry_and_launch_shape(lib, S):
    out = (ctypes.c_long * 10)()
    lib.nlc_t_rows(S, out)
    r = dict(zip(_ROWS, list(out)))
    assert r["TILE"] == 64 * S * 8
    assert r["SLOT"] % 1024 == 0 and r["SLOT"] >= r["TILE"] and r["SLOT"] == (r["TILE"] + 1023) // 1024 * 1024
    assert (r["NLD"], r["REM"], r["LPT"]) == (r["TILE"] // 1024, r["TILE"] % 1024, r["SLOT"] // 1024)
    assert r["REM"] % 16 == 0  # the last load's lanes carry 16 bytes each
    # the rules as the launchers and launch bounds spelled them out
    depth = 2 if S <= 17 else 1
    assert r["depth"] == depth
    assert r["fwd_per_cu"] == (2 if (S <= 17 and depth == 1) else 1)
    assert r["bwd_per_cu"] == (2 if S <= 17 else 1)
    assert r["fwd_lds"] == 4 * depth * 2 * r["SLOT"] + 16 * S and r["fwd_lds"] <= 160 * 1024
    assert r["bwd_lds"] == 4 * 2 * r["SLOT"] and r["bwd_per_cu"] * r["bwd_lds"] <= 160 * 1024


def test_row_grid_cap(lib):
    for tiles in (0, 1, 4, 5, 1023, 1024, 1025, 2048, 2049, 10**9):
        for per_cu in (1, 2):
            assert lib.nlc_t_rows_grid(ctypes.c_long(tiles), per_cu) == min((tiles + 3) // 4, 256 * per_cu)


def test_row_kernel_acceptance_table(lib):
    """Forward: odd S in 3 .. 33, 16-byte aligned theta / phi, and never one linear table without the other; any scale (the
    general-phase instance takes scale != 2 and the linear algorithms).  Backward: the same term counts and alignment, the
    Fourier series at scale == 2 only."""
    base = 0x7F0000001000
    for S in range(1, 41):
        terms = 3 <= S <= 33 and S % 2 == 1
        for scale in (2.0, 3.0):
            for wr in (0, 1):
                for wi in (0, 1):
                    for off in (0, 8):
                        v = lib.nlc_t_rows_accept(S, ctypes.c_double(scale), wr, wi, ctypes.c_ulong(base + off))
                        case = (S, scale, wr, wi, off)
                        assert bool(v & 1) == (terms and off == 0 and not (wr and not wi)), case
                        assert bool(v & 2) == (bool(wr) or scale != 2.0), case
                        assert bool(v & 4) == (terms and off == 0 and scale == 2.0), case

