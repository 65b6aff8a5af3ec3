"""CPU: the layout of the "gru_prefix" table's hidden-side products (csrc/nlc_gru_prefix.h), built with g++ -- which entries
start a tile, how many steps the table build runs to see every one of them, and where a lane finds its accumulator sets."""

import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("gruprefixproducts") / "libgru_prefix_products_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "gru_prefix_products_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.nlc_gpp_products_doubles.restype = ctypes.c_long
    lib.nlc_gpp_products_entry_offset.restype = ctypes.c_long
    return lib


def test_which_entries_start_a_tile(lib):
    """A tile starts from an entry of length 1 .. min(B, 5) - 1: the lists below B, four steps at most.  B = 4: 2 + 4 + 8
    = 14 entries; from B = 5 on all 30."""
    for B in range(1, 10):
        lens = [n for n in range(0, 7) if lib.nlc_gpp_starts_tile(n, B)]
        assert lens == list(range(1, min(B, 5)))
    assert sum(1 << n for n in range(1, 7) if lib.nlc_gpp_starts_tile(n, 4)) == 14
    assert sum(1 << n for n in range(1, 7) if lib.nlc_gpp_starts_tile(n, 5)) == 30
    assert not lib.nlc_gpp_starts_tile(1, 1) and lib.nlc_gpp_starts_tile(1, 2) and not lib.nlc_gpp_starts_tile(2, 2)


def test_build_runs_the_step_after_every_starting_entry(lib):
    """The products of an entry of length n are stored by step n of the build, so the build runs steps 0 .. n for the longest
    starting entry -- and never more than B steps."""
    for B in range(1, 34):
        steps = lib.nlc_gpp_build_steps(B)
        assert steps <= B and steps == min(B, 5)
        longest = max([n for n in range(1, 7) if lib.nlc_gpp_starts_tile(n, B)], default=0)
        assert steps >= longest + 1
        assert steps >= min(B, 4)  # every image is still stored


@pytest.mark.parametrize("g", [32, 64, 128])
def test_products_layout(lib, g):
    """6 g doubles per entry 1 .. 30, back to back; inside an entry every (layer, chunk, set, q, r) has a slot of its own, a
    lane's four registers are contiguous and the v4d starts on a multiple of four doubles."""
    assert lib.nlc_gpp_products_doubles(g) == 30 * 6 * g
    assert [lib.nlc_gpp_products_entry_offset(e, g) for e in (1, 2, 30)] == [0, 6 * g, 29 * 6 * g]
    assert lib.nlc_gpp_products_entry_offset(30, g) + 6 * g == lib.nlc_gpp_products_doubles(g)
    seen = set()
    for layer in range(2):
        for j in range(g // 16):
            for s in range(3):
                for q in range(4):
                    base = lib.nlc_gpp_products_index(layer, j, s, q, 0, g)
                    assert base % 4 == 0
                    for r in range(4):
                        i = lib.nlc_gpp_products_index(layer, j, s, q, r, g)
                        assert i == base + r
                        seen.add(i)
    assert seen == set(range(6 * g))
    if g == 64:
        assert 14 * 6 * g * 8 == 43008  # the 42 KB that B = 4 uses
