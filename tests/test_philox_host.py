"""CPU: the counter-based generator behind every device draw (csrc/nlc_philox.h: philox4x32_10, u53), built with g++, and the
independent reference the GPU stream tests compare against (tests/philox_ref.py): the published known answers, the library
against the reference word for word, the 53-bit uniform against its definition in exact rationals, and the counter builders
of the documented streams -- no two draws share a (counter, key), and a dropped or swapped input word changes every word."""

import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import philox_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
U32P = F64P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("philoxhost") / "libphilox_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "philox_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.nlc_p_philox.argtypes = [U32P, U32P, ctypes.c_long, U32P]
    lib.nlc_p_u53.argtypes = [U32P, U32P, ctypes.c_long, F64P]
    return lib


def _lib_philox(lib, counter, key):
    c = np.ascontiguousarray(counter, dtype=np.uint32).reshape(-1, 4)
    k = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
    out = np.empty_like(c)
    lib.nlc_p_philox(c.ctypes.data, k.ctypes.data, len(c), out.ctypes.data)
    return out


def _lib_u53(lib, hi, lo):
    hi, lo = np.ascontiguousarray(hi, dtype=np.uint32), np.ascontiguousarray(lo, dtype=np.uint32)
    out = np.empty(len(hi), dtype=np.float64)
    lib.nlc_p_u53(hi.ctypes.data, lo.ctypes.data, len(hi), out.ctypes.data)
    return out


# Random123's kat_vectors for philox4x32_10: counter, key, output
KAT = [
    ([0x00000000] * 4, [0x00000000] * 2, [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


def test_known_answer_vectors(lib):
    """The three published Random123 known answers, from the reference and from the library's generator."""
    for counter, key, want in KAT:
        ref = pr.philox4x32(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(x) for x in ref] == want, ("reference", [hex(int(x)) for x in ref])
        got = _lib_philox(lib, counter, key)[0]
        assert [int(x) for x in got] == want, ("library", [hex(int(x)) for x in got])
    # the round count is part of the answer: 7 rounds (the paper's other recommended count) give other words
    assert [int(x) for x in pr.philox4x32(np.zeros(4, np.uint64), np.zeros(2, np.uint64), rounds=7)] != KAT[0][2]


def test_library_generator_equals_the_reference_word_for_word(lib):
    """100 000 random (counter, key) pairs, then 6 x 2 000 pairs that differ from a base pair in ONE of the six input words
    only (random other value, and the lowest and the highest bit flipped): every output word equal."""
    rng = np.random.default_rng(1)
    words = rng.integers(0, 2**32, size=(100_000, 6), dtype=np.uint64)
    base = rng.integers(0, 2**32, size=6, dtype=np.uint64)
    single = []
    for w in range(6):
        x = np.tile(base, (2000, 1))
        x[:, w] = rng.integers(0, 2**32, size=2000, dtype=np.uint64)
        x[0, w], x[1, w] = base[w] ^ np.uint64(1), base[w] ^ np.uint64(0x80000000)
        single.append(x)
    words = np.concatenate([words, base[None]] + single)
    ref = pr.philox4x32(words[:, :4], words[:, 4:])
    got = _lib_philox(lib, words[:, :4], words[:, 4:])
    assert ref.shape == got.shape == (112_001, 4)
    assert np.array_equal(ref, got.astype(np.uint64))
    # and the single-word variants are all different blocks (every word of the block moves with one input bit)
    b = ref[100_000]
    for w in range(6):
        rows = ref[100_001 + 2000 * w : 100_001 + 2000 * w + 2]
        assert np.all(rows != b), w


# ---------------------------------------------------------------------------------------------------- u53
def _definition(hi, lo):
    """(v + 1/2) / 2^53 as an exact rational, v = the top 53 bits of hi:lo."""
    v = ((int(hi) << 32) | int(lo)) >> 11
    return (Fraction(v) + Fraction(1, 2)) / 2**53


def _both(lib, hi, lo):
    ref, got = pr.u53(np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)), _lib_u53(lib, hi, lo)
    assert np.array_equal(ref, got), "library u53 != reference u53"
    return got


def test_u53_end_points(lib):
    """All-zero words: (0 + 1/2) / 2^53 = 2^-54, exactly.  All-one words: v = 2^53 - 1 and the definition gives 1 - 2^-54,
    which no double holds: it lies half way between 1 - 2^-53 and 1.  The result must be a double within that half spacing
    (2^-54) of the defined value AND below 1: the largest double below 1.  (Round-to-nearest-even of the sum v + 0.5 alone gives
    1.0, which log() turns into a zero interval; u53 takes the double below.)"""
    zero, ones = _both(lib, [0, 0xFFFFFFFF], [0, 0xFFFFFFFF])
    assert Fraction(float(zero)) == _definition(0, 0) == Fraction(1, 2**54)
    want = _definition(0xFFFFFFFF, 0xFFFFFFFF)
    assert want == 1 - Fraction(1, 2**54)
    assert 0.0 < ones < 1.0
    assert abs(Fraction(float(ones)) - want) <= Fraction(1, 2**54)
    assert float(ones) == np.nextafter(1.0, 0.0)


def test_u53_range_definition_monotonicity_and_ignored_bits(lib):
    """Over 200 000 random 64-bit words and the words around every boundary (0, 2^63 -- where v + 1/2 stops being exact --
    and 2^64 - 1): never 0, never 1; equal to the definition exactly while v < 2^52 and within the half spacing 2^-54 above;
    non-decreasing in the 64-bit word hi:lo and strictly increasing in v below 2^52; the low 11 bits of lo do not matter, the
    12th does."""
    rng = np.random.default_rng(2)
    w = rng.integers(0, 2**64, size=200_000, dtype=np.uint64)
    edge = [0, 1, 2047, 2048, 4095, 4096, 2**32 - 1, 2**32, 2**63 - 2048, 2**63 - 1, 2**63, 2**63 + 2048, 2**63 + 4096,
            2**64 - 6144, 2**64 - 4096, 2**64 - 4095, 2**64 - 2049, 2**64 - 2048, 2**64 - 1]
    w = np.sort(np.concatenate([w, np.array(edge, dtype=np.uint64)]))
    hi, lo = (w >> np.uint64(32)).astype(np.uint32), (w & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    u = _both(lib, hi, lo)
    assert u.size == 200_019 and float(u.min()) > 0.0 and float(u.max()) < 1.0
    v = w >> np.uint64(11)
    d = np.diff(u)
    assert np.all(d >= 0.0)
    below = (v[1:] < 2**52) & (v[1:] != v[:-1])
    assert int(below.sum()) > 90_000 and np.all(d[below] > 0.0)
    checked = 0
    for k in list(range(0, w.size, 997)) + [int(np.searchsorted(w, np.uint64(e))) for e in edge]:
        want, got = _definition(hi[k], lo[k]), Fraction(float(u[k]))
        if int(v[k]) < 2**52:
            assert got == want, hex(int(w[k]))
        else:
            assert abs(got - want) <= Fraction(1, 2**54) and got < 1, hex(int(w[k]))
        checked += 1
    assert checked >= 200
    # the low 11 bits of lo are ignored: all-ones and all-zeros there give the same double; bit 11 does not
    lo_clear, lo_set = lo & np.uint32(0xFFFFF800), lo | np.uint32(0x7FF)
    assert np.array_equal(_both(lib, hi, lo_clear), _both(lib, hi, lo_set))
    small = v < 2**52
    flipped = _both(lib, hi[small], lo[small] ^ np.uint32(0x800))
    assert np.all(flipped != u[small])


# ---------------------------------------------------------------------------------------------------- counters of the streams
SEEDS = (7, 2**32 + 5)


def _rows(words):
    return words.reshape(-1, 6)


def _distinct(words, expect):
    w = _rows(words)
    assert w.shape[0] == expect, (w.shape, expect)
    assert np.unique(w, axis=0).shape[0] == expect


def test_no_two_draws_of_a_family_share_a_counter():
    """One of each: a planner's commands 0 and 1 (K = 300, T = 3; and 3 episodes of a batched planner, global indices e K + k),
    a collector step (300 episodes x streams 0 .. 4, over three steps), a synthetic dataset's blocks (pendulum
    samples_per_dim = 3: S = 9, A = 3, 4 blocks, B = 4 -- streams 0 .. 4 of the table): all (counter, key) pairs distinct
    within each, so no two draws of a command, a step or a dataset are the same numbers."""
    for seed in SEEDS:
        kg, t, c = np.meshgrid(np.arange(3 * 300), np.arange(3), np.arange(2), indexing="ij")
        _distinct(pr.planner_counter(kg, t, seed, c), 900 * 3 * 2)
        ep, it, st = np.meshgrid(5 + np.arange(300), np.arange(3), np.arange(5), indexing="ij")
        _distinct(pr.collector_counter(seed, ep, it, st), 300 * 3 * 5)
        TI, A, S, B = 4, 3, 9, 4
        ti_s, j = np.meshgrid(np.arange(TI), np.arange(S), indexing="ij")
        ti_a, i = np.meshgrid(np.arange(TI), np.arange(A), indexing="ij")
        r, b = np.meshgrid(np.arange(TI * A * S), np.arange(B), indexing="ij")
        words = [_rows(pr.synth_counter(seed, j, ti_s, pr.SYNTH_STATE_01)), _rows(pr.synth_counter(seed, j, ti_s, pr.SYNTH_STATE_23)),
                 _rows(pr.synth_counter(seed, i, ti_a, pr.SYNTH_ACTION)),
                 _rows(pr.synth_counter(seed, 0, np.arange(TI), pr.SYNTH_INTERVAL)), _rows(pr.synth_counter(seed, r, b, pr.SYNTH_FILL))]
        _distinct(np.concatenate(words), 2 * TI * S + TI * A + TI + TI * A * S * B)
    # the stream numbers are the documented ones
    assert (pr.COLLECT_INTERVAL, pr.COLLECT_ACTION_NOISE, pr.COLLECT_OBS_NOISE_01, pr.COLLECT_OBS_NOISE_23,
            pr.COLLECT_RANDOM_POLICY) == (0, 1, 2, 3, 4)
    assert (pr.SYNTH_STATE_01, pr.SYNTH_STATE_23, pr.SYNTH_ACTION, pr.SYNTH_INTERVAL, pr.SYNTH_FILL) == (0, 1, 2, 3, 4)


def test_high_words_reach_the_counter_and_the_key():
    """What only shows past 2^32: the high word of the global sample / episode / row index is counter word 1, the high word
    of the seed is key word 1, and the planner XORs the high word of its command counter into key word 1."""
    w = pr.planner_counter(2**32 + 3, 2, 2**32 * 9 + 7, 2**32 * 5 + 1)
    assert [int(x) for x in w] == [3, 1, 2, 1, 7, 9 ^ 5]
    assert [int(x) for x in pr.collector_counter(2**33 + 1, 2**32 * 6 + 4, 2, 3)] == [4, 6, 2, 3, 1, 2]
    assert [int(x) for x in pr.synth_counter(2**34 + 2, 2**32 + 8, 11, 4)] == [8, 1, 11, 4, 2, 4]


def _block_words(words):
    return pr.philox4x32(words[..., :4], words[..., 4:])


def test_one_changed_input_word_changes_every_output_word():
    """The value-for-value GPU comparison cannot pass by coincidence of a dropped or swapped word: the reference with any
    single input of a draw changed -- t + 1, kg + 1, kg + 2^32, seed + 2^32, counter + 2^32, stream + 1, ti <-> j -- differs
    from the unchanged one in EVERY output word of every draw (900 planner draws, 900 collector draws per stream, 81
    synthetic ones per stream; both seeds)."""
    compared = 0
    for seed in SEEDS:
        kg, t = np.meshgrid(np.arange(300), np.arange(3), indexing="ij")
        cnt = 1
        base = _block_words(pr.planner_counter(kg, t, seed, cnt))
        for name, words in (("t+1", pr.planner_counter(kg, t + 1, seed, cnt)), ("kg+1", pr.planner_counter(kg + 1, t, seed, cnt)),
                            ("kg+2^32", pr.planner_counter(kg + 2**32, t, seed, cnt)),
                            ("seed+2^32", pr.planner_counter(kg, t, seed + 2**32, cnt)),
                            ("counter+2^32", pr.planner_counter(kg, t, seed, cnt + 2**32)),
                            ("counter+1", pr.planner_counter(kg, t, seed, cnt + 1))):
            other = _block_words(words)
            assert other.shape == base.shape == (300, 3, 4) and np.all(other != base), (seed, name)
            compared += base.size
        ep, it = np.meshgrid(5 + np.arange(300), np.arange(3), indexing="ij")
        for stream in range(5):
            base = _block_words(pr.collector_counter(seed, ep, it, stream))
            for name, words in (("stream+1", pr.collector_counter(seed, ep, it, stream + 1)),
                                ("episode+2^32", pr.collector_counter(seed, ep + 2**32, it, stream)),
                                ("seed+2^32", pr.collector_counter(seed + 2**32, ep, it, stream)),
                                ("it+1", pr.collector_counter(seed, ep, it + 1, stream))):
                assert np.all(_block_words(words) != base), (seed, stream, name)
                compared += base.size
        # synthetic: the state counter is (j, ti) and the action counter (i, ti): transposed indices are other draws
        ti, j = np.meshgrid(np.arange(1, 10), np.arange(20, 29), indexing="ij")  # (ti != j everywhere)
        for stream in (pr.SYNTH_STATE_01, pr.SYNTH_STATE_23, pr.SYNTH_ACTION, pr.SYNTH_FILL):
            base = _block_words(pr.synth_counter(seed, j, ti, stream))
            for name, words in (("ti<->j", pr.synth_counter(seed, ti, j, stream)), ("stream+1", pr.synth_counter(seed, j, ti, stream + 1)),
                                ("index+2^32", pr.synth_counter(seed, j + 2**32, ti, stream)),
                                ("seed+2^32", pr.synth_counter(seed + 2**32, j, ti, stream))):
                assert np.all(_block_words(words) != base), (seed, stream, name)
                compared += base.size
    assert compared == 2 * (6 * 3600 + 5 * 4 * 3600 + 4 * 4 * 324)
    # the same through the draw functions: reuse moves the state and the action, not the interval or the fill
    a = pr.synth_draws(7, 3, 2, 5, 100, 1, reuse=False)
    b = pr.synth_draws(7, 3, 2, 5, 100, 1, reuse=True)
    assert np.all(a["state"] != b["state"]) and np.all(a["action"] != b["action"])
    assert a["interval"] == b["interval"] and np.array_equal(a["fill"], b["fill"])
    z = pr.synth_draws(7, 0, 2, 5, 100, 1, reuse=False)
    assert np.array_equal(z["state"], b["state"]) and np.array_equal(z["action"], b["action"]) and z["interval"] != b["interval"]


def test_normal_pair_and_the_coloured_draw():
    """normal_pair against mpmath-free closed forms: u2 = 1/2 is angle 0 (z = (rad, 0)), u2 = 3/4 is angle pi/2 (z = (0, rad)) --
    cos belongs to the first normal, sin to the second, and the angle is 2 pi u2 - pi; u1 = exp(-1/2) gives rad = 1.
    planner_eps applies the LOWER factor: eps_1 carries L_10 z_0, eps_0 carries nothing of z_1."""
    ld = np.longdouble
    u1 = np.exp(ld(-0.5))
    z0, z1, rad = pr.normal_pair(u1, ld(0.5))
    assert abs(rad - 1) < 1e-18 and abs(z0 - 1) < 1e-18 and abs(z1) < 1e-18
    z0, z1, _ = pr.normal_pair(u1, ld(0.75))
    assert abs(z0) < 1e-18 and abs(z1 - 1) < 1e-18
    z0, z1, _ = pr.normal_pair(u1, ld(0.25))
    assert abs(z0) < 1e-18 and abs(z1 + 1) < 1e-18
    mu, L = [0.25, -0.5], [[2.0, 0.0], [0.5, 3.0]]
    eps, rad = pr.planner_eps(11, 2, 7, 1, mu, L, with_rad=True)
    one = pr.planner_eps(11, 2, 7, 1, [0.0, 0.0], [[1.0, 0.0], [0.0, 1.0]])
    assert abs(eps[0] - (ld(0.25) + 2 * one[0])) < 1e-17 and abs(eps[1] - (ld(-0.5) + one[0] / 2 + 3 * one[1])) < 1e-17
    assert abs(one[0] ** 2 + one[1] ** 2 - rad**2) < 1e-17
    # a scalar planner (nu = 1) takes the first normal
    assert abs(pr.planner_eps(11, 2, 7, 1, [0.0], [[1.0]])[0] - one[0]) == 0
