"""CPU: the window classification of the "gru_prefix" encoder launch (csrc/nlc_gru_prefix.h), built with g++, against a
restatement in Python -- which windows of the MPPI history start with clipped actions, how many of them, and with which
pattern of upper / lower bound."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("gruprefix") / "libgru_prefix_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "gru_prefix_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.nlc_gp_worst_case_tiles.restype = ctypes.c_long
    return lib


def restate(perturbed, B, u_max, u_min, u_scale):
    """(len, pattern) of every window (k, t): GRU step s consumes history element t + B - 1 - s; elements below B - 1 come from
    the action buffer and end the count; an element counts while its stored bits are those of a bound's image."""
    K, T = perturbed.shape
    bits = perturbed.view(np.uint64)
    hi, lo = ((np.array([b], np.float64) / np.float64(u_scale)).view(np.uint64)[0] for b in (u_max, u_min))
    out = np.zeros((K, T, 2), np.int32)
    for k in range(K):
        for t in range(T):
            for s in range(min(B, 4)):
                i = t + B - 1 - s
                if i < B - 1 or bits[k, i - (B - 1)] not in (hi, lo):
                    break
                out[k, t, 0] = s + 1
                out[k, t, 1] |= int(bits[k, i - (B - 1)] != hi) << s
    return out


def classify(lib, perturbed, B, u_max, u_min, u_scale):
    K, T = perturbed.shape
    p = np.ascontiguousarray(perturbed, np.float64)
    out = np.zeros((K, T, 2), np.int32)
    lib.nlc_gp_classify(p.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(K), T, B, ctypes.c_double(u_max),
                        ctypes.c_double(u_min), ctypes.c_double(u_scale), out.ctypes.data_as(ctypes.c_void_p))
    return out


def clipped_draw(rng, K, T, u_max, u_min, u_scale, sigma=1.0, U=0.0):
    """What perturb_kernel stores: clip(u_scale (U + eps)) / u_scale."""
    v = (U + sigma * rng.standard_normal((K, T))) * u_scale
    return np.maximum(np.minimum(v, u_max), u_min) / u_scale


@pytest.mark.parametrize("B", [2, 4, 5])
@pytest.mark.parametrize("u_max,u_min,u_scale", [(3.0, -3.0, 3.0), (2.0, -0.5, 3.0), (1.5, 0.25, 0.7), (10.0, -10.0, -3.0)])
def test_random_windows(lib, B, u_max, u_min, u_scale):
    """Symmetric bounds at one sigma (the reference's configuration), asymmetric bounds, u_max != u_scale, a negative
    u_scale; B = 2 / 4 / 5 (the count is capped at min(B, 4)); T = 9 so that t < B - 1 (the history reaches the action
    buffer) and t >= B - 1 both occur."""
    rng = np.random.default_rng(B * 100 + int(u_max * 10))
    p = clipped_draw(rng, 400, 9, u_max, u_min, u_scale, sigma=2.0 * abs(u_max / u_scale))
    got, want = classify(lib, p, B, u_max, u_min, u_scale), restate(p, B, u_max, u_min, u_scale)
    assert np.array_equal(got, want)
    assert set(np.unique(want[:, :, 0])) == set(range(min(B, 4) + 1))  # every length occurs
    assert want[:, :, 0].max() == min(B, 4)
    # a window at t reaches at most t + 1 perturbed elements
    for t in range(9):
        assert got[:, t, 0].max() <= min(t + 1, B, 4)


def test_crafted_windows(lib):
    """Every length 0 .. 4 with every pattern at B = 4, placed by hand."""
    u_max, u_min, u_scale, B, T = 3.0, -3.0, 3.0, 4, 8
    hi, lo = u_max / u_scale, u_min / u_scale
    rows, want = [], []
    for length in range(5):
        for pattern in range(1 << length):
            row = np.full(T, 0.125)
            t = 5  # consumes perturbed elements 5, 4, 3, 2
            for s in range(length):
                row[t - s] = lo if (pattern >> s) & 1 else hi
            rows.append(row)
            want.append((length, pattern))
    got = classify(lib, np.array(rows), B, u_max, u_min, u_scale)
    assert [tuple(x) for x in got[:, 5]] == want
    assert np.array_equal(got, restate(np.array(rows), B, u_max, u_min, u_scale))
    for length, pattern in want:
        assert lib.nlc_gp_entry_index(length, pattern) == (1 << length) - 1 + pattern
    assert lib.nlc_gp_entries() == 31 and lib.nlc_gp_entry_index(4, 15) == 30


def test_action_buffer_elements_never_count(lib):
    """An all-clipped sample: window t counts its t + 1 perturbed elements and stops at the action buffer, whatever the
    buffer holds (the classification never sees it -- an entry equal to a bound is ordinary data)."""
    for B in (2, 4, 5):
        p = np.full((1, 7), 1.0)
        got = classify(lib, p, B, 3.0, -3.0, 3.0)
        assert list(got[0, :, 0]) == [min(t + 1, B, 4) for t in range(7)]
        assert not got[0, :, 1].any()


def test_signed_zero_and_nan(lib):
    """u_min = 0: the image is +0.0; a stored -0.0 is other data (bit compare), and so is a NaN."""
    p = np.array([[0.0, -0.0, 0.0, 0.0], [0.0, 0.0, np.nan, 0.0], [1.0, 0.0, 1.0, 0.0]])
    got = classify(lib, p, 2, 2.0, 0.0, 2.0)
    assert np.array_equal(got, restate(p, 2, 2.0, 0.0, 2.0))
    assert list(got[0, :, 0]) == [1, 0, 1, 2] and list(got[1, :, 0]) == [1, 2, 0, 1]
    assert list(got[2, :, 0]) == [1, 2, 2, 2] and list(got[2, :, 1]) == [0, 1, 2, 1]


def test_equal_bounds_pattern_zero(lib):
    p = np.full((2, 6), 0.5)
    got = classify(lib, p, 4, 1.0, 1.0, 2.0)
    assert list(got[0, :, 0]) == [1, 2, 3, 4, 4, 4] and not got[:, :, 1].any()


def test_null_action_sample_is_ordinary_data(lib):
    """The sample forced to the null action stores 0 everywhere: no prefix unless 0 is a bound."""
    p = np.zeros((1, 6))
    assert not classify(lib, p, 4, 3.0, -3.0, 3.0)[:, :, 0].any()
    assert classify(lib, p, 4, 3.0, 0.0, 3.0)[0, :, 0].tolist() == [1, 2, 3, 4, 4, 4]


def test_lists_and_scope(lib):
    assert [lib.nlc_gp_n_lists(B) for B in (1, 2, 4, 5, 9)] == [1, 2, 4, 5, 5]
    for N, B in ((336, 4), (32, 4), (768, 5), (655360, 4), (5, 2)):
        # any split of N windows over the lists needs at most this many 16-window tiles
        assert lib.nlc_gp_worst_case_tiles(N, B) >= -(-N // 16) + lib.nlc_gp_n_lists(B) - 1
    assert lib.nlc_gp_in_scope(1, 1, 1, 4, ctypes.c_long(655360), 1)
    assert not lib.nlc_gp_in_scope(2, 2, 1, 4, ctypes.c_long(100), 1)  # acrobot
    assert not lib.nlc_gp_in_scope(1, 2, 1, 4, ctypes.c_long(100), 1)  # encode_obs_time channel
    assert not lib.nlc_gp_in_scope(1, 1, 0, 4, ctypes.c_long(100), 1)  # no bounds
    assert not lib.nlc_gp_in_scope(1, 1, 1, 4, ctypes.c_long(1 << 28), 1)
    assert not lib.nlc_gp_in_scope(1, 1, 1, 4, ctypes.c_long(100), 0)
