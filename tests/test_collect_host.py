"""CPU: the element math of the expert-data collector's control step (csrc/nlc_collect.h), built with g++, against numpy /
torch restatements of the reference's lines (mppi_dataset_collector.py:20-24, 206-208, 250-254; base_env.py:103-120), and the
declaration / binding of nlc_collect_step."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
F64P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("collecthost") / "libcollect_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "collect_host.cpp")])
    return ctypes.CDLL(str(out))


def _u(n, seed):
    """Uniforms in (0, 1) with the extremes of the 53-bit draw: (0 + 1/2) 2^-53 and 1 - 2^-53."""
    u = np.random.default_rng(seed).random(n)
    u[0], u[1], u[2] = 0.5 * 2.0**-53, 1.0 - 2.0**-53, 0.5
    return np.ascontiguousarray(u)


def _interval(lib, grid, dt, u):
    out = np.empty_like(u)
    lib.nlc_c_interval.argtypes = [ctypes.c_int, ctypes.c_double, F64P, F64P, ctypes.c_long]
    lib.nlc_c_interval(grid, dt, u.ctypes.data, out.ctypes.data, len(u))
    return out


def test_interval_transforms_vs_numpy(lib):
    """fixed: dt exactly.  uniform: 2 dt u exactly (a product by a power of two times dt: one rounding on both sides).
    exp: -dt log(u) to 2 ulp (libm's and numpy's log each within 1 ulp, then one product), finite and > 0 at the extremes
    of the draw, and the largest possible interval is -dt log(2^-54) = 37.4 dt."""
    dt = 0.05
    u = _u(4000, 0)
    assert np.array_equal(_interval(lib, 0, dt, u), np.full_like(u, dt))
    assert np.array_equal(_interval(lib, 1, dt, u), 2 * dt * u)
    got, ref = _interval(lib, 2, dt, u), -dt * np.log(u)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    assert (np.abs(got - ref) / np.spacing(ref)).max() <= 2
    assert got[0] == got.max() and abs(got[0] - dt * 54 * np.log(2.0)) < 1e-12


def test_action_noise_and_clip(lib):
    """action + ((rand - 0.5) * 2 * high) * scale, clipped to [low, high] (:250-254) against the same expression in torch
    (float64): bit-equal inside, at and beyond the bounds; a negative scale (None) returns the action untouched, even
    outside the bounds; the random policy is low + (high - low) u and stays inside [low, high]."""
    low, high = -3.0, 3.0
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.uniform(-3, 3, 500), [3.0, -3.0, 3.0, -3.0, 0.0, 2.9, -2.9, 7.0, -7.0]])
    u = np.concatenate([rng.random(500), [1 - 2.0**-53, 0.5 * 2.0**-53, 0.5 * 2.0**-53, 1 - 2.0**-53, 0.5, 0.99, 0.01, 0.5, 0.5]])
    rows = np.ascontiguousarray(np.stack([a, u], axis=1))
    f = lib.nlc_c_noisy_action
    f.argtypes = [F64P, ctypes.c_double, ctypes.c_double, ctypes.c_double, F64P, ctypes.c_long]
    for scale in (1.0, 0.01):
        out = np.empty(len(a))
        f(rows.ctypes.data, low, high, scale, out.ctypes.data, len(a))
        ta, tu = torch.from_numpy(a), torch.from_numpy(u)
        ref = (ta + ((tu - 0.5) * 2.0 * high) * scale).clip(min=low, max=high).numpy()
        assert np.array_equal(out, ref), scale
        assert out.max() <= high and out.min() >= low
    assert out[-2] == high and out[-1] == low  # beyond the bounds: clipped
    out = np.empty(len(a))
    f(rows.ctypes.data, low, high, -1.0, out.ctypes.data, len(a))
    assert np.array_equal(out, a)
    g = lib.nlc_c_random_action
    g.argtypes = [F64P, ctypes.c_double, ctypes.c_double, F64P, ctypes.c_long]
    uu = _u(1000, 2)
    out = np.empty(len(uu))
    g(uu.ctypes.data, low, high, out.ctypes.data, len(uu))
    assert np.array_equal(out, low + (high - low) * uu) and out.min() >= low and out.max() <= high


@pytest.mark.parametrize("B,nu", [(4, 1), (4, 2), (1, 1)])
def test_time_channel_recurrence_vs_reference_lines(lib, B, nu):
    """Six control steps of the time column against the reference's three lines restated in torch: torch.roll(-1) with
    buffer[-1, nu:] = 0 (:20-24), then buffer[:, nu:] += tsn; buffer[-1, nu:] = 0 (:206-208), from the initial column
    flip(arange(B)) * dt (:232-233).  Bit-equal; the action columns are not touched."""
    dt, W, steps = 0.05, nu + 1, 6
    ts = -dt * np.log(_u(steps, 3)[::-1].copy())
    buf = torch.zeros(B, W, dtype=torch.float64)
    buf[:, :nu] = torch.arange(B * nu, dtype=torch.float64).view(B, nu) + 1.0
    buf[:, nu:] = (torch.flip(torch.arange(B), (0,)) * dt).view(-1, 1)
    mine = np.ascontiguousarray(buf.numpy().copy())
    out = np.empty((steps, B, W))
    f = lib.nlc_c_time_channel
    f.argtypes = [F64P, ctypes.c_int, ctypes.c_int, ctypes.c_int, F64P, ctypes.c_int, F64P]
    f(mine.ctypes.data, B, W, nu, np.ascontiguousarray(ts).ctypes.data, steps, out.ctypes.data)
    actions = buf[:, :nu].clone()
    for s in range(steps):
        rolled = torch.roll(buf, -1, dims=0)
        rolled[-1, nu:] = 0
        rolled[:, :nu] = actions  # (the action columns are the env-step body's: held fixed here)
        rolled[:, nu:] += ts[s]
        rolled[-1, nu:] = 0
        buf = rolled
        assert np.array_equal(out[s], buf.numpy()), s


def test_row_index_corners(lib):
    f = lib.nlc_c_row_index
    f.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    f.restype = ctypes.c_longlong
    assert f(0, 0, 200, 0) == 0
    assert f(0, 0, 200, 199) == 199
    assert f(0, 1, 200, 0) == 200
    assert f(4, 3, 5, 2) == 37
    assert f(4999, 0, 200, 199) == 10**6 - 1
    # past 2^31 rows: 64-bit arithmetic
    assert f(2**31, 255, 200, 7) == (2**31 + 255) * 200 + 7


def test_streams_are_distinct_small_integers(lib):
    """interval, action noise, observation noise (which also takes the next one for states 2, 3) and random policy."""
    s = [lib.nlc_c_stream(i) for i in range(4)]
    assert s == [0, 1, 2, 4]


def test_header_declares_abi_13_and_collect_step():
    hdr = open(os.path.join(REPO, "include", "nlc.h")).read()
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 13
    assert re.search(r"int\s+nlc_collect_step\s*\(\s*nlc_ctx\s*\*\s*ctx\s*,\s*const\s+nlc_collect_desc\s*\*", hdr)
    body = re.search(r"typedef struct nlc_collect_desc \{(.*?)\} nlc_collect_desc;", hdr, re.S).group(1)
    for field in ("env", "friction", "dt", "delay", "E", "B", "nu", "time_channel", "ts_grid", "policy", "action_noise",
                  "obs_noise", "action_low", "action_high", "steps_per_episode", "seed"):
        assert re.search(rf"\b{field}\b\s*[;,]", body), field


def test_lib_binds_collect_step():
    from neurallaplacecontrol_amd import _lib

    assert "nlc_collect_step" in _lib.SYMBOLS
    hdr = open(os.path.join(REPO, "include", "nlc.h")).read()
    body = re.search(r"typedef struct nlc_collect_desc \{(.*?)\} nlc_collect_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [m.group(1) for m in re.finditer(r"(\w+)\s*[;,]", body)]
    assert [n for n, _ in _lib.CollectDesc._fields_] == declared
    for g, v in (("fixed", "FIXED"), ("uniform", "UNIFORM"), ("exp", "EXP")):
        assert _lib.TS_GRIDS[g] == int(re.search(rf"#define\s+NLC_TS_GRID_{v}\s+(\d+)", hdr).group(1))
    for g, v in (("planner", "PLANNER"), ("random", "RANDOM")):
        assert _lib.POLICIES[g] == int(re.search(rf"#define\s+NLC_POLICY_{v}\s+(\d+)", hdr).group(1))


def test_replay_buffer_file_name_is_the_references():
    from neurallaplacecontrol_amd.collector import replay_buffer_file_name

    assert replay_buffer_file_name("oderl-cartpole", 2) == (
        "replay_buffer_env-name-oderl-cartpole_delay-2_model-name-oracle_encode-obs-time-False_action-buffer-size-4_"
        "ts-grid-exp_random-action-noise-1.0_observation-noise-0.0_friction-False.pt")
