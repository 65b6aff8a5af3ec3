"""CPU: the element math of the synthetic transition dataset (csrc/nlc_synth.h), built with g++, against brute force in
Python integers / numpy restatements of the reference's lines (overlay.py:605-629, 718-731; base_env.py:263-276), and the
declaration / binding of nlc_synth_generate."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
F64P = I64P = ctypes.c_void_p
LL = ctypes.c_longlong


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("synthhost") / "libsynth_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "synth_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.nlc_s_row_index.argtypes = [I64P, ctypes.c_long, LL, LL, I64P]
    lib.nlc_s_row_of.argtypes = [LL, LL, LL, LL, LL]
    lib.nlc_s_row_of.restype = LL
    lib.nlc_s_global_row.argtypes = [LL, LL, LL, LL]
    lib.nlc_s_global_row.restype = LL
    lib.nlc_s_max_rows.restype = LL
    lib.nlc_s_box.argtypes = [F64P, ctypes.c_double, F64P, ctypes.c_long]
    lib.nlc_s_buffer.argtypes = [ctypes.c_int] * 4 + [F64P, F64P, ctypes.c_double, F64P]
    return lib


def _row_index(lib, rows, A, S):
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.empty((len(rows), 3), dtype=np.int64)
    lib.nlc_s_row_index(rows.ctypes.data, len(rows), A, S, out.ctypes.data)
    return out


def test_row_decomposition_over_every_row_of_a_small_case(lib):
    """S = 5, A = 3, TI = 4: the 60 rows against the nested loops of the reference -- blocks concatenated (overlay.py:713),
    actions outer and states inner within a block (base_env.py:263-276) -- and back through row_of."""
    S, A, TI = 5, 3, 4
    want = [(ti, i, j) for ti in range(TI) for i in range(A) for j in range(S)]
    got = _row_index(lib, np.arange(TI * A * S), A, S)
    assert [tuple(x) for x in got.tolist()] == want
    for r, (ti, i, j) in enumerate(want):
        assert lib.nlc_s_row_of(ti, i, j, A, S) == r


def test_row_decomposition_past_2_pow_31(lib):
    """The acrobot default (S = 15^4, A = 15) carried to 2^40 rows: rows 2^31 - 1, 2^31 and 2^39 (and the last row below
    the limit) against Python's integers -- 64-bit arithmetic throughout."""
    S, A = 15**4, 15
    assert lib.nlc_s_max_rows() == 2**40
    rows = [2**31 - 1, 2**31, 2**39, 2**40 - 1]
    got = _row_index(lib, rows, A, S)
    for r, (ti, i, j) in zip(rows, got.tolist()):
        q, jj = divmod(r, S)
        assert (ti, i, j) == (q // A, q % A, jj), r
        assert lib.nlc_s_row_of(ti, i, j, A, S) == r


def test_ti_begin_offsets_the_global_row(lib):
    """Row `local` of a call that starts at block ti_begin is global row ti_begin * A * S + local: block ti_begin + local's
    block, the same (i, j) -- so a call over [7, 30) draws what the full call draws for those rows."""
    S, A = 5, 3
    for ti_begin in (0, 1, 7):
        local = np.arange(2 * A * S)
        glob = np.array([lib.nlc_s_global_row(int(x), ti_begin, A, S) for x in local])
        assert np.array_equal(glob, ti_begin * A * S + local)
        got, base = _row_index(lib, glob, A, S), _row_index(lib, local, A, S)
        assert np.array_equal(got[:, 0], base[:, 0] + ti_begin) and np.array_equal(got[:, 1:], base[:, 1:])
    assert lib.nlc_s_global_row(5, 2**20, 15, 15**4) == 2**20 * 15 * 15**4 + 5  # past 2^31


def _box(lib, u, mx):
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty_like(u)
    lib.nlc_s_box(u.ctypes.data, mx, out.ctypes.data, len(u))
    return out


def test_box_sample_is_symmetric_and_bounded(lib):
    """(2u - 1) * max equals the reference's (rand - 0.5) * 2.0 * max bit for bit (a scaling by two commutes with the
    rounding), is odd about u = 1/2 on the 2^-53 grid (1 - u and 2u - 1 are exact there), and stays inside [-max, max] at
    the constants u = 2^-53 and u = 1 - 2^-53."""
    pi32 = float(np.float32(np.pi))
    rng = np.random.default_rng(0)
    k = rng.integers(1, 2**53, 4000)
    u = np.concatenate([[2.0**-53, 1.0 - 2.0**-53, 0.5], k * 2.0**-53])
    for mx in (5.0, 20.0, 30.0, pi32, 3.0):
        got = _box(lib, u, mx)
        assert np.array_equal(got, (u - 0.5) * 2.0 * mx)
        assert np.array_equal(got, -_box(lib, 1.0 - u, mx))
        assert got.min() >= -mx and got.max() <= mx
        assert -mx <= got[0] < -mx * (1 - 1e-15) and mx * (1 - 1e-15) < got[1] <= mx and got[2] == 0.0


@pytest.mark.parametrize("time_channel", [0, 1])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("B,delay", [(4, 0), (4, 3), (1, 0)])
def test_buffer_fill(lib, B, delay, nu, time_channel):
    """a = (rand(B, nu) - 0.5) * 2 * high; a[-(delay + 1)] = the action (overlay.py:718-720); with the time channel the last
    column is flip(arange(B)) (:722-731).  The row B - 1 - delay holds the action, every other entry is the box sample of
    its uniform and within [-high, high], the time column is B - 1 .. 0."""
    high, W = 3.0, nu + time_channel
    rng = np.random.default_rng(10 * B + delay)
    u = np.ascontiguousarray(rng.random((B, nu)))
    u.flat[0] = 1.0 - 2.0**-53
    act = np.ascontiguousarray([7.0, -9.0][:nu])  # outside the box: recognisable
    out = np.empty((B, W))
    lib.nlc_s_buffer(B, nu, time_channel, delay, act.ctypes.data, u.ctypes.data, high, out.ctypes.data)
    ref = (u - 0.5) * 2.0 * high
    ref[-(delay + 1)] = act
    assert np.array_equal(out[:, :nu], ref)
    assert np.array_equal(out[B - 1 - delay, :nu], act)
    others = np.delete(out[:, :nu], B - 1 - delay, axis=0)
    assert others.size == (B - 1) * nu and (np.abs(others) <= high).all()
    if time_channel:
        assert np.array_equal(out[:, nu], np.arange(B - 1, -1, -1, dtype=np.float64))


def test_streams_are_distinct_small_integers(lib):
    """state (which also takes the next one for components 2, 3), action, interval, fill."""
    assert [lib.nlc_s_stream(i) for i in range(4)] == [0, 2, 3, 4]


# ---------------------------------------------------------------------------------------------------- ABI
def _header():
    return open(os.path.join(REPO, "include", "nlc.h")).read()


def test_header_declares_synth_generate():
    hdr = _header()
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 15
    assert re.search(r"int\s+nlc_synth_generate\s*\(\s*nlc_ctx\s*\*\s*ctx\s*,\s*const\s+nlc_synth_desc\s*\*\s*desc\s*,\s*"
                     r"int64_t\s+ti_begin\s*,\s*int64_t\s+ti_end\s*,", hdr)
    body = re.search(r"typedef struct nlc_synth_desc \{(.*?)\} nlc_synth_desc;", hdr, re.S).group(1)
    for field in ("env", "friction", "dt", "delay", "B", "nu", "time_channel", "ts_grid", "reuse", "S", "A", "action_high",
                  "state_max", "seed"):
        assert re.search(rf"\b{field}\b\s*(\[4\])?\s*[;,]", body), field


def test_lib_binds_synth_generate_and_mirrors_the_desc():
    from neurallaplacecontrol_amd import _lib

    assert "nlc_synth_generate" in _lib.SYMBOLS
    body = re.search(r"typedef struct nlc_synth_desc \{(.*?)\} nlc_synth_desc;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [m.group(1) for m in re.finditer(r"(\w+)\s*(?:\[4\])?\s*[;,]", body)]
    assert [n for n, _ in _lib.SynthDesc._fields_] == declared


def test_synth_desc_size_matches_the_header():
    from neurallaplacecontrol_amd import _lib

    src = '#include <stdio.h>\n#include "nlc.h"\nint main(){ printf("%zu\\n", sizeof(nlc_synth_desc)); return 0; }\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(td, "s"), os.path.join(td, "s.c")])
        size = int(subprocess.check_output([os.path.join(td, "s")]).split()[0])
    assert size == ctypes.sizeof(_lib.SynthDesc)


def test_package_exports_generate_synthetic_dataset():
    import neurallaplacecontrol_amd as nlc

    assert "generate_synthetic_dataset" in nlc.__all__ and callable(nlc.generate_synthetic_dataset)


def test_sizes_and_boxes_are_the_references():
    """samples_per_dim defaults 33 / 20 / 15 (overlay.py:675-681), S = spd^n, A = spd, TI = 10 spd; state_max with the
    reference's float32 pi widened to double (:689-694)."""
    from neurallaplacecontrol_amd import synthetic as syn

    assert syn.synthetic_dataset_shape("oderl-cartpole") == (200, 20, 20**4)
    assert syn.synthetic_dataset_shape("oderl-pendulum") == (330, 33, 33**2)
    assert syn.synthetic_dataset_shape("oderl-acrobot") == (150, 15, 15**4)
    assert syn.synthetic_dataset_shape("oderl-cartpole", 3) == (30, 3, 81)
    pi32 = float(np.float32(np.pi))
    assert pi32 == 3.1415927410125732
    assert syn.STATE_MAX == {"oderl-cartpole": (5.0, 20.0, pi32, 30.0), "oderl-pendulum": (pi32, 5.0),
                             "oderl-acrobot": (pi32, pi32, 5.0, 5.0)}
    with pytest.raises(ValueError):
        syn.synthetic_dataset_shape("oderl-cartpole-notrig")


def test_refusals_that_need_no_device():
    """The out-of-scope modes raise NotImplementedError with the reason, and bad arguments ValueError, before anything
    touches a device (this test runs without one)."""
    import neurallaplacecontrol_amd as nlc
    from neurallaplacecontrol_amd import synthetic as syn

    with pytest.raises(NotImplementedError, match="grid mode"):
        nlc.generate_synthetic_dataset("oderl-cartpole", 0, 3, rand=False)
    with pytest.raises(NotImplementedError, match="observation noise"):
        nlc.generate_synthetic_dataset("oderl-cartpole", 0, 3, observation_noise=0.1)
    with pytest.raises(NotImplementedError, match="double_time"):
        syn.generate_irregular_data_delay_latent("oderl-cartpole", None, 0)
    with pytest.raises(NotImplementedError, match="validation loss"):
        syn.get_val_loss_delay_time_multi(None, "oderl-cartpole", None, 0)
    with pytest.raises(ValueError, match="unknown env"):
        nlc.generate_synthetic_dataset("oderl-hopper", 0, 3)
    with pytest.raises(ValueError, match="delay"):
        nlc.generate_synthetic_dataset("oderl-cartpole", 4, 3, action_buffer_size=4)
    for blocks in ((-1, 5), (0, 31), (5, 5), (7, 3)):
        with pytest.raises(ValueError, match="blocks"):
            nlc.generate_synthetic_dataset("oderl-cartpole", 0, 3, blocks=blocks)
    with pytest.raises(ValueError, match="ts_grid"):
        nlc.generate_synthetic_dataset("oderl-cartpole", 0, 3, ts_grid="poisson")
