"""CPU: the rational exponential of csrc/nlc_math.h (exp_ratio_parts: e^y = 2^n num / den) and the sigmoid / tanh forms the
GRU gates and the rollout's hidden layers build on it, built with g++, against mpmath (or numpy's long double where mpmath is
missing) over dense and adversarial arguments.

Bounds: e^y relative 1.5e-14 (the minimax ratio's own 1.11e-14, tools/exp_ratio_remez.py, plus the rounding of num and den),
plus |n| 2.4e-17 for y = n ln2 + r (the reduction's one ln2 constant is off by 2.3e-17: 1.4e-15 at |y| = 40, where the gates
stop resolving anything).
A relative error eps of e^{-x} moves sigmoid(x) by at most eps / 4 and tanh by at most eps / 2, so sigmoid and tanh are held
to 5e-15 and 8e-15 absolute.

tests/test_gpu_math_device.py runs every test of this module again on the device build of the same symbols
(tools/math_dev_check.hip), where the gate forms are the shipped sigmoid_pair2 / tanh2 of csrc/nlc_gru_tile.h themselves."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

try:
    import mpmath

    mpmath.mp.dps = 40
except ImportError:  # pragma: no cover
    mpmath = None


def _exp_ref(y):
    """e^y for a float64 array, as float64 pairs (hi, lo) with hi + lo exact to ~1e-30 relative."""
    if mpmath is not None:
        hi = np.empty_like(y)
        lo = np.empty_like(y)
        for i, v in enumerate(y):
            e = mpmath.exp(mpmath.mpf(float(v)))
            hi[i] = float(e)
            lo[i] = float(e - mpmath.mpf(hi[i]))
        return hi, lo
    e = np.exp(y.astype(np.longdouble))
    hi = e.astype(np.float64)
    return hi, (e - hi).astype(np.float64)


def _exp_rel_err(m, d, y):
    hi, lo = _exp_ref(y)
    # (m / d) / e^y - 1 = (m - d e^y) / (d e^y), the numerator with one rounding in long double
    num = m.astype(np.longdouble) - d.astype(np.longdouble) * (hi.astype(np.longdouble) + lo.astype(np.longdouble))
    return np.abs((num / (d.astype(np.longdouble) * hi.astype(np.longdouble))).astype(np.float64))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("expratio") / "libexp_ratio_host.so"
    subprocess.check_call(
        ["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), os.path.join(HERE, "helpers", "exp_ratio_host.cpp")]
    )
    return ctypes.CDLL(str(out))


def exp_ratio(lib, y, half=False):
    y = np.ascontiguousarray(y, dtype=np.float64)
    m = np.empty_like(y)
    d = np.empty_like(y)
    f = lib.nlc_t_exp_ratio
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int]
    f.restype = ctypes.c_int
    # (the device build also runs the two-wide instantiation and returns non-zero unless it agrees with the scalar one bit for bit)
    assert f(y.ctypes.data, m.ctypes.data, d.ctypes.data, y.size, int(half)) == 0
    return m, d


def call(lib, name, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.full_like(x, np.nan)
    f = getattr(lib, name)
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    f.restype = ctypes.c_int
    assert f(x.ctypes.data, y.ctypes.data, x.size) == 0, name
    return y


def _sigmoid_ref(x):
    hi, lo = _exp_ref(-np.abs(x))
    e = hi.astype(np.longdouble) + lo.astype(np.longdouble)
    s = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
    return s.astype(np.float64)


def _tanh_ref(x):
    if mpmath is not None:
        return np.array([float(mpmath.tanh(mpmath.mpf(float(v)))) for v in x])
    return np.tanh(x.astype(np.longdouble)).astype(np.float64)


# the reduction's rounding boundaries (y = (k + 1/2) ln2: |r| at its largest) and both sides of each
_LN2 = np.log(2.0)
_EDGES = np.concatenate([(np.arange(-1075, 246) + 0.5) * _LN2, np.nextafter((np.arange(-1075, 246) + 0.5) * _LN2, np.inf)])


@pytest.mark.parametrize("half", [False, True])
def test_exp_ratio_relative_error(lib, half):
    """Dense over the sigmoid gate's range (y <= 170) and tanh's (y = -2|x| >= -745), plus every reduction boundary."""
    rng = np.random.default_rng(7)
    y = np.concatenate([np.linspace(-708, 170, 60001), rng.uniform(-1, 1, 20001), _EDGES[(_EDGES > -708) & (_EDGES < 170)], [0.0]])
    if half:
        y = y[y <= 0]
    m, d = exp_ratio(lib, y, half)
    assert np.all(np.isfinite(m)) and np.all(d > 0.8) and np.all(d < 1.2)
    err = _exp_rel_err(m, d, y)
    bound = 1.5e-14 + np.abs(np.round(y / _LN2)) * 2.4e-17
    print(f"exp_ratio_parts half={half}: max rel err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (err.max(), y[np.argmax(err - bound)])
    assert err[np.abs(y) <= 0.5 * _LN2].max() <= 1.3e-14


def test_exp_ratio_half_is_the_same_value(lib):
    """exp_ratio_parts<true> on y / 2 returns exactly what exp_ratio_parts<false> does on y (coefficients scaled by 2^k)."""
    y = np.concatenate([np.linspace(-745, 0, 100001), -_EDGES[_EDGES > 0]])
    m0, d0 = exp_ratio(lib, y, False)
    m1, d1 = exp_ratio(lib, y, True)
    assert np.array_equal(m0, m1) and np.array_equal(d0, d1)


def test_exp_ratio_denormal_and_flushed_results(lib):
    """Below e^-708 the scaled numerator becomes subnormal (absolute error within its spacing), and 0 below e^-745."""
    y = np.concatenate([np.linspace(-745.1, -708, 20001), _EDGES[(_EDGES > -745.1) & (_EDGES < -708)]])
    m, d = exp_ratio(lib, y)
    hi, _ = _exp_ref(y)
    tiny = np.finfo(np.float64).smallest_subnormal
    assert np.all(np.abs(m / d - hi) <= 4e-14 * hi + 2 * tiny)
    m, d = exp_ratio(lib, np.array([-746.0, -800.0, -1000.0, -1e4]))
    assert np.all(m == 0.0) and np.all(d > 0)


def test_sigmoid_gate_form(lib):
    """sigmoid_pair2's arithmetic: dense, the tails past +-40 and +-745, the clamp at 170 and +-1e9 (the reduction's integer
    is exact while |x| log2(e) < 2^31, far beyond any gate pre-activation)."""
    x = np.concatenate([np.linspace(-60, 60, 120001), np.linspace(-800, 800, 16001), np.logspace(-300, 2, 4001), -np.logspace(-300, 2, 4001),
                        [169.9, 170.0, 170.1, -169.9, -170.0, -170.1, 745.0, -745.0, 746.0, -746.0, 1e9, -1e9, 0.0, -0.0, 40.0, -40.0]])
    x = np.concatenate([x, np.zeros((-x.size) % 4)])
    y = call(lib, "nlc_t_sigmoid_ratio", x)
    ref = _sigmoid_ref(x)
    assert np.all(np.isfinite(y)) and np.all(y >= 0) and np.all(y <= 1.0 + 2.3e-16)
    print(f"sigmoid gate form: max abs err {np.abs(y - ref).max():.3e}")
    assert np.abs(y - ref).max() <= 5e-15
    far = x < -170  # clamped: ~1e-74 instead of the true value, never 0 (the product of four denominators stays finite)
    assert np.all((y[far] > 0) & (y[far] < 1e-73))
    assert np.all(np.abs(y[x > 40] - 1.0) <= 2.3e-16)


def test_sigmoid_gate_form_nonfinite(lib):
    """-inf and NaN hit the clamp (the encoder marks a non-finite window's latents NaN itself: nan_if_bad_window)."""
    y = call(lib, "nlc_t_sigmoid_ratio", np.array([-np.inf, np.nan, 0.0, 1.0]))
    assert 0 < y[0] < 1e-73 and 0 < y[1] < 1e-73 and abs(y[2] - 0.5) <= 1.2e-16


def test_tanh_gate_form(lib):
    """tanh_pair_fast / tanh2: dense, tiny, the tails past +-40 and +-372.5 (the clamp), +-inf, NaN; exactly odd."""
    x = np.concatenate([np.linspace(-40, 40, 160001), np.logspace(-300, 3, 4001), -np.logspace(-300, 3, 4001),
                        [372.5, -372.5, np.nextafter(372.5, 0), 745.0, -745.0, 1e300, -1e300, 0.0, -0.0]])
    x = np.concatenate([x, np.zeros(x.size % 2)])
    y = call(lib, "nlc_t_tanh_ratio", x)
    print(f"tanh gate form: max abs err {np.abs(y - _tanh_ref(x)).max():.3e}")
    assert np.abs(y - _tanh_ref(x)).max() <= 8e-15
    assert np.all(np.abs(y) <= 1.0 + 2.3e-16)
    assert np.array_equal(call(lib, "nlc_t_tanh_ratio", -x), -y)
    y = call(lib, "nlc_t_tanh_ratio", np.array([np.inf, -np.inf, np.nan, -np.nan]))
    assert np.all(np.abs(np.abs(y) - 1.0) <= 2.3e-16)


def test_tanh_gate_form_keeps_the_sign_of_zero(lib):
    """tanh_pair_fast / tanh2: -0.0 for -0.0 and +0.0 for +0.0, whatever the other value of the pair is (the comparisons above use
    ==, which does not see the sign of a zero)."""
    x = np.array([-0.0, 0.0, 0.0, -0.0, -0.0, -0.0, 0.0, 0.0, -0.0, 0.5, 0.5, -0.0, 0.0, -19.0, 400.0, -0.0])
    y = call(lib, "nlc_t_tanh_ratio", x)
    zero = x == 0.0
    assert np.all(y[zero] == 0.0) and np.array_equal(np.signbit(y[zero]), np.signbit(x[zero])), y
