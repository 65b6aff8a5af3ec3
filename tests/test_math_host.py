"""CPU: the bounded-range FP64 math used inside the HIP kernels (csrc/nlc_math.h), built with g++,
against numpy/libm (long double where a bound is an ulp or two) on dense grids.  The device build takes other code where it
matters (v_rcp_f64 + refinement for every division, inline-assembly clamps, hipcc's contraction): tests/test_gpu_math_device.py
runs every test of this module again on tools/math_dev_check.hip's build of the same symbols, with the same grids and bounds."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("mathhost") / "libmath_host.so"
    subprocess.check_call(
        ["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), os.path.join(HERE, "helpers", "math_host.cpp")]
    )
    return ctypes.CDLL(str(out))


def call(lib, name, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    f = getattr(lib, name)
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    f.restype = ctypes.c_int
    assert f(x.ctypes.data, y.ctypes.data, x.size) == 0, name
    return y


def ulp_err(y, ref):
    return np.abs(y - ref) / np.spacing(np.abs(ref) + 1e-300)


def test_tanh(lib):
    x = np.concatenate([np.linspace(-40, 40, 400001), np.logspace(-300, 1, 20001), -np.logspace(-12, 1, 2001), [0.0]])
    err = ulp_err(call(lib, "nlc_t_tanh", x), np.tanh(x))
    print(f"tanh_d: max {err.max():.3f} ulp")
    assert err.max() <= 4


def test_tanh_pair_fast(lib):
    """Hidden-layer activation of the rollout kernels (round 3): absolute error <= 1.5e-13 everywhere (degree-9 Horner exp,
    one-constant reduction), exact sign symmetry, 1 within an ulp at saturation, finite for huge arguments."""
    x = np.concatenate([np.linspace(-40, 40, 400001), np.logspace(-300, 3, 20001), -np.logspace(-12, 3, 2001), [0.0, 1e300, -1e300]])
    y = call(lib, "nlc_t_tanh_pair_fast", x)
    print(f"tanh_pair_fast: max abs err {np.abs(y - np.tanh(x)).max():.3e}")
    assert np.abs(y - np.tanh(x)).max() <= 1.5e-13
    assert np.all(np.abs(y) <= 1.0 + 3e-16) and np.all(np.isfinite(y))
    assert np.array_equal(call(lib, "nlc_t_tanh_pair_fast", -x), -y)


def test_sigmoid(lib):
    x = np.concatenate([np.linspace(-800, 800, 400001), np.logspace(-12, 2, 2001)])
    ref = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    y = call(lib, "nlc_t_sigmoid", x)
    ok = np.abs(x) < 700
    print(f"sigmoid_d: max {ulp_err(y[ok], ref[ok]).max():.3f} ulp")
    assert ulp_err(y[ok], ref[ok]).max() <= 4
    assert np.all(np.isfinite(y)) and np.all(y >= 0) and np.all(y <= 1)


def test_exp(lib):
    x = np.linspace(-700, 700, 400001)
    err = ulp_err(call(lib, "nlc_t_exp", x), np.exp(x))
    print(f"exp_d: max {err.max():.3f} ulp")
    assert err.max() <= 2


def test_sincos(lib):
    x = np.concatenate([np.linspace(-2 * np.pi, 2 * np.pi, 800001), np.logspace(-300, 0, 3001)])
    s, c = call(lib, "nlc_t_sin", x), call(lib, "nlc_t_cos", x)
    print(f"sincos_bounded: max abs err sin {np.abs(s - np.sin(x)).max():.3e} cos {np.abs(c - np.cos(x)).max():.3e}")
    # absolute accuracy 1e-16-ish everywhere (near the zeros relative error is limited by the 2-term pi/2)
    assert np.abs(s - np.sin(x)).max() < 2.5e-16
    assert np.abs(c - np.cos(x)).max() < 2.5e-16
    small = np.abs(x) < 0.7
    assert ulp_err(s[small], np.sin(x[small])).max() <= 2


def test_tan(lib):
    x = np.concatenate([np.linspace(0, np.pi / 2, 400001), np.logspace(-300, -1, 2001)])
    y, ref = call(lib, "nlc_t_tan", x), np.tan(x)
    ok = x < 1.5707
    print(f"tan_0_halfpi: max {ulp_err(y[ok], ref[ok]).max():.3f} ulp")
    assert ulp_err(y[ok], ref[ok]).max() <= 4
    assert np.all(np.abs(y[~ok] - ref[~ok]) <= 1e-11 * np.abs(ref[~ok]))


def test_tan_pi4_plus(lib):
    x = np.concatenate([np.linspace(0, np.pi / 2, 400001), np.logspace(-18, -1, 2001)])
    ref = np.tan(x.astype(np.longdouble)).astype(np.float64)  # tan of that very double, 80-bit
    y = call(lib, "nlc_t_tan_pi4", x)
    # (cos a + sin a)/(cos a - sin a) amplifies the 1e-16 absolute rounding of sin/cos near the zero and the pole:
    # absolute error O(1e-16 (1 + tan^2)), the same conditioning tan has w.r.t. a one-ulp change of its argument
    ok = x < 1.57
    print(f"tan_pi4_plus: max err / (1 + tan^2) {np.max(np.abs(y[ok] - ref[ok]) / (1.0 + ref[ok] ** 2)):.3e}")
    assert np.all(np.abs(y[ok] - ref[ok]) <= 4e-16 * (1.0 + ref[ok] ** 2))
    assert np.isfinite(y).all() and y.min() > -3e-16 and y[400000] > 1e15


def test_cos_quadrant(lib):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 700001)
    j0 = (np.arange(x.size) % 7) - 3
    pi_l = np.longdouble("3.14159265358979323846264338327950288")
    ref = np.cos(x.astype(np.longdouble) + j0 * pi_l / 2).astype(np.float64)
    print(f"cos_quadrant: max abs err {np.abs(call(lib, 'nlc_t_cosq', x) - ref).max():.3e}")
    assert np.abs(call(lib, "nlc_t_cosq", x) - ref).max() < 3e-16


def test_table_driven_tanh_sigmoid(lib):
    x = np.concatenate([np.linspace(-40, 40, 400001), np.logspace(-300, 1, 20001), -np.logspace(-12, 1, 2001), [0.0]])
    # the rounded table entry leaves an ABSOLUTE error of ~1e-16 on e^{-2a}-1, so for 0.003 < |x| < 0.03 the
    # result is exact to 2e-16 absolute rather than to a few ulp (it feeds matmuls: same as any rounding of O(1) data)
    y, ref = call(lib, "nlc_t_tanh_t", x), np.tanh(x)
    assert np.all(np.abs(y - ref) <= 2.5e-16 + 4 * np.spacing(np.abs(ref)))
    assert ulp_err(y[np.abs(x) > 0.05], ref[np.abs(x) > 0.05]).max() <= 6
    assert ulp_err(y[np.abs(x) < 0.002], ref[np.abs(x) < 0.002]).max() <= 4
    xs = np.concatenate([np.linspace(-800, 800, 400001), np.logspace(-12, 2, 2001)])
    ref = np.where(xs >= 0, 1 / (1 + np.exp(-np.abs(xs))), np.exp(-np.abs(xs)) / (1 + np.exp(-np.abs(xs))))
    y = call(lib, "nlc_t_sigmoid_t", xs)
    ok = np.abs(xs) < 700
    assert ulp_err(y[ok], ref[ok]).max() <= 4
    assert np.all(np.isfinite(y)) and np.all(y >= 0) and np.all(y <= 1)


def test_ilt_short_forms(lib):
    """The instruction-count-trimmed trig of the stand-alone Fourier ILT kernel: absolute accuracy ~2e-16 for the
    cosine (one reduction by pi, quarter-turn parity in the reduction), tan as num/den within a few ulp away from the
    pole and tracking the conditioning of the argument's own rounding next to it."""
    x = np.concatenate([np.linspace(-7.0, 7.0, 800001), np.linspace(-1e3, 1e3, 20001), [0.0, np.pi, -np.pi]])
    mm = (np.arange(x.size) & 1).astype(np.float64)
    y = call(lib, "nlc_t_cos_mpio2", x)
    xl = x.astype(np.longdouble)
    ref = np.where(mm == 0, np.cos(xl), -np.sin(xl))  # cos(x + pi/2) = -sin(x)
    bound = 3e-16 + 1.2e-16 * np.abs(x) / np.pi  # 2-term pi/2: the reduction error grows with the quotient
    print(f"cos_plus_mpio2: max err / bound {np.max(np.abs(y - ref.astype(np.float64)) / bound):.3f}")
    assert np.all(np.abs(y - ref.astype(np.float64)) <= bound)
    ys = call(lib, "nlc_t_sin_mpio2", x)
    ref_s = np.where(mm == 0, np.sin(xl), np.cos(xl))  # sin(x + pi/2) = cos(x)
    assert np.all(np.abs(ys - ref_s.astype(np.float64)) <= bound)
    xt = np.linspace(0.0, np.pi / 2, 400001)[:-1]
    t = call(lib, "nlc_t_tan_short", xt)
    ref_t = np.tan(xt)
    # relative error bounded by a few ulp plus the pole's conditioning: d tan / tan = dx (1 + tan^2)/tan
    cond = (1 + ref_t ** 2) / np.maximum(ref_t, 1e-300) * 2.3e-16
    print(f"tan_parts_short: max err / bound {np.max(np.abs(t - ref_t) / ((6e-16 + cond) * np.maximum(np.abs(ref_t), 1.0))):.3f}")
    assert np.all(np.abs(t - ref_t) <= (6e-16 + cond) * np.maximum(np.abs(ref_t), 1.0))


def test_ilt_row_forms(lib):
    """Round 6, the row-per-lane Fourier ILT kernel: tan(pi/4 + a) = num/den from the Cephes rational (|a| <= pi/4) within a few
    ulp away from the pole and tracking the argument's own conditioning next to it; cos(x + m pi/2) by one reduction by pi with
    the cosine (m = 0) or sine (m = 1) polynomial: absolute accuracy ~2e-16."""
    a = np.linspace(-np.pi / 4, np.pi / 4, 400001)[1:-1]
    t = call(lib, "nlc_t_tan_rat", a)
    al = a.astype(np.longdouble)
    ref = np.tan(al + np.longdouble(np.pi) / 4 + np.longdouble(6.123233995736766e-17) / 2).astype(np.float64)  # (pi/4 to ~1e-33)
    cond = (1 + ref ** 2) / np.maximum(ref, 1e-300) * 1.2e-16  # the rounding of a itself
    print(f"tan_parts_rat: max err / bound {np.max(np.abs(t - ref) / ((6e-16 + cond) * np.maximum(np.abs(ref), 1.0))):.3f}")
    assert np.all(np.abs(t - ref) <= (6e-16 + cond) * np.maximum(np.abs(ref), 1.0))
    x = np.concatenate([np.linspace(-7.0, 7.0, 800001), np.linspace(-1e3, 1e3, 20001), [0.0, np.pi, -np.pi]])
    mm = (np.arange(x.size) & 1).astype(np.float64)
    y = call(lib, "nlc_t_cos_kpio2", x)
    xl = x.astype(np.longdouble)
    want = np.where(mm == 0, np.cos(xl), -np.sin(xl)).astype(np.float64)
    bound = 3e-16 + 1.2e-16 * np.abs(x) / np.pi
    print(f"cos_or_sin_reduced: max err / bound {np.max(np.abs(y - want) / bound):.3f}")
    assert np.all(np.abs(y - want) <= bound)


def test_sincos_reduced(lib):
    """Backward of the row-per-lane Fourier ILT kernel: sin x and cos x from ONE reduction by pi, absolute accuracy ~2e-16."""
    x = np.ascontiguousarray(np.concatenate([np.linspace(-7.0, 7.0, 400001), np.linspace(-1e3, 1e3, 20001), [0.0, np.pi, -np.pi]]))
    sn, cs = np.empty_like(x), np.empty_like(x)
    f = lib.nlc_t_sincos_reduced
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    f.restype = ctypes.c_int
    assert f(x.ctypes.data, sn.ctypes.data, cs.ctypes.data, x.size) == 0
    xl = x.astype(np.longdouble)
    bound = 3e-16 + 1.2e-16 * np.abs(x) / np.pi
    print(f"sincos_reduced: max err / bound {max(np.max(np.abs(sn - np.sin(xl).astype(np.float64)) / bound), np.max(np.abs(cs - np.cos(xl).astype(np.float64)) / bound)):.3f}")
    assert np.all(np.abs(sn - np.sin(xl).astype(np.float64)) <= bound)
    assert np.all(np.abs(cs - np.cos(xl).astype(np.float64)) <= bound)


# ---- the functions every other one is built from, and the edges the grids above do not reach.  References are long double (64-bit
# mantissa: its own error is 2^-11 of a float64 ulp), errors are measured in ulps of the binade the exact result lies in.
LD = np.longdouble


def call2(lib, name, a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape
    y = np.full_like(a, np.nan)
    f = getattr(lib, name)
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    f.restype = ctypes.c_int
    assert f(a.ctypes.data, b.ctypes.data, y.ctypes.data, a.size) == 0, name
    return y


def ulp_err_ld(y, ref):
    """|y - ref| in float64 ulps of ref's binade (subnormal spacing below 2^-1022); ref: long double."""
    ref = np.asarray(ref, dtype=LD)
    _, e = np.frexp(np.abs(ref))
    ulp = np.ldexp(LD(1.0), np.maximum(e - 53, -1074))
    return (np.abs(y.astype(LD) - ref) / ulp).astype(np.float64)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def test_long_double_reference_is_wider_than_float64():
    assert np.finfo(np.longdouble).nmant >= 63


DEN_MIN = 8.659560562354934e-17  # the sphere map's clamped denominator (tan_parts_0_halfpi, IltTrigK::den_min)


def rcp_grid():
    rng = np.random.default_rng(11)
    unit = 1.0 + np.arange(2 ** 20) / 2.0 ** 20  # [1, 2): the denominators 1 + e, 2 + em
    pair = np.concatenate([np.linspace(0.8, 2.4, 100001), rng.uniform(0.8, 2.4, 100000)])  # D + M of tanh_pair_fast / tanh2
    four = np.prod(rng.uniform(0.8, 2.4, (4, 100000)), axis=0)
    # the four denominators D + M of sigmoid_pair2, M = e^y with y clamped at 170: products up to e^680
    gate = np.prod(rng.uniform(0.8, 1.2, (4, 100000)) + np.exp(rng.uniform(-40.0, 170.0, (4, 100000))), axis=0)
    top = np.array([(1.2 + np.exp(170.0)) ** 4, np.exp(170.0) ** 4, np.exp(680.0)])
    log = np.exp2(np.linspace(-500.0, 500.0, 100001))
    return np.concatenate([unit, pair, four, gate, top, log, -log, [DEN_MIN, -DEN_MIN, 1.0, 2.0, 0.5]])


def check_rcp(lib, name):
    d = rcp_grid()
    err = ulp_err_ld(call(lib, name, d), 1 / d.astype(LD))
    print(f"{name}: max {err.max():.3f} ulp at d = {d[np.argmax(err)]!r}")
    assert err.max() <= 1.0


def test_rcp_refined(lib):
    """1 / d within 1 ulp (the header's claim for v_rcp_f64 + one cubic step; a division on the host) wherever a kernel takes
    it: [1, 2), [0.8, 2.4], products of four denominators up to e^680, 2^-500 .. 2^500 of both signs, the sphere map's den_min."""
    check_rcp(lib, "nlc_t_rcp_refined")


def test_div_fast(lib):
    """n / d within 1 ulp for |n|, |d| in [2^-250, 2^250], both signs (reciprocal, product, one residual-correction step)."""
    rng = np.random.default_rng(12)
    e = np.linspace(-250.0, 250.0, 1001)
    gn, gd = np.meshgrid(np.exp2(e[::4]), np.exp2(e[1::4]))
    n = np.concatenate([gn.ravel(), np.exp2(rng.uniform(-250, 250, 300000)) * rng.choice([-1.0, 1.0], 300000)])
    d = np.concatenate([gd.ravel(), np.exp2(rng.uniform(-250, 250, 300000)) * rng.choice([-1.0, 1.0], 300000)])
    err = ulp_err_ld(call2(lib, "nlc_t_div_fast", n, d), n.astype(LD) / d.astype(LD))
    print(f"div_fast: max {err.max():.3f} ulp at {n[np.argmax(err)]!r} / {d[np.argmax(err)]!r}")
    assert err.max() <= 1.0


def clamp_inputs():
    big = np.logspace(-323, 308, 6001)  # subnormals included
    return np.concatenate([np.linspace(-1000, 1000, 200001), big, -big,
                           [0.0, -0.0, np.inf, -np.inf, 372.5, -372.5, np.nextafter(372.5, 0), np.nextafter(372.5, 1e3),
                            -np.nextafter(372.5, 0), -np.nextafter(372.5, 1e3), 170.0, -170.0, np.nextafter(170.0, 0), np.nextafter(170.0, 1e3),
                            -np.nextafter(170.0, 0), -np.nextafter(170.0, 1e3), np.finfo(np.float64).max, -np.finfo(np.float64).max,
                            np.finfo(np.float64).tiny, 5e-324, -5e-324]])


def test_min_abs_clamp(lib):
    """min_abs(x, 372.5) (tanh's clamp: a bare v_min_f64 with the |.| modifier on the device): the bits of min(|x|, 372.5) for finite
    x, subnormals included, +-0 and +-inf."""
    x = clamp_inputs()
    assert same_bits(call(lib, "nlc_t_min_abs", x), np.minimum(np.abs(x), 372.5))


TANH_PAIR_PARTNERS = (0.0, 1e-300, 0.5, 19.0, 400.0)


def test_tanh_pair_d(lib):
    """The NL rollout's hidden activation, two values on one reciprocal: <= 5 ulp (tanh_d's 4 plus the two extra products) with
    every partner -- tiny, ordinary, saturating, beyond the clamp -- so the shared reciprocal does not couple the two errors; exactly
    odd; |t| <= 1 + 1 ulp up to |x| = 1e300."""
    x = np.concatenate([np.linspace(-40, 40, 100001), np.logspace(-300, 1, 10001), -np.logspace(-12, 1, 1001), np.logspace(1, 300, 2001),
                        -np.logspace(1, 300, 2001), [0.0, 1e300, -1e300]])
    worst = 0.0
    for partner in TANH_PAIR_PARTNERS:
        for sign in (1.0, -1.0):
            xp = np.empty(2 * x.size)
            xp[0::2], xp[1::2] = x, sign * partner
            for arg in (xp, xp.reshape(-1, 2)[:, ::-1].ravel()):  # the partner as the second and as the first of the pair
                y = call(lib, "nlc_t_tanh_pair_d", arg)
                err = ulp_err_ld(y, np.tanh(arg.astype(LD)))
                worst = max(worst, err.max())
                assert err.max() <= 5, (partner, arg[np.argmax(err)], err.max())
                assert np.all(np.abs(y) <= 1.0 + 2.3e-16)
                assert np.array_equal(call(lib, "nlc_t_tanh_pair_d", -arg), -y)
    print(f"tanh_pair_d: max {worst:.3f} ulp")


_LN2 = np.log(2.0)


def exp_neg_inputs():
    k = np.arange(-1075, 0) + 0.5
    edges = np.concatenate([k * _LN2, np.nextafter(k * _LN2, np.inf), np.nextafter(k * _LN2, -np.inf)])
    return np.concatenate([np.linspace(-745, 0, 200001), np.linspace(-1, 0, 100001), edges[edges >= -745.0], -np.logspace(-300, 0, 3001),
                           [-1e-300, 0.0, -745.0]])


def test_exp_neg(lib):
    """e^y for y <= 0: <= 2 ulp (exp_d's bound) down to e^-708; below, where the result is subnormal, within two subnormal
    spacings; past the clamp at -745 the smallest subnormal."""
    y = exp_neg_inputs()
    got, ref = call(lib, "nlc_t_exp_neg", y), np.exp(y.astype(LD))
    err = ulp_err_ld(got, ref)
    print(f"exp_neg: max {err[y >= -708].max():.3f} ulp on [-708, 0], {err[y < -708].max():.3f} subnormal spacings below")
    assert err[y >= -708].max() <= 2
    assert err[y < -708].max() <= 2  # (ulp_err_ld counts subnormal spacings there)
    assert same_bits(call(lib, "nlc_t_exp_neg", np.array([-746.0, -1000.0, -1e300])), np.full(3, 5e-324))


def test_expm1_neg(lib):
    """e^y - 1 for y <= 0, the numerator and denominator of tanh_d: <= 3 ulp on [-745, 0], dense on [-1, 0], at every reduction
    boundary (k + 1/2) ln2 and its neighbours, and down to -1e-300."""
    y = exp_neg_inputs()
    err = ulp_err_ld(call(lib, "nlc_t_expm1_neg", y), np.expm1(y.astype(LD)))
    print(f"expm1_neg: max {err.max():.3f} ulp at y = {y[np.argmax(err)]!r}")
    assert err.max() <= 3


def saturated_inputs():
    return np.concatenate([np.linspace(19.1, 100.0, 50001), np.logspace(np.log10(19.1), 300, 50001), [1e300, np.inf]])


def test_tanh_saturates_exactly(lib):
    """tanh_d has no saturation branch: from 19.1 on (e^{-2x} < 2^-54) the quotient must round to EXACTLY 1 -- the sphere map's
    clamped |F| depends on phi = pi/2 to the bit (csrc/nlc_rollout.h: sphere_phi)."""
    x = saturated_inputs()
    assert same_bits(call(lib, "nlc_t_tanh", x), np.ones_like(x))
    assert same_bits(call(lib, "nlc_t_tanh", -x), -np.ones_like(x))


@pytest.mark.parametrize("name", ["nlc_t_tanh", "nlc_t_tanh_pair_d", "nlc_t_tanh_pair_fast", "nlc_t_sin"])
def test_odd_functions_keep_the_sign_of_zero(lib, name):
    """f(-0.0) = -0.0 and f(+0.0) = +0.0, whatever the other value of a pair is.

    (sincos_bounded's reduction and polynomial each add a +0 to a -0 argument, so it hands a zero argument back itself.)"""
    x = np.array([-0.0, 0.0, 0.0, -0.0, -0.0, -0.0, 0.0, 0.0, -0.0, 0.5, 0.5, -0.0, 0.0, -19.0, 400.0, -0.0])
    y = call(lib, name, x)
    zero = x == 0.0
    assert np.all(y[zero] == 0.0) and np.array_equal(np.signbit(y[zero]), np.signbit(x[zero])), y


def test_tan_parts_short_at_the_saturated_argument(lib):
    """tan_parts_short at the double nearest pi/2 (the sphere map's argument for a saturated phi): the reference's clamped
    |F| = 1.633123935319537e16 within 4 ulp.  (test_ilt_short_forms stops short of the pole, where its conditioning term would let
    any radius through.)"""
    got = call(lib, "nlc_t_tan_short", np.array([np.pi / 2]))
    assert abs(got[0] - 1.633123935319537e16) <= 4 * np.spacing(1.633123935319537e16), got
