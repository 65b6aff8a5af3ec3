"""GPU tests (``-m gpu``): the kernel math AS THE DEVICE BUILD COMPUTES IT.  tools/math_dev_check.hip wraps every inline function of
csrc/nlc_math.h, and the device-only forms of nlc_gru_tile.h, nlc_rollout.h and nlc_cplx.h, in one-thread-per-element kernels
compiled with the library's flags (tools/libnlc_math_dev.so, built by `make -C neurallaplacecontrol_amd/csrc tools`).

Every test of tests/test_math_host.py and tests/test_exp_ratio_host.py is collected here again against that library -- the same
grids, the same references (libm / long double / mpmath), the same bounds: one statement of each, two builds.  Where the host
build is a division and the device build v_rcp_f64 + refinement, inline assembly, the two-wide instantiation or the shipped
sigmoid_pair2 / tanh2 instead of their transcription, this is the test that sees it.  Below them: the functions that exist on the
device only.  Every comparison is done on the CPU; a test is a copy, a launch and a copy."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_exp_ratio_host as _exp_host
import test_math_host as _math_host
from test_math_host import LD, call, check_rcp, clamp_inputs, same_bits, saturated_inputs

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53

# the host modules' tests, collected again here: their `lib` is this module's fixture
for _mod in (_math_host, _exp_host):
    for _name, _fn in list(vars(_mod).items()):
        if _name.startswith("test_") and callable(_fn):
            assert _name not in globals(), f"{_name} is defined twice"
            globals()[_name] = _fn


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(REPO, "tools", "libnlc_math_dev.so")
    csrc = os.path.join(REPO, "neurallaplacecontrol_amd", "csrc")
    # what the library is compiled from: a library older than any of it would test yesterday's math
    srcs = [os.path.join(REPO, "tools", f) for f in ("math_dev_check.hip", "nlc_math_table.h", "nlc_exp_table.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", csrc, "-shared",
                               os.path.join(REPO, "tools", "math_dev_check.hip"), "-o", so])
    return ctypes.CDLL(so)


def test_rcp_refined1(lib):
    """The GRU tile's own copy of the refined reciprocal (nlc_gru_tile.h): the grid and the 1 ulp of rcp_refined."""
    check_rcp(lib, "nlc_t_rcp_refined1")


def test_min_neg_clamp(lib):
    """min_neg(x, 170) (the sigmoid gates' clamp: a bare v_min_f64 with the negate modifier): the bits of min(-x, 170) for finite x,
    subnormals included, +-0 and +-inf."""
    x = clamp_inputs()
    assert same_bits(call(lib, "nlc_t_min_neg", x), np.minimum(-x, 170.0))


def test_saturated_phi_is_exactly_half_pi(lib):
    """From 19.1 on tanh_d is exactly 1, sphere_phi exactly the double pi/2, and the tangent's argument the float64 phi/2 + pi/4
    -- the argument at which the clamped denominator reproduces the reference's saturated |F|."""
    x = saturated_inputs()
    phi = call(lib, "nlc_t_sphere_phi", x)
    assert same_bits(phi, np.full_like(x, np.pi / 2))
    assert same_bits(call(lib, "nlc_t_sphere_tan_arg", phi), phi / 2 + np.pi / 4)


def test_sphere_angles_are_the_reference_op_sequence(lib):
    """sphere_theta / sphere_phi / sphere_tan_arg: every product and sum a separate float64 operation (`fp contract(off)`), applied
    to the device's own tanh_d -- t pi, t pi / 2 - pi / 2 + pi / 2, phi / 2 + pi / 4 in numpy give the same bits."""
    y = np.concatenate([np.linspace(-25, 25, 400001), np.logspace(-300, 1.4, 20001), -np.logspace(-300, 1.4, 20001), [0.0, -0.0]])
    t = call(lib, "nlc_t_tanh", y)
    assert same_bits(call(lib, "nlc_t_sphere_theta", y), t * np.pi)
    phi = t * np.pi / 2 - np.pi / 2 + np.pi / 2
    assert same_bits(call(lib, "nlc_t_sphere_phi", y), phi)
    assert same_bits(call(lib, "nlc_t_sphere_tan_arg", phi), phi / 2 + np.pi / 4)


RAD_SAT = 1.633123935319537e16  # tan of the double nearest pi/2: the reference's saturated |F|


def _sphere_grid():
    theta = np.concatenate([np.linspace(-np.pi, np.pi, 601), [0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2]])
    phi = np.concatenate([np.linspace(-np.pi / 2 * 0.999999, np.pi / 2, 601), np.pi / 2 - np.logspace(-15, 0, 61), [np.pi / 2, 0.0]])
    th, ph = np.meshgrid(theta, phi)
    return th.ravel(), ph.ravel()


def _sphere_ref(theta, phi):
    """tan(phi/2 + pi/4) in long double AT the float64 argument, its bound as tests/test_math_host.py::test_ilt_short_forms states
    it, and cos / sin(theta) in long double."""
    a = phi / 2 + np.pi / 4
    t = np.tan(a.astype(LD))
    # (the argument's own conditioning: d tan / tan = dx (1 + tan^2) / tan for one rounding of x)
    cond = ((1 + t ** 2) / np.maximum(t, LD(1e-300)) * 2.3e-16).astype(np.float64)
    t_bound = (6e-16 + cond) * np.maximum(np.abs(t.astype(np.float64)), 1.0)
    return t, t_bound, np.cos(theta.astype(LD)), np.sin(theta.astype(LD))


def _sphere_bound(t, t_bound, trig):
    """|radius trig| error: the tangent's bound times |trig|, plus the radius times the 3e-16 absolute error of the short-form
    cosine on [-pi, pi] (the issue's "times |trig| + 3e-16": the second term scales with the radius, as an absolute error of a
    factor does)."""
    return t_bound * np.abs(trig).astype(np.float64) + 3e-16 * np.abs(t).astype(np.float64)


@pytest.mark.parametrize("odd", [0, 1])
def test_sphere_term(lib, odd):
    """|F| cos(theta) (even terms) / |F| sin(theta) (odd terms) of the Fourier path: (num trig) rcp_refined(den)."""
    theta, phi = _sphere_grid()
    f = lib.nlc_t_sphere_term
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int]
    f.restype = ctypes.c_int
    got = np.full_like(theta, np.nan)
    assert f(theta.ctypes.data, phi.ctypes.data, got.ctypes.data, theta.size, odd) == 0
    t, t_bound, cs, sn = _sphere_ref(theta, phi)
    trig = sn if odd else cs
    err = np.abs(got.astype(LD) - t * trig).astype(np.float64)
    bound = _sphere_bound(t, t_bound, trig)
    print(f"sphere_term odd={odd}: max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (theta[np.argmax(err / bound)], phi[np.argmax(err / bound)], np.max(err / bound))


def test_sphere_terms_lin(lib):
    """Both components of F = R e^{i theta} (fixed Talbot / Stehfest instances)."""
    theta, phi = _sphere_grid()
    f = lib.nlc_t_sphere_terms_lin
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_long]
    f.restype = ctypes.c_int
    rc, rs = np.full_like(theta, np.nan), np.full_like(theta, np.nan)
    assert f(theta.ctypes.data, phi.ctypes.data, rc.ctypes.data, rs.ctypes.data, theta.size) == 0
    t, t_bound, cs, sn = _sphere_ref(theta, phi)
    for got, trig, what in ((rc, cs, "cos"), (rs, sn, "sin")):
        err = np.abs(got.astype(LD) - t * trig).astype(np.float64)
        bound = _sphere_bound(t, t_bound, trig)
        print(f"sphere_terms_lin {what}: max err / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound), (what, theta[np.argmax(err / bound)], phi[np.argmax(err / bound)], np.max(err / bound))


@pytest.mark.parametrize("form", ["sphere_term", "sphere_terms_lin"])
def test_saturated_radius_is_the_reference_clamp(lib, form):
    """At phi = pi/2 exactly (a saturated tanh) the radius must be the reference's clamped |F| = tan(double nearest pi/2) =
    1.633123935319537e16 within 4 ulp.  The polynomials' own cos a - sin a is 2^-52 there (their absolute error is ~2e-16), above
    den_min = 8.66e-17, so the clamp engages only because tan_parts_short recognises the saturated argument itself; without that
    the radius is 6.37e15."""
    theta, phi = np.zeros(2), np.full(2, np.pi / 2)
    got = np.full(2, np.nan)
    if form == "sphere_term":
        f = lib.nlc_t_sphere_term
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int]
        f.restype = ctypes.c_int
        assert f(theta.ctypes.data, phi.ctypes.data, got.ctypes.data, 2, 0) == 0
    else:
        f = lib.nlc_t_sphere_terms_lin
        f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_long]
        f.restype = ctypes.c_int
        rs = np.full(2, np.nan)
        assert f(theta.ctypes.data, phi.ctypes.data, got.ctypes.data, rs.ctypes.data, 2) == 0
    print(f"{form}: radius at phi = pi/2: {got[0]!r}")
    assert np.all(np.abs(got - RAD_SAT) <= 4 * np.spacing(RAD_SAT)), got


def _gru_call(lib, ar, az, ain, ahn, hold):
    arrs = [np.ascontiguousarray(v, dtype=np.float64) for v in (ar, az, ain, ahn, hold)]
    h = np.full_like(arrs[0], np.nan)
    f = lib.nlc_t_gru_gates
    f.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_long]
    f.restype = ctypes.c_int
    assert f(*[v.ctypes.data for v in arrs], h.ctypes.data, h.size) == 0
    return h


def _gru_check(lib, ar, az, ain, ahn, hold, what):
    h = _gru_call(lib, ar, az, ain, ahn, hold)
    assert np.all(np.isfinite(h)), what

    def sig(x):
        e = np.exp(-np.abs(x.astype(LD)))
        return np.where(x >= 0, 1 / (1 + e), e / (1 + e))

    n = np.tanh(ain.astype(LD) + sig(ar) * ahn.astype(LD))
    ref = (hold.astype(LD) - n) * sig(az) + n
    # a sigmoid is good to 5e-15, the tanh to 8e-15 (tests/test_exp_ratio_host.py): r's error reaches n through ahn (|tanh'| <= 1),
    # z's error h' through hold - n, and the last FMA rounds a value of at most 1
    bound = 5e-15 * (np.abs(ahn) + np.abs(hold.astype(LD) - n).astype(np.float64)) + 8e-15 + 2.3e-16
    err = np.abs(h.astype(LD) - ref).astype(np.float64)
    print(f"gru_gates {what}: max err / bound {np.max(err / bound):.3f}, max err {err.max():.2e}")
    assert np.all(err <= bound), (what, np.max(err / bound))


@pytest.mark.parametrize("scale", [8.0, 60.0, 800.0])
def test_gru_gates(lib, scale):
    """The shipped gru_gates (sigmoid_pair2 on r and z, tanh2 on the candidate, the convex combination as one FMA) on random
    pre-activations against n = tanh(in + sigmoid(r) hn), h' = (h - n) sigmoid(z) + n in long double; ragged length (the last
    group of four hidden units is padded)."""
    rng = np.random.default_rng(int(scale))
    N = 200003
    ar, az, ain, ahn = (rng.uniform(-scale, scale, N) for _ in range(4))
    _gru_check(lib, ar, az, ain, ahn, rng.uniform(-1, 1, N), f"+-{scale:g}")


def test_gru_gates_at_the_sigmoid_clamp(lib):
    """Every combination of the four sigmoid arguments that share one reciprocal (r and z of a pair of hidden units) from the clamp's
    neighbourhood and far beyond it: the product of four denominators (up to e^680) stays finite, no NaN, the same bound."""
    import itertools

    vals = (-1000.0, -170.1, -169.9, 0.0, 170.0, 1000.0)
    combos = np.array(list(itertools.product(vals, repeat=4)))  # (r0, z0, r1, z1) of the pair
    rng = np.random.default_rng(5)
    ar, az = combos[:, [0, 2]].ravel(), combos[:, [1, 3]].ravel()
    for scale in (8.0, 800.0):
        ain, ahn = rng.uniform(-scale, scale, ar.size), rng.uniform(-scale, scale, ar.size)
        _gru_check(lib, ar, az, ain, ahn, rng.uniform(-1, 1, ar.size), f"clamp combos, +-{scale:g}")


def _cplx_operands(seed, n):
    rng = np.random.default_rng(seed)
    mod = 10.0 ** rng.uniform(-100, 100, n)
    arg = rng.uniform(-np.pi, np.pi, n)
    return mod * np.cos(arg) + 1j * mod * np.sin(arg)


def _cplx_call(lib, name, *ops):
    ops = [np.ascontiguousarray(o, dtype=np.complex128) for o in ops]
    y = np.full_like(ops[0], np.nan + 1j * np.nan)
    f = getattr(lib, name)
    f.argtypes = [ctypes.c_void_p] * (len(ops) + 1) + [ctypes.c_long]
    f.restype = ctypes.c_int
    assert f(*[o.ctypes.data for o in ops], y.ctypes.data, y.size) == 0, name
    return y


def _cancelling_pairs(seed, n, sign):
    """(a, b) with a.re b.re = sign * a.im b.im to 1e-8 relative: one component of the product (sign +1) or of the quotient
    (sign -1) cancels to 1e-8 of its terms."""
    rng = np.random.default_rng(seed)
    a = _cplx_operands(seed + 1, n)
    b_re = 10.0 ** rng.uniform(-50, 50, n) * rng.choice([-1.0, 1.0], n)
    b_im = sign * a.real * b_re / a.imag * (1 + 1e-8 * rng.uniform(-1, 1, n))
    return a, b_re + 1j * b_im


def _norm_err(got, ref):
    """|got - ref| / |ref| in units of eps = 2^-53; ref: complex long double."""
    return (np.abs(got.astype(np.clongdouble) - ref) / np.abs(ref)).astype(np.float64) / EPS


def test_cmul(lib):
    """Norm-wise 3 eps: each component is one fused sum of a rounded and an exact product."""
    a = np.concatenate([_cplx_operands(1, 200000), *(_cancelling_pairs(3 + s, 50000, sg)[0] for s, sg in ((0, 1), (10, -1)))])
    b = np.concatenate([_cplx_operands(2, 200000), *(_cancelling_pairs(3 + s, 50000, sg)[1] for s, sg in ((0, 1), (10, -1)))])
    err = _norm_err(_cplx_call(lib, "nlc_t_cmul", a, b), a.astype(np.clongdouble) * b.astype(np.clongdouble))
    print(f"cmul: max {err.max():.3f} eps")
    assert err.max() <= 3


def test_cdiv(lib):
    """Norm-wise 6 eps: two fused sums (1.5 eps sqrt 2), the refined reciprocal of a fused sum of squares (2 eps), one product."""
    a = np.concatenate([_cplx_operands(4, 200000), *(_cancelling_pairs(6 + s, 50000, sg)[0] for s, sg in ((0, 1), (10, -1)))])
    b = np.concatenate([_cplx_operands(5, 200000), *(_cancelling_pairs(6 + s, 50000, sg)[1] for s, sg in ((0, 1), (10, -1)))])
    err = _norm_err(_cplx_call(lib, "nlc_t_cdiv", a, b), a.astype(np.clongdouble) / b.astype(np.clongdouble))
    print(f"cdiv: max {err.max():.3f} eps")
    assert err.max() <= 6


def test_csqrt(lib):
    """Norm-wise 4 eps; the principal branch and the sign of the imaginary part as numpy.sqrt on complex128 has them: z = 0, both
    sides of the negative real axis (im = +-0.0, +-1e-300), purely imaginary z."""
    z = _cplx_operands(8, 300000)
    err = _norm_err(_cplx_call(lib, "nlc_t_csqrt", z), np.sqrt(z.astype(np.clongdouble)))
    print(f"csqrt: max {err.max():.3f} eps")
    assert err.max() <= 4
    mod = 10.0 ** np.linspace(-100, 100, 401)

    def rows(re, im):  # (set the parts one by one: arithmetic on complex scalars loses the sign of a zero)
        out = np.empty(mod.size, dtype=np.complex128)
        out.real, out.imag = re, im
        return out

    zeros = np.empty(4, dtype=np.complex128)  # every signed zero: +0 +0i, -0 +0i, +0 -0i, -0 -0i
    zeros.real, zeros.imag = [0.0, -0.0, 0.0, -0.0], [0.0, 0.0, -0.0, -0.0]
    edge = np.concatenate([zeros, rows(-mod, 0.0), rows(-mod, -0.0), rows(-mod, 1e-300), rows(-mod, -1e-300), rows(0.0, mod),
                           rows(0.0, -mod), rows(mod, 0.0), rows(mod, 1e-300), rows(mod, -1e-300)])
    got, want = _cplx_call(lib, "nlc_t_csqrt", edge), np.sqrt(edge)
    assert np.array_equal(np.signbit(got.real), np.signbit(want.real)) and np.array_equal(np.signbit(got.imag), np.signbit(want.imag))
    assert np.all(got.real >= 0)
    nz = edge != 0
    assert _norm_err(got[nz], np.sqrt(edge[nz].astype(np.clongdouble))).max() <= 4
    assert np.all(got[:4] == 0)
