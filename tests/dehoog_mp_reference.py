"""60-digit reference of the de Hoog, Knight & Stokes inverse Laplace transform and of its gradient, for the tests of the
de Hoog HIP kernels (tests/test_dehoog_mp_host.py validates it on the CPU, tests/test_gpu_ilt_dehoog_mp.py holds the kernels to it).

Written from mpmath 1.3.0 calculus/inverselaplace.py (deHoog.calc_laplace_parameter / calc_time_domain_solution): the
quotient-difference table filled column by column with the rhombus rules, the continued-fraction coefficients d, the A / B
recurrence and the improved remainder -- in mpmath's own arbitrary-precision numbers at 60 digits.  Nothing here is derived
from the kernels or from oracle/ilt.py; the host test pins it to the installed mpmath's deHoog class.

The gradient comes from a small generic reverse-mode tape over complex values (+, -, *, /, sqrt and a real-part read-out):
plain automatic differentiation of the same forward, not a hand-derived adjoint of the table.

Also here, because both test modules need them on the same inputs: the fixed inputs per term count, the rows whose gradient
is checked, the float64 CPU roundings the kernels are measured against, and the margins (derived in the host test's
docstring from the CPU roundings alone).
"""

import functools
import math

import mpmath as mp
import numpy as np
import torch

DPS = 60
TERM_COUNTS = tuple(range(3, 34, 2))
N_POINTS, N_DIMS = 67, 3  # 201 rows: three full 64-row blocks and a ragged block of 9
# flat rows whose gradient is compared with the tape: every block edge and the whole ragged block
GRAD_ROWS = tuple(list(range(0, 8)) + list(range(60, 72)) + list(range(124, 132)) + list(range(188, 201)))

# margins of a kernel's error quantiles over the larger of the two CPU roundings' (tests/test_dehoog_mp_host.py: 3 x the worst
# ratio between the two CPU roundings' q50 / q90, 6 x the worst ratio between their maxima, rounded to a power of two)
FWD_MARGIN_Q, FWD_MARGIN_MAX = 4.0, 32.0
GRAD_MARGIN_Q50, GRAD_MARGIN_MAX = 8.0, 64.0


def at_dps(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)

    return run


def _terms(theta, phi):
    """F_k = tan(phi_k / 2 + pi / 4) e^{i theta_k} (the sphere map's inverse), theta / phi float64 taken exactly."""
    return [mp.tan(mp.mpf(p) / 2 + mp.pi / 4) * mp.expj(mp.mpf(th)) for th, p in zip(theta, phi)]


def _abscissa(t, alpha, tol, scale):
    t = mp.mpf(t)
    T = scale * t
    gamma = mp.mpf(alpha) - mp.log(mp.mpf(tol)) / (scale * T)
    return t, T, gamma


def _continued_fraction(fp, z, sqrt, one, zero):
    """A_2M+1 / B_2M+1 of the 2M + 1 terms fp (fp[0] NOT yet halved) at z = e^{i pi t / T}.  Works on any number type that has
    + - * / (mpc, or the tape's nodes); `sqrt`, `one`, `zero` are that type's square root and constants."""
    S = len(fp)
    M = (S - 1) // 2
    a = [fp[0] / 2] + list(fp[1:])
    # column 1 of the table: q_1^(i) = a_(i+1) / a_i; e_0 = 0
    q = [a[i + 1] / a[i] for i in range(2 * M)]
    e = [zero] * S
    d = [a[0], -q[0]]
    for r in range(1, M + 1):
        mr = 2 * (M - r) + 1
        e = [q[i + 1] - q[i] + e[i + 1] for i in range(mr)]  # e_r^(i) = q_r^(i+1) - q_r^(i) + e_(r-1)^(i+1)
        d.append(-e[0])
        if r != M:
            q = [q[i + 1] * e[i + 1] / e[i] for i in range(mr - 1)]  # q_(r+1)^(i) = q_r^(i+1) e_r^(i+1) / e_r^(i)
            d.append(-q[0])
    A_prev, A_cur, B_prev, B_cur = zero, d[0], one, one
    for i in range(1, 2 * M):
        A_prev, A_cur = A_cur, A_cur + d[i] * A_prev * z
        B_prev, B_cur = B_cur, B_cur + d[i] * B_prev * z
    brem = (one + (d[2 * M - 1] - d[2 * M]) * z) / 2
    rem = brem * (sqrt(one + d[2 * M] * z / brem) - one)
    return (A_cur + rem * A_prev) / (B_cur + rem * B_prev)


@at_dps
def dehoog_mp(theta, phi, t, alpha, tol, scale):
    """x(t) of one row: theta, phi sequences of S = 2M + 1 floats, t a float.  Returns an mpf."""
    t, T, gamma = _abscissa(t, alpha, tol, scale)
    z = mp.expjpi(t / T)
    res = _continued_fraction(_terms(theta, phi), z, mp.sqrt, mp.mpc(1), mp.mpc(0))
    return mp.exp(gamma * t) / T * res.real


class _Node:
    """One value of the reverse-mode tape.  Adjoint convention: wbar = dL/dRe w + i dL/dIm w, so a holomorphic w = f(u) sends
    ubar += conj(f'(u)) wbar."""

    __slots__ = ("v", "bar", "args", "tape")

    def __init__(self, tape, v, args=()):
        self.v, self.bar, self.args, self.tape = v, mp.mpc(0), args, tape
        tape.append(self)

    @staticmethod
    def _val(x):
        return x.v if isinstance(x, _Node) else x

    def _make(self, v, *pairs):  # pairs: (operand, dw/d operand); constants carry no adjoint
        return _Node(self.tape, v, tuple((u, p) for u, p in pairs if isinstance(u, _Node)))

    def __add__(self, o):
        return self._make(self.v + self._val(o), (self, 1), (o, 1))

    __radd__ = __add__

    def __sub__(self, o):
        return self._make(self.v - self._val(o), (self, 1), (o, -1))

    def __rsub__(self, o):
        return self._make(self._val(o) - self.v, (self, -1))

    def __neg__(self):
        return self._make(-self.v, (self, -1))

    def __mul__(self, o):
        ov = self._val(o)
        return self._make(self.v * ov, (self, ov), (o, self.v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        ov = self._val(o)
        w = self.v / ov
        return self._make(w, (self, 1 / ov), (o, -w / ov))

    def __rtruediv__(self, o):
        w = self._val(o) / self.v
        return self._make(w, (self, -w / self.v))

    def sqrt(self):
        w = mp.sqrt(self.v)
        return self._make(w, (self, 1 / (2 * w)))


def _backward_from_real_part(tape, out):
    """L = Re out: adjoints of every node of the tape."""
    out.bar = mp.mpc(1)
    for n in reversed(tape):
        if n.bar != 0:
            for u, p in n.args:
                u.bar += mp.conj(p) * n.bar


@at_dps
def dehoog_mp_grad(theta, phi, t, alpha, tol, scale):
    """(x, dx/dtheta[S], dx/dphi[S]) of one row, mpf each, through the tape."""
    t, T, gamma = _abscissa(t, alpha, tol, scale)
    z = mp.expjpi(t / T)
    tape = []
    F = _terms(theta, phi)
    leaves = [_Node(tape, f) for f in F]
    res = _continued_fraction(leaves, z, _Node.sqrt, mp.mpc(1), mp.mpc(0))
    _backward_from_real_part(tape, res)
    c = mp.exp(gamma * t) / T
    # F = r(phi) e^{i theta}, r = tan(phi / 2 + pi / 4): dF/dtheta = i F, dF/dphi = r' e^{i theta} with r' = (1 + r^2) / 2;
    # for a real parameter p, dL/dp = Re(conj(dF/dp) Fbar)
    gth, gph = [], []
    for th, p, f, leaf in zip(theta, phi, F, leaves):
        r = mp.tan(mp.mpf(p) / 2 + mp.pi / 4)
        gth.append(c * (mp.conj(1j * f) * leaf.bar).real)
        gph.append(c * (mp.conj((1 + r * r) / 2 * mp.expj(mp.mpf(th))) * leaf.bar).real)
    return c * res.v.real, gth, gph


# ---- the fixed inputs, the float64 CPU roundings and the error measures shared by the host and the GPU test


def options():
    from oracle import ilt as oilt

    return oilt.ilt_options("dehoog")


def make_inputs(S):
    """t (N,), theta, phi (N, d, S), w (N, d): the fixed inputs of term count S."""
    g = torch.Generator().manual_seed(300 + S)
    t = torch.rand(N_POINTS, dtype=torch.float64, generator=g) * 2 + 0.05
    theta = (torch.rand(N_POINTS, N_DIMS, S, dtype=torch.float64, generator=g) * 2 - 1) * 3.0
    phi = (torch.rand(N_POINTS, N_DIMS, S, dtype=torch.float64, generator=g) * 2 - 1) * 1.2
    w = torch.randn(N_POINTS, N_DIMS, dtype=torch.float64, generator=g)
    return t, theta, phi, w


def mp_forward(theta, phi, t):
    """dehoog_mp of every (point, dim) row with the default options: a flat list of mpf."""
    alpha, tol, scale = options()
    d, S = theta.shape[1], theta.shape[2]
    th, ph = theta.reshape(-1, S).tolist(), phi.reshape(-1, S).tolist()
    return [dehoog_mp(th[i], ph[i], float(t[i // d]), alpha, tol, scale) for i in range(len(th))]


def mp_gradient(theta, phi, t, rows):
    """dehoog_mp_grad of the given flat rows: {row: (gtheta[S], gphi[S])} of mpf lists."""
    alpha, tol, scale = options()
    d, S = theta.shape[1], theta.shape[2]
    th, ph = theta.reshape(-1, S), phi.reshape(-1, S)
    return {i: dehoog_mp_grad(th[i].tolist(), ph[i].tolist(), float(t[i // d]), alpha, tol, scale)[1:] for i in rows}


@at_dps
def forward_errors(x, x_mp):
    """|x - x_mp| / (1 + |x_mp|) per flat row; x a float64 tensor (taken exactly), x_mp the list of mpf."""
    x = x.reshape(-1).tolist()
    assert len(x) == len(x_mp)
    return np.array([float(abs(mp.mpf(v) - r) / (1 + abs(r))) for v, r in zip(x, x_mp)])


@at_dps
def gradient_errors(gtheta, gphi, g_mp, w=None):
    """Per checked row: max_k |g_k - w g_mp_k| / max_k |w g_mp_k| over the row's 2S gradient entries.  gtheta, gphi (N, d, S)
    float64 tensors, g_mp from mp_gradient, w (N, d) the weights of the rows (1 if None)."""
    S = gtheta.shape[-1]
    gt, gp = gtheta.reshape(-1, S), gphi.reshape(-1, S)
    out = []
    for i, (mt, mph) in sorted(g_mp.items()):
        wi = mp.mpf(1) if w is None else mp.mpf(float(w.reshape(-1)[i]))
        ref = [wi * v for v in list(mt) + list(mph)]
        got = gt[i].tolist() + gp[i].tolist()
        sc = max(abs(v) for v in ref)
        out.append(float(max(abs(mp.mpf(a) - b) for a, b in zip(got, ref)) / sc))
    return np.array(out)


def _line_integrate(theta, phi, t, fn):
    from oracle import ilt as oilt

    alpha, tol, scale = options()
    T = scale * t
    gamma = alpha - math.log(tol) / (scale * T)
    fr, fi = oilt.sphere_to_complex(theta, phi)
    return fn(fr, fi, t.unsqueeze(-1), T.unsqueeze(-1), gamma.unsqueeze(-1))


def dehoog_line_integrate_real_pairs(f_real, f_imag, t, T, gamma):
    """gpu_common.dehoog_line_integrate_functional with every complex division carried out on (re, im) pairs of real tensors
    the way oracle.ilt._cdiv does: a second differentiable float64 rounding of the same recurrences."""
    from oracle import ilt as oilt

    def cdiv(a, b):
        return torch.complex(*oilt._cdiv(a.real, a.imag, b.real, b.imag))

    S = f_real.shape[-1]
    M = (S - 1) // 2
    fp = torch.complex(f_real, f_imag)
    t, T, gamma = (v.squeeze(-1) if torch.is_tensor(v) and v.dim() == fp.dim() else v for v in (t, T, gamma))
    a = [fp[..., 0] / 2.0] + [fp[..., i] for i in range(1, S)]
    q = [cdiv(a[i + 1], a[i]) for i in range(2 * M)]
    e = [torch.zeros_like(a[0]) for _ in range(S)]
    dco = [a[0], -q[0]]
    for rr in range(1, M + 1):
        mr = 2 * (M - rr) + 1
        e = [q[i + 1] - q[i] + e[i + 1] for i in range(mr)]
        dco.append(-e[0])
        if rr != M:
            q = [cdiv(q[i + 1] * e[i + 1], e[i]) for i in range(mr - 1)]
            dco.append(-q[0])
    ang = math.pi * (t / T)
    z = torch.complex(torch.cos(ang), torch.sin(ang))
    A_prev, A_cur = torch.zeros_like(dco[0]), dco[0]
    B_prev, B_cur = torch.ones_like(dco[0]), torch.ones_like(dco[0])
    for i in range(1, 2 * M):
        A_prev, A_cur = A_cur, A_cur + dco[i] * A_prev * z
        B_prev, B_cur = B_cur, B_cur + dco[i] * B_prev * z
    brem = (1.0 + (dco[2 * M - 1] - dco[2 * M]) * z) / 2.0
    rem = brem * (torch.sqrt(1.0 + cdiv(dco[2 * M] * z, brem)) - 1.0)
    res = cdiv(A_cur + rem * A_prev, B_cur + rem * B_prev)
    return torch.exp(gamma * t) / T * res.real


def cpu_forward_roundings(theta, phi, t):
    """The two float64 CPU roundings of the forward: the oracle's in-place table and the functional twin.  (N, d) each."""
    from gpu_common import dehoog_line_integrate_functional
    from oracle import ilt as oilt

    with torch.no_grad():
        return (_line_integrate(theta, phi, t, oilt.dehoog_line_integrate),
                _line_integrate(theta, phi, t, dehoog_line_integrate_functional))


def cpu_gradient_roundings(theta, phi, t):
    """The two float64 CPU roundings of d sum(x) / d(theta, phi) (every row's own gradient, weight 1): autograd through the
    functional twin and through its real-pair-division form.  ((gtheta, gphi), (gtheta, gphi))."""
    from gpu_common import dehoog_line_integrate_functional

    out = []
    for fn in (dehoog_line_integrate_functional, dehoog_line_integrate_real_pairs):
        th, ph = theta.clone().requires_grad_(), phi.clone().requires_grad_()
        out.append(torch.autograd.grad(_line_integrate(th, ph, t, fn).sum(), (th, ph)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_case(S):
    """Everything the tests need of term count S that does not involve the GPU, computed once per process: the inputs, the
    mp forward of all 201 rows, the mp gradient of GRAD_ROWS, and the CPU roundings' error quantiles."""
    t, theta, phi, w = make_inputs(S)
    x_mp = mp_forward(theta, phi, t)
    g_mp = mp_gradient(theta, phi, t, GRAD_ROWS)
    fwd_err = [forward_errors(x, x_mp) for x in cpu_forward_roundings(theta, phi, t)]
    grad_err = [gradient_errors(gt, gp, g_mp) for gt, gp in cpu_gradient_roundings(theta, phi, t)]
    return dict(S=S, t=t, theta=theta, phi=phi, w=w, x_mp=x_mp, g_mp=g_mp,
                fwd_err=fwd_err, fwd_q=[np.quantile(e, [0.5, 0.9, 1.0]) for e in fwd_err],
                grad_err=grad_err, grad_q=[np.quantile(e, [0.5, 1.0]) for e in grad_err])
