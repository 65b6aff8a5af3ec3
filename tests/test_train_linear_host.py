"""CPU: the linear-ILT (fixed Talbot / Stehfest) element math of the fused training step (csrc/nlc_train.h: linear_phase,
linear_row_sum, linear_row_bwd, linear_query_point), built with g++ as tests/test_train_host.py builds the rest, against
torch float64 autograd through oracle.ilt.ilt_from_sphere.

Bounds.  A term is v = R Re(W e^{i theta}), R = tan(phi / 2 + pi / 4).  Its own magnitude is |W| R for the value and for
d v / d theta, and |W| (1 + R^2) / 2 for d v / d phi (the factors the phase multiplies); each is held to 1e-13 of that, times
1 / t where the oracle's 1 / t is in.  A row's line integral is the sum of its S terms, each carrying that bound, so its value is
held to 1e-13 of sum_k |W_k| R_k / t: Stehfest's weights alternate in sign and reach 1e8 at S = 16, so the sum itself can be
orders below its terms, and no float64 evaluation (the oracle's included) resolves it better than an ulp of the terms.  A
row's derivatives are single terms'.  Gradients down to the pre-activations carry the sphere map's pi (theta) or pi / 2 (phi)
on top; its factor 1 - y^2 cancels near saturation, so the bound is on the product's scale (as in test_train_host.py)."""

import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import ilt as oilt

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "helpers", "train_linear_host.cpp")
TOL = 1e-13

# (algorithm, terms) of the issue; every one at t in TS
CASES = [("fixed_tablot", 8), ("fixed_tablot", 17), ("fixed_tablot", 33), ("stehfest", 2), ("stehfest", 8), ("stehfest", 16)]
TS = (0.02, 0.1, 1.0)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("trainlinhost") / "libtrain_linear_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), SRC])
    lib = ctypes.CDLL(str(out))
    vp = ctypes.c_void_p
    lib.nlc_t_linear_rows.argtypes = [vp, vp, vp, vp, ctypes.c_long, ctypes.c_int, vp, vp, vp, vp, vp]
    lib.nlc_t_linear_query.argtypes = [vp, vp, vp, ctypes.c_long, ctypes.c_int, vp, vp]
    return lib


def _ptr(a):
    return a.ctypes.data


def _host_rows(lib, y, t, wr, wi):
    n, _, S = y.shape
    y, t, wr, wi = (np.ascontiguousarray(a, dtype=np.float64) for a in (y, t, wr, wi))
    x, val, dth, dph, dpre = np.empty(n), np.empty((n, S)), np.empty((n, S)), np.empty((n, S)), np.empty((n, 2, S))
    lib.nlc_t_linear_rows(_ptr(y), _ptr(t), _ptr(wr), _ptr(wi), n, S, _ptr(x), _ptr(val), _ptr(dth), _ptr(dph), _ptr(dpre))
    return x, val, dth, dph, dpre


def _oracle_rows(algo, pre, t):
    """The sphere map of the reference (w_nl.py:59-62) and oracle.ilt.ilt_from_sphere under autograd: x (n), the term values,
    d x / d theta, d x / d phi, d x / d pre and the magnitudes the bounds are written in."""
    n, _, S = pre.shape
    pre = pre.clone().requires_grad_()
    y = torch.tanh(pre)
    theta = y[:, 0] * math.pi
    phi = y[:, 1] * math.pi / 2.0 - math.pi / 2.0 + math.pi / 2.0
    theta.retain_grad()
    phi.retain_grad()
    x = oilt.ilt_from_sphere(theta.view(n, 1, S), phi.view(n, 1, S), t, algo).reshape(n)
    x.sum().backward()
    _, _, wr, wi = oilt.linear_tables(algo, S)
    with torch.no_grad():
        fr, fi = oilt.sphere_to_complex(theta, phi)
        val = fr * wr - fi * wi
        R = torch.tan(phi / 2.0 + math.pi / 4.0)
        mag_v = torch.hypot(wr, wi) * R  # value and d / d theta
        mag_p = torch.hypot(wr, wi) * (0.5 * (1.0 + R * R))  # d / d phi
    return (y.detach(), x.detach(), val, theta.grad, phi.grad, pre.grad, mag_v, mag_p, wr, wi)


@pytest.mark.parametrize("t0", TS)
@pytest.mark.parametrize("algo,S", CASES)
def test_linear_term_and_row_vs_autograd(lib, algo, S, t0):
    """Value and both derivatives of every single term, and value and pre-activation gradients of whole rows, at the row time
    t0 (and, in the same call, rows spread around it), to 1e-13 of the term's own magnitude (module docstring)."""
    gen = torch.Generator().manual_seed(1000 * S + int(t0 * 100))
    n = 96
    pre = torch.randn(n, 2, S, dtype=torch.float64, generator=gen)
    t = torch.full((n,), t0, dtype=torch.float64)
    t[n // 2 :] *= 0.5 + torch.rand(n - n // 2, dtype=torch.float64, generator=gen)
    y, x_ref, val_ref, dth_ref, dph_ref, dpre_ref, mag_v, mag_p, wr, wi = _oracle_rows(algo, pre, t)
    x, val, dth, dph, dpre = _host_rows(lib, y.numpy(), t.numpy(), wr.numpy(), wi.numpy())
    inv_t = (1.0 / t).view(n, 1)

    def worst(got, ref, mag):
        return float((torch.as_tensor(got) - ref).abs().div(mag).max())

    figures = {
        "term value": worst(val, val_ref, mag_v),
        "term d/dtheta": worst(dth, dth_ref, mag_v * inv_t),
        "term d/dphi": worst(dph, dph_ref, mag_p * inv_t),
        "row value": worst(x, x_ref, (mag_v * inv_t).sum(-1)),
        "row d/dpre theta": worst(dpre[:, 0], dpre_ref[:, 0], mag_v * inv_t * math.pi),
        "row d/dpre phi": worst(dpre[:, 1], dpre_ref[:, 1], mag_p * inv_t * (math.pi / 2.0)),
    }
    print(algo, S, t0, {k: f"{v:.2e}" for k, v in figures.items()})
    assert np.isfinite(x).all() and np.isfinite(dpre).all()
    for what, err in figures.items():
        assert err <= TOL, f"{algo} S={S} t={t0}: {what} off by {err:.3e} of its magnitude"
    # the check is not vacuous: the derivatives are not all zero, and the row sums are not all cancelled away
    assert float(dpre_ref.abs().max()) > 0 and float(x_ref.abs().max()) > 0


@pytest.mark.parametrize("algo,S", CASES)
def test_linear_query_points_vs_oracle(lib, algo, S):
    """linear_query_point == oracle.ilt.complex_to_sphere of node_k / t: the same float64 expressions in the same order, so the
    two differ by their atan2 / asin only -- 4 ulp of the result (each library's is within 1)."""
    nr, ni, _, _ = oilt.linear_tables(algo, S)
    t = torch.tensor(list(TS) + [0.037, 0.5], dtype=torch.float64)
    th_ref, ph_ref = oilt.complex_to_sphere(nr / t.unsqueeze(-1), ni / t.unsqueeze(-1))
    n = t.numel()
    th, ph = np.empty((n, S)), np.empty((n, S))
    nr_, ni_, t_ = (np.ascontiguousarray(a.numpy()) for a in (nr, ni, t))
    lib.nlc_t_linear_query(_ptr(nr_), _ptr(ni_), _ptr(t_), n, S, _ptr(th), _ptr(ph))
    for got, ref in ((th, th_ref.numpy()), (ph, ph_ref.numpy())):
        assert (np.abs(got - ref) <= 4 * np.spacing(np.abs(ref))).all()


def test_stand_alone_program_agrees_with_the_library_build(tmp_path):
    """The same source with its own main() (-DNLC_T_MAIN: the program a sanitizer build runs, nothing loaded into python)
    builds and runs every entry at S = 1 .. 33."""
    exe = tmp_path / "train_linear_host_main"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-DNLC_T_MAIN", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("ok ") and math.isfinite(float(out.stdout.split()[1]))
