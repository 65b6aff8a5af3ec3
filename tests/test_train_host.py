"""CPU: the element math of the fused training step (csrc/nlc_train.h), built with g++, against torch on the CPU:
GRU-cell backward (autograd through torch.nn.GRUCell), sphere-map backward (autograd through the reference's expression),
clip_grad_norm_'s coefficient and torch.optim.Adam's element update (weight decay included)."""

import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("trainhost") / "libtrain_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "train_host.cpp")])
    return ctypes.CDLL(str(out))


def _call(lib, name, x, ncols_out):
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.shape[0]
    y = np.empty((n, ncols_out), dtype=np.float64)
    f = getattr(lib, name)
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    f(x.ctypes.data, y.ctypes.data, n)
    return y


def _ulp(y, ref):
    return np.abs(y - ref) / np.spacing(np.abs(ref) + 1e-300)


def test_gru_cell_backward_vs_autograd(lib):
    """Given the gates torch.nn.GRUCell computes, the gate / hidden gradients equal autograd's through the cell (a 1-unit
    cell, so every product is one element).  Bound: 1e-15 relative to the gradient's scale (autograd's own chain of the
    same products; the two sides round differently in the last bits)."""
    torch.manual_seed(0)
    n = 4000
    x = torch.randn(n, 1, dtype=torch.float64)
    h = torch.randn(n, 1, dtype=torch.float64) * 0.8
    dh = torch.randn(n, 1, dtype=torch.float64)
    Wi = torch.randn(n, 3, dtype=torch.float64)
    Wh = torch.randn(n, 3, dtype=torch.float64)
    bi = torch.randn(n, 3, dtype=torch.float64)
    bh = torch.randn(n, 3, dtype=torch.float64)
    gi = (Wi * x + bi).requires_grad_()  # input-side pre-activations [r z n] per row
    gh = (Wh * h + bh).requires_grad_()
    hp = h.clone().requires_grad_()
    r = torch.sigmoid(gi[:, 0] + gh[:, 0])
    z = torch.sigmoid(gi[:, 1] + gh[:, 1])
    nn_ = torch.tanh(gi[:, 2] + r * gh[:, 2])
    hnew = (1.0 - z) * nn_ + z * hp[:, 0]
    hnew.backward(dh[:, 0])
    inp = torch.stack([dh[:, 0], r.detach(), z.detach(), nn_.detach(), gh[:, 2].detach(), h[:, 0]], dim=1).numpy()
    out = _call(lib, "nlc_t_gru_cell_bwd", inp, 5)
    ref = np.stack([gi.grad[:, 0], gi.grad[:, 1], gi.grad[:, 2], gh.grad[:, 2], hp.grad[:, 0]], axis=1)
    # hidden side r / z gradients equal the input side's
    np.testing.assert_allclose(gh.grad[:, :2].numpy(), gi.grad[:, :2].numpy(), rtol=0, atol=0)
    scale = np.abs(ref).max(axis=0) + 1e-300
    assert (np.abs(out - ref) / scale).max() <= 1e-15


def test_sphere_map_backward_vs_autograd(lib):
    """theta = tanh(o) pi, phi = tanh(o) pi / 2 - pi/2 + pi/2 (w_nl.py:59-62): the pre-activation gradients equal autograd's
    to 4 ulp of g * pi (the factor 1 - y^2 cancels near saturation, and torch's CPU kernel may contract it to an FMA: the
    bound is on the scale of the product, not on the cancelled result)."""
    torch.manual_seed(1)
    o = (torch.randn(20000, dtype=torch.float64) * 3).requires_grad_()
    g = torch.randn(20000, dtype=torch.float64)
    y = torch.tanh(o)
    th = y * torch.pi
    th.backward(g)
    ref_t = o.grad.clone()
    o.grad = None
    phi_scale = torch.pi / 2.0 - -torch.pi / 2.0
    ph = torch.tanh(o) * phi_scale / 2.0 - torch.pi / 2.0 + phi_scale / 2.0
    ph.backward(g)
    ref_p = o.grad.clone()
    out = _call(lib, "nlc_t_sphere_bwd", np.stack([g.numpy(), y.detach().numpy()], axis=1), 2)
    sc = np.spacing(np.abs(g.numpy()) * np.pi)
    assert (np.abs(out[:, 0] - ref_t.numpy()) / sc).max() <= 4
    assert (np.abs(out[:, 1] - ref_p.numpy()) / sc).max() <= 4


def test_clip_coefficient_vs_clip_grad_norm(lib):
    """clip_grad_norm_ multiplies by min(1, max_norm / (total + 1e-6)): a one-element gradient of value `total` (its own
    norm) clipped by torch equals total * the host coefficient to 2 ulp (active and inactive; torch's division may round the
    coefficient one ulp differently)."""
    rng = np.random.default_rng(2)
    rows = []
    for total in np.concatenate([rng.uniform(1e-3, 10, 200), [0.05, 0.1, 0.1000001, 1e6]]):
        for max_norm in (0.1, 1.0):
            p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
            p.grad = torch.tensor([float(total)], dtype=torch.float64)
            torch.nn.utils.clip_grad_norm_([p], max_norm)
            rows.append((max_norm, total, float(p.grad[0])))
    rows = np.array(rows)
    out = _call(lib, "nlc_t_clip_coef", rows[:, :2], 1)[:, 0]
    assert _ulp(out * rows[:, 1], rows[:, 2]).max() <= 2
    assert out.max() == 1.0 and out.min() < 1.0


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_element_vs_torch_adam(lib, wd):
    """Three torch.optim.Adam steps (foreach off and on give the same element formula) against the host element update
    with the host-side scalars of nlc_train_step: parameters and exp_avg_sq to 4 ulp; exp_avg to 4 ulp of |exp_avg| + max |g|
    over the steps (the lerp m + w (g - m) cancels when g and m have opposite signs)."""
    torch.manual_seed(3)
    n = 5000
    p0 = torch.randn(n, dtype=torch.float64)
    grads = [torch.randn(n, dtype=torch.float64) * 10.0 ** torch.randint(-9, 2, (n,)).double() for _ in range(3)]
    lr, b1, b2, eps = 1e-4, 0.9, 0.999, 1e-8
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    state = np.ascontiguousarray(np.stack([p0.numpy(), np.zeros(n), np.zeros(n)], axis=1))
    f = lib.nlc_t_adam
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    for step, g in enumerate(grads, start=1):
        p.grad = g.clone()
        opt.step()
        bc1, bc2 = 1 - b1**step, 1 - b2**step
        k = np.array([wd, 1 - b1, b2, 1 - b2, (lr / bc1) * -1, bc2**0.5, eps])
        gn = np.ascontiguousarray(g.numpy())
        f(state.ctypes.data, gn.ctypes.data, k.ctypes.data, n)
    st = opt.state[p]
    assert _ulp(state[:, 0], p.detach().numpy()).max() <= 4
    m_ref = st["exp_avg"].numpy()
    assert (np.abs(state[:, 1] - m_ref) / np.spacing(np.abs(m_ref) + np.abs(torch.stack(grads).numpy()).max(axis=0) + wd * np.abs(p0.numpy()))).max() <= 4
    assert _ulp(state[:, 2], st["exp_avg_sq"].numpy()).max() <= 4
