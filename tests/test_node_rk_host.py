"""CPU: the NODE's fixed-grid solvers as the kernels hold them (csrc/nlc_node_rk.h, csrc/nlc_train_node.h), built with g++:
the tableaus against a NumPy restatement of the three steps, the order of convergence on y' = -y (a mistyped tableau shows
there: upstream torchdiffeq cannot be consulted offline), the sub-step backward of midpoint and rk4 against float64 autograd
of the restated step (tests/node_rk_reference.py), the grid against oracle.node_model.euler_substeps, the per-method cap, and
the Python mirror's host-side pieces (method accepted / refused, tableau restatement, ABI)."""

import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import node_rk_reference as rk
from oracle import node_model as on

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "helpers", "node_rk_host.cpp")
P = "x_ode_func_in_x_and_u.linear_tanh_stack."
KEYS = [P + f"{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]
TOL = 1e-13  # of each quantity's magnitude: tests/test_train_node_host.py's bound for the same kind of check


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("noderkhost") / "libnode_rk_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), SRC])
    lib = ctypes.CDLL(str(out))
    vp, dbl, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    lib.nlc_t_rk_tableau.argtypes = [i32, vp, vp]
    lib.nlc_t_rk_linear.argtypes = [i32, dbl, dbl, i32]
    lib.nlc_t_rk_linear.restype = dbl
    lib.nlc_t_rk_grid.argtypes = [i32, dbl, dbl, vp, vp]
    lib.nlc_t_rk_substep.argtypes = [i32, vp, i32, i32, i32, vp, vp, dbl, vp, vp, vp, vp]
    return lib


def _tableau(lib, method):
    a, b = np.zeros((4, 4)), np.zeros(4)
    s = lib.nlc_t_rk_tableau(rk.OPTION[method], a.ctypes.data, b.ctypes.data)
    return s, a, b


def _tableau_step(s, a, b, f, y, h):
    k = []
    for i in range(s):
        k.append(f(y + h * sum(a[i, j] * k[j] for j in range(i)) if i else y))
    return y + h * sum(b[i] * k[i] for i in range(s))


@pytest.mark.parametrize("method", rk.METHODS)
def test_tableau_equals_the_restated_step(lib, method):
    """The header's (s, a_ij, b_i) applied as Y_i = y + h sum a_ij k_j, y' = y + h sum b_i k_i give the step of
    node_rk_reference.rk_step (the formulas in their stated evaluation order) on a nonlinear f, to rounding; the tableau is
    strictly lower triangular, consistent (sum b = 1) and zero past its s stages."""
    s, a, b = _tableau(lib, method)
    assert s == rk.STAGES[method]
    assert np.all(np.triu(a) == 0) and np.all(a[s:] == 0) and np.all(b[s:] == 0)
    assert abs(b.sum() - 1.0) <= 1e-15
    f = lambda y: np.sin(3 * y) - 0.5 * y * y  # noqa: E731
    rng = np.random.RandomState(0)
    for h in (0.05, 0.025, 1e-9, -7e-18, 0.4):
        y = rng.randn(7)
        got = _tableau_step(s, a, b, f, y, h)
        ref = rk.rk_step(method, f, y, h)
        assert np.abs(got - ref).max() <= 4e-16 * max(1.0, np.abs(ref).max())
    exact = {"euler": ([], [1.0]), "midpoint": ([0.5], [0.0, 1.0]),
             "rk4": ([1 / 3, -1 / 3, 1.0, 1.0, -1.0, 1.0], [1 / 8, 3 / 8, 3 / 8, 1 / 8])}[method]
    assert a[np.tril_indices(s, -1)].tolist() == exact[0] and b[:s].tolist() == exact[1]


def test_unknown_methods_are_not_ok(lib):
    assert [lib.nlc_t_rk_ok(m) for m in (-1, 0, 1, 2, 3)] == [0, 1, 1, 1, 0]


@pytest.mark.parametrize("method,lo,hi", [("euler", 1.8, 2.2), ("midpoint", 3.5, 4.5), ("rk4", 14.0, 18.0)])
def test_order_of_convergence(lib, method, lo, hi):
    """y' = -y over [0, 1] through the functions the kernels call: halving the step from 1/16 to 1/32 divides the end error by
    about 2 (euler), 4 (midpoint), 16 (rk4)."""
    m = rk.OPTION[method]
    e16 = abs(lib.nlc_t_rk_linear(m, -1.0, 1.0, 16) - math.exp(-1.0))
    e32 = abs(lib.nlc_t_rk_linear(m, -1.0, 1.0, 32) - math.exp(-1.0))
    print(f"{method}: error {e16:.3e} at 1/16, {e32:.3e} at 1/32, ratio {e16 / e32:.3f}")
    assert lo <= e16 / e32 <= hi


@pytest.mark.parametrize("method", rk.METHODS)
def test_caps_and_grid_equal_the_oracle_exactly(lib, method):
    """Count and widths == oracle.node_model.euler_substeps at grid points, one ulp to either side and in between, for every
    method; the cap is 256 evaluations of the ODE function: 256 / s sub-steps, the last time within it not flagged, the next
    one flagged and clamped."""
    m = rk.OPTION[method]
    cap = lib.nlc_t_rk_max_sub(m)
    assert cap == 256 // rk.STAGES[method]
    times = [0.125, 1e-9, 0.399999]
    for k in list(range(1, 9)) + [40, cap]:
        t = k * 0.05
        times += [t, math.nextafter(t, 0.0)] + ([math.nextafter(t, 1e9)] if k < cap else [])
    h, bad = np.full(cap, np.nan), ctypes.c_int(7)
    for t in times:
        n = lib.nlc_t_rk_grid(m, t, 0.05, ctypes.byref(bad), h.ctypes.data)
        ref = on.euler_substeps(t, 0.05)
        assert bad.value == 0 and n == len(ref) and h[:n].tolist() == ref, (method, t)
    for t, n_ref in ((math.nextafter(0.05 * cap, 1e9), cap), (1e300, cap), (float("inf"), cap), (0.0, 0), (-1.0, 0),
                     (float("nan"), 0)):
        assert lib.nlc_t_rk_grid(m, t, 0.05, ctypes.byref(bad), h.ctypes.data) == n_ref and bad.value == 1


def _substep(lib, method, sd, H, dy, nu, y, u, h, ybn):
    blob = np.ascontiguousarray(torch.cat([sd[k].reshape(-1) for k in KEYS]).numpy())
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (y, u, ybn)]
    yn, ybar, grad = np.empty(dy), np.empty(dy), np.empty(blob.size)
    lib.nlc_t_rk_substep(rk.OPTION[method], blob.ctypes.data, H, dy, nu, arrs[0].ctypes.data, arrs[1].ctypes.data, h,
                         arrs[2].ctypes.data, yn.ctypes.data, ybar.ctypes.data, grad.ctypes.data)
    out, o = {}, 0
    for k in KEYS:
        out[k] = grad[o : o + sd[k].numel()].reshape(tuple(sd[k].shape))
        o += sd[k].numel()
    return yn, ybar, out


@pytest.mark.parametrize("method", ["midpoint", "rk4", "euler"])
@pytest.mark.parametrize("H", [5, 33])
@pytest.mark.parametrize("d,aug,nu", [(5, 1, 1), (2, 1, 2), (1, 0, 1)])
def test_substep_backward_vs_autograd(lib, method, H, d, aug, nu):
    """One sub-step with L = <ybar', y'>: y', dL/dy and the six weight gradients equal float64 autograd through the restated
    step (node_rk_reference.rk_step over oracle.node_model.ode_func) to 1e-13 of each quantity's max."""
    dy = d + aug
    worst = 0.0
    for seed in range(12):
        sd = on.make_synthetic_state_dict(seed, d, nu, H, aug, out_scale=1.0)
        g = torch.Generator().manual_seed(100 + seed)
        y = torch.randn(dy, dtype=torch.float64, generator=g)
        u = torch.randn(nu, dtype=torch.float64, generator=g) * 2
        ybn = torch.randn(dy, dtype=torch.float64, generator=g)
        h = [0.05, 0.025, 1e-9, -7e-18][seed % 4]
        leaves = {k: sd[k].clone().requires_grad_() for k in KEYS}
        yl = y.clone().requires_grad_()
        yn = rk.rk_step(method, lambda v: on.ode_func(leaves, v, u.view(1, -1)), yl.view(1, -1), h)[0]
        (yn * ybn).sum().backward()
        got_yn, got_ybar, grads = _substep(lib, method, sd, H, dy, nu, y.numpy(), u.numpy(), h, ybn.numpy())
        pairs = [("y'", got_yn, yn.detach().numpy()), ("ybar", got_ybar, yl.grad.numpy())]
        pairs += [(k[len(P):], grads[k], leaves[k].grad.numpy()) for k in KEYS]
        for what, got, ref in pairs:
            assert np.isfinite(got).all()
            scale = np.abs(ref).max()
            assert scale > 0, what
            err = np.abs(got - ref).max() / scale
            worst = max(worst, err)
            assert err <= TOL, f"{method} H={H} seed={seed}: {what} off by {err:.3e} of its magnitude"
    print(f"{method} H={H} d={d} aug={aug} nu={nu}: worst {worst:.2e}")


def test_stand_alone_program_runs(tmp_path):
    """The same source with its own main() (-DNLC_T_MAIN: the program a sanitizer build runs, nothing loaded into python)."""
    exe = tmp_path / "node_rk_host_main"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DNLC_T_MAIN", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("ok ") and math.isfinite(float(out.stdout.split()[1]))


# ---------------------------------------------------------------------------------------------------------------------
def _node(method):
    import neurallaplacecontrol_amd as nlc

    return nlc.NODE(3, 1, 3, hidden_units=5, state_mean=np.zeros(3), state_std=np.ones(3), action_mean=np.array([0]),
                    action_std=np.array([1.0]), normalize=True, normalize_time=True, method=method, augment_dim=1)


@pytest.mark.parametrize("method", rk.METHODS)
def test_mirror_accepts_the_three_methods(method):
    m = _node(method)
    assert m.method == method and m.stages == rk.STAGES[method]
    assert method in m._weights_key_extra()


@pytest.mark.parametrize("method", ["dopri5", "adams", "rk4_classic", "", None])
def test_mirror_refuses_other_methods(method):
    with pytest.raises(NotImplementedError):
        _node(method)


@pytest.mark.parametrize("method", rk.METHODS)
def test_python_tableau_restates_the_header(lib, method):
    from neurallaplacecontrol_amd.node_model import RK_TABLEAUS

    s, a, b = _tableau(lib, method)
    opt, rows, bs = RK_TABLEAUS[method]
    assert opt == rk.OPTION[method] and len(bs) == s and list(bs) == b[:s].tolist()
    for i, row in enumerate(rows):
        assert list(row) == a[i, :i].tolist()


def test_a_changed_method_changes_the_weights_key():
    m = _node("euler")
    k0 = m._weights_key()
    m.method = "rk4"
    assert m._weights_key() != k0
    m.method = "euler"
    assert m._weights_key() == k0


def test_header_documents_the_option_and_the_abi_moved():
    hdr = open(os.path.join(REPO, "include", "nlc.h")).read()
    assert '"node_method"' in hdr and "midpoint" in hdr and "3/8" in hdr
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 20
    assert "PARITY UNPINNED" in hdr


def test_trainer_cap_per_method():
    import neurallaplacecontrol_amd as nlc

    assert nlc.NODETrainer.MAX_SUBSTEPS == 256
    for method in rk.METHODS:
        tr = nlc.NODETrainer.__new__(nlc.NODETrainer)
        tr.model = _node(method)
        assert tr.max_substeps() == 256 // rk.STAGES[method]
