"""CPU: the element math of the NODE training step (csrc/nlc_train_node.h), built with g++ as tests/test_train_host.py
builds the rest: torchdiffeq's fixed Euler grid against oracle.node_model.euler_substeps (exactly), the clamp at bad and
over-long times, and the backward of one Euler sub-step against float64 autograd through oracle.node_model.ode_func; the five
nlc_node_train_group_* entries in the header, the binding and the built library; the package's exports."""

import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import node_model as on

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "helpers", "train_node_host.cpp")
ENTRIES = ["nlc_node_train_group_" + w for w in ("workspace_bytes", "loss_grad", "step", "eval_workspace_bytes", "eval")]
P = "x_ode_func_in_x_and_u.linear_tanh_stack."
KEYS = [P + f"{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]
TOL = 1e-13  # of each quantity's magnitude: the bound of tests/test_train_linear_host.py for the same kind of check


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("trainnodehost") / "libtrain_node_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), SRC])
    lib = ctypes.CDLL(str(out))
    vp, dbl = ctypes.c_void_p, ctypes.c_double
    lib.nlc_t_node_grid.argtypes = [vp, dbl, ctypes.c_long, vp, vp, vp]
    lib.nlc_t_node_substep.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, dbl] + [vp] * 8
    return lib


def _grid(lib, times, step=0.05):
    cap = lib.nlc_t_node_max_sub()
    t = np.ascontiguousarray(times, dtype=np.float64)
    nsub, bad = np.zeros(t.size, dtype=np.int32), np.zeros(t.size, dtype=np.int32)
    h = np.full((t.size, cap), np.nan)
    lib.nlc_t_node_grid(t.ctypes.data, step, t.size, nsub.ctypes.data, bad.ctypes.data, h.ctypes.data)
    return nsub, bad, h


def test_the_cap_is_256(lib):
    assert lib.nlc_t_node_max_sub() == 256


def test_grid_equals_the_oracle_exactly(lib):
    """Count and every width == oracle.node_model.euler_substeps: at the grid points k * 0.05, one ulp to either side of each
    (where ceil moves), and at times between them."""
    times = []
    for k in range(1, 9):
        t = k * 0.05
        times += [t, math.nextafter(t, 0.0), math.nextafter(t, 1.0)]
    times += [0.125, 1e-9, 0.399999]
    nsub, bad, h = _grid(lib, times)
    for i, t in enumerate(times):
        ref = on.euler_substeps(t, 0.05)
        assert not bad[i] and nsub[i] == len(ref), (t, nsub[i], len(ref))
        assert h[i, : nsub[i]].tolist() == ref, t
        assert np.isnan(h[i, nsub[i] :]).all()  # nothing written past the count
    assert len(set(nsub.tolist())) >= 8


def test_grid_at_other_step_sizes(lib):
    for step in (0.01, 0.03, 0.125):
        times = [step * k for k in (1, 2, 3, 7)] + [0.77 * step, 5.5 * step]
        nsub, bad, h = _grid(lib, times, step)
        for i, t in enumerate(times):
            ref = on.euler_substeps(t, step)
            assert not bad[i] and h[i, : nsub[i]].tolist() == ref


def test_bad_times_give_the_clamped_counts(lib):
    """0, -1 and NaN: no sub-step; a time past the cap (and inf): the cap; all flagged, so the kernels give the row a NaN squared
    error.  The last time within the cap is not flagged."""
    cap = lib.nlc_t_node_max_sub()
    last_ok = 0.05 * cap  # ceil(256 + 1) = 257 points
    nsub, bad, _ = _grid(lib, [0.0, -1.0, float("nan"), -0.0, last_ok, math.nextafter(last_ok, 100.0), 1e3, 1e300, float("inf")])
    assert nsub.tolist() == [0, 0, 0, 0, cap, cap, cap, cap, cap]
    assert bad.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert len(on.euler_substeps(last_ok, 0.05)) == cap


def _substep(lib, sd, H, dy, nu, x, u, h, xbn):
    blob = np.ascontiguousarray(torch.cat([sd[k].reshape(-1) for k in KEYS]).numpy())
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, u, xbn)]
    outs = [np.empty(n) for n in (dy, H, H, dy, H, H, dy)]
    lib.nlc_t_node_substep(blob.ctypes.data, H, dy, nu, arrs[0].ctypes.data, arrs[1].ctypes.data, h, arrs[2].ctypes.data,
                           *[o.ctypes.data for o in outs])
    return outs  # f, a1, a2, d3, d2, d1, xbar


@pytest.mark.parametrize("H", [5, 33])
@pytest.mark.parametrize("d,aug,nu", [(5, 1, 1), (2, 1, 2), (1, 0, 1)])
def test_substep_backward_vs_autograd(lib, H, d, aug, nu):
    """x' = x + h f(cat(x, u)) with L = <xbar', x'>: f, dL/dx, the three bias gradients (the deltas) and the three weight
    gradients (delta outer input) equal float64 autograd through oracle.node_model.ode_func to 1e-13 of each quantity's max."""
    dy = d + aug
    worst = 0.0
    for seed in range(20):
        sd = on.make_synthetic_state_dict(seed, d, nu, H, aug, out_scale=1.0)
        g = torch.Generator().manual_seed(100 + seed)
        x = torch.randn(dy, dtype=torch.float64, generator=g)
        u = torch.randn(nu, dtype=torch.float64, generator=g) * 2
        xbn = torch.randn(dy, dtype=torch.float64, generator=g)
        h = [0.05, 0.025, 1e-9, -7e-18][seed % 4]  # the last width of a grid can be tiny or negative
        leaves = {k: sd[k].clone().requires_grad_() for k in KEYS}
        xl = x.clone().requires_grad_()
        f = on.ode_func(leaves, xl.view(1, -1), u.view(1, -1))[0]
        ((xl + h * f) * xbn).sum().backward()
        got_f, a1, a2, d3, d2, d1, xbar = _substep(lib, sd, H, dy, nu, x.numpy(), u.numpy(), h, xbn.numpy())
        z = np.concatenate([x.numpy(), u.numpy()])
        pairs = [
            ("f", got_f, f.detach().numpy()), ("xbar", xbar, xl.grad.numpy()),
            ("4.bias", d3, leaves[P + "4.bias"].grad.numpy()), ("2.bias", d2, leaves[P + "2.bias"].grad.numpy()),
            ("0.bias", d1, leaves[P + "0.bias"].grad.numpy()),
            ("4.weight", np.outer(d3, a2), leaves[P + "4.weight"].grad.numpy()),
            ("2.weight", np.outer(d2, a1), leaves[P + "2.weight"].grad.numpy()),
            ("0.weight", np.outer(d1, z), leaves[P + "0.weight"].grad.numpy()),
        ]
        for what, got, ref in pairs:
            assert np.isfinite(got).all()
            scale = np.abs(ref).max()
            assert scale > 0, what
            err = np.abs(got - ref).max() / scale
            worst = max(worst, err)
            assert err <= TOL, f"H={H} seed={seed}: {what} off by {err:.3e} of its magnitude"
    print(f"H={H} d={d} aug={aug} nu={nu}: worst {worst:.2e}")


def test_stand_alone_program_runs(tmp_path):
    """The same source with its own main() (-DNLC_T_MAIN: the program a sanitizer build runs, nothing loaded into python)."""
    exe = tmp_path / "train_node_host_main"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-DNLC_T_MAIN", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("ok ") and math.isfinite(float(out.stdout.split()[1]))


# ---------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(REPO, "include", "nlc.h")).read()


@pytest.mark.parametrize("name", ENTRIES)
def test_header_declares_the_entry_and_cites_the_reference(name):
    hdr = _header()
    m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(\s*nlc_ctx\s*\*\s*ctx\s*,", hdr)
    assert m, f"{name}(nlc_ctx* ctx, ...) is not declared in include/nlc.h"
    assert (m.group(1) == "int64_t") == name.endswith("workspace_bytes")
    before = hdr[: hdr.index(name + "(")]
    comment = before[before.rindex("/*") :]
    assert ("train_utils.py:3" in comment or "overlay.py:112-115" in comment) and "run_exp_multi.py:105-110" in comment
    if not name.endswith("workspace_bytes"):
        decl = hdr[hdr.index(name + "(") :]
        assert re.search(r"int row_times\s*\)\s*;", decl[: decl.index(";") + 1]), f"{name} does not end with int row_times"


def test_abi_version_is_at_least_18():
    assert int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", _header()).group(1)) >= 18


def test_binding_lists_and_library_exports_the_entries():
    from neurallaplacecontrol_amd import _lib

    for name in ENTRIES:
        assert name in _lib.SYMBOLS, name
    so = _lib.LIB_PATH
    if not os.path.exists(so):
        pytest.fail(f"{so} is not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(so)
    for name in ENTRIES:
        assert hasattr(lib, name), f"libnlc_hip.so does not export {name}"
    assert lib.nlc_abi_version() >= 18


def test_package_exports_the_node_trainers():
    import neurallaplacecontrol_amd as nlc

    for name in ("NODETrainer", "NODETrainerGroup"):
        assert name in nlc.__all__ and hasattr(nlc, name)
    assert issubclass(nlc.NODETrainerGroup, nlc.NODETrainer)
    assert nlc.NODETrainer.MAX_SUBSTEPS == 256


def test_slab_and_blob_layout_do_not_depend_on_the_data(lib):
    """The Python-side cap equals the header's, which sizes the slab (nlc_train_node.h node_act_layout)."""
    import neurallaplacecontrol_amd as nlc

    assert nlc.NODETrainer.MAX_SUBSTEPS == lib.nlc_t_node_max_sub()
