"""GPU tests (run with ``-m gpu`` on an MI355X): the stand-alone de Hoog ILT kernels, forward (`ilt_dehoog_kernel<M>`) and
backward (`ilt_dehoog_bwd_kernel<M>`), at EVERY term count S = 2M + 1 = 3 .. 33 -- each M is separately unrolled code -- against
a 60-digit evaluation of the same recurrences and its tape gradient (tests/dehoog_mp_reference.py).

The bounds are not tolerances picked for the kernel: the kernel is one more float64 rounding of arithmetic that two CPU
roundings also carry out, and its error quantiles against the 60-digit values must lie within fixed margins of theirs.  The
margins and the measurements behind them are in tests/test_dehoog_mp_host.py, which also confirms on the CPU that the
reference alone meets every condition on exactly these inputs (seed 300 + S, 67 points x 3 dims = 201 rows: three full 64-row
blocks and a ragged block of 9).  No row is left out of any comparison.
"""

import numpy as np
import pytest
import torch

import dehoog_mp_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=R.TERM_COUNTS)
def case(request):
    """Inputs, 60-digit values / gradients and the CPU roundings' quantiles of one term count: shared by forward and backward."""
    return R.reference_case(request.param)


def _report(what, S, got, ref, names):
    print(f"dehoog mp S={S} {what}: " + "  ".join(f"{n} {g:.2e} (x{g / r:.2f} of CPU {r:.2e})" for n, g, r in zip(names, got, ref)))


def test_dehoog_forward_every_term_count_vs_60_digits(nlc, case):
    S = case["S"]
    x = nlc.ilt_reconstruct(case["theta"].cuda(), case["phi"].cuda(), case["t"].cuda(), "dehoog").cpu()
    assert x.shape == (R.N_POINTS, R.N_DIMS)
    err = R.forward_errors(x, case["x_mp"])
    assert err.shape == (R.N_POINTS * R.N_DIMS,) and np.isfinite(err).all()
    got = np.quantile(err, [0.5, 0.9, 1.0])
    cpu = np.maximum(*case["fwd_q"])
    _report("forward", S, got, cpu, ("q50", "q90", "max"))
    assert got[0] <= R.FWD_MARGIN_Q * cpu[0], (S, "q50", got[0], cpu[0])
    assert got[1] <= R.FWD_MARGIN_Q * cpu[1], (S, "q90", got[1], cpu[1])
    assert got[2] <= R.FWD_MARGIN_MAX * cpu[2], (S, "max", got[2], cpu[2], int(err.argmax()))


def _forward_backward(nlc, theta, phi, t, w):
    th, ph = theta.cuda().requires_grad_(), phi.cuda().requires_grad_()
    x = nlc.ilt_reconstruct(th, ph, t.cuda(), "dehoog")
    gth, gph = torch.autograd.grad(x, (th, ph), w.cuda())
    return x.detach().cpu(), gth.cpu(), gph.cpu()


def test_dehoog_backward_every_term_count_vs_60_digit_tape(nlc, case):
    S, theta, phi, t, w = (case[k] for k in ("S", "theta", "phi", "t", "w"))
    x, gth, gph = _forward_backward(nlc, theta, phi, t, w)
    assert torch.isfinite(gth).all() and torch.isfinite(gph).all()
    # the rows at every block edge and the whole ragged block against w * (tape gradient), scaled by the row's largest entry
    err = R.gradient_errors(gth, gph, case["g_mp"], w)
    assert err.shape == (len(R.GRAD_ROWS),) and np.isfinite(err).all()
    got = np.quantile(err, [0.5, 1.0])
    cpu = case["grad_q"][0]  # autograd through the functional twin
    _report("gradient", S, got, cpu, ("q50", "max"))
    assert got[0] <= R.GRAD_MARGIN_Q50 * cpu[0], (S, "q50", got[0], cpu[0])
    assert got[1] <= R.GRAD_MARGIN_MAX * cpu[1], (S, "max", got[1], cpu[1], R.GRAD_ROWS[int(err.argmax())])
    # every other row: a row's result must not depend on where it sits.  Reversing points and dims sends flat row i to
    # 200 - i, which moves each checked row into the lanes and blocks of the unchecked ones
    xf, gthf, gphf = _forward_backward(nlc, theta.flip(0, 1), phi.flip(0, 1), t.flip(0), w.flip(0, 1))
    assert torch.equal(xf, x.flip(0, 1))
    assert torch.equal(gthf, gth.flip(0, 1)) and torch.equal(gphf, gph.flip(0, 1))
