"""Block-wise comparison of gradients for the fused training step's tests (tests/test_gpu_train.py, and its unit test in
tests/test_train_host.py).

A per-tensor scale (max |grad| of the whole tensor) lets a wrong block hide under a larger one: the [r; z; n] gate blocks
of a GRU tensor can differ by orders of magnitude (a saturated gate), and so can the theta / phi halves of the last
representation layer.  Each such block is compared against its own max |grad| instead, floored at 1e-6 of the tensor's so
that a block made of roundoff alone does not fail for no reason."""

import torch

GRU_PREFIX = "action_encoder.gru."
LAST_LAYER = "laplace_rep_func.linear_tanh_stack.4."
BLOCK_FLOOR = 1e-6


def grad_blocks(name, t):
    """(label, view) of the blocks ``name``'s gradient is compared in: the three gate blocks of a GRU tensor (rows
    [r; z; n], torch.nn.GRU's order), the theta / phi halves of the last rep-func layer (rows [theta | phi]), the whole
    tensor otherwise."""
    if name.startswith(GRU_PREFIX):
        g = t.shape[0] // 3
        return [(f"{name}[{gate}]", t[i * g : (i + 1) * g]) for i, gate in enumerate("rzn")]
    if name.startswith(LAST_LAYER):
        half = t.shape[0] // 2
        return [(f"{name}[theta]", t[:half]), (f"{name}[phi]", t[half:])]
    return [(name, t)]


def blockwise_errors(name, got, ref):
    """[(label, max |got - ref|, scale)] per block, scale = max(block max |ref|, BLOCK_FLOOR x tensor max |ref|)."""
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to("cpu", torch.float64)
    tmax = float(ref.abs().max())
    out = []
    for (label, g), (_, r) in zip(grad_blocks(name, got), grad_blocks(name, ref)):
        scale = max(float(r.abs().max()), BLOCK_FLOOR * tmax) + 1e-300
        out.append((label, float((g - r).abs().max()), scale))
    return out


def assert_grad_close(name, got, ref, tol, sens=None, factor=200.0):
    """Every block of ``got`` within ``tol`` of its own scale.  ``sens`` (same shape as ``ref``): the reference's own
    response to a tiny input perturbation; the bound then widens by ``factor`` x that block's max response (a
    condition-aware bound, for cases whose conditioning is shown, never a default)."""
    if not bool(torch.isfinite(got.detach().cpu()).all()):
        raise AssertionError(f"{name}: non-finite gradient")
    blocks_s = grad_blocks(name, sens.detach().cpu()) if sens is not None else None
    for i, (label, err, scale) in enumerate(blockwise_errors(name, got, ref)):
        bound = tol * scale
        if blocks_s is not None:
            bound += factor * float(blocks_s[i][1].abs().max())
        assert err <= bound, f"{label}: max err {err:.3e} > bound {bound:.3e} (block scale {scale:.3e})"


def per_tensor_close(got, ref, tol):
    """The earlier comparison: max |got - ref| within tol x the whole tensor's max |ref|."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    return float((got - ref).abs().max()) <= tol * (float(ref.abs().max()) + 1e-300)
