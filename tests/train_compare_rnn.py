"""Block-wise comparison of DeltaTRNN / RNN gradients for tests/test_gpu_train_rnn.py, on the scales of
tests/train_compare.py: each block against its own max |grad|, floored at BLOCK_FLOOR of its tensor's.

Blocks: the three [r; z; n] row blocks of each GRU tensor; linear_out.weight by columns -- hidden [:, :H], state
[:, H:H+d] and time [:, H+d:] (their inputs differ in scale); linear_out.bias as a whole."""

import torch
from train_compare import BLOCK_FLOOR, blockwise_errors


def rnn_grad_blocks(name, t, H, d):
    if name.startswith("gru."):
        return [(f"{name}[{gate}]", t[i * H : (i + 1) * H]) for i, gate in enumerate("rzn")]
    if name == "linear_out.weight":
        blocks = [(f"{name}[hidden]", t[:, :H]), (f"{name}[state]", t[:, H : H + d])]
        if t.shape[1] > H + d:
            blocks.append((f"{name}[time]", t[:, H + d :]))
        return blocks
    return [(name, t)]


def rnn_blockwise_errors(name, got, ref, H, d):
    """[(label, max |got - ref|, scale)] per block, scale = max(block max |ref|, BLOCK_FLOOR x tensor max |ref|)."""
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to("cpu", torch.float64)
    tmax = float(ref.abs().max())
    out = []
    for (label, g), (_, r) in zip(rnn_grad_blocks(name, got, H, d), rnn_grad_blocks(name, ref, H, d)):
        (_, err, _), = blockwise_errors(label, g, r)  # one block: a view's label matches no prefix of train_compare
        out.append((label, err, max(float(r.abs().max()), BLOCK_FLOOR * tmax) + 1e-300))
    return out


def assert_rnn_grad_close(name, got, ref, H, d, tol, report=None):
    if not bool(torch.isfinite(got.detach().cpu()).all()):
        raise AssertionError(f"{name}: non-finite gradient")
    errs = rnn_blockwise_errors(name, got, ref, H, d)
    if report is not None:
        for label, err, scale in errs:
            report(f"{label}: err {err:.3e} scale {scale:.3e} ratio {err / scale:.3e}")
    for label, err, scale in errs:
        assert err <= tol * scale, f"{label}: max err {err:.3e} > {tol:g} x block scale {scale:.3e}"
