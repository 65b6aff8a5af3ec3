"""The reference's synthetic transition dataset on the device (``overlay.py:664-737``).

The reference's training loop draws a fresh dataset every epoch unless it trains on expert trajectories
(``train_utils.py:353-370``): ``generate_irregular_data_delay_time_multi`` samples states and actions uniformly over a box
(``compute_state_actions``, ``overlay.py:603-631``), integrates one Euler step per (action, state) pair on the CPU
(``batch_integrate_system``, ``base_env.py:231-280``) and wraps every action into a random action buffer (``:718-731``).
:func:`generate_synthetic_dataset` forms the same rows with one HIP launch (``nlc_synth_generate``) and returns
``(s0, a0, sn, ts)`` in the layout every trainer here takes::

    s0, a0, sn, ts = generate_synthetic_dataset("oderl-cartpole", delay=2, rand=True, action_buffer_size=4, ts_grid="exp")
    trainer.run(s0, a0, sn, ts, torch.randperm(s0.shape[0]), batch_size)

A dataset is ``TI = 10 * samples_per_dim`` time blocks x ``A = samples_per_dim`` actions x ``S = samples_per_dim ** n``
states; row ``(ti * A + i) * S + j``.  Every draw is counter-based (Philox keyed by ``seed``) and indexed by what it belongs
to -- (ti, j), (ti, i), ti, (row, buffer row) -- so ``blocks=(begin, end)`` slices concatenate to the whole dataset bit for
bit and an epoch that does not fit in memory can be streamed.  docs/synthetic.md has the dataflow, the stream table and
what differs from the reference by construction.
"""

import ctypes as C

import torch

from . import _lib
from .envs import ENV_DIMS
from .laplace import default_ctx

__all__ = ["generate_synthetic_dataset", "synthetic_dataset_shape", "STATE_MAX", "DEFAULT_SAMPLES_PER_DIM"]

# torch.pi in the reference's float32 state_max tensor, widened to double: the sampled box is the reference's
_PI32 = 3.1415927410125732
# the box of the REDUCED state (overlay.py:689-694): cartpole [x, xdot, theta, thetadot], pendulum [theta, thetadot],
# acrobot [theta1, theta2, v1, v2]
STATE_MAX = {
    "oderl-cartpole": (5.0, 20.0, _PI32, 30.0),
    "oderl-pendulum": (_PI32, 5.0),
    "oderl-acrobot": (_PI32, _PI32, 5.0, 5.0),
}
DEFAULT_SAMPLES_PER_DIM = {"oderl-pendulum": 33, "oderl-cartpole": 20, "oderl-acrobot": 15}  # (overlay.py:675-681)
TIME_MULTIPLIER = 10  # (overlay.py:682)


def synthetic_dataset_shape(env_name, samples_per_dim=None):
    """``(TI, A, S)``: time blocks, actions per block and states per block of a dataset (``overlay.py:608, 621, 698``)."""
    if env_name not in STATE_MAX:
        raise ValueError(f"unknown env {env_name!r}; expected one of {sorted(STATE_MAX)}")
    spd = DEFAULT_SAMPLES_PER_DIM[env_name] if samples_per_dim is None else int(samples_per_dim)
    if spd < 1:
        raise ValueError("samples_per_dim must be >= 1")
    return TIME_MULTIPLIER * spd, spd, spd ** len(STATE_MAX[env_name])


def generate_synthetic_dataset(env_name, delay, samples_per_dim=None, *, rand=True, action_buffer_size=5,
                               encode_obs_time=False, reuse_state_actions_when_sampling_times=False, dt=0.05,
                               ts_grid="fixed", friction=False, seed=0, blocks=None, device=None, observation_noise=0.0):
    """``generate_irregular_data_delay_time_multi(env_name, env, delay, samples_per_dim, rand=True, ...)`` for an env created
    with ``dt``, ``ts_grid`` and ``friction`` (``overlay.py:19-42``): float64 device tensors ``s0 (R, d)``,
    ``a0 (R, B, nu [+ 1])``, ``sn (R, d)``, ``ts (R, 1)`` with ``R = TI * A * S`` rows (:func:`synthetic_dataset_shape`).

    ``blocks=(begin, end)`` generates time blocks ``[begin, end)`` only, ``(end - begin) * A * S`` rows; consecutive slices
    concatenate to the whole dataset bit for bit.  ``seed`` keys every draw.

    Not implemented (``NotImplementedError``): the grid mode ``rand=False`` (the reference's own default is
    ``rand_sample=True``, its grid is built in float32 and its pendulum grid is degenerate) and env observation noise."""
    if not rand:
        raise NotImplementedError(
            "rand=False: the grid mode is not implemented -- the reference builds its grid in float32 and its pendulum "
            "branch is degenerate (overlay.py:643-650, linspace(max, max)); the reference trains with rand_sample=True")
    if observation_noise != 0.0:
        raise NotImplementedError("observation_noise: the synthetic generator has no env observation noise "
                                  "(base_env.py:277-278); the expert collector (collect_expert_dataset) has it")
    TI, A, S = synthetic_dataset_shape(env_name, samples_per_dim)
    nx, nu, high = ENV_DIMS[env_name]
    B, delay = int(action_buffer_size), int(delay)
    if B < 1 or not 0 <= delay <= B - 1:
        raise ValueError("delay must be in [0, action_buffer_size - 1], action_buffer_size >= 1")
    if ts_grid not in _lib.TS_GRIDS:
        raise ValueError(f"unknown ts_grid {ts_grid!r}; expected one of {sorted(_lib.TS_GRIDS)}")
    begin, end = (0, TI) if blocks is None else (int(blocks[0]), int(blocks[1]))
    if not 0 <= begin < end <= TI:
        raise ValueError(f"blocks must satisfy 0 <= begin < end <= {TI}")
    if not torch.cuda.is_available():
        raise RuntimeError("neurallaplacecontrol_amd.generate_synthetic_dataset needs an AMD MI355X; there is no CPU path")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    smax = STATE_MAX[env_name]
    desc = _lib.SynthDesc(
        env=_lib.ENV_IDS[env_name], friction=int(bool(friction)), dt=float(dt), delay=delay, B=B, nu=nu,
        time_channel=int(bool(encode_obs_time)), ts_grid=_lib.TS_GRIDS[ts_grid],
        reuse=int(bool(reuse_state_actions_when_sampling_times)), S=S, A=A, action_high=high,
        state_max=(C.c_double * 4)(*smax, *([0.0] * (4 - len(smax)))), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
    )
    R, W = (end - begin) * A * S, nu + int(bool(encode_obs_time))
    mk = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
    s0, a0, sn, ts = mk(R, nx), mk(R, B, W), mk(R, nx), mk(R, 1)
    ctx = default_ctx(dev.index)
    ctx.launch(ctx.lib.nlc_synth_generate, C.byref(desc), begin, end, _lib.ptr(s0), _lib.ptr(a0), _lib.ptr(sn), _lib.ptr(ts))
    return s0, a0, sn, ts


def _out_of_scope(name, reason):
    def refuse(*args, **kwargs):
        raise NotImplementedError(f"{name}: {reason}")

    refuse.__name__ = refuse.__qualname__ = name
    refuse.__doc__ = f"Not implemented: {reason}"
    return refuse


# the reference's other synthetic entry points, named so that a port of its call sites fails with the reason
generate_irregular_data_delay_latent = _out_of_scope(
    "generate_irregular_data_delay_latent",
    "the _latent generator integrates two intervals per row (batch_integrate_system_double_time, overlay.py:222-397) for "
    "the latent baselines, which no trainer here consumes")
get_val_loss_delay_time_multi = _out_of_scope(
    "get_val_loss_delay_time_multi",
    "there is no device form of the validation loss (overlay.py:137-177); generate a dataset with "
    "generate_synthetic_dataset and evaluate the model on it")
