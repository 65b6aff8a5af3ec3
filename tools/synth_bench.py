"""Time of one epoch's synthetic dataset (generate_synthetic_dataset: synth_kernel behind nlc_synth_generate) beside the same
rows formed with PyTorch-ROCm tensor ops in the same process.

The default is the reference's cartpole epoch (train_samples_per_dim = 10, config.py:35): 100 time blocks x 10 actions x 10^4
states = 10^7 rows, with the generator's default buffer of 5 rows and the time channel 21 doubles each (1.68 GB).  One
warm-up call, then the median of --repeats timed calls of each form, alternately.

The tensor-op form is written out below (`tensor_op_dataset`): torch.rand for the states, actions, intervals and fills, one
vectorised Euler step of the cartpole rhs over all rows, torch.stack / torch.cat for the observations and the buffer -- the
whole dataset in one pass, no loop over blocks or actions (the reference loops over both on the CPU).

    python tools/synth_bench.py [--samples-per-dim 10] [--ts-grid exp] [--no-time-channel] [--out profiles/synth_bench.json]
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import neurallaplacecontrol_amd as nlc  # noqa: E402
from neurallaplacecontrol_amd.synthetic import STATE_MAX  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specified peak


def cartpole_rhs(s, a, friction=False):
    """ctcartpole.py:185-237 on reduced states (R, 4), actions (R, 1)."""
    xd, th, thd = s[:, 1], s[:, 2], s[:, 3]
    c, sn = torch.cos(th), torch.sin(th)
    g, fmag, mp, length = 9.8, 3.0, 0.1, 1.0
    mt, pml = mp + 1.0, mp * length
    force = torch.clamp(a[:, 0], -fmag, fmag) * fmag
    if friction:
        temp = (force + pml * thd * thd * sn - 5e-4 * torch.sign(xd)) / mt
        thacc = (g * sn - c * temp - 2e-6 * thd / pml) / (length * (4.0 / 3.0 - mp * c * c / mt))
    else:
        temp = (force + pml * thd * thd * sn) / mt
        thacc = (g * sn - c * temp) / (length * (4.0 / 3.0 - mp * c * c / mt))
    return torch.stack((xd, temp - pml * thacc * c / mt, thd, thacc), dim=1)


def cartpole_obs(s):
    return torch.stack((s[:, 0], s[:, 1], torch.cos(s[:, 2]), torch.sin(s[:, 2]), s[:, 3]), dim=1)


def tensor_op_dataset(TI, A, S, B, delay, dt, ts_grid, enc, dev):
    """The rows of generate_synthetic_dataset("oderl-cartpole", ...) with torch's generator and tensor ops."""
    f64 = dict(dtype=torch.float64, device=dev)
    smax = torch.tensor(STATE_MAX["oderl-cartpole"], **f64)
    high = 3.0
    states = (torch.rand(TI, 1, S, 4, **f64) * 2 - 1) * smax
    actions = (torch.rand(TI, A, 1, 1, **f64) * 2 - 1) * high
    if ts_grid == "exp":
        tsn = -dt * torch.log(torch.rand(TI, 1, 1, 1, **f64))
    elif ts_grid == "uniform":
        tsn = 2 * dt * torch.rand(TI, 1, 1, 1, **f64)
    else:
        tsn = torch.full((TI, 1, 1, 1), dt, **f64)
    R = TI * A * S
    s = states.expand(TI, A, S, 4).reshape(R, 4)
    a = actions.expand(TI, A, S, 1).reshape(R, 1)
    ts = tsn.expand(TI, A, S, 1).reshape(R, 1)
    s0 = cartpole_obs(s)
    sn = cartpole_obs(s + ts * cartpole_rhs(s, a))
    a0 = (torch.rand(R, B, 1, **f64) * 2 - 1) * high
    a0[:, B - 1 - delay] = a
    if enc:
        a0 = torch.cat((a0, torch.flip(torch.arange(B, **f64), (0,)).view(1, B, 1).expand(R, B, 1)), dim=2)
    return s0, a0, sn, ts.contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples-per-dim", type=int, default=10)
    ap.add_argument("--delay", type=int, default=2)
    ap.add_argument("--buffer", type=int, default=5, help="action_buffer_size (the reference's default: 5)")
    ap.add_argument("--no-time-channel", action="store_true", help="encode_obs_time=False: a (B, 1) buffer")
    ap.add_argument("--ts-grid", default="exp", choices=["fixed", "uniform", "exp"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "synth_bench.json"))
    a = ap.parse_args()
    env, dt = "oderl-cartpole", 0.05
    TI, A, S = nlc.synthetic_dataset_shape(env, a.samples_per_dim)
    R = TI * A * S
    dev = torch.device("cuda", torch.cuda.current_device())
    enc = not a.no_time_channel
    row_bytes = 8 * (2 * 5 + a.buffer * (1 + int(enc)) + 1)
    kernel = lambda: nlc.generate_synthetic_dataset(env, a.delay, a.samples_per_dim, action_buffer_size=a.buffer,  # noqa: E731
                                                    ts_grid=a.ts_grid, dt=dt, seed=0, encode_obs_time=enc)
    tensor = lambda: tensor_op_dataset(TI, A, S, a.buffer, a.delay, dt, a.ts_grid, enc, dev)  # noqa: E731
    with torch.no_grad():
        timed(kernel)  # warm-up: the library, the allocator's blocks
        timed(tensor)
        tk, tt = [], []
        for _ in range(a.repeats):
            tk.append(timed(kernel))
            tt.append(timed(tensor))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    res = {
        "workload": f"{env} samples_per_dim={a.samples_per_dim} TI={TI} A={A} S={S} rows={R} B={a.buffer} W={1 + int(enc)} delay={a.delay} "
                    f"ts_grid={a.ts_grid}",
        "rows": R, "bytes_stored": R * row_bytes, "repeats": a.repeats,
        "kernel_ms": 1e3 * med(tk), "kernel_ms_min_max": [1e3 * min(tk), 1e3 * max(tk)],
        "tensor_op_ms": 1e3 * med(tt), "tensor_op_ms_min_max": [1e3 * min(tt), 1e3 * max(tt)],
        "tensor_op_over_kernel": med(tt) / med(tk),
        "kernel_store_bandwidth_TBps": R * row_bytes / med(tk) / 1e12,
        "kernel_fraction_of_hbm_peak": R * row_bytes / med(tk) / HBM_PEAK,
        "rows_per_s": R / med(tk),
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
