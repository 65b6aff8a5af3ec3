"""Training-step throughput of NeuralLaplaceModel on cartpole (d = 5, h = 128, S = 17, B = 4), one JSON line:

  (a) the reference's iteration (train_utils.py:391-408) through the existing grad-mode model(...): forward, MSELoss,
      backward, clip_grad_norm_(0.1), torch.optim.Adam.step(), loss.item() every iteration;
  (b) NLTrainer.step() with loss.item() every iteration;
  (c) NLTrainer.run() over a permutation of --run-iters iterations (one host read at the end).

Every variant runs a warm-up first and every timing ends with torch.cuda.synchronize().  Iterations / s per variant and the
ratios (b) / (a), (c) / (a) at each batch size.  `--only run --run-iters 200` is the shape for a rocprofv3 kernel trace.

    python tools/train_bench.py [--batches 16 256] [--ref-iters 200] [--step-iters 1000] [--run-iters 10000] [--out FILE]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import neurallaplacecontrol_amd as nlc  # noqa: E402
from oracle import nl_model as onl  # noqa: E402

ENV, D, NU, H, S, B = "oderl-cartpole", 5, 1, 128, 17, 4


def make_model():
    st = onl.ENV_STATS[ENV]
    sd = onl.make_synthetic_state_dict(0, D, NU, H, S, st["state_std"], [st["act_high"] / 2], tame=True)
    m = nlc.NeuralLaplaceModel(D, NU, D, hidden_units=H, s_recon_terms=S, ilt_algorithm="fourier", state_mean=np.zeros(D),
                               state_std=np.ones(D), action_mean=np.array([0]), action_std=np.array([1.0]), normalize=True,
                               normalize_time=True).double()
    m.load_state_dict(sd)
    return m.to("cuda")


def dataset(M, seed=0):
    st = onl.ENV_STATS[ENV]
    g = torch.Generator().manual_seed(seed)
    std = torch.tensor(st["state_std"], dtype=torch.float64)
    s0 = torch.randn(M, D, dtype=torch.float64, generator=g) * std
    a0 = (torch.rand(M, B, NU, dtype=torch.float64, generator=g) * 2 - 1) * st["act_high"]
    sn = s0 + torch.randn(M, D, dtype=torch.float64, generator=g) * 0.05 * std
    ts = torch.rand(M, 1, dtype=torch.float64, generator=g) * 0.08 + 0.02
    return [t.cuda() for t in (s0, a0, sn, ts)]


def time_ref(bs, iters, warm):
    model = make_model()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    loss_func = torch.nn.MSELoss()
    s0, a0, sn, ts = dataset(bs * (iters + warm))
    perm = torch.randperm(s0.shape[0]).cuda()

    def it(i):
        opt.zero_grad()
        ind = perm[i * bs : i * bs + bs]
        bs0, ba0, bsn, bts = s0[ind], a0[ind], sn[ind], ts[ind]
        bsd = bsn - bs0
        loss = loss_func(model(bs0, ba0, bts).squeeze(), bsd.squeeze())
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)
        opt.step()
        return loss.item()

    for i in range(warm):
        it(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warm, warm + iters):
        it(i)
    torch.cuda.synchronize()
    return iters / (time.perf_counter() - t0)


def time_step(bs, iters, warm):
    tr = nlc.NLTrainer(make_model())
    s0, a0, sn, ts = dataset(bs * (iters + warm))
    perm = torch.randperm(s0.shape[0]).cuda()

    def it(i):
        ind = perm[i * bs : i * bs + bs]
        bs0, ba0, bsn, bts = s0[ind], a0[ind], sn[ind], ts[ind]
        return tr.step(bs0, ba0, bts, bsn - bs0).item()

    for i in range(warm):
        it(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warm, warm + iters):
        it(i)
    torch.cuda.synchronize()
    return iters / (time.perf_counter() - t0)


def time_run(bs, iters, warm):
    tr = nlc.NLTrainer(make_model())
    s0, a0, sn, ts = dataset(bs * iters)
    perm = torch.randperm(s0.shape[0]).cuda()
    tr.run(s0, a0, sn, ts, perm[: bs * warm], batch_size=bs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = tr.run(s0, a0, sn, ts, perm, batch_size=bs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert bool(torch.isfinite(losses).all())
    return iters / dt


def flops_per_iter(bs):
    """Multiply-adds x 2 of the dense products (forward + the two backward products per weight matrix); transcendentals
    and element-wise work not counted."""
    g, K0, O = H // 2, 2 * S + D + 2, 2 * D * S
    gru = B * (3 * g * (NU + g) + 3 * g * (g + g))  # both layers, per row per window
    mlp = K0 * H + H * H + H * O
    lin = 2 * g
    fwd = gru + mlp + lin
    return int(2 * bs * 3 * fwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--ref-iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=1000)
    ap.add_argument("--run-iters", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=["ref", "step", "run"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    res = {"workload": "NeuralLaplaceModel training step, cartpole d=5 h=128 S=17 B=4, float64", "device": torch.cuda.get_device_name(0),
           "batches": {}}
    for bs in args.batches:
        r = {"flops_per_iter": flops_per_iter(bs)}
        if args.only in (None, "ref"):
            r["ref_it_s"] = time_ref(bs, args.ref_iters, args.warmup)
        if args.only in (None, "step"):
            r["step_it_s"] = time_step(bs, args.step_iters, args.warmup)
        if args.only in (None, "run"):
            r["run_it_s"] = time_run(bs, args.run_iters, args.warmup)
            r["run_iters"] = args.run_iters
        if "ref_it_s" in r:
            for k in ("step", "run"):
                if f"{k}_it_s" in r:
                    r[f"{k}_over_ref"] = r[f"{k}_it_s"] / r["ref_it_s"]
        res["batches"][str(bs)] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
