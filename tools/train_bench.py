"""Training-step throughput on cartpole of NeuralLaplaceModel (d = 5, h = 128, S = 17, B = 4; --model nl, the default), of
the DeltaTRNN baseline (d = 5, H = 160, B = 4; --model delta_t_rnn, RNNTrainer) or of the NODE baseline (d = 5, augment 1,
H = 270; --model node, NODETrainer; give it --batches 1 16: the reference trains NODE at batch 1, train_utils.py:319-320, and
every variant is then timed --repeats times, median and min .. max), one JSON line:

  (a) the reference's iteration (train_utils.py:391-408) through the existing grad-mode model(...): forward, MSELoss,
      backward, clip_grad_norm_(0.1), torch.optim.Adam.step(), loss.item() every iteration;
  (b) NLTrainer.step() with loss.item() every iteration;
  (c) NLTrainer.run() over a permutation of --run-iters iterations (one host read at the end).

Every variant runs a warm-up first and every timing ends with torch.cuda.synchronize().  Iterations / s per variant and the
ratios (b) / (a), (c) / (a) at each batch size.  `--only run --run-iters 200` is the shape for a rocprofv3 kernel trace.
Each (batch size, variant) measurement is a child process of its own under --step-timeout seconds; the first one that fails or
runs out of time ends the tool (nothing more is started on the GPU).  `--kernel-ms` adds the mean time of each kernel of the
fused step from the library's event profiling (200 step()s).  `--ilt-algorithm fixed_tablot|stehfest` (with `--terms S`)
times the NL model under one of the linear ILT algorithms instead of the Fourier series; the grad-mode reference (a) is then
that algorithm's grad-mode path, and the result records both settings.

`--group M [M ...]` measures grouped training instead (NLTrainerGroup / RNNTrainerGroup, run_exp_multi.py:105-110): for both
families and every M, run() of a group of M differently seeded models at the first --batches size (16) over one shared
dataset with a permutation per member; a warm-up run, then --repeats timed runs of --run-iters iterations in one child
process per (family, M).  Per M: iterations / s (median and the min .. max spread over the repeats) and the aggregate
member-iterations / s = M x that; M = 1 is timed twice, as the group class and as this commit's single trainer.
`--parent-tree DIR` names a built checkout of the parent commit (git worktree + its build()): the tool then times that tree's
own `tools/train_bench.py --only run` --repeats times per family between this commit's measurements, in the same session, and
records `parent_single`, `m1_over_parent` (M = 1 of this commit against it) and `aggregate_over_parent` per M.  Writes
profiles/train_bench_group.json unless --out says otherwise.

    python tools/train_bench.py [--model nl|delta_t_rnn] [--ilt-algorithm fourier] [--terms 17] [--batches 16 256] [--ref-iters 200] [--step-iters 1000] [--run-iters 10000] [--out FILE]
    python tools/train_bench.py --group 1 8 64 256 [--repeats 3] [--run-iters 10000] [--parent-tree DIR]

`--evaluate` times the held-out loss instead (``evaluate``, overlay.py:112-115): both families at N = 256 and N = 156 250 (the
reference's validation set at samples_per_dim = 5: 50 x 5 x 5^4 rows), one warm-up and --repeats timed calls each (median
and min .. max, ms), beside (a) ``loss_and_grad`` on the same rows, (b) ``model(...)`` under ``no_grad`` + ``mse_loss`` after a
parameter change (so the inference path's weight re-upload is inside), and (c) for groups of --group members (default 1 8
64) at N = 256, the group's one ``evaluate`` against the loop of M single calls.  One child process per family under
--step-timeout; writes profiles/train_eval_bench.json unless --out says otherwise.

    python tools/train_bench.py --evaluate [--group 1 8 64] [--repeats 3]

`--fit` times the validated loop (``fit``: ``run`` + ``evaluate`` + ``keep_best`` per slice, train_utils.py:345-468): both
families, the single trainer and groups of --group members (default 1 8 64), batch 16, --eval-every 100, --fit-iters 2000, a
validation set of 256 rows; (a) ``fit`` and (b) the host loop it replaces (a read of the criteria at every check, ``clone()``
of a member's parameters on improvement), one warm-up and --repeats timed runs each (median and min .. max, ms).  Also
nlc_train_keep_best alone at the family's parameter count: 100 enqueued calls ended by one synchronise, with every member
improving at every call and with none.  One child process per (family, M) under --step-timeout; writes
profiles/train_select_bench.json unless --out says otherwise.

    python tools/train_bench.py --fit [--group 1 8 64] [--repeats 3] [--fit-iters 2000] [--eval-every 100]

`--members` times per-member settings: run() at the first --batches size (16) over --run-iters iterations of a group of
--group members (default 64) built with a learning rate per member (the library's ``_members`` step) against the same group
with one learning rate (the step it has always called), both families (--model node: that family), the two variants taking
turns in one child process per family: a warm-up run of --warmup iterations each, then --repeats timed runs each (median and
min .. max, iterations / s).  Writes profiles/train_members_bench.json unless --out says otherwise.

    python tools/train_bench.py --members [--group 64] [--repeats 3] [--run-iters 10000]

`--ilt-algorithm dehoog` times a de Hoog NL model (tamed weights, a narrow band of short times).  Only the grad-mode path
(`--only ref`) can be timed without `--dehoog-fused`, which builds the trainers with ``dehoog="fused"``.  With `--group` the NL
family alone is measured, every timed run in a child process of its own after that child's warm-up run: first (a) --repeats
times, then run() of the single trainer and of each group size --repeats times; per M also member-iterations / s over (a).
Writes profiles/train_bench_dehoog.json unless --out says otherwise.

    python tools/train_bench.py --ilt-algorithm dehoog --terms 33 --dehoog-fused --batches 16 --group 1 8 64 [--run-iters 1000]
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import neurallaplacecontrol_amd as nlc  # noqa: E402
from oracle import nl_model as onl  # noqa: E402

ENV, D, NU, H, S, B = "oderl-cartpole", 5, 1, 128, 17, 4
RNN_H = 160  # rnn_hidden_units, config.py:43
NODE_H, NODE_AUG = 270, 1  # node_hidden_units, node_augment_dim, config.py:41-42
NODE_METHOD = "euler"  # --node-method: the NODE's fixed-grid solver
MODEL = "nl"
ILT = "fourier"  # --ilt-algorithm (NL model)
DEHOOG_FUSED = False  # --dehoog-fused: NL trainers are built with dehoog="fused"
WORKLOADS = {"nl": "NeuralLaplaceModel training step, cartpole d=5 h=128 S=17 B=4, float64",
             "delta_t_rnn": "DeltaTRNN training step, cartpole d=5 H=160 B=4, float64",
             "node": "NODE training step, cartpole d=5 augment=1 H=270 (Euler, step 0.05, normalize_time), float64"}
TRAINERS = {"nl": ("NLTrainer", "NLTrainerGroup"), "delta_t_rnn": ("RNNTrainer", "RNNTrainerGroup"),
            "node": ("NODETrainer", "NODETrainerGroup")}


def trainer_kw():
    return {"dehoog": "fused"} if MODEL == "nl" and DEHOOG_FUSED else {}


def make_trainer(model):
    tr = getattr(nlc, TRAINERS[MODEL][0])(model, **trainer_kw())
    assert tr.fused, "the benchmark times the fused step"
    return tr


def make_model(seed=0):
    st = onl.ENV_STATS[ENV]
    if MODEL == "delta_t_rnn":
        from oracle import rnn_model as orn

        sd = orn.make_synthetic_state_dict(seed, D, NU, RNN_H, st["state_std"], [st["act_high"] / 2])
        m = nlc.DeltaTRNN(D, NU, hidden_units=RNN_H, state_mean=np.zeros(D), state_std=np.ones(D), action_mean=np.array([0]),
                          action_std=np.array([1.0]), normalize=True, normalize_time=True).double()
        m.load_state_dict(sd)
        return m.to("cuda")
    if MODEL == "node":
        from oracle import node_model as ond

        sd = ond.make_synthetic_state_dict(seed, D, NU, NODE_H, NODE_AUG, st["state_std"], None)
        m = nlc.NODE(D, NU, D, hidden_units=NODE_H, state_mean=np.zeros(D), state_std=np.ones(D), action_mean=np.array([0]),
                     action_std=np.array([1.0]), normalize=True, normalize_time=True, augment_dim=NODE_AUG,
                     method=NODE_METHOD).double()
        m.load_state_dict(sd)
        return m.to("cuda")
    # (de Hoog: weights whose terms sample a transform -- the table is ill-conditioned on a random network's)
    sd = onl.make_synthetic_state_dict(seed, D, NU, H, S, st["state_std"], [st["act_high"] / 2],
                                       tame="dehoog" if ILT == "dehoog" else True)
    m = nlc.NeuralLaplaceModel(D, NU, D, hidden_units=H, s_recon_terms=S, ilt_algorithm=ILT, state_mean=np.zeros(D),
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
    if MODEL == "nl" and ILT == "dehoog":  # a narrow band of short times (5e-3 .. 7.5e-3 before the model's normalisation)
        ts = (torch.rand(M, 1, dtype=torch.float64, generator=g) * 0.05 + 0.1) * 0.05
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
    tr = make_trainer(make_model())
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
    tr = make_trainer(make_model())
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


def time_group(bs, iters, warm, M, repeats):
    """run() of a group of M (M = 0: the single trainer) over one shared dataset, a permutation per member: iterations / s of
    each of `repeats` timed runs after one warm-up run of `warm` iterations."""
    s0, a0, sn, ts = dataset(bs * iters)
    n = max(M, 1)
    perms = torch.stack([torch.randperm(s0.shape[0], generator=torch.Generator().manual_seed(i)) for i in range(n)]).cuda()
    models = [make_model(seed=i) for i in range(n)]
    if M == 0:
        tr, perms = make_trainer(models[0]), perms[0]
    else:
        tr = getattr(nlc, TRAINERS[MODEL][1])(models, **trainer_kw())
    assert tr.fused
    tr.run(s0, a0, sn, ts, perms[..., : bs * warm], batch_size=bs)
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        losses = tr.run(s0, a0, sn, ts, perms, batch_size=bs)
        torch.cuda.synchronize()
        out.append(iters / (time.perf_counter() - t0))
        assert bool(torch.isfinite(losses).all())
    return out


def time_members(bs, iters, warm, M, repeats):
    """run() of two groups of the same M models over one shared dataset, a permutation per member: one with a learning rate
    per member (all equal to the other's, so the two do the same arithmetic), one with a number.  Iterations / s of `repeats`
    timed runs each, taken in turns, after a warm-up run of `warm` iterations each."""
    import copy

    s0, a0, sn, ts = dataset(bs * iters)
    perms = torch.stack([torch.randperm(s0.shape[0], generator=torch.Generator().manual_seed(i)) for i in range(M)]).cuda()
    models = [make_model(seed=i) for i in range(M)]
    Group = getattr(nlc, TRAINERS[MODEL][1])
    groups = {"scalar": Group([copy.deepcopy(m) for m in models], lr=1e-4), "members": Group(models, lr=[1e-4] * M)}
    assert groups["members"]._per_member() and not groups["scalar"]._per_member()
    out = {k: [] for k in groups}
    for tr in groups.values():
        assert tr.fused
        tr.run(s0, a0, sn, ts, perms[..., : bs * warm], batch_size=bs)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, tr in groups.items():
            t0 = time.perf_counter()
            losses = tr.run(s0, a0, sn, ts, perms, batch_size=bs)
            torch.cuda.synchronize()
            out[k].append(iters / (time.perf_counter() - t0))
            assert bool(torch.isfinite(losses).all())
    return out


def kernel_ms(bs, iters=200, warm=20):
    """Mean milliseconds per launch of each kernel of step() (the library's event pairs around every launch)."""
    tr = make_trainer(make_model())
    s0, a0, sn, ts = dataset(bs)
    for _ in range(warm):
        tr.step(s0, a0, ts, sn - s0)
    torch.cuda.synchronize()
    tr._ctx.profile(True)
    tr._ctx.profile_reset()
    for _ in range(iters):
        tr.step(s0, a0, ts, sn - s0)
    torch.cuda.synchronize()
    out = {k: v["total_ms"] / max(v["launches"], 1) for k, v in tr._ctx.profile_read().items()}
    tr._ctx.profile(False)
    return out


def _timed(fn, repeats):
    """One warm-up, then `repeats` timed calls, each ended by a synchronise: median, min and max in ms."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def time_evaluate(sizes, groups, repeats):
    """The --evaluate measurements of the family MODEL names."""
    Single, Group = (nlc.RNNTrainer, nlc.RNNTrainerGroup) if MODEL == "delta_t_rnn" else (nlc.NLTrainer, nlc.NLTrainerGroup)
    res = {"workload": WORKLOADS[MODEL].replace("training step", "held-out loss"), "sizes": {}, "groups": {}}
    model = make_model()
    tr = make_trainer(model)
    first = next(model.parameters())
    for N in sizes:
        s0, a0, sn, ts = dataset(N)
        tgt = sn - s0

        def forward_after_a_change():
            with torch.no_grad():
                first.mul_(1.0)  # the version moves: the inference path packs and uploads the weights again
                return torch.nn.functional.mse_loss(model(s0, a0, ts).squeeze(), tgt.squeeze())

        res["sizes"][str(N)] = {"evaluate": _timed(lambda: tr.evaluate(s0, a0, ts, tgt), repeats),
                                "loss_and_grad": _timed(lambda: tr.loss_and_grad(s0, a0, ts, tgt), repeats),
                                "no_grad_forward_mse": _timed(forward_after_a_change, repeats)}
    s0, a0, sn, ts = dataset(sizes[0])
    tgt = sn - s0
    for M in groups:
        models = [make_model(seed=i) for i in range(M)]
        grp = Group(models)
        singles = [Single(m) for m in models]
        res["groups"][str(M)] = {"N": sizes[0], "group_evaluate": _timed(lambda: grp.evaluate(s0, a0, ts, tgt), repeats),
                                 "loop_of_singles": _timed(lambda: [t.evaluate(s0, a0, ts, tgt) for t in singles], repeats)}
    return res


def time_fit(M, iters, every, repeats, val_rows=256, bs=16):
    """The --fit measurements of the family MODEL names at M members (1: the single trainer): ``fit`` against the host loop
    a user writes without it, and nlc_train_keep_best alone."""
    import ctypes as C

    Group = nlc.RNNTrainerGroup if MODEL == "delta_t_rnn" else nlc.NLTrainerGroup
    models = [make_model(seed=i) for i in range(M)]
    tr = make_trainer(models[0]) if M == 1 else Group(models)
    assert tr.fused
    R = iters * bs
    data = dataset(R)
    vs0, va0, vsn, vts = dataset(val_rows, seed=1)
    val = (vs0, va0, vts, vsn - vs0)

    def host_loop():
        """``.item()`` (one read of the M criteria) at every check, ``clone()`` of a member's parameters on improvement."""
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)
        perm = torch.randperm(R, device="cuda", generator=gen)
        best, kept = [float("inf")] * M, [None] * M
        for chunk in perm.split(every * bs):
            if chunk.numel() < bs:
                continue
            tr.run(*data, chunk, bs)
            crit = tr.evaluate(*val).reshape(-1).tolist()
            for m, c in enumerate(crit):
                if c < best[m]:
                    best[m], kept[m] = c, [p.detach().clone() for p in tr.models[m].parameters()]
        with torch.no_grad():
            for m, ps in enumerate(kept):
                for p, q in zip(tr.models[m].parameters(), ps or ()):
                    p.copy_(q)

    res = {"M": M, "iters": iters, "eval_every": every, "batch": bs, "val_rows": val_rows, "P": int(tr._flat.shape[1]),
           "fit": _timed(lambda: tr.fit(data, val, epochs=1, batch_size=bs, eval_every=every, seed=0), repeats),
           "host_loop": _timed(host_loop, repeats)}
    # the entry alone: 100 enqueued calls ended by one synchronise (inside _timed), every member improving at every call
    # (a falling loss), and none (+inf)
    P, ctx, calls = res["P"], tr._ctx, 100
    flat = torch.randn(M, P, dtype=torch.float64, device="cuda")
    best = torch.empty_like(flat)
    best_loss = torch.empty(M, dtype=torch.float64, device="cuda")
    best_tag = torch.empty(M, dtype=torch.int64, device="cuda")
    improved = torch.empty(M, dtype=torch.int32, device="cuda")
    falling = torch.arange(calls, 0, -1, dtype=torch.float64, device="cuda").repeat_interleave(M).contiguous()  # [calls][M]
    never = torch.full((calls * M,), float("inf"), dtype=torch.float64, device="cuda")

    def keep(losses):
        best_loss.fill_(float("inf"))
        with ctx.stream():
            for k in range(calls):
                ctx.check(ctx.lib.nlc_train_keep_best(
                    ctx.h, M, P, C.c_void_p(losses.data_ptr() + 8 * k * M), C.c_void_p(flat.data_ptr()),
                    C.c_void_p(best_loss.data_ptr()), C.c_void_p(best.data_ptr()), C.c_void_p(best_tag.data_ptr()), k,
                    C.c_void_p(improved.data_ptr())))

    res["keep_best_100_calls"] = {"all_improve": _timed(lambda: keep(falling), repeats), "none_improves": _timed(lambda: keep(never), repeats),
                                  "bytes_copied_per_call_all_improve": 2 * 8 * M * P}
    return res


def flops_per_iter(bs):
    """Multiply-adds x 2 of the dense products (forward + the two backward products per weight matrix); transcendentals
    and element-wise work not counted."""
    if MODEL == "delta_t_rnn":
        return int(2 * bs * 3 * (B * 3 * RNN_H * (NU + RNN_H) + D * (RNN_H + D + 1)))
    if MODEL == "node":  # at the fixed grid's 3 sub-steps (ts = dt under normalize_time)
        dy = D + NODE_AUG
        return int(2 * bs * 3 * 3 * (NODE_H * (dy + NU) + NODE_H * NODE_H + dy * NODE_H))
    g, K0, O = H // 2, 2 * S + D + 2, 2 * D * S
    gru = B * (3 * g * (NU + g) + 3 * g * (g + g))  # both layers, per row per window
    mlp = K0 * H + H * H + H * O
    lin = 2 * g
    fwd = gru + mlp + lin
    return int(2 * bs * 3 * fwd)


def main():
    global MODEL, ILT, S, DEHOOG_FUSED, NODE_METHOD
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--ref-iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=1000)
    ap.add_argument("--run-iters", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=["ref", "step", "run"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", choices=sorted(WORKLOADS), default="nl")
    ap.add_argument("--ilt-algorithm", choices=["fourier", "fixed_tablot", "stehfest", "dehoog"], default="fourier",
                    help="--model nl: the ILT algorithm of the model (the fused step has an instance for each of the first three; "
                         "dehoog: with --dehoog-fused)")
    ap.add_argument("--dehoog-fused", action="store_true",
                    help="--ilt-algorithm dehoog: trainers are built with dehoog='fused' (singles and --group); without it only "
                         "the grad-mode path (--only ref) can be timed")
    ap.add_argument("--terms", type=int, default=S, help="--model nl: ilt_reconstruction_terms (stehfest: even, 2 .. 20)")
    ap.add_argument("--kernel-ms", action="store_true")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds each child measurement may take")
    ap.add_argument("--group", type=int, nargs="+", default=None, metavar="M", help="grouped training: members per group")
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per --group measurement")
    ap.add_argument("--parent-tree", default=None, help="--group: a built checkout of the parent commit to time beside this one")
    ap.add_argument("--evaluate", action="store_true", help="time the held-out loss (evaluate) instead of training")
    ap.add_argument("--eval-sizes", type=int, nargs="+", default=[256, 156250], help="--evaluate: rows per call")
    ap.add_argument("--fit", action="store_true", help="time fit() against the host loop it replaces, and nlc_train_keep_best")
    ap.add_argument("--fit-iters", type=int, default=2000, help="--fit: iterations per timed run (one epoch)")
    ap.add_argument("--eval-every", type=int, default=100, help="--fit: iterations between checks")
    ap.add_argument("--members", action="store_true", help="time a group with per-member learning rates against the scalar group")
    ap.add_argument("--node-method", choices=["euler", "midpoint", "rk4"], default="euler",
                    help="--model node: the fixed-grid solver (profiles/train_bench_node_rk.json: --batches 1 --only run)")
    ap.add_argument("--child", nargs=2, metavar=("BATCH", "VARIANT"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    MODEL, ILT, S, DEHOOG_FUSED = args.model, args.ilt_algorithm, args.terms, args.dehoog_fused
    NODE_METHOD = args.node_method
    if MODEL == "node" and NODE_METHOD != "euler":
        WORKLOADS["node"] = WORKLOADS["node"].replace("Euler", NODE_METHOD)
    if MODEL == "nl" and (ILT, S) != ("fourier", 17):
        WORKLOADS["nl"] = f"NeuralLaplaceModel training step, cartpole d=5 h=128 {ILT} S={S} B=4, float64"
    torch.manual_seed(0)
    if args.child:
        bs, variant = int(args.child[0]), args.child[1]
        if variant == "evaluate":
            print("RESULT " + json.dumps(time_evaluate(args.eval_sizes, args.group or [1, 8, 64], args.repeats)))
            return
        if variant.startswith("fit"):
            print("RESULT " + json.dumps(time_fit(int(variant[3:]), args.fit_iters, args.eval_every, args.repeats)))
            return
        if variant.startswith("members"):
            print("RESULT " + json.dumps(time_members(bs, args.run_iters, args.warmup, int(variant[7:]), args.repeats)))
            return
        if variant.startswith("group"):
            print("RESULT " + json.dumps(time_group(bs, args.run_iters, args.warmup, int(variant[5:]), args.repeats)))
            return
        fn = {"ref": lambda: time_ref(bs, args.ref_iters, args.warmup), "step": lambda: time_step(bs, args.step_iters, args.warmup),
              "run": lambda: time_run(bs, args.run_iters, args.warmup), "kernel_ms": lambda: kernel_ms(bs)}[variant]
        print("RESULT " + json.dumps(fn()))
        return

    def measure(bs, variant, repeats=None):
        cmd = [sys.executable, os.path.abspath(__file__), "--model", MODEL, "--ilt-algorithm", ILT, "--terms", str(S),
               "--ref-iters", str(args.ref_iters), "--step-iters",
               str(args.step_iters), "--run-iters", str(args.run_iters), "--warmup", str(args.warmup), "--repeats",
               str(repeats or args.repeats), *(["--dehoog-fused"] if DEHOOG_FUSED else []),
               *(["--node-method", NODE_METHOD] if NODE_METHOD != "euler" else []), "--child", str(bs), variant]
        out = subprocess.run(cmd, timeout=args.step_timeout, check=True, capture_output=True, text=True).stdout
        return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])

    def spread(runs):
        runs = sorted(runs)
        return {"it_s": runs[len(runs) // 2], "it_s_min": runs[0], "it_s_max": runs[-1]}

    def measure_parent(bs):
        """run() of the parent tree's single trainer through that tree's own tool (its package, its library)."""
        tree = os.path.abspath(args.parent_tree)
        cmd = [sys.executable, os.path.join(tree, "tools", "train_bench.py"), "--model", MODEL, "--batches", str(bs), "--only",
               "run", "--run-iters", str(args.run_iters), "--warmup", str(args.warmup), "--step-timeout", str(args.step_timeout)]
        runs = []
        for _ in range(args.repeats):
            out = subprocess.run(cmd, cwd=tree, timeout=args.step_timeout + 60, check=True, capture_output=True, text=True).stdout
            runs.append(json.loads(out.splitlines()[-1])["batches"][str(bs)]["run_it_s"])
        return spread(runs)

    if args.evaluate:
        res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats}
        for fam in ("nl", "delta_t_rnn"):
            cmd = [sys.executable, os.path.abspath(__file__), "--model", fam, "--repeats", str(args.repeats), "--eval-sizes",
                   *map(str, args.eval_sizes), "--group", *map(str, args.group or [1, 8, 64]), "--child", "0", "evaluate"]
            out = subprocess.run(cmd, timeout=args.step_timeout, check=True, capture_output=True, text=True).stdout
            res[fam] = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(json.dumps(res))
        with open(args.out or os.path.join(REPO, "profiles", "train_eval_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if args.fit:
        res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "families": {}}
        for fam in ("nl", "delta_t_rnn"):
            res["families"][fam] = {"workload": WORKLOADS[fam].replace("training step", "fit"), "groups": {}}
            for M in args.group or [1, 8, 64]:
                cmd = [sys.executable, os.path.abspath(__file__), "--model", fam, "--repeats", str(args.repeats), "--fit-iters",
                       str(args.fit_iters), "--eval-every", str(args.eval_every), "--child", "16", f"fit{M}"]
                out = subprocess.run(cmd, timeout=args.step_timeout, check=True, capture_output=True, text=True).stdout
                r = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
                r["host_loop_over_fit"] =r["host_loop"]["median_ms"] / r["fit"]["median_ms"]
                res["families"][fam]["groups"][str(M)] = r
                print(f"# {fam} M={M}: {r}", file=sys.stderr, flush=True)
        print(json.dumps(res))
        with open(args.out or os.path.join(REPO, "profiles", "train_select_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if args.members:
        bs = args.batches[0]
        res = {"device": torch.cuda.get_device_name(0), "batch": bs, "run_iters": args.run_iters, "repeats": args.repeats,
               "families": {}}
        for MODEL in (["node"] if args.model == "node" else ["delta_t_rnn", "nl"]):
            fam = {"workload": WORKLOADS[MODEL], "groups": {}}
            for M in args.group or [64]:
                r = measure(bs, f"members{M}")
                r = {"scalar": spread(r["scalar"]), "members": spread(r["members"])}
                r["members_over_scalar"] = r["members"]["it_s"] / r["scalar"]["it_s"]
                fam["groups"][str(M)] = r
                print(f"# {MODEL} M={M}: {r}", file=sys.stderr, flush=True)
            res["families"][MODEL] = fam
        print(json.dumps(res))
        with open(args.out or os.path.join(REPO, "profiles", "train_members_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if args.group:
        bs = args.batches[0]
        res = {"device": torch.cuda.get_device_name(0), "batch": bs, "run_iters": args.run_iters, "repeats": args.repeats,
               "families": {}}
        # --model node: that family alone, at its own batch size; else the two families the tool has always timed together
        for MODEL in (["node"] if args.model == "node" else ["nl"] if ILT == "dehoog" else ["delta_t_rnn", "nl"]):
            fam = {"workload": WORKLOADS[MODEL], "groups": {}}
            if ILT == "dehoog":  # the path the fused step replaces, in the same session: a child process per timed run
                fam["grad_mode_ref"] = spread([measure(bs, "ref") for _ in range(args.repeats)])
                print(f"# {MODEL} grad-mode: {fam['grad_mode_ref']}", file=sys.stderr, flush=True)
            for M in [0] + list(args.group):  # 0: the single trainer, in the same session
                # (dehoog: every timed run in a child process of its own, after that child's warm-up run)
                r = spread([measure(bs, f"group{M}", repeats=1)[0] for _ in range(args.repeats)] if ILT == "dehoog"
                           else measure(bs, f"group{M}"))
                if M == 0:
                    fam["single"] = r
                    if args.parent_tree:
                        fam["parent_single"] = measure_parent(bs)
                        print(f"# {MODEL} parent single: {fam['parent_single']}", file=sys.stderr, flush=True)
                else:
                    r["member_it_s"] = M * r["it_s"]
                    r["aggregate_over_single"] = r["member_it_s"] / fam["single"]["it_s"]
                    if "grad_mode_ref" in fam:
                        r["member_it_s_over_grad_mode"] = r["member_it_s"] / fam["grad_mode_ref"]["it_s"]
                    if args.parent_tree:
                        r["aggregate_over_parent"] = r["member_it_s"] / fam["parent_single"]["it_s"]
                        if M == 1:
                            fam["m1_over_parent"] = r["it_s"] / fam["parent_single"]["it_s"]
                    fam["groups"][str(M)] = r
                print(f"# {MODEL} M={M or 'single'}: {r}", file=sys.stderr, flush=True)
            res["families"][MODEL] = fam
        line = json.dumps(res)
        print(line)
        default = ("train_bench_node_group.json" if args.model == "node" else
                   "train_bench_dehoog.json" if ILT == "dehoog" else "train_bench_group.json")
        with open(args.out or os.path.join(REPO, "profiles", default), "w") as f:
            f.write(line + "\n")
        return

    res = {"workload": WORKLOADS[MODEL], "device": torch.cuda.get_device_name(0), "batches": {}}
    if MODEL == "node":
        res["node_method"] = NODE_METHOD
    if MODEL == "nl":
        res["ilt_algorithm"], res["terms"] = ILT, S
    for bs in args.batches:
        r = {"flops_per_iter": flops_per_iter(bs)}

        def timed(variant):
            """One measurement; --model node: --repeats of them (a child process each), the median kept as VARIANT_it_s."""
            if MODEL != "node":
                return measure(bs, variant)
            s = spread([measure(bs, variant) for _ in range(args.repeats)])
            r[f"{variant}_it_s_min"], r[f"{variant}_it_s_max"] = s["it_s_min"], s["it_s_max"]
            return s["it_s"]

        if args.only in (None, "ref"):
            r["ref_it_s"] = timed("ref")
        if args.only in (None, "step"):
            r["step_it_s"] = timed("step")
        if args.only in (None, "run"):
            r["run_it_s"] = timed("run")
            r["run_iters"] = args.run_iters
        if args.kernel_ms:
            r["kernel_ms"] = measure(bs, "kernel_ms")
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
