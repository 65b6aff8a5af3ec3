"""The reference's expert-data collector on the device (``mppi_dataset_collector.py:33-321, 324-443``).

The reference collects ``collect_expert_samples = 1e6`` transitions per (env, delay): 5 000 episodes of 200 control steps,
one episode per worker process.  Each step integrates the env over an irregular interval (``ts_grid="exp"``,
``base_env.py:112-120``), adds uniform noise to the expert's command and clips it (``:250-254``), can add Gaussian
observation noise (``:209-210``), and records ``(s0, a0, sn, ts)`` -- the ``bs0, ba0, bsn, bts`` every trainer here
consumes.  :class:`ExpertCollector` runs that step for E envs with one HIP launch (``nlc_collect_step``) next to a
:class:`~neurallaplacecontrol_amd.BatchedMPPIDelay`, so collect -> train -> evaluate never leaves the GPU::

    s0, a0, sn, ts = collect_expert_dataset("oderl-cartpole", action_delay=2, collect_samples=1e6, num_envs=256)
    trainer.run(s0, a0, sn, ts, permutation, batch_size)      # the trainers form the target sn - s0 themselves

The collector's own randomness is keyed by the global episode index: the kernel's draws are counter-based (Philox keyed by
``seed``, counter = (global episode, step, stream)) and episode g starts from the first draw of ``RandomState(seed + g)``.
So with given actions, or with ``policy="random"``, a dataset does not depend on ``num_envs`` or on how the episodes are
batched, and collectors on several GPUs only need disjoint ``episode_base`` ranges.  A planner's own sampling noise is
drawn per batch, so an expert dataset does depend on the batching.  docs/collector.md has the layout and what differs
from the reference by construction.
"""

import ctypes as C
import os

import torch

from . import _lib
from .env_loop import BatchedEnv, _same_cost_branch
from .envs import ENV_DIMS, EnvCost, NLDynamics, OracleDynamics, noise_sigma

__all__ = ["ExpertCollector", "collect_expert_dataset", "replay_buffer_file_name"]


def replay_buffer_file_name(env_name, action_delay, model_name="oracle", encode_obs_time=False, action_buffer_size=4,
                            ts_grid="exp", random_action_noise=1.0, observation_noise=0.0, friction=False):
    """The reference's replay-buffer file name (``mppi_dataset_collector.py:354-359``)."""
    return (
        f"replay_buffer_env-name-{env_name}_delay-{action_delay}_model-name-{model_name}"
        f"_encode-obs-time-{encode_obs_time}_action-buffer-size-{action_buffer_size}_ts-grid-{ts_grid}_"
        f"random-action-noise-{random_action_noise}_"
        f"observation-noise-{observation_noise}_friction-{friction}.pt"
    )


class ExpertDataset(tuple):
    """``(s0, a0, sn, ts)`` as ``collect_expert_dataset`` returns it; ``returns`` holds the episodes' total rewards."""

    returns = None


class _Storage:
    """The dataset on the device: rows of ``steps_per_episode`` per episode, episode-major.  Collectors that fill disjoint
    episode ranges of one dataset share one of these."""

    def __init__(self, nx, B, W, steps_per_episode, device):
        self.nx, self.B, self.W, self.spe, self.device = nx, B, W, steps_per_episode, device
        self.capacity = 0  # episodes the tensors hold
        self.episodes = 0  # episodes written (high-water mark)
        self.s0 = self.a0 = self.sn = self.ts = self.returns = None

    def reserve(self, episodes):
        if episodes <= self.capacity:
            return
        mk = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.device)  # noqa: E731
        rows = episodes * self.spe
        new = dict(s0=mk(rows, self.nx), a0=mk(rows, self.B, self.W), sn=mk(rows, self.nx), ts=mk(rows), returns=mk(episodes))
        for k, t in new.items():
            old = getattr(self, k)
            if old is not None:
                t[: old.shape[0]] = old
            setattr(self, k, t)
        self.capacity = episodes


class ExpertCollector:
    """E envs of the collector's ``loop()`` side by side (``mppi_dataset_collector.py:224-309``).

    * ``collect_step(actions)``: one launch -- records s0, perturbs and clips the planner's ``actions`` (E, nu), rolls the
      action buffers, draws the intervals, integrates, adds the observation noise and records a0, sn, ts
    * ``run_episodes(n_batches)``: ``n_batches`` x E whole episodes with ``planner`` (or the random policy); no host
      synchronisation inside the step loop
    * ``dataset()`` -> ``(s0 (N, nx), a0 (N, B, nu [+ 1]), sn (N, nx), ts (N, 1))`` float64 device tensors of the episodes
      written so far; ``returns`` their total rewards

    ``random_action_noise=None`` is the reference's ``None``: no noise and no clip.  ``policy="random"`` is
    ``model_name == "random"`` (``:255-256``).  ``episode_base`` is the global index of this collector's first episode; a
    draw of the kernel depends only on (seed, global episode, step), and episode g resets from the first draw of
    ``RandomState(seed + g)``, whichever batch and lane run it."""

    def __init__(self, env_name, action_delay, num_envs, *, dt=0.05, ts_grid="exp", random_action_noise=1.0,
                 observation_noise=0.0, friction=False, encode_obs_time=False, action_buffer_size=4, steps_per_episode=200,
                 policy="planner", planner=None, seed=0, device=None, episode_base=0, storage=None,
                 state_constraint=False, change_goal=False):
        # the reference collector's two experiment flags (mppi_dataset_collector.py:45-46, 137-156): they select the branch of
        # the PLANNER's running cost; the recorded reward stays the env's own (integrate_system, base_env.py:164)
        self.cost = EnvCost(env_name, state_constraint=state_constraint, change_goal=change_goal)
        if planner is not None and not _same_cost_branch(getattr(planner, "running_cost", None), self.cost):
            raise ValueError("the planner's running cost is not the EnvCost of state_constraint / change_goal given here")
        self.episode_base = int(episode_base)
        # env e starts global episode episode_base + e from that episode's own reset stream (reset() re-keys per batch)
        self.env = BatchedEnv(env_name, num_envs, dt=dt, action_delay=action_delay, action_buffer_size=action_buffer_size,
                              friction=friction, device=device, seed=int(seed) + self.episode_base)
        self.env_name, self.E, self.device, self.ctx = env_name, self.env.E, self.env.device, self.env.ctx
        self.dt, self.delay, self.B = float(dt), int(action_delay), int(action_buffer_size)
        self.nx, self.nu, self.action_high = ENV_DIMS[env_name]
        self.action_low = -self.action_high
        self.ts_grid, self.policy = ts_grid, policy
        self.random_action_noise = None if random_action_noise is None else float(random_action_noise)
        self.observation_noise = float(observation_noise)
        self.friction, self.encode_obs_time = bool(friction), bool(encode_obs_time)
        self.W = self.nu + int(self.encode_obs_time)
        self.steps_per_episode = int(steps_per_episode)
        if self.steps_per_episode < 1:
            raise ValueError("steps_per_episode must be >= 1")
        self.planner, self.seed = planner, int(seed)
        if self.encode_obs_time:
            self.action_buffer = torch.zeros(self.E, self.B, self.W, dtype=torch.float64, device=self.device)
        else:
            self.action_buffer = self.env.action_buffer
        self._ret = torch.zeros(self.E, dtype=torch.float64, device=self.device)
        self.storage = storage if storage is not None else _Storage(self.nx, self.B, self.W, self.steps_per_episode, self.device)
        if (self.storage.nx, self.storage.B, self.storage.W, self.storage.spe) != (self.nx, self.B, self.W, self.steps_per_episode):
            raise ValueError("shared storage has another row shape")
        self._it = 0
        self._reset_buffers()  # (the BatchedEnv constructor has drawn the first reset state)

    # ------------------------------------------------------------------ state
    @property
    def state(self):
        return self.env.state

    def reset(self):
        """``env.reset()`` for every env (plain reset, as ``loop()`` calls it: no harness start state), the initial action
        buffer (``:231-235``) and a zero episode return; the next ``collect_step`` is step 0.  Env e starts global episode
        ``episode_base + e`` from the first draw of ``RandomState(seed + episode_base + e)``."""
        for e, rng in enumerate(self.env._rngs):  # (re-seeded in place: the stream of RandomState(seed + g), cheaply)
            rng.seed((self.seed + self.episode_base + e) % 2**32)  # (as BatchedEnv.seed: RandomState seeds are 32-bit)
        self.env.reset(harness_start=False)
        self._reset_buffers()
        return self.env.get_obs()

    def _reset_buffers(self):
        self.action_buffer.zero_()
        if self.encode_obs_time:
            tcol = torch.flip(torch.arange(self.B, device=self.device), (0,)).to(torch.float64) * self.dt
            self.action_buffer[:, :, self.nu] = tcol
        self._ret.zero_()
        self._it = 0

    def _desc(self, **over):
        f = dict(
            env=_lib.ENV_IDS[self.env_name], friction=int(self.friction), dt=self.dt, delay=self.delay, B=self.B, E=self.E,
            nu=self.nu, time_channel=int(self.encode_obs_time), ts_grid=_lib.TS_GRIDS.get(self.ts_grid, -1),
            policy=_lib.POLICIES.get(self.policy, -1),
            action_noise=-1.0 if self.random_action_noise is None else self.random_action_noise,
            obs_noise=self.observation_noise, action_low=self.action_low, action_high=self.action_high,
            steps_per_episode=self.steps_per_episode, seed=self.seed,
        )
        f.update(over)
        return _lib.CollectDesc(**f)

    def _launch(self, desc, actions, it=None):
        st = self.storage
        self.ctx.launch(
            self.ctx.lib.nlc_collect_step, C.byref(desc), self._it if it is None else int(it), self.episode_base,
            _lib.ptr(self.env.state), _lib.ptr(self.action_buffer), _lib.ptr(actions), _lib.ptr(self._ret), _lib.ptr(st.s0),
            _lib.ptr(st.a0), _lib.ptr(st.sn), _lib.ptr(st.ts),
        )

    def collect_step(self, actions=None):
        """One control step of every env, recorded as dataset rows ``(episode_base + e) * steps_per_episode + it``.
        ``actions``: the planner's commands (E, nu); ``None`` with ``policy="random"``."""
        if self._it >= self.steps_per_episode:
            raise RuntimeError("the episodes are complete: call reset() (or run_episodes) before the next collect_step")
        self.storage.reserve(self.episode_base + self.E)
        act = None
        if actions is not None:
            act = torch.as_tensor(actions).detach().to(self.device, torch.float64).reshape(self.E, self.nu).contiguous()
        self._launch(self._desc(), act)
        self._it += 1
        self.env.time_step += 1
        if self._it == self.steps_per_episode:
            self.storage.returns[self.episode_base : self.episode_base + self.E] = self._ret
            self.storage.episodes = max(self.storage.episodes, self.episode_base + self.E)

    def _command(self, obs):
        ab = self.action_buffer
        if self.encode_obs_time and not getattr(self.planner, "encode_obs_time", False):
            ab = ab[..., : self.nu]
        if getattr(self.planner, "E", 1) == 1:  # a single MPPIDelay plans the one episode
            return self.planner.command(obs[0], ab[0]).reshape(1, self.nu)
        return self.planner.command(obs, ab)

    def run_episodes(self, n_batches=1):
        """``n_batches`` batches of E whole episodes, appended to the dataset; advances ``episode_base`` by E per batch.
        Each batch starts from ``reset()`` (and ``planner.reset()``, ``:238-240``)."""
        if self.policy == "planner" and self.planner is None:
            raise ValueError("policy='planner' needs a planner")
        self.storage.reserve(self.episode_base + int(n_batches) * self.E)
        with torch.no_grad():
            for b in range(int(n_batches)):
                obs = self.reset()
                if self.planner is not None:
                    self.planner.reset()
                for _ in range(self.steps_per_episode):
                    self.collect_step(self._command(obs) if self.policy == "planner" else None)
                    obs = self.env.get_obs()
                self.episode_base += self.E
                self._it = self.steps_per_episode  # the next batch (or call) starts from a reset
        return self

    # ------------------------------------------------------------------ results
    def dataset(self):
        st, n = self.storage, self.storage.episodes * self.steps_per_episode
        if st.s0 is None:
            raise RuntimeError("nothing collected yet")
        return st.s0[:n], st.a0[:n], st.sn[:n], st.ts[:n].view(-1, 1)

    @property
    def returns(self):
        return self.storage.returns[: self.storage.episodes]


def _model_name(policy, dynamics):
    """The reference's ``model_name`` of what plans (``run_exp_multi.py:19``), which its file name carries."""
    if policy == "random":
        return "random"
    if isinstance(dynamics, str):
        return dynamics
    model = dynamics.model if isinstance(dynamics, NLDynamics) else dynamics
    names = {_lib.DYN_NL: "nl", _lib.DYN_DTRNN: "delta_t_rnn", _lib.DYN_NODE: "node"}
    if getattr(model, "_dyn_id", None) not in names:
        raise ValueError("save_path: pass model_name for a model that is none of the reference's kinds")
    return names[model._dyn_id]


def _make_planner(env_name, action_delay, num_envs, dynamics, roll_outs, time_steps, lambda_, sigma, dt, friction,
                  encode_obs_time, seed, device, cost=None):
    """The collector's planner (``mppi_dataset_collector.py:69-74, 166-180``) over ``num_envs`` episodes; ``cost``: its
    running cost (default: the env's plain ``EnvCost``)."""
    from .planners.mppi_batch import BatchedMPPIDelay
    from .planners.mppi_delay import MPPIDelay

    nx, nu, high = ENV_DIMS[env_name]
    if isinstance(dynamics, str):
        if dynamics != "oracle":
            raise ValueError("dynamics must be 'oracle' or a model")
        dyn = OracleDynamics(env_name, dt, action_delay, friction)
    else:
        dyn = dynamics if isinstance(dynamics, NLDynamics) else NLDynamics(dynamics, dt)
    # the time-stamp column: a planner with oracle dynamics drops it itself; a model's planner is handed the action columns
    # (ExpertCollector._command), and NLDynamics gives an encode_obs_time model the evaluation harness's constant channel
    # B-1 .. 0 (mppi_with_model.py:110-119) -- see docs/collector.md
    enc = bool(encode_obs_time) and isinstance(dyn, OracleDynamics)
    kw = dict(lambda_=lambda_, u_min=torch.tensor(-high), u_max=torch.tensor(high), u_scale=high, encode_obs_time=enc, dt=dt,
              noise_rng="philox", seed=seed, store_rollouts=False)
    sig = noise_sigma(nu, sigma)
    dev = str(device)
    cost = cost if cost is not None else EnvCost(env_name)
    if num_envs == 1:
        return MPPIDelay(dyn, cost, nx, sig, roll_outs, time_steps, dev, **kw)
    return BatchedMPPIDelay(dyn, cost, nx, sig, num_envs, roll_outs, time_steps, dev, **kw)


def collect_expert_dataset(env_name, action_delay, collect_samples=1e6, roll_outs=1000, time_steps=40, lambda_=1.0,
                           sigma=1.0, dt=0.05, num_envs=256, dynamics="oracle", save_path=None, model_name=None,
                           **collector_kwargs):
    """``mppi_with_model_collect_data`` (``mppi_dataset_collector.py:324-443``): ``int(collect_samples / steps_per_episode)``
    episodes of the MPPI expert -- ``dynamics="oracle"`` or a trained model -- in batches of ``num_envs``; a short last
    batch gets a planner of its own size.  Returns ``(s0, a0, sn, ts)`` on the device (a tuple whose ``returns``
    attribute holds the per-episode total rewards).  With ``save_path`` (a directory)
    the tuple is also written there as CPU tensors under the reference's file name, which the reference's
    ``load_expert_irregular_data_delay_time_multi`` reads; the name carries ``model_name``, by default that of the
    dynamics' kind ("oracle", "random", "nl", "delta_t_rnn", "node").  ``collector_kwargs`` go to :class:`ExpertCollector`,
    ``state_constraint`` / ``change_goal`` (the reference's names, ``:45-46``) among them: the expert then plans with that
    branch of the cartpole running cost.  The reference collector's loop never flips the goal (``:242-244`` assign a local)."""
    kw = dict(collector_kwargs)
    spe = int(kw.get("steps_per_episode", 200))
    seed = int(kw.pop("seed", 0))
    policy = kw.get("policy", "planner")
    friction, enc = bool(kw.get("friction", False)), bool(kw.get("encode_obs_time", False))
    total = int(collect_samples / spe)
    if total < 1:
        raise ValueError("collect_samples is less than one episode")
    if save_path is not None:  # (named before the collection: an unnamed model is refused before any work)
        file_name = replay_buffer_file_name(
            env_name, action_delay, model_name if model_name is not None else _model_name(policy, dynamics), enc,
            int(kw.get("action_buffer_size", 4)), kw.get("ts_grid", "exp"), kw.get("random_action_noise", 1.0),
            kw.get("observation_noise", 0.0), friction)
    E = min(int(num_envs), total)
    n_full, rem = divmod(total, E)
    main = None
    for n_batches, size, base in ((n_full, E, 0), (1 if rem else 0, rem, n_full * E)):
        if n_batches == 0:
            continue
        col = ExpertCollector(env_name, action_delay, size, dt=dt, seed=seed, episode_base=base,
                              storage=None if main is None else main.storage, **kw)
        if policy == "planner":
            col.planner = _make_planner(env_name, action_delay, size, dynamics, roll_outs, time_steps, lambda_, sigma, dt,
                                        friction, enc, seed + base, col.device, cost=col.cost)
        if main is None:
            main = col
            main.storage.reserve(total)
        col.run_episodes(n_batches)
    data = main.dataset()
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
        torch.save(tuple(t.cpu() for t in data), os.path.join(save_path, file_name))
    out = ExpertDataset(data)
    out.returns = main.returns
    return out
