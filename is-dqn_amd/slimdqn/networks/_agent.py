"""Engine plumbing shared by the agents (iSDQN, DQN, TFDQN): one QNetEngine per batch size, parameter handles, batch
conversion, single-observation forward.  No arithmetic of the hot path lives here."""
from __future__ import annotations

import dataclasses
import typing

import numpy as np
import torch

from slimdqn import _conservative, _hip, _mixture, _optimizer, _projection, _sparsity
from slimdqn._engine import NetOptions, QNetEngine, check_augment, check_noisy, check_redo


class DeviceParams:
    """Handle on the flat device parameter buffer; ``handle["params"]`` gives the Flax-layout pytree (a copy)."""

    def __init__(self, engine: QNetEngine, tensor: torch.Tensor):
        self._engine = engine
        self.tensor = tensor

    @staticmethod
    def _nest(flat):
        out = {}
        for mod, leaves in flat.items():
            node = out
            for part in mod.split("/"):
                node = node.setdefault(part, {})
            node.update(leaves)
        return out

    def to_flax(self):
        """The reference's ``params["params"]`` pytree; nested modules (the impala Stacks) as nested dicts like Flax's."""
        # (the engine's own buffer of a noisy engine: the sigma leaves "sigma_kernel" / "sigma_bias" ride beside kernel / bias)
        return self._nest(self._engine.export_flax(None if self.tensor is self._engine.params else self.tensor))

    def batch_stats(self):
        """Flax's second collection of a BatchNorm network (isdqn.py:87-88): {"BatchNorm_i": {"mean", "var"}} (the impala Stacks'
        own modules nested: {"Stack_0": {"BatchNorm_1": ...}})."""
        return self._nest(self._engine.export_batch_stats(self.tensor))

    def __getitem__(self, key):
        if key == "batch_stats" and self._engine.batch_norm:
            return self.batch_stats()
        if key != "params":
            raise KeyError(key)
        return self.to_flax()

    def clone(self) -> "DeviceParams":
        return DeviceParams(self._engine, self.tensor.clone())

    copy = clone  # the reference's ``self.params.copy()`` (dqn.py:34, 50)


def _is_one_frame_shift(old: np.ndarray, new: np.ndarray) -> bool:
    """new[..., :-1] == old[..., 1:] for (h, w, stack) uint8 stacks.  stack == 4: one pixel's frames are one little-endian
    uint32, so the test is a shift and a mask over contiguous words (a few us; the strided comparison costs ~70 us)."""
    if old.shape[-1] == 4 and old.flags.c_contiguous and new.flags.c_contiguous:
        o, n = old.reshape(-1).view("<u4"), new.reshape(-1).view("<u4")
        return bool(np.array_equal(n & np.uint32(0x00FFFFFF), o >> np.uint32(8)))
    return bool(np.array_equal(new[..., :-1], old[..., 1:]))


def importance_beta(beta_start: float, beta_end, n_steps: int, step: int) -> np.float32:
    """The importance-sampling exponent of gradient step ``step`` (0-based): linear from ``beta_start`` at step 0 to ``beta_end``
    at step ``n_steps``, ``beta_end`` from there on; ``beta_start`` throughout when ``beta_end`` is None.  Host float64
    arithmetic, stored as float32 -- the value the eager and the captured update both hand to the device."""
    if beta_end is None:
        return np.float32(beta_start)
    if step >= n_steps:
        return np.float32(beta_end)
    b0, b1 = np.float64(beta_start), np.float64(beta_end)
    return np.float32(b0 + (b1 - b0) * (np.float64(max(step, 0)) / np.float64(n_steps)))


def horizon_schedule(n_start: int, n_end: int, gamma_start: float, gamma_end: float, period: int, t: int):
    """(update horizon, float32 discount) of gradient step ``t`` (0-based) under the annealing of SR-SPR and BBF: with
    p = min(t / period, 1), n is exponential from ``n_start`` to ``n_end`` and rounded to the nearest integer, and 1 - gamma is
    exponential from 1 - ``gamma_start`` to 1 - ``gamma_end``.  Host float64 arithmetic; at p = 0 and p = 1 exactly the end values."""
    if t <= 0:
        return int(n_start), np.float32(gamma_start)
    if t >= period:
        return int(n_end), np.float32(gamma_end)
    p = np.float64(t) / np.float64(period)
    ln0, ln1 = np.log(np.float64(n_start)), np.log(np.float64(n_end))
    lg0, lg1 = np.log(1.0 - np.float64(gamma_start)), np.log(1.0 - np.float64(gamma_end))
    return int(np.rint(np.exp(ln0 + (ln1 - ln0) * p))), np.float32(1.0 - np.exp(lg0 + (lg1 - lg0) * p))


def recycle_seed(seed: int, k: int) -> int:
    """Seed of the fresh parameters of the agent's k-th recycle (0-based): a child of the agent's seed in numpy's SeedSequence tree,
    never the seed itself (``init_params(seed)`` draws from SeedSequence(seed) with an empty spawn key)."""
    state = np.random.SeedSequence(entropy=int(seed), spawn_key=(1, int(k))).generate_state(4)
    return int.from_bytes(state.tobytes(), "little")


def reset_seed(seed: int, k: int) -> int:
    """Seed of the fresh parameters of the agent's k-th reset (0-based): a child of the agent's seed in numpy's SeedSequence tree under a
    spawn key of its own ((3, k); ``recycle_seed`` has (1, k), ``augment_seed`` (2,)), never the seed itself."""
    state = np.random.SeedSequence(entropy=int(seed), spawn_key=(3, int(k))).generate_state(4)
    return int.from_bytes(state.tobytes(), "little")


EMA_REFUSED = (
    "ema_tau > 0 needs a target network held in a buffer of its own: only DQN has one (iS-DQN's target is a head of the online "
    "parameters, moved by the head shift; the target-free agents have none)")


def check_ema_tau(ema_tau, supported: bool = False) -> float:
    """ema_tau of an agent's constructor: in [0, 1] (NaN refused), and 0 for every agent but DQN (EMA_REFUSED)."""
    tau = float(ema_tau)
    if not 0.0 <= tau <= 1.0:
        raise ValueError("ema_tau must be in [0, 1] (0 = off: hard target updates)")
    if tau > 0.0 and not supported:
        raise ValueError(EMA_REFUSED)
    return tau


SOFT_SHIFT_REFUSED = (
    "soft_shift_tau > 0 needs heads to shift: only iS-DQN and its analysis agent keep 1 + K heads in one set of parameters (DQN's "
    "soft target is ema_tau, on its target buffer; the target-free agents have no target)")


def check_soft_shift_tau(soft_shift_tau, supported: bool = False) -> float:
    """soft_shift_tau of an agent's constructor: in [0, 1] (NaN refused), and 0 for every agent but iS-DQN's (SOFT_SHIFT_REFUSED)."""
    tau = float(soft_shift_tau)
    if not 0.0 <= tau <= 1.0:
        raise ValueError("soft_shift_tau must be in [0, 1] (0 = off: the hard head shift at every target update)")
    if tau > 0.0 and not supported:
        raise ValueError(SOFT_SHIFT_REFUSED)
    return tau


def augment_seed(seed: int) -> int:
    """64-bit seed of the agent's random-shift draws: a child of the agent's seed in numpy's SeedSequence tree under a spawn key of its
    own ((2,); ``recycle_seed`` has (1, k)), never the seed itself."""
    state = np.random.SeedSequence(entropy=int(seed), spawn_key=(2,)).generate_state(2)
    return int.from_bytes(state.tobytes(), "little")


class Stage(typing.NamedTuple):
    """One launch behind the learn call of a gradient step ("The step as a schedule")."""

    tag: tuple            # what the captured step's key says of it
    run: typing.Callable  # takes no arguments, enqueues on the current stream
    state: tuple = ()     # the device tensors it writes besides the engine's own


class EngineAgent:
    """Common state: ``n_heads`` network heads of ``n_actions`` outputs each on the HIP engine."""

    _is_schedule = None  # (beta_start, beta_end, n_steps) once set_importance_sampling was called; None: no weights anywhere
    _is_step = 0         # gradient steps taken under the schedule

    # ------------------------------------------------------------------ importance sampling (prioritized replay)
    def set_importance_sampling(self, beta_start: float, beta_end: float | None = None, n_steps: int = 0) -> None:
        """Weigh the loss of every sampled transition with the importance-sampling weight of its draw (Schaul et al. 2016, 3.4;
        computed by the sum-tree query: include/isdqn_hip.h, isdqn_tree_query_weighted).  beta is linear in gradient steps from
        ``beta_start`` to ``beta_end`` over ``n_steps`` steps, constant when ``beta_end`` is None.  Needs a prioritized replay.
        Until this is called no weight is computed and the learn calls get a NULL weights pointer."""
        self._is_schedule = (float(beta_start), None if beta_end is None else float(beta_end), int(n_steps))
        self._is_step = 0
        self._drop_graph()  # (the captured step has the weighted query and the weights pointer, or not)

    @property
    def importance_sampling(self) -> bool:
        return self._is_schedule is not None

    def _next_betas(self, n: int = 1):
        """float32 betas of the next ``n`` gradient steps (None when importance sampling is off); advances the step count."""
        if self._is_schedule is None:
            return None
        t = self._is_step
        self._is_step = t + n
        return np.asarray([importance_beta(*self._is_schedule, t + i) for i in range(n)], dtype=np.float32)

    def _sample(self, replay_buffer):
        """The training batch of one eager gradient step: with importance sampling on, drawn with this step's beta; with a horizon
        schedule, cut at this step's horizon and discount."""
        betas = self._next_betas()
        kw = {} if betas is None else dict(beta=float(betas[0]))
        pairs = self._next_horizons(1, replay_buffer)
        if pairs is not None:
            kw.update(horizon=int(pairs[0][0]), gamma=float(pairs[1][0]))
        return self._augment(replay_buffer, replay_buffer.sample(**kw))

    def _sample_eval(self, replay_buffer):
        """The second ("eval") batch of an analysis agent's update: as sampled, at the horizon and discount of the step's training batch."""
        if self._hz_schedule is None:
            return replay_buffer.sample()
        n, g = self._hz_last
        return replay_buffer.sample(horizon=int(n), gamma=float(g))

    # ------------------------------------------------------------------ annealed update horizon and discount
    _hz_schedule = None  # (n_start, n_end, gamma_start, gamma_end, period) once set_horizon_schedule was called; None: off
    _hz_step = 0         # gradient steps since the call or since the last reset_parameters
    _hz_last = None      # (horizon, float32 gamma) of the last gradient step taken under the schedule

    def set_horizon_schedule(self, n_start: int, n_end: int, gamma_start: float, gamma_end: float, period: int, replay_buffer=None) -> None:
        """Anneal the update horizon from ``n_start`` to ``n_end`` and the discount from ``gamma_start`` to ``gamma_end`` over ``period``
        gradient steps (``horizon_schedule``; SR-SPR and BBF: 10 -> 3 and 0.97 -> 0.997), counted from this call and again from every
        ``reset_parameters``.  Needs a replay built with ``horizon_window=True`` whose n_max covers both horizons (checked here when
        ``replay_buffer`` is given, else at the first update): every batch is then cut at the step's horizon on the device and carries
        its discount per row (include/isdqn_hip.h, isdqn_replay_gather_horizon and isdqn_batch_discount::discount); the engine's ``gamma_n`` is
        not read.  Until this is called the learn calls get a NULL discount pointer."""
        n_start, n_end, period = int(n_start), int(n_end), int(period)
        if period < 1:
            raise ValueError("set_horizon_schedule: period must be >= 1")
        if n_start < 1 or n_end < 1:
            raise ValueError("set_horizon_schedule: horizons must be >= 1")
        for g in (gamma_start, gamma_end):
            if not 0.0 <= float(g) < 1.0:
                raise ValueError("set_horizon_schedule: discounts must be in [0, 1)")
        self._hz_schedule = (n_start, n_end, float(gamma_start), float(gamma_end), period)
        if replay_buffer is not None:
            self._check_horizon_replay(replay_buffer)
        self._hz_step = 0
        self._hz_last = horizon_schedule(*self._hz_schedule, 0)
        self._drop_graph()  # (the captured step has the gather at a horizon and the discount pointer, or not)

    def _check_horizon_replay(self, replay_buffer) -> None:
        n_need = max(self._hz_schedule[0], self._hz_schedule[1])
        if not getattr(replay_buffer, "_horizon_window", False):
            raise ValueError("a horizon schedule (set_horizon_schedule) needs a replay built with horizon_window=True")
        if replay_buffer._update_horizon < n_need:
            raise ValueError(f"a horizon schedule up to n = {n_need} needs a replay with n_max >= {n_need}, this one has "
                             f"{replay_buffer._update_horizon}")

    def _next_horizons(self, n: int = 1, replay_buffer=None):
        """(int32 horizons, float32 discounts) of the next ``n`` gradient steps (None when the schedule is off); advances the count."""
        if self._hz_schedule is None:
            return None
        if replay_buffer is not None:
            self._check_horizon_replay(replay_buffer)
        t = self._hz_step
        self._hz_step = t + n
        pairs = [horizon_schedule(*self._hz_schedule, t + i) for i in range(n)]
        self._hz_last = pairs[-1]
        return np.asarray([p[0] for p in pairs], dtype=np.int32), np.asarray([p[1] for p in pairs], dtype=np.float32)

    def _run_graph(self, g) -> None:
        """One replay of the captured update ``g``: the betas and the (horizon, discount) pairs of its S steps are its input."""
        self._stepped(g.S)
        betas = self._next_betas(g.S)
        pairs = self._next_horizons(g.S, g.rb)
        g.run(betas) if pairs is None else g.run(betas, horizons=pairs[0], gammas=pairs[1])

    # ------------------------------------------------------------------ what stands behind the learn call
    def _after_learn(self, eng) -> list:
        """The Stages behind the learn call of a gradient step on ``eng``, in order: stated once per agent, read by the eager and by
        the captured step.  Here the two every agent shares, the prune apply (only while ``prune_active``), then the projection
        (only with ``weight_projection``); iSDQN and DQN place their own around them."""
        prune = [Stage(("prune",), eng.prune_apply)] if self.prune_active else []
        return prune + ([Stage(("nap",), eng.project_weights)] if self.weight_projection else [])

    def _step_engine(self, replay_buffer):
        """The engine of a gradient step on ``replay_buffer``'s batches."""
        return self._engine_for(replay_buffer._batch_size) if hasattr(replay_buffer, "_batch_size") else self._engine

    def _captured_step(self, eng, learn=None, key=(), state=()) -> dict:
        """What _graphed_update is handed: ``learn`` on a C batch (None: the engine's learn_on_batch) with the stages behind it on the
        same stream -- further nodes of the captured step, no new branch --, the agent's base ``key`` with the stages' tags behind it
        as one flat tuple (None when empty), and the tensors the stages write in front of the base ``state``.  An agent with nothing
        on hands over no learn call, no state and no key: the captured step is the engine's own."""
        stages = self._after_learn(eng)
        if learn is None and not stages:
            return {}
        first = eng.learn_on_batch if learn is None else learn

        def step(cb):
            first(cb)
            for s in stages:
                s.run()

        key = tuple(key) + tuple(x for s in stages for x in s.tag)
        return dict(learn=step, key=key or None, state=[t for s in stages for t in s.state] + list(state))

    def _own_step(self, replay_buffer) -> dict:
        """``_captured_step`` of an agent whose learn call is the engine's own (iSDQN, TFDQN); the engine is asked for only where a
        stage needs it, else behind the guards of _graphed_update as ever."""
        return self._captured_step(self._step_engine(replay_buffer)) if self._after_learn(self._engine) else {}

    def _eager_after_learn(self) -> None:
        """Behind the agent's learn_on_batch in an eager gradient step: the same stages, in the same order."""
        self._stepped(1)
        for s in self._after_learn(self._engine):
            s.run()

    def _stepped(self, n: int) -> None:
        """``n`` gradient steps were taken, eager or replayed: the pruning schedule's clock runs while the option is on, whether or not
        anything is pruned yet."""
        if self._prune is not None:
            self._prune_t += n

    def _horizon_logs(self) -> dict:
        """The update horizon and the discount of the last gradient step, logged where the loss is; {} when the schedule is off."""
        if self._hz_schedule is None:
            return {}
        return {"update_horizon": int(self._hz_last[0]), "gamma": float(self._hz_last[1])}

    # ------------------------------------------------------------------ random-shift augmentation
    augment_pad = 0   # 0: off
    aug_count = None  # device int64 [1]: augmented gradient steps so far (selects the draws; the captured step advances it on the device)

    def _augment(self, replay_buffer, batch):
        """The training batch of one gradient step, shifted (``augment_pad`` > 0; include/isdqn_hip.h, isdqn_replay_augment_shift): once
        per update -- the analysis agents make all their passes over the one augmented batch, and their evaluation batch stays as
        sampled.  ``recycle_dormant``, acting and ``_q_row`` never come here."""
        if not self.augment_pad:
            return batch
        if not hasattr(replay_buffer, "augment"):
            raise ValueError("augment_pad > 0 needs the device replay (ReplayBuffer.augment): the shift runs on its frame store")
        return replay_buffer.augment(batch, *self._aug_state())

    def _aug_state(self):
        """(pad, seed, device counter) of the augmentation.  The counter is made at first use: ``augment_pad`` may be switched on
        behind the constructor (the live captured update is then captured again: _graphed_update)."""
        check_augment(self.augment_pad, self.architecture_type)
        if self.aug_count is None:
            self._aug_seed = augment_seed(self._seed)
            self.aug_count = torch.zeros(1, dtype=torch.int64, device=self._engine.device)
        return int(self.augment_pad), self._aug_seed, self.aug_count

    def _init_engine_agent(self, key, observation_dim, n_actions, n_heads, features, layer_norm, architecture_type,
                           learning_rate, gamma, update_horizon, adam_eps, batch_size, precision, device, options: NetOptions,
                           batch_norm=False, augment_pad=0, weight_decay=0.0, weight_decay_all=False, cql_alpha=0.0,
                           prune_sparsity=0.0, prune_start=0, prune_end=0, prune_period=0, weight_projection=False):
        """``options``: what the constructor picked and checked (NetOptions.check, behind its own rules); the two rules that stand
        behind it follow here.  Every option becomes a plain attribute of the agent and goes to every engine it builds.
        ``augment_pad`` > 0: DrQ random-shift augmentation (Kostrikov et al. 2020; include/isdqn_hip.h, isdqn_replay_augment_shift) --
        every gradient step trains on its sampled batch with each state stack and each next-state stack shifted by a draw of its own in
        [-pad, pad]^2, borders replicated, on the device (eager and captured alike; the device counter ``aug_count`` selects the
        draws).  Acting, ``recycle_dormant`` and the analysis agents' evaluation passes see the frames as stored.  Every torso but 'fc'
        (ValueError); needs the device replay.  0 is off.
        ``weight_decay`` > 0: AdamW (optax.adamw, as BBF and SR-SPR train; include/isdqn_hip.h, isdqn_batch_decay) -- every learn step of
        every engine the agent builds also decays the conv and dense kernels by ``learning_rate * weight_decay`` of their value, with
        ``weight_decay_all`` the biases and the normalisation scales and biases too (QNetEngine.set_weight_decay).  0 is off: the bits
        of an agent built without the argument.  Refused with ``noisy`` (ValueError), before anything is built.
        ``cql_alpha`` > 0: the conservative term of CQL(H) (Kumar et al. 2020; include/isdqn_hip.h, isdqn_batch_conservative) -- every
        loss and every learn step of every engine the agent builds adds ``cql_alpha * (logsumexp_a Q(s, a) - Q(s, a_b))`` per regressed
        head (QNetEngine.set_conservative): the offline recipe with ``n_quantiles`` is QR-DQN + CQL.  0 is off: the bits of an agent
        built without the argument.  Negative, NaN or infinite: ValueError, before anything is built.
        ``prune_sparsity`` > 0: gradual magnitude pruning (``_init_pruning`` below) from gradient step ``prune_start`` to ``prune_end``,
        the mask updated every ``prune_period`` steps.  0 is off: the calls and the bits of an agent built without the argument.
        ``weight_projection``: Normalize-and-Project (``_init_projection`` below) -- every gradient step is followed by the projection
        of every conv and Dense kernel but the last Dense's back to its initial norm.  False is off: the calls and the bits of an agent
        built without the argument."""
        check_augment(augment_pad, architecture_type)
        check_noisy(options.noisy, architecture_type, batch_norm, options.max_grad_norm)
        self._init_pruning(prune_sparsity, prune_start, prune_end, prune_period, noisy=options.noisy, batch_norm=batch_norm,
                           architecture_type=architecture_type)
        self._init_projection(weight_projection, layer_norm=layer_norm, noisy=options.noisy, batch_norm=batch_norm,
                              architecture_type=architecture_type)
        self.weight_decay = _optimizer.check_weight_decay(weight_decay, noisy=options.noisy)
        self.weight_decay_all = bool(weight_decay_all)
        self.cql_alpha = _conservative.check_cql_alpha(cql_alpha)
        self.options = options
        for name, value in dataclasses.asdict(options).items():
            setattr(self, name, value)
        self.noisy_eval = False  # True: acting calls run the mean network (zero noise) instead of drawing
        self._bound_sigma = None
        self._grad_clip_count = 0  # Adam step count at the last read of the gradient-norm accumulators (_grad_clip_logs)
        self.n_actions = n_actions
        self.batch_norm = bool(batch_norm)
        self._n_heads = int(n_heads)
        self.features = [int(f) for f in features]
        self.architecture_type = architecture_type
        self.layer_norm = bool(layer_norm)
        self.observation_dim = tuple(int(d) for d in np.atleast_1d(observation_dim))
        self.learning_rate = learning_rate
        self.adam_eps = adam_eps
        self.gamma = gamma
        self.update_horizon = update_horizon
        self.precision = precision
        self.device = device
        self._seed = int(key) if not isinstance(key, torch.Generator) else int(key.initial_seed())
        self._engine = None
        self._graphed = None
        self._trust_mirror = None  # None: the engine's default (_engine.py: rebuild in every call); see the property below
        self._ring = None  # device copy of the acting path's frame stack (see _obs_to_device)
        self._make_engine(batch_size, init=True)
        self.augment_pad = int(augment_pad)
        if self.augment_pad:  # (off: no buffer, no launch -- the agent is the one built without the argument)
            self._aug_state()

    rem_heads = 0  # REM (DQN's ``rem_heads``): the engine has this many heads and a mixture; acting is on the head average.  0: off

    def _act_kw(self) -> dict:
        """What the acting calls add to ``best_actions``: nothing, or the head average of a mixture agent."""
        return dict(mean_heads=True) if self.rem_heads else {}

    # ------------------------------------------------------------------ engine management
    def _make_engine(self, batch_size: int, init: bool = False) -> None:
        old = self._engine
        eng = QNetEngine(
            self.observation_dim, self.n_actions, self._n_heads, self.features, self.architecture_type, self.layer_norm, batch_size,
            gamma_n=self.gamma**self.update_horizon, learning_rate=self.learning_rate, adam_eps=self.adam_eps, precision=self.precision,
            device=self.device, batch_norm=self.batch_norm, **self.options.engine_kwargs(noisy_seed=self._seed),
        )
        if self.noisy:
            eng.resample_on_learn = True  # every learn step of an agent draws first (eager and captured alike)
        if self.weight_decay > 0.0:
            eng.set_weight_decay(self.weight_decay, self.weight_decay_all)
        if self.cql_alpha > 0.0:
            eng.set_conservative(self.cql_alpha)
        if self.rem_heads:  # (off: no buffer, no launch -- the engine is the one built without the option)
            eng.set_mixture(_mixture.mixture_seed(self._seed))
            if old is not None and old.mix_count is not None:
                eng.mix_count.copy_(old.mix_count)
        if init:
            eng.init_params(self._seed)
        else:  # a batch of another size arrived: same parameter layout, new workspace
            eng.copy_state_from(old)
        if self._prune_args is not None:  # (off: no buffer, no call -- the engine is the one built without the option)
            n_real = eng.set_pruning()
            if self._prune is None:
                self._prune = _sparsity.Schedule(*self._prune_args, n_real)
            if old is not None and old.prune_mask is not None:
                eng.prune_mask.copy_(old.prune_mask)
        if self.weight_projection:  # (off: no buffer, no call -- the engine is the one built without the option)
            # the first engine measures the initial parameters; every later one is handed the same target norms
            self._nap_targets = eng.set_weight_projection(self._nap_targets)
            if old is not None and old.project_scales is not None:
                eng.project_scales.copy_(old.project_scales)
        self._drop_graph()  # captured against the old engine's buffers
        self._engine = eng
        if self._trust_mirror is not None:
            eng.trust_mirror = self._trust_mirror
        self._ring = None
        self.params = DeviceParams(eng, eng.params)
        self.optimizer_state = {"count": eng.adam_count, "mu": eng.adam_m, "nu": eng.adam_v}
        self._engine_changed(old)

    @property
    def trust_mirror(self) -> bool:
        """Whether the engine may skip the weight-mirror rebuild while its bookkeeping says nothing wrote the parameters (an owner's
        declaration that every write goes through torch or the agent: _engine.py).  Setting it re-captures the update graph."""
        return bool(self._engine.trust_mirror)

    @trust_mirror.setter
    def trust_mirror(self, value: bool) -> None:
        value = bool(value)
        if value != bool(self._engine.trust_mirror):
            self._drop_graph()  # (the captured replay has the rebuild node or not)
            self._ring = None   # (and so have the acting graphs)
        self._trust_mirror = value
        self._engine.trust_mirror = value

    def _grad_clip_logs(self) -> dict:
        """Read and zero the gradient-norm accumulators of the engine (region "grad_clip"[2:4], kept on the device by every update
        step): the mean gradient norm and the fraction of clipped steps over the gradient steps since the last read.  {} when
        ``max_grad_norm`` is off.  Called where ``update_target_params`` reads ``losses_accum``."""
        if not self.max_grad_norm > 0.0:
            return {}
        eng = self._engine
        acc = eng.grad_clip[2:4]
        norm_sum, n_clipped = (float(x) for x in acc.cpu().numpy())
        acc.zero_()
        count = int(eng.adam_count.item())
        steps = max(count - self._grad_clip_count, 1)
        self._grad_clip_count = count
        return {"grad_norm": norm_sum / steps, "grad_clipped_fraction": n_clipped / steps}

    def _engine_changed(self, old) -> None:
        """Hook: a new engine replaced ``old`` (subclasses re-home extra device state)."""

    def _drop_graph(self) -> None:
        """Destroy the live captured update, if any (one executable graph per agent: _graph.py, "hipGraphLaunch fault")."""
        g, self._graphed = self._graphed, None
        if g is not None:
            g.destroy()

    def _graphed_update(self, replay_buffer, learn=None, key=None, steps: int = 1, state=()):
        """The captured sample -> learn -> [write-back] update of ``steps`` consecutive steps for this (replay, engine) pair, or None
        when the replay is not the device replay of this GPU (reference-layout buffers take the eager path).  ``learn`` / ``key``:
        another learn call than the engine's learn_on_batch and what it is bound to (DQN: the target parameters' buffer); ``state``:
        the device tensors that call writes besides the engine's own (GraphedUpdate).  The agent
        owns ONE executable graph at a time: a request that does not match the live one destroys it first, then captures."""
        if not getattr(self, "use_graph", True) or not hasattr(replay_buffer, "_d_elem_frames") or getattr(replay_buffer, "_lib", None) is None:
            return None
        if replay_buffer.add_count == 0:
            return None
        if self.architecture_type == "fc" and not (replay_buffer._obs_float and replay_buffer._stack_size == 1):
            return None  # (the captured fc step reads float32 vector observations with stack_size 1: _graph.py)
        if self._hz_schedule is not None:
            self._check_horizon_replay(replay_buffer)
        eng = self._engine_for(replay_buffer._batch_size)
        prioritized = hasattr(replay_buffer._sampling_distribution, "_tree")
        writeback = bool(getattr(self, "priority_writeback", False))
        weighted = self.importance_sampling
        if weighted and not prioritized:
            raise ValueError("importance-sampling weights (set_importance_sampling) need the prioritized sampling distribution")
        g = self._graphed
        if (g is None or g.rb is not replay_buffer or g.eng is not eng or g.writeback != (writeback and prioritized)
                or g.weighted != weighted or getattr(g, "key", None) != key or g.S != steps or g.augment_pad != self.augment_pad
                or g.horizon != (self._hz_schedule is not None)):
            from slimdqn._graph import GraphedUpdate

            self._drop_graph()
            g = self._graphed = GraphedUpdate(replay_buffer, eng, prioritized, steps_per_graph=steps, writeback=writeback, learn=learn,
                                              weighted=weighted, horizon=self._hz_schedule is not None,
                                              augment=self._aug_state() if self.augment_pad else None, state=state)
            g.key = key
            self._captures = getattr(self, "_captures", 0) + 1
        return g

    def _engine_for(self, batch_size: int) -> QNetEngine:
        if self._engine.batch_size != batch_size:
            self._make_engine(batch_size)
        return self._engine

    def _bind(self, params):
        """Accept the agent's own handle, another DeviceParams, or a Flax-layout pytree."""
        if params is None or params is self.params:
            return None
        if isinstance(params, DeviceParams):
            return params.tensor
        def flatten(tree):  # Flax nesting -> the engine's flattened "Stack_0/Conv_1" keys
            if tree is None or not any(k.startswith("Stack_") and "/" not in k for k in tree):
                return tree
            return {**{f"{k}/{m}": v for k, sub in tree.items() if k.startswith("Stack_") for m, v in sub.items()},
                    **{k: v for k, v in tree.items() if not k.startswith("Stack_")}}

        # a model pickle `{"params": variables}` (get_model), the variables dict `{"params": tree[, "batch_stats": tree]}`
        # (the reference's agent.params), or the bare tree
        while isinstance(params.get("params"), dict) and isinstance(params["params"].get("params"), dict):
            params = params["params"]
        tree = flatten(params["params"] if "params" in params else params)
        t = torch.empty_like(self._engine.params)
        # noisy agents: the sigma leaves of the tree, kept beside the returned mu (a learn call loads both; acting on a foreign model
        # runs its mean network)
        self._bound_sigma = None
        if self.noisy and any("sigma_kernel" in leaves for leaves in tree.values()):
            self._bound_sigma = torch.empty_like(self._engine.params)
            self._engine._import_sigma(tree, self._bound_sigma)
        self._engine.import_flax(tree, target=t, batch_stats=flatten(params.get("batch_stats")) if "params" in params else None)
        return t

    # ------------------------------------------------------------------ batches
    def _c_batch(self, eng: QNetEngine, samples):
        weights = getattr(samples, "weights", None)  # importance-sampling weights of the draw, when the batch carries them
        discount = getattr(samples, "discount", None)  # per-row discounts of a gather at a horizon, when the batch carries them
        if hasattr(samples, "frame_ids") and self.architecture_type == "fc":
            # device replay of vector observations (LunarLander): the stored float32 bytes come back as (B, d) rows
            return eng.make_batch(state=samples.state, next_state=samples.next_state, action=samples.action, reward=samples.reward,
                                  terminal=samples.is_terminal, loss_weights=weights, discount=discount)
        if hasattr(samples, "frame_ids"):  # DeviceBatch from the device replay
            return eng.make_batch(
                frames=samples.frames, frame_stride=samples.frame_stride, frame_ids=samples.frame_ids,
                action=samples.action, reward=samples.reward, terminal=samples.is_terminal, loss_weights=weights,
                discount=discount,
            )
        dev = eng.device
        as_t = lambda x, dt: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(dev).to(dt).contiguous()
        if weights is not None:
            weights = as_t(weights, torch.float32)
        action = as_t(samples.action, torch.int32)
        reward = as_t(samples.reward, torch.float32)
        terminal = as_t(samples.is_terminal, torch.uint8)
        if self.architecture_type == "fc":
            st = as_t(samples.state, torch.float32).reshape(len(action), -1)
            nx = as_t(samples.next_state, torch.float32).reshape(len(action), -1)
            return eng.make_batch(state=st, next_state=nx, action=action, reward=reward, terminal=terminal, loss_weights=weights)
        st = as_t(samples.state, torch.uint8)
        nx = as_t(samples.next_state, torch.uint8)
        B, h, w, stack = st.shape
        planes = torch.empty(2 * B * stack, h * w, dtype=torch.uint8, device=dev)
        ids = torch.empty(B, 2 * stack, dtype=torch.int32, device=dev)
        _hip.check(
            eng.lib.isdqn_replay_deinterleave(_hip.ptr(st), _hip.ptr(nx), h, w, stack, B, _hip.ptr(planes), _hip.ptr(ids), _hip.stream_ptr(dev))
        )
        return eng.make_batch(frames=planes, frame_stride=h * w, frame_ids=ids, action=action, reward=reward, terminal=terminal,
                              loss_weights=weights)

    @staticmethod
    def _batch_len(samples) -> int:
        return int(samples.action.shape[0])

    def _obs_to_device(self, state):
        eng = self._engine
        if self.architecture_type == "fc":
            obs = torch.as_tensor(np.asarray(state, dtype=np.float32)).reshape(1, -1).to(eng.device)
            return dict(obs=obs)
        s = np.asarray(state)
        s = s.astype(np.uint8) if s.dtype != np.uint8 else s.copy()
        h, w, stack = s.shape
        ring = self._ring
        if ring is None or ring["last"].shape != s.shape:
            rot = (torch.arange(stack)[None, :] + torch.arange(stack)[:, None]) % stack
            ring = self._ring = dict(
                planes=torch.empty(stack, h * w, dtype=torch.uint8, device=eng.device),
                rot=rot.to(torch.int32).to(eng.device),  # row r: plane slots oldest..newest after r one-frame shifts
                shifts=0,
                last=None,
            )
        # Consecutive acting states differ by one frame (atari.py:71-78 rolls the stack): the device keeps the stack as a
        # ring of planes and only the newest 7 KB frame crosses PCIe; anything else (reset, a foreign state) is a full upload.
        if ring["last"] is not None and _is_one_frame_shift(ring["last"], s):
            slot = ring["shifts"] % stack  # the oldest plane's slot
            ring["planes"][slot].copy_(torch.from_numpy(np.ascontiguousarray(s[..., -1]).reshape(-1)))
            ring["shifts"] += 1
        else:
            ring["planes"].copy_(torch.from_numpy(np.ascontiguousarray(np.moveaxis(s, -1, 0)).reshape(stack, h * w)))
            ring["shifts"] = 0
        ring["last"] = s
        return dict(frames=ring["planes"], frame_stride=h * w, frame_ids=ring["rot"][ring["shifts"] % stack])

    def _states_to_device(self, states):
        """n observations (n, h, w, stack) or (n, d) -> planes / rows for one batched forward."""
        eng = self._engine
        if self.architecture_type == "fc":
            s = np.asarray(states, dtype=np.float32)
            return dict(obs=torch.from_numpy(s.reshape(s.shape[0], -1)).to(eng.device))
        s = np.asarray(states)
        s = s.astype(np.uint8) if s.dtype != np.uint8 else s
        n, h, w, stack = s.shape
        planes = torch.from_numpy(np.ascontiguousarray(np.moveaxis(s, -1, 1)).reshape(n * stack, h * w)).to(eng.device)
        ids = torch.arange(n * stack, dtype=torch.int32, device=eng.device)
        return dict(frames=planes, frame_stride=h * w, frame_ids=ids)

    # ------------------------------------------------------------------ one environment step as one graph launch
    def _act_graph_step(self, s: np.ndarray, idx_network: int):
        """The common acting step -- the new state is the previous one shifted by a frame -- as ONE hipGraph launch: newest
        frame and head index up (one pinned 7 KB copy), frame into the ring slot of the oldest plane, the forward with the
        plane ids of this rotation, the action back into pinned memory.  One graph per (ring slot, weight mirror trusted or
        rebuilt), captured at first use; eager launches cost ~45 us of launch calls for the nine kernels of this forward."""
        eng, ring = self._engine, self._ring
        h, w, stack = s.shape
        hw = h * w
        g = ring.get("graph")
        if g is None:
            g = ring["graph"] = dict(
                pin_in=torch.empty(hw + 16, dtype=torch.uint8).pin_memory(),
                dev_in=torch.empty(hw + 16, dtype=torch.uint8, device=eng.device),
                out=torch.zeros(1, dtype=torch.int32, device=eng.device),
                pin_out=torch.zeros(1, dtype=torch.int32).pin_memory(),
                graphs={},
            )
            g["np_in"] = g["pin_in"].numpy()
        slot = ring["shifts"] % stack
        g["np_in"][:hw] = s[..., -1].reshape(-1)
        g["np_in"][hw : hw + 4].view(np.int32)[0] = idx_network
        current = eng._mirror_is_current(None)
        key = (slot, current)
        graph = g["graphs"].get(key)
        if graph is None:
            ids = ring["rot"][(ring["shifts"] + 1) % stack]
            idx_dev = g["dev_in"][hw : hw + 4].view(torch.int32)

            def enqueue():
                g["dev_in"].copy_(g["pin_in"], non_blocking=True)
                ring["planes"][slot].copy_(g["dev_in"][:hw])
                eng.best_actions(frames=ring["planes"], frame_stride=hw, frame_ids=ids, idx_networks=idx_dev, out=g["out"],
                                 mirror_current=current, **self._act_kw())
                g["pin_out"].copy_(g["out"], non_blocking=True)

            torch.cuda.synchronize(eng.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                enqueue()
            g["graphs"][key] = graph
        graph.replay()
        eng._mirror_holds(None)
        ring["shifts"] += 1
        ring["last"] = s
        torch.cuda.current_stream(eng.device).synchronize()
        return int(g["pin_out"][0])

    def _best_action(self, params, state, idx_network: int) -> int:
        """One observation: newest frame up, one forward (weight mirror reused when nothing wrote the parameters since the
        last learn step), one 4-byte read back."""
        eng = self._engine
        self._noisy_act(params)
        if self._bind(params) is None and self.architecture_type != "fc" and getattr(self, "act_graph", True):
            ring = self._ring
            s = np.asarray(state)
            s = s.astype(np.uint8) if s.dtype != np.uint8 else s.copy()
            if ring is not None and ring["last"] is not None and ring["last"].shape == s.shape and _is_one_frame_shift(ring["last"], s):
                return self._act_graph_step(s, int(idx_network))
            state = s
        heads = getattr(self, "_head_ids", None)
        if heads is None or heads.device != eng.device:
            heads = self._head_ids = torch.arange(max(self._n_heads, 1), dtype=torch.int32, device=eng.device)
        out = eng.best_actions(idx_networks=heads[idx_network : idx_network + 1], params=self._bind(params), **self._obs_to_device(state),
                               **self._act_kw())
        return int(out.item())

    def _best_actions(self, params, states, idx_networks) -> np.ndarray:
        """Greedy actions of n observations in one forward and one device->host copy.  Noisy agents: ONE draw serves all n rows."""
        eng = self._engine
        self._noisy_act(params)
        idx = torch.as_tensor(np.array(idx_networks, dtype=np.int32)).to(eng.device)
        out = eng.best_actions(idx_networks=idx, params=self._bind(params), **self._states_to_device(states), **self._act_kw())
        return out.cpu().numpy()

    def _best_actions_planes(self, params, planes: np.ndarray, rows: np.ndarray, idx_networks, wait: bool = True):
        """Greedy actions of the environments ``rows`` of a VectorEnv: ``planes`` is its host block uint8 [n][stack][h*w]
        (planar stacks, oldest .. newest; pinned when the runtime registered the mapping).  ONE host-to-device copy of the
        block, one small copy of (plane ids, head indices), one forward over len(rows) observations, one read-back."""
        eng = self._engine
        self._noisy_act(params)  # (one draw serves all rows of the round)
        n, stack, hw = planes.shape
        v = getattr(self, "_vec", None)
        if v is None or v["dev"].shape != (n * stack, hw) or v["dev"].device != eng.device:
            v = self._vec = dict(
                dev=torch.empty(n * stack, hw, dtype=torch.uint8, device=eng.device),
                small=torch.empty(n * (stack + 1), dtype=torch.int32, device=eng.device),
                host_small=torch.empty(n * (stack + 1), dtype=torch.int32).pin_memory(),
                out=torch.empty(n, dtype=torch.int32, device=eng.device),
                host_out=torch.empty(n, dtype=torch.int32).pin_memory(),
                ar=np.arange(stack, dtype=np.int32),
            )
        m = len(rows)
        v["dev"].copy_(torch.from_numpy(planes.reshape(n * stack, hw)), non_blocking=True)
        hs = v["host_small"].numpy()
        hs[: m * stack] = (np.asarray(rows, np.int32)[:, None] * stack + v["ar"][None, :]).reshape(-1)
        hs[n * stack : n * stack + m] = np.asarray(idx_networks, np.int32)
        v["small"].copy_(v["host_small"], non_blocking=True)
        eng.best_actions(frames=v["dev"], frame_stride=hw, frame_ids=v["small"][: m * stack], idx_networks=v["small"][n * stack : n * stack + m],
                         params=self._bind(params), out=v["out"][:m], **self._act_kw())
        v["host_out"][:m].copy_(v["out"][:m], non_blocking=True)
        ev = v.setdefault("event", torch.cuda.Event())
        ev.record(torch.cuda.current_stream(eng.device))

        def result() -> np.ndarray:
            ev.synchronize()  # (this forward only: work enqueued behind it -- the round's gradient steps -- keeps running)
            return v["host_out"][:m].numpy().astype(np.int64)

        return result() if wait else result

    # ------------------------------------------------------------------ noisy Dense layers
    def _noisy_act(self, params) -> None:
        """In front of every acting call on the agent's own parameters: a new draw, or zero noise with ``noisy_eval``."""
        if getattr(self, "noisy", False) and (params is None or params is self.params):
            if self.noisy_eval:
                self._engine.zero_noise()
            else:
                self._engine.resample_noise()

    def noisy_evaluation(self):
        """Context: acting calls inside run the mean network (``noisy_eval`` = True), the previous setting returns behind it."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            old, self.noisy_eval = self.noisy_eval, True
            try:
                yield self
            finally:
                self.noisy_eval = old

        return ctx()

    def _one_draw(self, eng):
        """Context for an update that makes several passes over one batch (the analysis agents): noisy engines draw ONCE in front and
        every pass inside -- gradient-only passes, the learn step, the loss passes behind it -- runs under that draw; the step's own
        draw is switched off for the duration.  Other engines: nothing."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            if not getattr(eng, "noisy", False):
                yield
                return
            eng.resample_noise()
            keep, eng.resample_on_learn = eng.resample_on_learn, False
            try:
                yield
            finally:
                eng.resample_on_learn = keep

        return ctx()

    def _load_bound(self, eng, bound) -> None:
        """A learn call on foreign parameters: they become the engine's (noisy: their sigma leaves with them)."""
        if bound is not None:
            eng.params.copy_(bound)
            if getattr(self, "noisy", False) and self._bound_sigma is not None:
                eng.sigma.copy_(self._bound_sigma)

    # ------------------------------------------------------------------ ReDo
    _recycles = 0  # recycles done so far: selects the seed of the next fresh parameters

    def recycle_dormant(self, replay_buffer, tau: float) -> list:
        """ReDo (Sokar et al. 2023; include/isdqn_hip.h, isdqn_net_redo): score the hidden neurons on the states of 2 * batch_size
        sampled transitions and recycle the dormant ones (score <= tau * layer mean) on the device, Adam moments included.  The
        online parameters only: a DQN's target parameters keep their bits.  Pointers do not move and the weight mirror is left
        current, so a captured update stays valid.  Returns the recycled neurons per hidden layer -- the only host read."""
        check_redo(self.architecture_type, self.batch_norm)
        check_noisy(getattr(self, "noisy", False), self.architecture_type, redo=True)
        eng = self._engine
        n = 2 * eng.batch_size
        samples = replay_buffer.sample(size=n)
        if self.architecture_type == "fc":
            inputs = dict(obs=torch.as_tensor(samples.state).to(eng.device).to(torch.float32).reshape(n, -1).contiguous())
        elif hasattr(samples, "frame_ids"):
            stack = samples.frame_ids.shape[1] // 2
            ids = samples.frame_ids[:, :stack].contiguous()  # the states of the sampled transitions
            inputs = dict(frames=samples.frames, frame_stride=samples.frame_stride, frame_ids=ids)
        else:
            inputs = self._states_to_device(np.asarray(samples.state))
        fresh = eng.fresh_params(recycle_seed(self._seed, self._recycles))
        self._recycles += 1
        _, _, n_recycled = eng.redo(n_rows=n, tau=float(tau), fresh=fresh, **inputs)
        return [int(c) for c in n_recycled.cpu().numpy()]

    # ------------------------------------------------------------------ gradual magnitude pruning
    _prune_args = None  # (final sparsity, start, end) once the option is on; None: off, call for call
    _prune = None       # _sparsity.Schedule of the run, made with the first engine
    prune_period = 0    # gradient steps between two mask updates
    _prune_t = 0        # gradient steps taken under the option: the schedule's clock

    def _init_pruning(self, sparsity, start, end, period, *, noisy, batch_norm, architecture_type) -> None:
        """Gradual magnitude pruning (Zhu & Gupta 2017; Obando-Ceron et al. 2024; include/isdqn_hip.h, isdqn_net_prune_*; the rules:
        slimdqn/_sparsity.py).  Every conv and Dense kernel but the last Dense's is pruned by magnitude towards ``sparsity`` on the
        cubic schedule between gradient steps ``start`` and ``end``; the mask is chosen on the device at target updates whose step is
        a multiple of ``period`` (``prune_target_update``), and once anything is pruned every gradient step is followed by the apply
        launch: the first shared stage of ``_after_learn`` (until the schedule starts the step, eager or captured,
        is the one without the option).  Gradients and
        Adam moments stay dense.  A target buffer (DQN) is masked at every mask update, so its zeros survive the hard copy and the
        EMA.  Refused with noisy layers, batch_norm and the impala torso, before anything is built."""
        if _sparsity.check_sparsity(sparsity) == 0.0:
            return
        _sparsity.check_network(noisy=bool(noisy), batch_norm=bool(batch_norm), architecture_type=architecture_type)
        start, end = _sparsity.check_schedule(start, end)
        self.prune_period = _sparsity.check_period(period, self.target_update_frequency)
        self._prune_args = (float(sparsity), start, end)

    @property
    def prune_active(self) -> bool:
        """Whether a gradient step is followed by the apply launch: the option is on and the last mask update pruned something."""
        return self._prune is not None and self._prune.active

    def prune_target_update(self, step: int, wrote: bool = False) -> dict:
        """Behind the -redo and -reset hooks of the target update at ``step``: a multiple of ``prune_period`` updates the mask with the
        schedule's counts at the agent's own count of gradient steps (select, write the mask, apply: one stream-ordered call, no host
        read) and masks the target buffer; any other target update at which a hook wrote the parameters (``wrote``) applies the mask
        once, to the target buffer too (a reset moves it).  Returns the logs: ``sparsity``, the pruned share of all real prunable
        elements from the host's own counts.  {} while the option is off."""
        if self._prune is None:
            return {}
        eng = self._engine
        target = getattr(self, "target_params", None)
        target = target.tensor if target is not None and target.tensor is not eng.params else None
        if step % self.prune_period == 0 and any(self._prune.step(self._prune_t)):
            eng.prune_update(self._prune.counts)
            if target is not None:
                eng.prune_apply(params=target)  # (no workspace: the target has no persistent mirror)
        elif wrote and self._prune.active:
            eng.prune_apply()
            if target is not None:
                eng.prune_apply(params=target)
        return {"sparsity": self._prune.sparsity}

    # ------------------------------------------------------------------ Normalize-and-Project
    weight_projection = False  # the option; False: off, call for call
    _nap_targets = None        # the target norm of every projected tensor: measured once, on the agent's initial parameters

    def _init_projection(self, on, *, layer_norm, noisy, batch_norm, architecture_type) -> None:
        """Normalize-and-Project (Lyle et al. 2024; include/isdqn_hip.h, isdqn_net_project_*; the rules: slimdqn/_projection.py).  Every
        conv and Dense kernel but the last Dense's is scaled back to the Frobenius norm it had at initialisation after every gradient
        step: the second shared stage of ``_after_learn``, behind pruning's apply launch where that is active,
        so the norm is the masked tensor's.  Biases and LayerNorm vectors are left alone.  The target norms are measured on the first engine's initial parameters and never again: not at a
        reset, whose fresh draw is simply projected at the next step, not at ReDo, not when an engine for another batch size is built.
        A DQN target is never projected itself: a hard copy already is, an EMA is a convex combination of projected parameters.
        Needs ``layer_norm``; refused with noisy layers, batch_norm and the impala torso, before anything is built."""
        if not on:
            return
        _projection.check_network(layer_norm=bool(layer_norm), noisy=bool(noisy), batch_norm=bool(batch_norm),
                                  architecture_type=architecture_type)
        self.weight_projection = True

    def nap_target_update(self, step: int) -> dict:
        """The logs of the target update at ``step``, where the losses are read anyway: the smallest and the largest scale the last
        gradient step applied.  Scales that sit at 1 say the run is not growing its norms; at 0.99 it would lose 2 % of its effective
        learning rate per step without the option.  {} while the option is off."""
        if not self.weight_projection:
            return {}
        eng = self._engine
        return _projection.scale_logs(eng.project_scales[: len(eng.project_infos)].cpu().numpy())

    # ------------------------------------------------------------------ periodic resets
    _resets = 0  # resets done so far: selects the seed of the next fresh parameters

    def reset_parameters(self, shrink: float = 0.5, n_top_layers: int = 0) -> None:
        """Periodic reset (Nikishin et al. 2022; SR-SPR, BBF; include/isdqn_hip.h, isdqn_net_reset) towards a new initialisation drawn
        from ``reset_seed(seed, k)``: the top layers -- every Dense layer with ``n_top_layers`` = 0 (the whole fc network), else the
        last ``n_top_layers`` entries of the layer list -- are re-initialised, the layers below are shrunk and perturbed, p <-
        shrink * p + (1 - shrink) * fresh, and Adam's moments of everything written and its step count are cleared.  iS-DQN's
        1 + K heads share the last Dense and are reset together, the target head included.  A target copy (DQN, AnalysisDQN)
        takes the same interpolation towards the SAME fresh parameters (BBF), without moments.  Noisy agents: ``sigma`` (and DQN's
        ``target_sigma``) takes the same rule towards its initial value, its moments cleared.  Everything runs on the device in
        stream order; no pointer moves and the weight mirror is left current, so a live captured update stays valid."""
        eng = self._engine
        n_layers, first_dense = eng.reset_layout()
        if not 0.0 <= float(shrink) <= 1.0:
            raise ValueError("shrink must be in [0, 1]")
        if not 0 <= int(n_top_layers) <= n_layers:
            raise ValueError(f"n_top_layers must be in [0, {n_layers}] (the length of the layer list)")
        s = np.float32(shrink)
        factors = dict(split_layer=first_dense if int(n_top_layers) == 0 else n_layers - int(n_top_layers), shrink_lower=float(s),
                       perturb_lower=float(np.float32(1.0) - s), shrink_upper=0.0, perturb_upper=1.0)
        fresh = eng.fresh_params(reset_seed(self._seed, self._resets))
        self._resets += 1
        eng.reset(fresh, **factors)
        self._grad_clip_count = 0  # (the step count _grad_clip_logs measures its interval with starts again)
        self._hz_step = 0  # (and the horizon schedule, as BBF's does after every reset)
        target = getattr(self, "target_params", None)
        if target is not None and target.tensor is not eng.params:
            eng.reset(fresh, params=target.tensor, **factors)
        if getattr(self, "noisy", False):
            fresh_sigma = eng.fresh_sigma()
            eng.reset(fresh_sigma, params=eng.sigma, **factors)
            if getattr(self, "target_sigma", None) is not None:
                eng.reset(fresh_sigma, params=self.target_sigma, **factors)

    # generic forms (one head, per-step replays); iSDQN overrides both
    def best_actions_planes(self, params, planes, rows, key=None, wait: bool = True):
        return self._best_actions_planes(params, planes, rows, np.zeros(len(rows), dtype=np.int32), wait=wait)

    def learn_steps(self, n_steps: int, replay_buffer) -> None:
        for _ in range(n_steps):
            self.update_online_params(0, replay_buffer)

    def _q_row(self, params, state) -> torch.Tensor:
        """network.apply on one observation: device row of n_heads * n_actions values (noisy agents: under a new draw, or the mean
        network with ``noisy_eval``)."""
        self._noisy_act(params)
        return self._engine.forward(n_rows=1, params=self._bind(params), **self._obs_to_device(state))

    def get_model(self):
        """The reference's `{"params": self.params}` (isdqn.py:137-138), where `self.params` is the full Flax variables dict that
        `network.init` returned: `{"params": tree}` plus, for a BatchNorm network, the second collection `"batch_stats"` beside it
        (isdqn.py:87-88).  The pickle the trainer writes is therefore `{"params": {"params": tree[, "batch_stats": tree]}}`, and
        `network.apply(model["params"], ...)` works on it where JAX exists.  `_bind` loads either nesting back."""
        variables = {"params": self.params.to_flax()}
        if self.batch_norm:
            variables["batch_stats"] = self.params.batch_stats()
        return {"params": variables}
