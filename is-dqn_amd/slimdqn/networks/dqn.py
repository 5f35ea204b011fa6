"""DQN with the reference's surface (slimdqn/networks/dqn.py:11-101) on the HIP engine.

One head of ``n_actions`` outputs.  ``learn_on_batch(params, params_target, optimizer_state, batch)`` regresses
Q(s)[a] on  r + (1 - terminal) * gamma**n * max_a Q_target(s')  (dqn.py:74-88): the next states go through the TARGET
parameters -- a copy of the online parameters refreshed every ``target_update_frequency`` steps (dqn.py:46-54) -- and the
states through the online ones (C ABI: isdqn_net_learn_on_batch_target, the iS-DQN kernels with n_heads = 1).
Same observable differences as iSDQN (int seed, in-place device handles, device loss accumulation)."""
from __future__ import annotations

import numpy as np
import torch

from slimdqn import _mixture
from slimdqn._engine import NetOptions, check_munchausen
from slimdqn.networks._agent import DeviceParams, EngineAgent, Stage, check_ema_tau, check_soft_shift_tau
from slimdqn.networks.architectures.dqn import DQNNet


class DQN(EngineAgent):
    def __init__(
        self,
        key,
        observation_dim,
        n_actions,
        features: list,
        layer_norm: bool,
        architecture_type: str,
        learning_rate: float,
        gamma: float,
        update_horizon: int,
        data_to_update: int,
        target_update_frequency: int,
        adam_eps: float = 1e-8,
        batch_size: int = 32,
        precision: str = "bf16x3",
        device: str | None = None,
        use_graph: bool = True,
        n_bins: int = 0,
        min_value: float = -100.0,
        max_value: float = 100.0,
        sigma: float = 3.0,
        double_q: bool = False,
        munchausen_tau: float = 0.0,
        munchausen_alpha: float = 0.9,
        munchausen_clip: float = -1.0,
        n_quantiles: int = 0,
        huber_delta: float = 0.0,
        categorical: bool = False,
        dueling: bool = False,
        max_grad_norm: float = 0.0,
        noisy: bool = False,
        noisy_sigma0: float = 0.5,
        augment_pad: int = 0,
        ema_tau: float = 0.0,
        *,
        weight_decay: float = 0.0,
        weight_decay_all: bool = False,
        cql_alpha: float = 0.0,
        soft_shift_tau: float = 0.0,
        prune_sparsity: float = 0.0,
        prune_start: int = 0,
        prune_end: int = 0,
        prune_period: int = 0,
        rem_heads: int = 0,
        weight_projection: bool = False,
    ):
        """The option keywords from ``n_bins`` to ``noisy_sigma0``: NetOptions (slimdqn/_engine.py); ``augment_pad``:
        EngineAgent._init_engine_agent.  Particular to DQN:
        ``ema_tau`` > 0: EMA (Polyak) target network (include/isdqn_hip.h, isdqn_net_ema; SR-SPR, BBF) -- every gradient step is
        followed by target <- (1 - tau) * target + tau * online on the device (noisy: ``target_sigma`` likewise), the last stage of
        ``_after_learn``; ``update_target_params`` then copies nothing and only reports its logs.  0 keeps the hard copy every ``target_update_frequency`` steps.  Outside [0, 1]: ValueError.
        ``noisy``: the target network has a sigma of its own (copied with the parameters at every target update) and, in every learn
        step, a draw of its own (stream 1), as in Fortunato's DQN.
        ``double_q``: the online parameters pick the next action, the target parameters value it: one more forward per step.
        ``munchausen_tau`` > 0: the target parameters run over the states as well as the next states: about one more forward of B
        images per step.
        ``weight_decay`` / ``weight_decay_all``: AdamW (EngineAgent._init_engine_agent) on the online parameters; the target parameters
        are never the optimizer's and never decay.
        ``cql_alpha``: the conservative term (EngineAgent._init_engine_agent) on the online parameters' state rows.
        ``soft_shift_tau`` > 0 is refused (SOFT_SHIFT_REFUSED): one head; the soft target here is ``ema_tau``.
        ``prune_sparsity`` / ``prune_start`` / ``prune_end`` / ``prune_period``: gradual magnitude pruning (EngineAgent._init_pruning) of
        the online parameters; the target buffer is masked at every mask update, so its zeros stay zero under the hard copy and under
        ``ema_tau``, whose stage stands behind the apply launch (``_after_learn``).
        ``weight_projection``: Normalize-and-Project (EngineAgent._init_projection) of the online parameters; the target buffer is
        never projected itself.
        ``rem_heads`` = H > 0: REM, the random ensemble mixture (Agarwal et al. 2020; include/isdqn_hip.h, isdqn_batch_mixture) -- the
        network has H heads on one torso, every gradient step (the draw is part of the learn call: DESIGN.md section 6) draws a new
        convex combination of the heads on the device and regresses the mixture on the target network's
        mixture; acting, ``q_values``, ``loss`` and ``compute_target`` use the head average.  0 is off: the agent built without the
        argument.  Refused with ``noisy``, ``n_bins``, ``n_quantiles``, ``munchausen_tau`` and ``cql_alpha`` (slimdqn/_mixture.py)."""
        options = NetOptions.pick(locals())
        check_munchausen(double_q, munchausen_tau)  # (in front of the other rules, where this constructor has always asked it)
        options.check(architecture_type, features)
        self.ema_tau = check_ema_tau(ema_tau, supported=True)
        check_soft_shift_tau(soft_shift_tau)
        H = _mixture.check_rem_heads(rem_heads, noisy=noisy, n_bins=n_bins, n_quantiles=n_quantiles, munchausen_tau=munchausen_tau, cql_alpha=cql_alpha)
        if H:  # (off: the class default, and an engine of one head as ever)
            self.rem_heads = H
        self.use_graph = bool(use_graph)  # update_online_params on a device replay replays a captured step (networks/_agent.py)
        self.network = DQNNet([int(f) for f in features], architecture_type, max(H, 1) * (n_actions + (1 if dueling else 0)) * max(int(n_bins), int(n_quantiles), 1), layer_norm, False)
        self.data_to_update = data_to_update
        self.target_update_frequency = target_update_frequency
        self.target_params = None
        self._init_engine_agent(key, observation_dim, n_actions, max(H, 1), features, layer_norm, architecture_type, learning_rate,
                                gamma, update_horizon, adam_eps, batch_size, precision, device, options, augment_pad=augment_pad, weight_decay=weight_decay, weight_decay_all=weight_decay_all,
                                cql_alpha=cql_alpha, prune_sparsity=prune_sparsity, prune_start=prune_start, prune_end=prune_end,
                                prune_period=prune_period, weight_projection=weight_projection)
        self.target_params = self.params.copy()  # dqn.py:34
        self.target_sigma = self._engine.sigma.clone() if self.noisy else None  # (one persistent buffer, refreshed in place like the target)
        self.cumulated_loss = 0

    def _engine_changed(self, old) -> None:
        if self.target_params is not None:  # re-home the target copy on the new engine (same layout)
            self.target_params = DeviceParams(self._engine, self.target_params.tensor)

    # ------------------------------------------------------------------ dqn.py:40-57
    def update_online_params(self, step: int, replay_buffer):
        if step % self.data_to_update == 0:
            target = self._target_tensor(self.target_params)
            eng, rem = self._step_engine(replay_buffer), bool(self.rem_heads)

            def learn(cb):  # (the mixture draw is part of the learn call: one more node in front of it, which the key names)
                if rem:
                    eng.mixture_draw()
                eng.learn_on_batch_target(cb, target, **self._target_sigma_kw())

            # (what the draw writes is state of the step, like the EMA's target buffers: a capture's warm-up must not move either)
            g = self._graphed_update(replay_buffer, **self._captured_step(
                eng, learn, key=(target.data_ptr(), self.ema_tau) + (("rem",) if rem else ()), state=[eng.mix_count, eng.mix_alpha] if rem else []))
            if g is not None:  # (captured against the target BUFFER: update_target_params refreshes it in place, nothing is captured again)
                self._run_graph(g)
                return
            batch_samples = self._sample(replay_buffer)
            self.params, self.optimizer_state, _ = self.learn_on_batch(self.params, self.target_params, self.optimizer_state, batch_samples)
            self._eager_after_learn()  # (behind the step, not inside learn_on_batch: that stays a function of what it is given)
            if getattr(self, "priority_writeback", False) and hasattr(replay_buffer, "update_device"):  # (as the captured step does)
                replay_buffer.update_device(batch_samples, self._engine.priorities)
            # `cumulated_loss += loss` (dqn.py:47) happens on the device inside the step

    def _after_learn(self, eng) -> list:
        """learn . prune apply . projection . EMA of the target: DESIGN.md section 6.  The target averages masked and projected
        parameters and is never projected itself.  ``ema_tau`` stands in the base key of the step, so the stage has no tag."""
        stages = super()._after_learn(eng)
        if self.ema_tau > 0.0:
            target = self._target_tensor(self.target_params)
            stages.append(Stage((), lambda: self._ema_target(eng, target), (target,) + ((self.target_sigma,) if self.noisy else ())))
        return stages

    def _ema_target(self, eng, target: torch.Tensor) -> None:
        """target <- (1 - ema_tau) * target + ema_tau * online behind a gradient step (noisy: the target's sigma likewise)."""
        eng.ema(target, self.ema_tau)
        if self.noisy:
            eng.ema(self.target_sigma, self.ema_tau, online=eng.sigma)

    def update_target_params(self, step: int):
        if step % self.target_update_frequency == 0:
            # `self.target_params = self.params.copy()` (dqn.py:50) as an in-place refresh of ONE persistent buffer: the captured
            # step reads the target through a fixed pointer, so a target update neither re-captures nor re-instantiates a graph.
            # With ema_tau > 0 the target follows every gradient step instead: nothing is copied here
            if not self.ema_tau > 0.0:
                self.target_params.tensor.copy_(self.params.tensor)
                if self.noisy:
                    self.target_sigma.copy_(self._engine.sigma)
            eng = self._engine
            self.cumulated_loss = self.cumulated_loss + float(eng.losses_accum.cpu().numpy()[0])
            eng.losses_accum.zero_()
            logs = {"loss": self.cumulated_loss / (self.target_update_frequency / self.data_to_update)}
            self.cumulated_loss = 0
            logs.update(self._grad_clip_logs())
            logs.update(self._horizon_logs())
            return True, logs
        return False, {}

    # ------------------------------------------------------------------ dqn.py:59-88
    def _target_sigma_kw(self) -> dict:
        return dict(target_sigma=self.target_sigma) if self.noisy else {}

    def _target_tensor(self, params_target) -> torch.Tensor:
        t = self._bind(params_target)
        return self._engine.params if t is None else t

    def learn_on_batch(self, params, params_target, optimizer_state, batch_samples):
        """In-place gradient step; returns (params, optimizer_state, loss) like the reference (loss: device scalar)."""
        eng = self._engine_for(self._batch_len(batch_samples))
        self._load_bound(eng, self._bind(params))
        if self.rem_heads:
            eng.mixture_draw()
        losses = eng.learn_on_batch_target(self._c_batch(eng, batch_samples), self._target_tensor(params_target), **self._target_sigma_kw())
        return self.params, self.optimizer_state, losses[0]

    def loss_on_batch(self, params, params_target, samples):
        eng = self._engine_for(self._batch_len(samples))
        losses = eng.loss_on_batch_target(self._c_batch(eng, samples), self._target_tensor(params_target), params=self._bind(params))
        return losses[0]

    def compute_target(self, params, sample):
        """reward + (1 - terminal) * gamma**n * max_a Q_params(next_state) for ONE sample (dqn.py:84-88); host helper."""
        nq = self._mean_q(self._q_row(params, sample.next_state))
        return float(sample.reward) + (1.0 - float(sample.is_terminal)) * (self.gamma**self.update_horizon) * float(nq.max())

    def loss(self, params, params_target, sample):
        q = self._mean_q(self._q_row(params, sample.state))
        return float((q[int(sample.action)] - self.compute_target(params_target, sample)) ** 2)

    def q_values(self, params, state) -> np.ndarray:
        row = self._q_row(params, state).cpu().numpy()
        return row.reshape(-1, self.n_actions).mean(axis=0, dtype=np.float32) if self.rem_heads else row.reshape(self.n_actions)

    def _mean_q(self, row) -> np.ndarray:
        """float64 action values of one device row: the row itself, or the head average of a mixture agent (uniform alpha)."""
        q = row.cpu().numpy().reshape(-1).astype(np.float64)
        return q.reshape(-1, self.n_actions).mean(axis=0) if self.rem_heads else q

    def best_action(self, params, state, **kwargs):
        return self._best_action(params, state, 0)

    def best_actions(self, params, states, **kwargs) -> np.ndarray:
        return self._best_actions(params, states, np.zeros(len(states), dtype=np.int32))
