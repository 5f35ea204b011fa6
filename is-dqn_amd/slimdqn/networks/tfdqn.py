"""Target-free DQN with the reference's surface (slimdqn/networks/tfdqn.py:11-101) on the HIP engine.

One head; the next states go through the SAME parameters as the states (one forward on concat(state, next_state),
stop-gradient target, tfdqn.py:68-86): the iS-DQN step with a single head that is regressed on its own target
(C ABI: isdqn_net_learn_on_batch with n_heads = 1).  ``update_target_params`` only reports the loss (tfdqn.py:47-54).
BatchNorm variants are outside the hot-path scope."""
from __future__ import annotations

import numpy as np

from slimdqn._engine import NetOptions
from slimdqn.networks._agent import EngineAgent, check_ema_tau, check_soft_shift_tau
from slimdqn.networks.architectures.dqn import DQNNet


DOUBLE_Q_REFUSED = (
    "double_q has no effect on target-free DQN: its single head both selects and values the next action through the same "
    "parameters, so Q[argmax Q] == max Q and the update would be the one without the option; use DQN or iSDQN for Double "
    "Q-learning targets")


class TFDQN(EngineAgent):
    def __init__(
        self,
        key,
        observation_dim,
        n_actions,
        features: list,
        layer_norm: bool,
        batch_norm: bool,
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
        weight_projection: bool = False,
    ):
        """The option keywords from ``n_bins`` to ``noisy_sigma0``: NetOptions (slimdqn/_engine.py); ``augment_pad``:
        EngineAgent._init_engine_agent.  Particular to target-free DQN:
        ``double_q`` is refused: see DOUBLE_Q_REFUSED.
        ``munchausen_tau`` > 0 is, unlike ``double_q``, well defined here: the single head is regularised by its own stop-gradient policy.
        ``ema_tau`` > 0 is refused (EMA_REFUSED): there is no target network.  ``weight_decay`` / ``weight_decay_all``: AdamW; ``cql_alpha``: the conservative term
        (EngineAgent._init_engine_agent).  ``soft_shift_tau`` > 0 is refused (SOFT_SHIFT_REFUSED): one head, nothing to shift.
        ``prune_sparsity`` / ``prune_start`` / ``prune_end`` / ``prune_period``: gradual magnitude pruning (EngineAgent._init_pruning).
        ``weight_projection``: Normalize-and-Project (EngineAgent._init_projection).  The step is EngineAgent._after_learn's: learn,
        prune apply, projection."""
        if double_q:
            raise ValueError(DOUBLE_Q_REFUSED)
        options = NetOptions.pick(locals())
        check_ema_tau(ema_tau)
        check_soft_shift_tau(soft_shift_tau)
        options.check(architecture_type, features, batch_norm)
        self.use_graph = bool(use_graph)  # update_online_params on a device replay replays a captured step (networks/_agent.py)
        self.network = DQNNet([int(f) for f in features], architecture_type, (n_actions + (1 if dueling else 0)) * max(int(n_bins), int(n_quantiles), 1), layer_norm, batch_norm)
        self.data_to_update = data_to_update
        self.target_update_frequency = target_update_frequency
        self._init_engine_agent(key, observation_dim, n_actions, 1, features, layer_norm, architecture_type, learning_rate,
                                gamma, update_horizon, adam_eps, batch_size, precision, device, options, batch_norm=batch_norm,
                                augment_pad=augment_pad, weight_decay=weight_decay, weight_decay_all=weight_decay_all,
                                cql_alpha=cql_alpha, prune_sparsity=prune_sparsity, prune_start=prune_start, prune_end=prune_end,
                                prune_period=prune_period, weight_projection=weight_projection)
        self.cumulated_loss = 0

    # ------------------------------------------------------------------ tfdqn.py:38-54
    def update_online_params(self, step: int, replay_buffer):
        if step % self.data_to_update == 0:
            g = self._graphed_update(replay_buffer, **self._own_step(replay_buffer))
            if g is not None:
                self._run_graph(g)  # same draws, same kernels, same bits as the eager branch below
                return
            batch_samples = self._sample(replay_buffer)
            self.params, self.optimizer_state, _ = self.learn_on_batch(self.params, self.optimizer_state, batch_samples)
            self._eager_after_learn()

    def update_target_params(self, step: int):
        if step % self.target_update_frequency == 0:
            eng = self._engine
            self.cumulated_loss = self.cumulated_loss + float(eng.losses_accum.cpu().numpy()[0])
            eng.losses_accum.zero_()
            logs = {"loss": self.cumulated_loss / (self.target_update_frequency / self.data_to_update)}
            self.cumulated_loss = 0
            logs.update(self._grad_clip_logs())
            logs.update(self._horizon_logs())
            return True, logs
        return False, {}

    # ------------------------------------------------------------------ tfdqn.py:56-86
    def learn_on_batch(self, params, optimizer_state, batch_samples):
        eng = self._engine_for(self._batch_len(batch_samples))
        self._load_bound(eng, self._bind(params))
        losses = eng.learn_on_batch(self._c_batch(eng, batch_samples))
        return self.params, self.optimizer_state, losses[0]

    def loss_on_batch(self, params, samples):
        eng = self._engine_for(self._batch_len(samples))
        losses = eng.loss_on_batch(self._c_batch(eng, samples), params=self._bind(params))
        return losses[0], None

    def compute_target(self, sample, next_q_values):
        """reward + (1 - terminal) * gamma**n * max_a next_q (tfdqn.py:82-86); host helper."""
        nq = np.asarray(next_q_values, np.float64)
        r = np.asarray(sample.reward, np.float64)
        t = np.asarray(sample.is_terminal, np.float64)
        return r + (1 - t) * (self.gamma**self.update_horizon) * nq.max(-1)

    def q_values(self, params, state) -> np.ndarray:
        return self._q_row(params, state).cpu().numpy().reshape(self.n_actions)

    def best_action(self, params, state, **kwargs):
        return self._best_action(params, state, 0)

    def best_actions(self, params, states, **kwargs) -> np.ndarray:
        return self._best_actions(params, states, np.zeros(len(states), dtype=np.int32))
