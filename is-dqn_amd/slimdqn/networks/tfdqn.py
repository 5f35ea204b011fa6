"""Target-free DQN with the reference's surface (slimdqn/networks/tfdqn.py:11-101) on the HIP engine.

One head; the next states go through the SAME parameters as the states (one forward on concat(state, next_state),
stop-gradient target, tfdqn.py:68-86): the iS-DQN step with a single head that is regressed on its own target
(C ABI: isdqn_net_learn_on_batch with n_heads = 1).  ``update_target_params`` only reports the loss (tfdqn.py:47-54).
BatchNorm variants are outside the hot-path scope."""
from __future__ import annotations

import numpy as np

from slimdqn._engine import check_categorical, check_dueling, check_grad_clip, check_quantiles
from slimdqn.networks._agent import EngineAgent, check_ema_tau
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
    ):
        """``ema_tau`` > 0 is refused (EMA_REFUSED): there is no target network.
        ``augment_pad`` > 0: DrQ random-shift augmentation (Kostrikov et al. 2020; include/isdqn_hip.h, isdqn_replay_augment_shift) --
        every gradient step trains on its sampled batch with each state stack and each next-state stack shifted by a draw of its own in
        [-pad, pad]^2, borders replicated, on the device (eager and captured alike; the device counter ``aug_count`` selects the
        draws).  Acting and ``recycle_dormant`` see the frames as stored.  Every torso but 'fc' (ValueError); needs the device replay.
        0 is off.
        ``noisy``: NoisyNet exploration (Fortunato et al. 2018; include/isdqn_hip.h, isdqn_noisy_layout) -- every Dense layer, the head
        included, carries factorised Gaussian noise with a learned scale sigma (initialised to ``noisy_sigma0`` / sqrt(fan-in)); every acting
        call on the agent's own parameters draws first (one draw serves all rows of a batched call), every learn step draws first, and
        ``noisy_eval`` = True (or the ``noisy_evaluation()`` context) acts with the mean network.  ``get_model()`` then carries
        "sigma_kernel" / "sigma_bias" beside the Dense leaves.  The epsilon schedule is the caller's: set it to 0 to explore by noise alone.
        Not with batch_norm, the impala torso or ``max_grad_norm`` > 0 (ValueError).
        ``max_grad_norm`` > 0 (``inf`` allowed): clip the gradient by its global norm in front of Adam, as
        optax.clip_by_global_norm chained with optax.adam does (include/isdqn_hip.h, isdqn_net_config::max_grad_norm); the norm stays on
        the device and ``update_target_params`` adds ``grad_norm`` (the mean over the interval's gradient steps) and
        ``grad_clipped_fraction`` to its logs.  ``inf`` measures and never clips; 0 is off.  Negative or NaN, batch_norm or the impala
        torso: ValueError.
        ``dueling``: dueling value / advantage heads (Wang et al. 2016; include/isdqn_hip.h, isdqn_net_config::dueling) -- the last
        Dense holds a value row and ``n_actions`` advantage rows per head (per bin / quantile with those heads), read from the two
        halves of the last hidden layer and combined on the device; every loss, target and acting rule then runs on the combined
        values.  Needs a hidden Dense layer of even width; not with batch_norm or the impala torso (ValueError).
        ``categorical``: with ``n_bins`` > 0, train the histogram heads on the C51 categorical projection loss (include/isdqn_hip.h,
        isdqn_net_config::categorical) instead of HL-Gauss: same heads, same acting, ``sigma`` ignored.  Not without ``n_bins``, nor with
        ``n_quantiles`` > 0 or Munchausen targets (ValueError).
        ``n_quantiles`` > 0: QR-DQN heads -- each action of each head predicts ``n_quantiles`` quantile values and trains on the
        quantile-regression loss with kappa = ``huber_delta`` (include/isdqn_hip.h, isdqn_net_config::n_quantiles); acting uses
        their means.  Not with ``n_bins`` > 0, Munchausen targets or batch_norm (ValueError).
        ``huber_delta``: 0 keeps the reference's squared TD error; > 0 trains on the Huber loss (with quantile heads: kappa).
        ``munchausen_tau`` > 0: Munchausen targets (include/isdqn_hip.h, isdqn_net_config::munchausen_tau) -- unlike ``double_q``
        well defined here: the single head is regularised by its own stop-gradient policy.
        ``n_bins`` > 0: HL-Gauss histogram loss over [min_value, max_value] with std ``sigma`` (include/isdqn_hip.h).
        ``double_q`` is refused: see DOUBLE_Q_REFUSED."""
        if double_q:
            raise ValueError(DOUBLE_Q_REFUSED)
        check_ema_tau(ema_tau)
        check_dueling(dueling, architecture_type, features, batch_norm)
        check_grad_clip(max_grad_norm, architecture_type, batch_norm)
        check_categorical(categorical, n_bins, n_quantiles, munchausen_tau)
        check_quantiles(n_quantiles, n_bins, munchausen_tau, batch_norm)
        self.use_graph = bool(use_graph)  # update_online_params on a device replay replays a captured step (networks/_agent.py)
        self.network = DQNNet([int(f) for f in features], architecture_type, (n_actions + (1 if dueling else 0)) * max(int(n_bins), int(n_quantiles), 1), layer_norm, batch_norm)
        self.data_to_update = data_to_update
        self.target_update_frequency = target_update_frequency
        self._init_engine_agent(key, observation_dim, n_actions, 1, features, layer_norm, architecture_type, learning_rate,
                                gamma, update_horizon, adam_eps, batch_size, precision, device, batch_norm=batch_norm,
                                n_bins=n_bins, min_value=min_value, max_value=max_value, sigma=sigma, munchausen_tau=munchausen_tau,
                                munchausen_alpha=munchausen_alpha, munchausen_clip=munchausen_clip, n_quantiles=n_quantiles,
                                huber_delta=huber_delta, categorical=categorical, dueling=dueling, max_grad_norm=max_grad_norm,
                                noisy=noisy, noisy_sigma0=noisy_sigma0, augment_pad=augment_pad)
        self.cumulated_loss = 0

    # ------------------------------------------------------------------ tfdqn.py:38-54
    def update_online_params(self, step: int, replay_buffer):
        if step % self.data_to_update == 0:
            g = self._graphed_update(replay_buffer)
            if g is not None:
                self._run_graph(g)  # same draws, same kernels, same bits as the eager branch below
                return
            batch_samples = self._sample(replay_buffer)
            self.params, self.optimizer_state, _ = self.learn_on_batch(self.params, self.optimizer_state, batch_samples)

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
