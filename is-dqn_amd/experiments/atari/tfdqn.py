"""Target-free DQN on Atari: the reference's entry point (experiments/atari/tfdqn.py) on the HIP engine.

    python experiments/atari/tfdqn.py -en LN1_cnn_Asterix -s 1 -f 32 64 64 512 -at cnn -ln ...

``experiment_name`` must end in ``_<Game>``; outputs go under experiments/atari/exp_output/<name>/tfdqn/.
"""
import os
import sys

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import numpy as np

from experiments.base.dqn import train
from experiments.atari.common import make_environment, make_replay, seeds
from experiments.base.utils import prepare_logs
from experiments.base.offline import environment_for
from experiments.base.parser_argument import histogram_loss_kwargs, munchausen_kwargs, quantile_kwargs, dueling_kwargs, grad_clip_kwargs, noisy_kwargs, ema_kwargs, weight_decay_kwargs, conservative_kwargs, prune_kwargs, projection_kwargs, augment_kwargs, quantile_kappa
from slimdqn.networks.tfdqn import TFDQN


def run(argvs=sys.argv[1:], root=None):
    from experiments.base import dist as replicas

    replicas.init_from_env()  # one process per GPU: picks this rank's device before the first GPU call (no-op alone)
    p = prepare_logs("atari", "tfdqn", argvs, root=root)
    q_seed, train_seed = seeds(p)
    env = environment_for(p, make_environment)  # (worker processes of a VectorEnv start here, before this process's first GPU call)
    rb = make_replay(p, prioritized=False)
    agent = TFDQN(
        q_seed,
        (env.state_height, env.state_width, env.n_stacked_frames),
        env.n_actions,
        features=p["features"],
        layer_norm=p["layer_norm"],
        batch_norm=p["batch_norm"],
        architecture_type=p["architecture_type"],
        learning_rate=p["learning_rate"],
        gamma=p["gamma"],
        update_horizon=p["update_horizon"],
        data_to_update=p["data_to_update"],
        target_update_frequency=p["target_update_frequency"],
        adam_eps=1.5e-4,
        batch_size=p["batch_size"],
        precision=p["precision"],
        **histogram_loss_kwargs(p),
        double_q=p["double_q"],
        **munchausen_kwargs(p),
        **quantile_kwargs(p),
        **dueling_kwargs(p),
        **grad_clip_kwargs(p),
        **noisy_kwargs(p),
        **ema_kwargs(p),
        **weight_decay_kwargs(p),
        **conservative_kwargs(p),
        **prune_kwargs(p),
        **projection_kwargs(p),
        **augment_kwargs(p),
        huber_delta=quantile_kappa(p),
    )
    try:
        out = train(np.random.default_rng(train_seed), p, agent, env, rb)
    finally:
        if hasattr(env, "close"):
            env.close()
    replicas.finalize()
    return out


if __name__ == "__main__":
    run()
