"""Command-line flags of the reference (experiments/base/parser_argument.py:27-156, 243-248), table-driven.

Every flag keeps its short name, long name, type and default so that launch scripts written for the reference
work unchanged.  ``add_base_arguments`` / ``add_isdqn_arguments`` return the list of long names they added,
which ``store_params`` uses to split ``parameters.json`` into shared and per-algorithm sections.
"""
import argparse
from typing import List

# (short, long, kwargs)
_BASE = [
    ("-en", "--experiment_name", dict(type=str, required=True, help="Experiment name.")),
    ("-s", "--seed", dict(type=int, required=True, help="Seed of the experiment.")),
    ("-dw", "--disable_wandb", dict(action="store_true", default=False, help="Disable wandb.")),
    ("-f", "--features", dict(type=int, nargs="*", default=[100, 100], help="List of features for the Q-networks.")),
    ("-rbc", "--replay_buffer_capacity", dict(type=int, default=10_000, help="Replay Buffer capacity.")),
    ("-bs", "--batch_size", dict(type=int, default=32, help="Batch size for training.")),
    ("-n", "--update_horizon", dict(type=int, default=1, help="Value of n in n-step TD update.")),
    ("-gamma", "--gamma", dict(type=float, default=0.99, help="Discounting factor.")),
    ("-lr", "--learning_rate", dict(type=float, default=3e-4, help="Learning rate.")),
    ("-horizon", "--horizon", dict(type=int, default=1_000, help="Horizon for truncation.")),
    ("-at", "--architecture_type", dict(type=str, default="fc", choices=["cnn", "impala", "fc"], help="Type of architecture.")),
    ("-ne", "--n_epochs", dict(type=int, default=50, help="Number of epochs to perform.")),
    ("-ntspe", "--n_training_steps_per_epoch", dict(type=int, default=10_000, help="Number of training steps per epoch.")),
    ("-utd", "--data_to_update", dict(type=float, default=1, help="Number of data points to collect per online Q-network update.")),
    ("-nis", "--n_initial_samples", dict(type=int, default=1_000, help="Number of initial samples before the training starts.")),
    ("-ee", "--epsilon_end", dict(type=float, default=0.01, help="Ending value for the linear decaying epsilon used for exploration.")),
    ("-ed", "--epsilon_duration", dict(type=float, default=1_000, help="Duration of epsilon's linear decay used for exploration.")),
    ("-a", "--analysis", dict(action="store_true", default=False, help="Flag to run analysis with the algorithm (srank and dormant neurons).")),
]
_ISDQN = [
    ("-nbi", "--n_bellman_iterations", dict(type=int, default=3, help="Number of bellman iterations to train in parallel. (K)")),
    ("-ln", "--layer_norm", dict(action="store_true", default=False, help="Flag to add layer norm.")),
    ("-bn", "--batch_norm", dict(action="store_true", default=False, help="Flag to add batch norm.")),
    ("-tuf", "--target_update_frequency", dict(type=int, default=200, help="Number of training steps before updating the target Q-network. (T)")),
]
_DQN = [_ISDQN[1], _ISDQN[3]]             # add_dqn_arguments: layer_norm, target_update_frequency (parser_argument.py:229-232)
_TFDQN = [_ISDQN[1], _ISDQN[2], _ISDQN[3]]  # add_tfdqn_arguments: layer_norm, batch_norm, target_update_frequency (:235-239)
# extras of this build (not in the reference): kept out of parameters.json comparisons by living in their own group
_ENGINE = [
    ("-prec", "--precision", dict(type=str, default="bf16x3", choices=["bf16x3", "bf16"], help="MFMA precision of the HIP engine.")),
    ("-per", "--prioritized", dict(action="store_true", default=False, help="Prioritized replay (sum-tree on the GPU) with TD-error writeback.")),
    ("-pe", "--priority_exponent", dict(type=float, default=1.0, help="alpha of prioritized replay: leaves hold priority ** alpha. Means nothing without -per.")),
    ("-isb", "--is_beta", dict(type=float, default=0.0, help="Importance-sampling exponent beta at the first gradient step; 0 = no importance-sampling weights. Needs -per.")),
    ("-isbe", "--is_beta_end", dict(type=float, default=None, help="beta at the last gradient step of the run (linear in between); default: constant -isb. Means nothing without -per and -isb.")),
    ("-hd", "--huber_delta", dict(type=float, default=0.0, help="0: squared TD error (the reference's loss); > 0: Huber loss with this delta. With -qr it is kappa of the quantile Huber loss (0: plain pinball loss); QR-DQN's usual value is 1.")),
    ("-hl", "--histogram_loss", dict(action="store_true", default=False, help="HL-Gauss histogram loss on the heads (the four flags below; off: scalar heads).")),
    # add_histogram_loss_parameters (reference parser_argument.py:199-228): names, types and defaults of the reference
    ("-nb", "--n_bins", dict(type=int, default=50, help="Number of bins composing the histogram.")),
    ("-minn", "--min_value", dict(type=float, default=-100, help="Value of the lowest learnable value of the target.")),
    ("-maxn", "--max_value", dict(type=float, default=100, help="Value of the highest learnable value of the target.")),
    ("-sigma", "--sigma", dict(type=float, default=3, help="Standard deviation of each target sample. If sigma / eta = 0.75, then sigma = 0.75 * (max_value - min_value) / n_bins")),
    ("-cat", "--categorical", dict(action="store_true", default=False, help="With -hl: train the histogram heads on the C51 categorical projection loss (Bellemare et al. 2017) instead of HL-Gauss; the atoms are the bin centres (the paper's 51 atoms on [-10, 10]: -nb 51 -minn -10.2 -maxn 10.2), -sigma is ignored. Needs -hl; not with -qr or -mq.")),
    ("-qr", "--quantile_regression", dict(action="store_true", default=False, help="QR-DQN quantile-regression heads (Dabney et al. 2018): every action of every head predicts -nq quantile values, acting uses their means; -hd is kappa. Not with -hl, -mq or -bn.")),
    ("-nq", "--n_quantiles", dict(type=int, default=32, help="Number of quantiles per action. Means nothing without -qr.")),
    ("-duel", "--dueling", dict(action="store_true", default=False, help="Dueling value / advantage heads (Wang et al. 2016): the last hidden layer of -f splits into two equal streams (-f 32 64 64 1024: two 512-wide ones), combined on the device as Q = V + A - mean(A), per bin with -hl and per quantile with -qr. Needs a hidden Dense layer of even width; not with -bn or -at impala.")),
    ("-gc", "--max_grad_norm", dict(type=float, default=0.0, help="Clip the gradient by its global norm in front of Adam (optax.clip_by_global_norm; the dueling, QR-DQN, C51 and Rainbow recipes use 10) and log grad_norm / grad_clipped_fraction at every target update; 0 = off, inf = measure and log only. Not with -bn or -at impala.")),
    ("-noisy", "--noisy_nets", dict(action="store_true", default=False, help="NoisyNet exploration (Fortunato et al. 2018): every Dense layer, the head included, carries factorised Gaussian noise with a learned scale; acting and every learn step draw on the device. The epsilon flags keep their meaning: -ee 0 -ed 1 explores by noise alone, as Rainbow does. Not with -bn, -at impala, -gc > 0 or -redo.")),
    ("-noisys", "--noisy_sigma0", dict(type=float, default=0.5, help="sigma_0 of the noisy layers: sigma starts at sigma_0 / sqrt(fan-in). Means nothing without -noisy.")),
    ("-aug", "--augment", dict(action="store_true", default=False, help="DrQ random-shift augmentation (Kostrikov et al. 2020; the DrQ(eps), DER, SPR and BBF recipes): every gradient step trains on its sampled batch with each state stack and each next-state stack shifted by a draw of its own in [-augp, augp]^2, borders replicated, on the device. With every image torso (-at cnn, -at impala, -ln, -bn) and every loss and target flag; not with -at fc.")),
    ("-augp", "--augment_pad", dict(type=int, default=4, help="Largest shift in pixels of -aug (DrQ: 4 on 84 x 84 frames), 0..127. Means nothing without -aug.")),
    ("-dq", "--double_q", dict(action="store_true", default=False, help="Double Q-learning targets: the online head (DQN: the online network) picks the next action, the target values it. Not for the target-free agents.")),
    ("-mq", "--munchausen", dict(action="store_true", default=False, help="Munchausen targets (Vieillard et al. 2020): soft-value bootstrap plus the scaled, clipped log-policy of the taken action (the three flags below). Not with -dq.")),
    ("-mqt", "--munchausen_tau", dict(type=float, default=0.03, help="Temperature tau of the soft value and of the policy softmax(Q / tau). Means nothing without -mq.")),
    ("-mqa", "--munchausen_alpha", dict(type=float, default=0.9, help="Scale alpha in [0, 1] of the log-policy bonus (0: soft-DQN targets). Means nothing without -mq.")),
    ("-mqc", "--munchausen_clip", dict(type=float, default=-1.0, help="Lower clip l0 <= 0 of tau * ln pi(a|s). Means nothing without -mq.")),
    ("-redo", "--redo_frequency", dict(type=int, default=0, help="ReDo (Sokar et al. 2023): training steps between two recycles of the dormant neurons of the hidden layers (incoming weights re-initialised, outgoing weights and Adam moments zeroed, on the device); 0 = off. A positive multiple of -tuf. Not with -bn or -at impala.")),
    ("-redot", "--redo_tau", dict(type=float, default=0.1, help="ReDo threshold tau: a neuron is dormant when its mean activation is at most tau times its layer's mean. Means nothing without -redo.")),
    ("-reset", "--reset_frequency", dict(type=int, default=0, help="Periodic resets (Nikishin et al. 2022; SR-SPR, BBF): training steps between two resets -- the top layers are re-initialised, the layers below shrunk towards a fresh initialisation (shrink and perturb), Adam's moments and step count cleared, on the device; a DQN's target network takes the same interpolation. 0 = off. A positive multiple of -tuf. With every torso and every agent.")),
    ("-resets", "--reset_shrink", dict(type=float, default=0.5, help="Shrink factor in [0, 1] of the layers below the reset ones: p <- s * p + (1 - s) * fresh (BBF: 0.5; 1 keeps them). Means nothing without -reset.")),
    ("-resetl", "--reset_top_layers", dict(type=int, default=0, help="Number of top layers that are re-initialised fully; 0 = every Dense layer (BBF, SR-SPR). Means nothing without -reset.")),
    ("-ema", "--ema_tau", dict(type=float, default=0.0, help="EMA (Polyak) target network: target <- (1 - tau) * target + tau * online after every gradient step, on the device, instead of a copy every -tuf steps (BBF, SR-SPR: 0.005); 0 = off, in [0, 1]. DQN only: iS-DQN's target is a head of the online network, the target-free agents have none.")),
    ("-sst", "--soft_shift_tau", dict(type=float, default=0.0, help="Soft head shift of iS-DQN: after every gradient step head k <- (1 - tau) * head k + tau * head k+1 for every k < -nbi, on the device, instead of the hard shift every -tuf steps (the counterpart of -ema, whose usual 0.005 fits here too; -nbi 1 is DQN's Polyak target on a shared torso); -tuf keeps the cadence of the logs, -redo and -reset. 0 = off, in [0, 1]. iS-DQN and its analysis agent only.")),
    ("-prune", "--prune_sparsity", dict(type=float, default=0.0, help="Gradual magnitude pruning (Zhu & Gupta 2017; Graesser et al. 2022; Obando-Ceron et al. 2024, with wide torsos such as -f 32 64 64 2048: -prune 0.95): final sparsity in [0, 1) of every conv and dense kernel but the last Dense, reached on the cubic schedule between -prunes and -prunee; the mask is chosen by magnitude on the device every -prunef steps and applied after every gradient step, gradients and Adam moments stay dense; 'sparsity' is logged at every target update. 0 = off (the calls and the bits of a run without the flag). With every agent; not with -noisy, -bn or -at impala.")),
    ("-prunes", "--prune_start", dict(type=int, default=0, help="Gradient step at which the sparsity of -prune leaves 0; 0 <= -prunes < -prunee. Means nothing without -prune.")),
    ("-prunee", "--prune_end", dict(type=int, default=100000, help="Gradient step from which the sparsity of -prune is the final one. Means nothing without -prune.")),
    ("-prunef", "--prune_frequency", dict(type=int, default=0, help="Steps between two mask updates of -prune, at target updates behind -redo and -reset: a positive multiple of -tuf (0 = -tuf). Means nothing without -prune.")),
    ("-nap", "--normalize_and_project", dict(default=False, action="store_true", help="Normalize-and-Project (Lyle et al. 2024): after every gradient step every conv and dense kernel but the last Dense is scaled back, on the device, to the norm it had at initialisation, so that the effective learning rate of a -ln network no longer decays as the parameter norm grows; biases and LayerNorm vectors are left alone; 'weight_scale_min' / 'weight_scale_max' are logged at every target update. Off = the calls and the bits of a run without the flag. Needs -ln; with every agent, -prune, -wd, -redo, -reset, -ema, -sst, -rr, -rem, -cql and every head and loss flag; not with -noisy, -bn or -at impala.")),
    ("-rr", "--replay_ratio", dict(type=int, default=1, help="Gradient steps per environment step past -nis (SR-SPR, BBF: 2 to 16), issued together as one captured update where the agent has one. Above 1, -tuf, -redo, -reset and the step of their logs count gradient steps, as -anneal and the -isb schedule always do. 1 = the loop without the flag. Above 1: -utd must be 1, -tuf a multiple of -rr, not with -offline.")),
    ("-wd", "--weight_decay", dict(type=float, default=0.0, help="AdamW (optax.adamw; BBF, SR-SPR: 0.1): decoupled weight decay -- every learn step also takes learning_rate * weight_decay of its value off every element of the conv and dense kernels, on the device, in every Adam kernel. 0 = off (plain Adam, the bits of a run without the flag); finite and >= 0. With every agent, torso, loss and -gc; not with -noisy.")),
    ("-wdall", "--weight_decay_all", dict(default=False, action="store_true", help="-wd also decays the biases and the LayerNorm / BatchNorm scales and biases (never the running statistics). Means nothing without -wd.")),
    ("-cql", "--cql_alpha", dict(type=float, default=0.0, help="CQL(H) (Kumar et al. 2020; offline QR-DQN + CQL: -qr -nq 200 -hd 1 -cql 1.0 -offline DIR): every loss also carries cql_alpha * (logsumexp_a Q(s, a) - Q(s, a_b)) per regressed head, on the device, its gradient dense over the actions. 0 = off (the bits of a run without the flag); finite and >= 0. With every agent, torso, head type, target flag, -gc, -noisy, -wd, -per, -aug and -anneal.")),
    ("-rem", "--rem_heads", dict(type=int, default=0, help="REM, the random ensemble mixture (Agarwal et al. 2020; offline: dqn.py ... -rem 200 -hd 1 -offline DIR): a DQN with this many heads on one torso, trained on a random convex combination of the heads drawn anew on the device for every gradient step, acting on the head average. 0 = off (a plain DQN, the bits of a run without the flag); at most 1024. dqn.py only; with -dq, -hd, -duel, -ema, -reset, -redo, -prune, -wd, -gc, -per / -isb, -anneal, -aug, -rr, -offline and -evals; not with -noisy, -hl, -qr, -mq or -cql.")),
    ("-logrb", "--log_replay", dict(type=str, default=None, help="Directory that receives every transition handed to the replay, in arrival order, as shard_%%06d.npz files (experiments/base/offline.py: TransitionLog) -- the dataset of a later -offline run. Single environment only: refused with -nenvs > 1.")),
    ("-offline", "--offline_dir", dict(type=str, default=None, help="Train from the transition log in this directory instead of an environment: the replay is filled once through its own add, then every epoch issues -ntspe gradient steps, with the target updates and their hooks (ReDo, resets, anneal, logs) counted in gradient steps. -utd must be 1; a dataset larger than -rbc is refused. Offline QR-DQN + CQL: -qr -nq 200 -hd 1 -cql 1.0 -offline DIR.")),
    ("-evals", "--evaluation_steps", dict(type=int, default=0, help="With -offline: environment steps of evaluation behind every epoch (epsilon = -ee, the running episode is finished, nothing enters the replay); 0 = none, and no environment is built.")),
    ("-anneal", "--anneal_period", dict(type=int, default=0, help="Anneal the update horizon and the discount (SR-SPR, BBF: -anneal 10000 -n 10 -nend 3 -gamma 0.97 -gammaend 0.997): over this many gradient steps, counted again from every -reset, n goes exponentially from -n to -nend and 1 - gamma from 1 - (-gamma) to 1 - (-gammaend); the replay keeps whole windows of max(-n, -nend) steps and every batch is cut at the step's horizon on the device. 0 = off. With every agent, torso, loss and target flag.")),
    ("-nend", "--update_horizon_end", dict(type=int, default=None, help="Final update horizon of -anneal (default: -n). Refused without -anneal.")),
    ("-gammaend", "--gamma_end", dict(type=float, default=None, help="Final discount of -anneal, in [0, 1) (default: -gamma). Refused without -anneal.")),
    ("-nenvs", "--n_envs", dict(type=int, default=1, help="Host environments stepped in lockstep with one batched best_actions forward (1 = the reference's loop).")),
    ("-nworkers", "--n_env_workers", dict(type=int, default=0, help="Host worker processes stepping the -nenvs environments in parallel (0 = in this process).")),
    ("-env", "--env_backend", dict(type=str, default="ale", choices=["ale", "synthetic"], help="'synthetic' replaces ALE by random frames (no ROMs needed).")),
]


def _add(parser: argparse.ArgumentParser, table) -> List[str]:
    for short, long, kw in table:
        parser.add_argument(short, long, **kw)
    return [long.lstrip("-") for _, long, _ in table]


def add_base_arguments(parser: argparse.ArgumentParser) -> List[str]:
    return _add(parser, _BASE)


def add_isdqn_arguments(parser: argparse.ArgumentParser) -> List[str]:
    return _add(parser, _ISDQN)


def add_dqn_arguments(parser: argparse.ArgumentParser) -> List[str]:
    return _add(parser, _DQN)


def add_tfdqn_arguments(parser: argparse.ArgumentParser) -> List[str]:
    return _add(parser, _TFDQN)


def add_analysisdqn_arguments(parser: argparse.ArgumentParser) -> List[str]:
    return _add(parser, _ISDQN)  # (parser_argument.py: the analysis agents take their base agents' flags)


def add_analysistfdqn_arguments(parser: argparse.ArgumentParser) -> List[str]:
    return _add(parser, _TFDQN)


def add_engine_arguments(parser: argparse.ArgumentParser) -> List[str]:
    return _add(parser, _ENGINE)


PRIORITIZED_FLAGS = ["priority_exponent", "is_beta", "is_beta_end"]  # stored in parameters.json with the algorithm's flags under -per


DOUBLE_Q_FLAGS = ["double_q"]  # stored with the algorithm's flags under -dq
TARGET_FREE_ALGOS = ("tfdqn", "analysistfdqn")


def check_double_q(p: dict, algo_name: str) -> None:
    """-dq on a target-free agent fails before anything is written, with the agent's own message."""
    if p.get("double_q") and algo_name in TARGET_FREE_ALGOS:
        from slimdqn.networks.tfdqn import DOUBLE_Q_REFUSED

        raise ValueError(DOUBLE_Q_REFUSED)


MUNCHAUSEN_FLAGS = ["munchausen", "munchausen_tau", "munchausen_alpha", "munchausen_clip"]  # stored with the algorithm's flags under -mq


def check_munchausen(p: dict) -> None:
    """-mq together with -dq fails before anything is written, with the agents' own message."""
    if p.get("munchausen") and p.get("double_q"):
        from slimdqn._engine import MUNCHAUSEN_DOUBLE_Q_REFUSED

        raise ValueError(MUNCHAUSEN_DOUBLE_Q_REFUSED)


def munchausen_kwargs(p) -> dict:
    """The agents' Munchausen keywords from parsed parameters: tau = 0 (off) unless -mq is given."""
    return dict(munchausen_tau=p["munchausen_tau"] if p["munchausen"] else 0.0, munchausen_alpha=p["munchausen_alpha"],
                munchausen_clip=p["munchausen_clip"])


# (-qr and -nq stay out of parameters.json like -hl, -hd and -prec: it holds the reference's groups, which the comparisons between runs read)
def check_quantiles(p: dict) -> None:
    """-qr together with -hl, -mq or -bn fails before anything is written, with the agents' own message."""
    if p.get("quantile_regression"):
        from slimdqn._engine import check_quantiles as check

        check(p["n_quantiles"], p["n_bins"] if p.get("histogram_loss") else 0, p["munchausen_tau"] if p.get("munchausen") else 0.0,
              bool(p.get("batch_norm", False)))


def quantile_kwargs(p) -> dict:
    """The agents' quantile-regression keyword from parsed parameters: n_quantiles = 0 (off) unless -qr is given."""
    return dict(n_quantiles=p["n_quantiles"] if p["quantile_regression"] else 0)


def quantile_kappa(p) -> float:
    """huber_delta for the agents whose entry points never took -hd (DQN, TF-DQN): kappa under -qr, else the 0 they always ran with."""
    return float(p["huber_delta"]) if p["quantile_regression"] else 0.0


# (-cat stays out of parameters.json like -hl, which it modifies)
def check_categorical(p: dict) -> None:
    """-cat without -hl, or with -qr or -mq, fails before anything is written, with the agents' own message."""
    if p.get("categorical"):
        from slimdqn._engine import check_categorical as check

        check(True, p["n_bins"] if p.get("histogram_loss") else 0, p["n_quantiles"] if p.get("quantile_regression") else 0,
              p["munchausen_tau"] if p.get("munchausen") else 0.0)


# (-duel stays out of parameters.json like -hl and -qr)
def check_dueling(p: dict) -> None:
    """-duel without a hidden Dense layer of even width, or with -bn or -at impala, fails before anything is written, with the
    agents' own message."""
    if p.get("dueling"):
        from slimdqn._engine import check_dueling as check

        check(True, p["architecture_type"], p["features"], bool(p.get("batch_norm", False)))


def dueling_kwargs(p) -> dict:
    """The agents' dueling keyword from parsed parameters; without -duel the keywords are the ones they were before the flag existed."""
    return dict(dueling=True) if p.get("dueling") else {}


# (-gc stays out of parameters.json like -duel)
def check_grad_clip(p: dict) -> None:
    """-gc negative or NaN, or > 0 with -bn or -at impala, fails before anything is written, with the agents' own message."""
    from slimdqn._engine import check_grad_clip as check

    check(p.get("max_grad_norm", 0.0), p["architecture_type"], bool(p.get("batch_norm", False)))


def grad_clip_kwargs(p) -> dict:
    """The agents' max_grad_norm keyword from parsed parameters; without -gc the keywords are the ones they were before the flag existed."""
    return dict(max_grad_norm=float(p["max_grad_norm"])) if p.get("max_grad_norm") else {}


# (-noisy and -noisys stay out of parameters.json like -duel)
def check_noisy(p: dict) -> None:
    """-noisy with -bn, -at impala, -gc > 0 or -redo fails before anything is written, with the agents' own message."""
    if p.get("noisy_nets"):
        from slimdqn._engine import check_noisy as check

        check(True, p["architecture_type"], bool(p.get("batch_norm", False)), p.get("max_grad_norm", 0.0), p.get("redo_frequency", 0) != 0)


def noisy_kwargs(p) -> dict:
    """The agents' noisy keywords from parsed parameters; without -noisy the keywords are the ones they were before the flag existed."""
    return dict(noisy=True, noisy_sigma0=float(p["noisy_sigma0"])) if p.get("noisy_nets") else {}


# (-aug and -augp stay out of parameters.json like -noisy)
def check_augment(p: dict, architecture_type=None) -> None:
    """-aug with -at fc, or with an -augp outside 0..127, fails before anything is written, with the agents' own message.
    ``architecture_type``: the torso of an entry point that fixes it (LunarLander's agents are built with "fc" whatever -at says)."""
    if p.get("augment"):
        from slimdqn._engine import check_augment as check

        check(p["augment_pad"], architecture_type or p["architecture_type"])


def augment_kwargs(p) -> dict:
    """The agents' augmentation keyword from parsed parameters; without -aug the keywords are the ones they were before the flag existed."""
    return dict(augment_pad=int(p["augment_pad"])) if p.get("augment") else {}


# (-redo and -redot stay out of parameters.json like -hl and -qr)
REDO_FREQUENCY_REFUSED = "-redo / --redo_frequency must be a positive multiple of -tuf / --target_update_frequency (recycling happens at target updates)"


def check_redo(p: dict) -> None:
    """-redo that is no positive multiple of -tuf, a tau that is negative or not finite, or -redo together with -bn or -at impala
    (the agents' own message) fails before anything is written."""
    if p.get("redo_frequency", 0) != 0:
        import math

        from slimdqn._engine import check_redo as check

        if p["redo_frequency"] < 0 or p["redo_frequency"] % p["target_update_frequency"] != 0:
            raise ValueError(REDO_FREQUENCY_REFUSED)
        if not (math.isfinite(p["redo_tau"]) and p["redo_tau"] >= 0.0):
            raise ValueError("-redot / --redo_tau must be finite and >= 0")
        check(p["architecture_type"], bool(p.get("batch_norm", False)))


# (-reset, -resets and -resetl stay out of parameters.json like -redo)
RESET_FREQUENCY_REFUSED = "-reset / --reset_frequency must be a positive multiple of -tuf / --target_update_frequency (resets happen at target updates)"
RESET_SHRINK_REFUSED = "-resets / --reset_shrink must be in [0, 1]"
RESET_TOP_LAYERS_REFUSED = "-resetl / --reset_top_layers must be >= 0 (0: every Dense layer)"


def check_reset(p: dict) -> None:
    """-reset that is no positive multiple of -tuf, a shrink factor outside [0, 1] or a negative layer count fails before anything is
    written.  Without -reset the other two flags mean nothing and are not looked at."""
    if p.get("reset_frequency", 0) != 0:
        if p["reset_frequency"] < 0 or p["reset_frequency"] % p["target_update_frequency"] != 0:
            raise ValueError(RESET_FREQUENCY_REFUSED)
        if not 0.0 <= p["reset_shrink"] <= 1.0:  # (NaN fails both comparisons)
            raise ValueError(RESET_SHRINK_REFUSED)
        if p["reset_top_layers"] < 0:
            raise ValueError(RESET_TOP_LAYERS_REFUSED)


def reset_kwargs(p) -> dict:
    """The keywords of ``agent.reset_parameters`` from parsed parameters."""
    return dict(shrink=float(p["reset_shrink"]), n_top_layers=int(p["reset_top_layers"]))


# (-ema stays out of parameters.json like -redo)
EMA_ALGOS = ("dqn",)
EMA_TAU_REFUSED = "-ema / --ema_tau must be in [0, 1] (0 = off)"


def check_ema(p: dict, algo_name: str) -> None:
    """-ema outside [0, 1], or > 0 on any agent but DQN (the agents' own message), fails before anything is written."""
    tau = p.get("ema_tau", 0.0)
    if not 0.0 <= tau <= 1.0:
        raise ValueError(EMA_TAU_REFUSED)
    if tau > 0.0 and algo_name not in EMA_ALGOS:
        from slimdqn.networks._agent import EMA_REFUSED

        raise ValueError(EMA_REFUSED)


def ema_kwargs(p) -> dict:
    """The agents' EMA keyword from parsed parameters; without -ema the keywords are the ones they were before the flag existed."""
    return dict(ema_tau=float(p["ema_tau"])) if p.get("ema_tau") else {}


# (-sst stays out of parameters.json like -ema)
SOFT_SHIFT_ALGOS = ("isdqn", "analysisdqn")
SOFT_SHIFT_TAU_REFUSED = "-sst / --soft_shift_tau must be in [0, 1] (0 = off)"


def check_soft_shift(p: dict, algo_name: str) -> None:
    """-sst outside [0, 1], or > 0 on any agent but iS-DQN and its analysis agent (the agents' own message), fails before anything is
    written."""
    tau = p.get("soft_shift_tau", 0.0)
    if not 0.0 <= tau <= 1.0:  # (NaN fails both comparisons)
        raise ValueError(SOFT_SHIFT_TAU_REFUSED)
    if tau > 0.0 and algo_name not in SOFT_SHIFT_ALGOS:
        from slimdqn.networks._agent import SOFT_SHIFT_REFUSED

        raise ValueError(SOFT_SHIFT_REFUSED)


def soft_shift_kwargs(p) -> dict:
    """The agents' soft-shift keyword from parsed parameters; without -sst the keywords are the ones they were before the flag existed."""
    return dict(soft_shift_tau=float(p["soft_shift_tau"])) if p.get("soft_shift_tau") else {}


# (-prune, -prunes, -prunee and -prunef stay out of parameters.json like -sst)
def check_pruning(p: dict) -> None:
    """-prune outside [0, 1), a schedule that is not 0 <= -prunes < -prunee, a -prunef that is no positive multiple of -tuf, or -prune
    together with -noisy, -bn or -at impala fails before anything is written, with the agents' own messages (slimdqn/_sparsity.py).
    Without -prune the other three flags mean nothing and are not looked at."""
    from slimdqn import _sparsity

    if _sparsity.check_sparsity(p.get("prune_sparsity", 0.0)) == 0.0:
        return
    _sparsity.check_network(noisy=bool(p.get("noisy_nets", False)), batch_norm=bool(p.get("batch_norm", False)),
                            architecture_type=p.get("architecture_type", "cnn"))
    _sparsity.check_schedule(p["prune_start"], p["prune_end"])
    _sparsity.check_period(p["prune_frequency"] or p["target_update_frequency"], p["target_update_frequency"])


def prune_kwargs(p) -> dict:
    """The agents' pruning keywords from parsed parameters; without -prune (or with -prune 0) the keywords are the ones they were before
    the flag existed."""
    if not p.get("prune_sparsity"):
        return {}
    return dict(prune_sparsity=float(p["prune_sparsity"]), prune_start=int(p["prune_start"]), prune_end=int(p["prune_end"]),
                prune_period=int(p["prune_frequency"] or p["target_update_frequency"]))


# (-nap stays out of parameters.json like -prune)
def check_projection(p: dict) -> None:
    """-nap together with -noisy, -bn or -at impala, or without -ln, fails before anything is written, with the agents' own messages
    (slimdqn/_projection.py)."""
    from slimdqn import _projection

    if not p.get("normalize_and_project"):
        return
    _projection.check_network(layer_norm=bool(p.get("layer_norm", False)), noisy=bool(p.get("noisy_nets", False)),
                              batch_norm=bool(p.get("batch_norm", False)), architecture_type=p.get("architecture_type", "cnn"))


def projection_kwargs(p) -> dict:
    """The agents' projection keyword from parsed parameters; without -nap the keywords are the ones they were before the flag existed."""
    return dict(weight_projection=True) if p.get("normalize_and_project") else {}


# (-rr stays out of parameters.json like -sst)
REPLAY_RATIO_REFUSED = "-rr / --replay_ratio must be >= 1 (1 = one gradient step every -utd environment steps)"
REPLAY_RATIO_UTD_REFUSED = "-rr / --replay_ratio above 1 issues several gradient steps per environment step: -utd / --data_to_update must be 1"
REPLAY_RATIO_OFFLINE_REFUSED = "-rr / --replay_ratio counts gradient steps per environment step: -offline / --offline_dir has no environment steps"
REPLAY_RATIO_TUF_REFUSED = ("-tuf / --target_update_frequency counts gradient steps under -rr / --replay_ratio and must be a multiple of it "
                            "(the gradient steps of one environment step never straddle a target update)")


def check_replay_ratio(p: dict) -> None:
    """-rr below 1, -rr above 1 with -utd other than 1 or with -offline, or a -tuf that is no multiple of -rr fails before anything is
    written."""
    rr = p.get("replay_ratio", 1)
    if rr < 1:
        raise ValueError(REPLAY_RATIO_REFUSED)
    if rr > 1 and p["data_to_update"] != 1:
        raise ValueError(REPLAY_RATIO_UTD_REFUSED)
    if rr > 1 and p.get("offline_dir"):
        raise ValueError(REPLAY_RATIO_OFFLINE_REFUSED)
    if p["target_update_frequency"] % rr != 0:
        raise ValueError(REPLAY_RATIO_TUF_REFUSED)


# (-wd and -wdall stay out of parameters.json like -reset)
def check_weight_decay(p: dict) -> None:
    """-wd negative, NaN or infinite, or > 0 with -noisy, fails before anything is written, with the agents' own message."""
    from slimdqn import _optimizer

    _optimizer.check_weight_decay(p.get("weight_decay", 0.0), noisy=bool(p.get("noisy_nets", False)))


def weight_decay_kwargs(p) -> dict:
    """The agents' weight-decay keywords from parsed parameters; without -wd (-wdall alone means nothing) the keywords are the ones they
    were before the flag existed."""
    if not p.get("weight_decay"):
        return {}
    return dict(weight_decay=float(p["weight_decay"]), weight_decay_all=bool(p.get("weight_decay_all", False)))


# (-cql stays out of parameters.json like -wd)
def check_conservative(p: dict) -> None:
    """-cql negative, NaN or infinite fails before anything is written, with the agents' own message."""
    from slimdqn import _conservative

    _conservative.check_cql_alpha(p.get("cql_alpha", 0.0))


def conservative_kwargs(p) -> dict:
    """The agents' keyword of the conservative term from parsed parameters; without -cql the keywords are the ones they were before the
    flag existed."""
    return dict(cql_alpha=float(p["cql_alpha"])) if p.get("cql_alpha") else {}


# (-rem stays out of parameters.json like -cql)
REM_ALGOS = ("dqn",)


def check_rem(p: dict, algo_name: str) -> None:
    """-rem outside [0, 1024], > 0 on any entry point but dqn.py, or together with -noisy, -hl, -qr, -mq or -cql fails before anything
    is written, with the agents' own messages (slimdqn/_mixture.py)."""
    from slimdqn import _mixture

    H = _mixture.check_rem_heads(p.get("rem_heads", 0))
    if H == 0:
        return
    if algo_name not in REM_ALGOS:
        raise ValueError(_mixture.REM_AGENT_REFUSED)
    _mixture.check_rem_heads(H, noisy=bool(p.get("noisy_nets", False)), n_bins=1 if p.get("histogram_loss") else 0,
                             n_quantiles=1 if p.get("quantile_regression") else 0, munchausen_tau=1.0 if p.get("munchausen") else 0.0,
                             cql_alpha=float(p.get("cql_alpha", 0.0) or 0.0))


def rem_kwargs(p) -> dict:
    """The DQN agent's mixture keyword from parsed parameters; without -rem the keywords are the ones they were before the flag
    existed."""
    return dict(rem_heads=int(p["rem_heads"])) if p.get("rem_heads") else {}


# (-logrb, -offline and -evals stay out of parameters.json like -cql)
def check_offline(p: dict) -> None:
    """-logrb with -nenvs > 1, -offline with -utd other than 1 and their kin fail before anything is written."""
    from experiments.base import offline

    offline.check_offline(p)


# (-anneal, -nend and -gammaend stay out of parameters.json like -reset)
ANNEAL_END_REFUSED = "-nend / --update_horizon_end and -gammaend / --gamma_end are the end points of -anneal / --anneal_period: they need it"
ANNEAL_MAX_HORIZON = 128  # slimdqn.sample_collection.replay_buffer.HORIZON_MAX


def check_anneal(p: dict) -> None:
    """-nend or -gammaend without -anneal, a negative period, a horizon outside 1..128 or a discount outside [0, 1) fails before
    anything is written."""
    period = p.get("anneal_period", 0)
    if period == 0:
        if p.get("update_horizon_end") is not None or p.get("gamma_end") is not None:
            raise ValueError(ANNEAL_END_REFUSED)
        return
    if period < 0:
        raise ValueError("-anneal / --anneal_period must be >= 0 (0 = off)")
    n0, n1, g0, g1 = anneal_schedule(p)[:4]
    if not (1 <= n0 <= ANNEAL_MAX_HORIZON and 1 <= n1 <= ANNEAL_MAX_HORIZON):
        raise ValueError(f"-anneal: -n and -nend must be in 1..{ANNEAL_MAX_HORIZON}")
    if not (0.0 <= g0 < 1.0 and 0.0 <= g1 < 1.0):  # (NaN fails both comparisons)
        raise ValueError("-anneal: -gamma and -gammaend must be in [0, 1)")


def anneal_schedule(p) -> tuple:
    """The arguments of ``agent.set_horizon_schedule`` from parsed parameters: (-n, -nend, -gamma, -gammaend, -anneal), an end point
    that is not given being its start."""
    n_end = p["update_horizon"] if p.get("update_horizon_end") is None else p["update_horizon_end"]
    gamma_end = p["gamma"] if p.get("gamma_end") is None else p["gamma_end"]
    return int(p["update_horizon"]), int(n_end), float(p["gamma"]), float(gamma_end), int(p["anneal_period"])


def replay_horizon_kwargs(p) -> dict:
    """The replay's horizon keywords from parsed parameters: under -anneal it keeps whole windows of the larger of -n and -nend; without
    it the keywords are the ones they were before the flag existed."""
    if not p.get("anneal_period"):
        return dict(update_horizon=p["update_horizon"])
    n0, n1 = anneal_schedule(p)[:2]
    return dict(update_horizon=max(n0, n1), horizon_window=True)


def check_engine_arguments(p: dict) -> None:
    if p["is_beta"] != 0.0 and not p["prioritized"]:
        raise ValueError("-isb / --is_beta weighs prioritized samples: it needs -per / --prioritized")


def n_gradient_steps(p: dict) -> int:
    """Gradient steps of a whole run (the length of the beta schedule): replay_ratio every data_to_update environment steps once
    n_initial_samples are in the buffer."""
    return max(1, int((p["n_epochs"] * p["n_training_steps_per_epoch"] - p["n_initial_samples"]) / p["data_to_update"]) * int(p.get("replay_ratio", 1)))


def histogram_loss_kwargs(p) -> dict:
    """The agents' histogram-loss keywords from parsed parameters: n_bins = 0 (scalar heads) unless -hl is given.  -cat adds
    categorical=True (the C51 loss on those heads); without it the keywords are the ones they were before the flag existed."""
    kw = dict(n_bins=p["n_bins"] if p["histogram_loss"] else 0, min_value=p["min_value"], max_value=p["max_value"], sigma=p["sigma"])
    if p.get("categorical"):
        kw["categorical"] = True
    return kw
