"""Offline training from logged transitions (not in the reference): a log of what an online run handed to its replay, and a training
loop that never steps an environment for data.

    TransitionLog(directory)     ``append`` writes the transitions of a run, in arrival order, into ``shard_%06d.npz`` files of
                                 ``observation`` (uint8 [n, h, w] frames or float32 [n, d] vectors), ``action`` int32, ``reward`` float32,
                                 ``terminal`` uint8 and ``episode_end`` uint8; ``-logrb DIR`` appends every transition handed to ``rb.add``.
    fill_replay(rb, directory)   replays the shards through ``rb.add`` in order: frame stacks, n-step returns, horizon windows and the sum
                                 tree are built by the code that builds them online.
    train_offline(...)           ``-offline DIR``: per epoch ``-ntspe`` gradient steps through ``agent.learn_steps``, cut at every target
                                 update, where ``update_target_params`` and the usual hooks run; ``-evals N`` environment steps of
                                 evaluation behind each epoch (epsilon = ``-ee``, nothing enters the replay).

The standard offline Atari agent is QR-DQN + CQL: ``dqn.py ... -qr -nq 200 -hd 1 -cql 1.0 -offline DIR``."""
import glob
import json
import os
import time

import numpy as np

from slimdqn.sample_collection.replay_buffer import TransitionElement

LOGRB_VECTOR_REFUSED = "-logrb / --log_replay writes one stream of transitions: with -nenvs > 1 the environments' streams interleave"
OFFLINE_UTD_REFUSED = "-offline / --offline_dir issues gradient steps only: -utd / --data_to_update must be 1"
OFFLINE_LOGRB_REFUSED = "-offline / --offline_dir adds nothing to the replay after the fill: -logrb / --log_replay has nothing to log"
OFFLINE_VECTOR_REFUSED = "-offline / --offline_dir evaluates on one environment: -nenvs must be 1"
EVALS_REFUSED = "-evals / --evaluation_steps must be >= 0, and means nothing without -offline / --offline_dir"
FIELDS = ("observation", "action", "reward", "terminal", "episode_end")
META = "meta.json"


class TransitionLog:
    def __init__(self, directory, shard_size=50_000, n_actions=None):
        """``n_actions``: kept in ``meta.json`` beside the shards (a run without an environment sizes its agent from it)."""
        assert shard_size >= 1
        self.directory, self.shard_size, self.n_actions = str(directory), int(shard_size), n_actions
        os.makedirs(self.directory, exist_ok=True)
        assert not shard_paths(self.directory), f"{self.directory} already holds a transition log"
        self.n_transitions = self._n_shards = 0
        self._rows = []
        self._obs = None  # (shape, dtype) of an observation

    def append(self, observation, action, reward, is_terminal, episode_end):
        obs = np.asarray(observation)
        obs = obs.astype(np.float32) if obs.dtype.kind == "f" else obs.astype(np.uint8)
        if self._obs is None:
            self._obs = (obs.shape, obs.dtype)
        assert (obs.shape, obs.dtype) == self._obs, "every observation of a log has the shape and type of the first"
        self._rows.append((obs.copy(), int(action), float(reward), bool(is_terminal), bool(episode_end)))
        self.n_transitions += 1
        if len(self._rows) == self.shard_size:
            self._write_shard()

    def _write_shard(self):
        if not self._rows:
            return
        obs, action, reward, terminal, end = zip(*self._rows)
        np.savez(os.path.join(self.directory, "shard_%06d.npz" % self._n_shards), observation=np.stack(obs), action=np.asarray(action, np.int32),
                 reward=np.asarray(reward, np.float32), terminal=np.asarray(terminal, np.uint8), episode_end=np.asarray(end, np.uint8))
        self._n_shards += 1
        self._rows = []

    def close(self):
        self._write_shard()
        meta = dict(n_transitions=self.n_transitions, n_actions=self.n_actions,
                    observation_shape=None if self._obs is None else list(self._obs[0]), observation_dtype=None if self._obs is None else str(self._obs[1]))
        json.dump(meta, open(os.path.join(self.directory, META), "w"), indent=4)


def shard_paths(directory):
    return sorted(glob.glob(os.path.join(str(directory), "shard_[0-9][0-9][0-9][0-9][0-9][0-9].npz")))


def dataset_size(directory) -> int:
    """Transitions in the shards of ``directory`` (reads the action arrays only)."""
    n = 0
    for path in shard_paths(directory):
        with np.load(path) as shard:
            n += int(shard["action"].shape[0])
    return n


def log_replay_adds(rb, log: TransitionLog) -> None:
    """``-logrb``: from here on every transition handed to ``rb.add`` is appended to ``log`` as well (the reward as the replay gets it)."""
    add = rb.add

    def logged_add(transition, stream=0, **kwargs):
        assert stream == 0, LOGRB_VECTOR_REFUSED
        log.append(transition.observation, transition.action, transition.reward, transition.is_terminal, transition.episode_end)
        return add(transition, stream=stream, **kwargs)

    rb.add = logged_add


def fill_replay(rb, directory) -> int:
    """Every logged transition through ``rb.add``, in order; returns their number.  A dataset larger than the replay's capacity is
    refused before anything is added: the first transitions would be evicted while the last ones arrive."""
    paths = shard_paths(directory)
    if not paths:
        raise ValueError(f"-offline: no shard_*.npz in {directory}")
    n = dataset_size(directory)
    if n > rb._max_capacity:
        raise ValueError(f"-offline: the dataset in {directory} holds {n} transitions, more than the replay's capacity -rbc {rb._max_capacity}")
    for path in paths:
        with np.load(path) as shard:
            cols = [shard[name] for name in FIELDS]
        for obs, action, reward, terminal, end in zip(*cols):
            rb.add(TransitionElement(observation=obs, action=int(action), reward=float(reward), is_terminal=bool(terminal), episode_end=bool(end)))
    return n


class DatasetShapes:
    """What an entry point reads off its environment to size the agent, read off a transition log instead (``-offline`` without
    ``-evals``: no environment is built)."""

    n_stacked_frames = 4  # (experiments/atari/common.py: make_replay's stack_size)

    def __init__(self, directory):
        paths = shard_paths(directory)
        if not paths:
            raise ValueError(f"-offline: no shard_*.npz in {directory}")
        with np.load(paths[0]) as shard:
            shape = tuple(shard["observation"].shape[1:])
        self.observation_shape = shape
        if len(shape) == 2:
            self.state_height, self.state_width = shape
        meta_path = os.path.join(str(directory), META)
        n_actions = json.load(open(meta_path)).get("n_actions") if os.path.exists(meta_path) else None
        if n_actions is None:  # (a log written without it: the largest action taken)
            n_actions = 0
            for path in paths:
                with np.load(path) as shard:
                    n_actions = max(n_actions, int(shard["action"].max()) + 1)
        self.n_actions = int(n_actions)


def environment_for(p: dict, make_environment):
    """The entry points' environment: ``make_environment(p)``, or the dataset's shapes when nothing will ever step one."""
    if p.get("offline_dir") and not p.get("evaluation_steps"):
        return DatasetShapes(p["offline_dir"])
    return make_environment(p)


def check_offline(p: dict) -> None:
    """-logrb with -nenvs > 1, -offline with -utd != 1, -logrb or -nenvs > 1, and a stray or negative -evals fail before anything is written."""
    if p.get("log_replay") and p.get("n_envs", 1) > 1:
        raise ValueError(LOGRB_VECTOR_REFUSED)
    if p.get("evaluation_steps", 0) < 0 or (p.get("evaluation_steps") and not p.get("offline_dir")):
        raise ValueError(EVALS_REFUSED)
    if p.get("offline_dir"):
        if p["data_to_update"] != 1:
            raise ValueError(OFFLINE_UTD_REFUSED)
        if p.get("log_replay"):
            raise ValueError(OFFLINE_LOGRB_REFUSED)
        if p.get("n_envs", 1) > 1:
            raise ValueError(OFFLINE_VECTOR_REFUSED)


def evaluate(rng, p, agent, env, n_steps: int):
    """``n_steps`` environment steps with epsilon = -ee, then the running episode to its end; nothing enters the replay.  Returns the
    finished episodes' (returns, lengths)."""
    from slimdqn.sample_collection.utils import select_action

    returns, lengths = [], []
    env.reset()
    ret, length, steps = 0.0, 0, 0
    while True:
        action = select_action(agent.best_action, agent.params, env.state, rng, env.n_actions, lambda _: p["epsilon_end"], 0)
        reward, absorbing = env.step(action)
        ret, length, steps = ret + reward, length + 1, steps + 1
        if absorbing or env.n_steps >= p["horizon"]:
            returns.append(ret)
            lengths.append(length)
            if steps >= n_steps:
                return returns, lengths
            env.reset()
            ret, length = 0.0, 0


def train_offline(rng, p: dict, agent, env, rb, after_target_update, analysis_logs):
    """The loop of ``-offline``: see the module docstring.  ``g`` counts gradient steps and stands where the online loop's environment
    step count stands (target updates, ReDo, resets, logs)."""
    from experiments.base.utils import save_data

    n_data = fill_replay(rb, p["offline_dir"])
    print(f"-offline: {n_data} transitions from {p['offline_dir']}, {rb.add_count} replay elements", flush=True)
    n_evals = int(p.get("evaluation_steps") or 0)
    tuf = int(agent.target_update_frequency)
    g = 0
    returns, lengths, gathered = [], [], []
    best = -float("inf")
    for idx_epoch in range(p["n_epochs"]):
        t_epoch = time.perf_counter()
        left = int(p["n_training_steps_per_epoch"])
        while left > 0:
            k = min(left, tuf - g % tuf)  # up to the next target-update boundary
            agent.learn_steps(k, rb)
            g, left = g + k, left - k
            updated, logs = agent.update_target_params(g)
            if updated:
                after_target_update(g, logs)
        rate = p["n_training_steps_per_epoch"] / max(time.perf_counter() - t_epoch, 1e-9)
        ep_returns, ep_lengths = evaluate(rng, p, agent, env, n_evals) if n_evals > 0 else ([], [])
        returns.append(ep_returns)
        lengths.append(ep_lengths)
        avg_return = float(np.mean(ep_returns)) if ep_returns else float("nan")
        avg_length = float(np.mean(ep_lengths)) if ep_lengths else float("nan")
        print(f"\nEpoch {idx_epoch}: {g} gradient steps, return {avg_return} averaged on {len(ep_returns)} evaluation episodes.\n", flush=True)
        p["wandb"].log({"epoch": idx_epoch, "n_training_steps": g, "avg_return": avg_return, "avg_length_episode": avg_length})
        gathered.append(np.asarray([avg_return, avg_length, g, rate], np.float32))
        model = None
        if not ep_returns or avg_return > best:  # (without evaluation: the latest model)
            best = max(best, avg_return) if ep_returns else best
            model = agent.get_model()
        save_data(p, returns, lengths, model, analysis_logs)
    return gathered
