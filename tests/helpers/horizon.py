"""Numpy restatements for the horizon windows (include/isdqn_hip.h, isdqn_replay_gather_horizon), written from the header text and
from plain trajectory lists -- none of it from the replay buffer's code:

  seeded_stream / frame_of / index_of   the transition stream the host tests feed (episodes of random length, terminal or truncated) and
                                        the 2 x 2 frames that hold their own index;
  window_tables                         the element tables a replay at n_max must hold after that stream;
  gather                                the gather definition in float64, one operation at a time (and its deliberately wrong variants);
  schedule                              the annealing of the update horizon and the discount.
"""
import numpy as np


# ---------------------------------------------------------------------------------------------- the stream
def seeded_stream(seed=0, n_episodes=400, max_len=15, p_terminal=0.6, n_actions=5):
    """Episodes as plain lists: (first frame index, actions, rewards, terminal).  Step t of an episode observes frame first + t; the
    last step of an episode is terminal, or (terminal False) ends the episode by truncation.  The rewards are float32 values (as
    python floats), so the float32 step table holds them exactly."""
    rng = np.random.default_rng(seed)
    episodes, first = [], 0
    for _ in range(n_episodes):
        L = int(rng.integers(1, max_len + 1))
        episodes.append((first, [int(a) for a in rng.integers(0, n_actions, L)], [float(np.float32(r)) for r in rng.normal(size=L)],
                         bool(rng.random() < p_terminal)))
        first += L
    return episodes


def frame_of(index: int) -> np.ndarray:
    """The 2 x 2 uint8 frame of observation ``index``: the little-endian bytes of index + 1 (never the zero frame of the padding)."""
    return np.array([index + 1], dtype="<u4").view(np.uint8).reshape(2, 2).copy()


def index_of(frames) -> np.ndarray:
    """Inverse over the last four bytes of an array of frames [..., 4]: the observation index, -1 for the zero frame."""
    f = np.ascontiguousarray(np.asarray(frames, dtype=np.uint8).reshape(frames.shape[:-1] + (4,)))
    return f.view("<u4")[..., 0].astype(np.int64) - 1


def transitions(episodes):
    """(observation index, action, reward, is_terminal, episode_end) per step, in stream order."""
    for first, actions, rewards, terminal in episodes:
        L = len(actions)
        for t in range(L):
            last = t == L - 1
            yield first + t, actions[t], rewards[t], last and terminal, last and not terminal


def n_elements(episodes, m: int) -> int:
    """Elements a replay at update horizon m emits for the stream: every state of a terminal episode, and of a truncated one only
    those that have m steps behind them."""
    return sum(len(a) if terminal else max(len(a) - m, 0) for _f, a, _r, terminal in episodes)


# ---------------------------------------------------------------------------------------------- the tables
def window_tables(episodes, stack: int, n_max: int):
    """The rows a horizon-window replay at n_max holds for the stream, in emission order (episodes in order, states ascending), with
    OBSERVATION INDICES where the replay has frame slots: window [E][stack + n_max] (-1: zero frame), steps [E][n_max] float32, len [E],
    action [E], terminal [E] (at n_max)."""
    window, steps, length, action, terminal = [], [], [], [], []
    for first, actions, rewards, term in episodes:
        L = len(actions)
        for s in range(L if term else max(L - n_max, 0)):
            window.append([first + p if 0 <= p < L else -1 for p in range(s - stack + 1, s + n_max + 1)])
            steps.append([rewards[t] if t < L else 0.0 for t in range(s, s + n_max)])
            length.append(min(s + n_max, L) - s)
            action.append(actions[s])
            terminal.append(1 if term and s + n_max >= L else 0)
    return dict(window=np.asarray(window, np.int64).reshape(-1, stack + n_max), steps=np.asarray(steps, np.float32).reshape(-1, n_max),
                len=np.asarray(length, np.int32), action=np.asarray(action, np.int32), terminal=np.asarray(terminal, np.uint8))


# ---------------------------------------------------------------------------------------------- the gather
VARIANTS = ("sum_over_m", "next_state_at_me", "terminal_strictly_behind")


def gather(window, steps, length, action, terminal, stack: int, n_max: int, slots, horizon: int, gamma, variant=None, reward_dtype=np.float32):
    """isdqn_replay_gather_horizon for the element slots ``slots``: (frame ids [B][2 stack], action, float32 reward, terminal, float32
    discount).  ``gamma`` is taken as the float32 the kernel reads.  ``variant``: one of VARIANTS, a deliberately wrong reading of the
    definition (the sum over m steps instead of min(m, len); the next state at min(m, len); terminal only for m > len).
    ``reward_dtype=np.float64`` returns the float64 sums in front of the final rounding."""
    assert variant is None or variant in VARIANTS
    m = min(max(int(horizon), 1), n_max)
    G = np.float64(np.float32(gamma))
    e = np.asarray(list(slots), dtype=np.int64)
    window, steps, length = np.asarray(window)[e], np.asarray(steps, np.float32)[e], np.asarray(length)[e].astype(np.int64)
    me = np.minimum(m, length)
    ids = np.empty((len(e), 2 * stack), dtype=window.dtype)
    ids[:, :stack] = window[:, :stack]
    at = me if variant == "next_state_at_me" else np.full_like(me, m)
    ids[:, stack:] = window[np.arange(len(e))[:, None], at[:, None] + np.arange(stack)[None]]
    # rows side by side, the steps of a row one after the other: every product and every sum is one float64 operation of its own
    g, acc = np.float64(1.0), np.zeros(len(e), np.float64)
    for t in range(m):
        term = steps[:, t].astype(np.float64) * g
        acc = np.where((t < me) | (variant == "sum_over_m"), acc + term, acc)
        g = g * G
    behind = m > length if variant == "terminal_strictly_behind" else m >= length
    out_terminal = ((np.asarray(terminal)[e] != 0) & behind).astype(np.uint8)
    return ids, np.asarray(action)[e].astype(np.int32), acc.astype(reward_dtype), out_terminal, np.full(len(e), np.float32(g))


# ---------------------------------------------------------------------------------------------- the schedule
def schedule(n_start, n_end, gamma_start, gamma_end, period, t):
    """(horizon, float32 discount) of gradient step t: p = min(t / period, 1), n exponential between its ends and rounded to the
    nearest integer, 1 - gamma exponential between its ends; float64 on the host."""
    p = min(max(t, 0) / period, 1.0)
    if p == 0.0:
        return int(n_start), np.float32(gamma_start)
    if p == 1.0:
        return int(n_end), np.float32(gamma_end)
    n = np.exp(np.log(np.float64(n_start)) + (np.log(np.float64(n_end)) - np.log(np.float64(n_start))) * p)
    g = 1.0 - np.exp(np.log(1.0 - np.float64(gamma_start)) + (np.log(1.0 - np.float64(gamma_end)) - np.log(1.0 - np.float64(gamma_start))) * p)
    return int(np.rint(n)), np.float32(g)
