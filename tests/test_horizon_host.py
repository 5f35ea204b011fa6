"""Horizon windows, the part that needs no GPU (include/isdqn_hip.h, isdqn_replay_gather_horizon; ReplayBuffer(horizon_window=True)):
the host tables of the real buffer (storage on the CPU) cut at every horizon m <= n_max by the numpy gather of tests/helpers/horizon.py
give the elements the oracle replay builds at update_horizon = m; eviction never recycles a frame a live window names; the annealing
schedule; deliberately wrong readings of the definition fail the same comparison; and a buffer without the option is the buffer it was."""
import numpy as np
import pytest

from oracle.replay_buffer import ReplayBuffer as OracleRB, TransitionElement as OT
from oracle.samplers import UniformSamplingDistribution as OracleUniform
from tests.helpers import horizon as hz

STACK, N_MAX = 3, 5
GAMMA = 0.96875  # 31 / 32: a float32 value whose powers up to N_MAX are exact, so the oracle's gamma ** k and the running product agree


def _replay(capacity, horizon_window=True, n=N_MAX, stack=STACK, gamma=GAMMA):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    return ReplayBuffer(UniformSamplingDistribution(0, device="cpu"), 8, capacity, stack_size=stack, update_horizon=n, gamma=gamma,
                        device="cpu", horizon_window=horizon_window)


def _feed(rb, episodes, make=None):
    from slimdqn.sample_collection.replay_buffer import TransitionElement

    make = make or TransitionElement
    for index, action, reward, terminal, end in hz.transitions(episodes):
        rb.add(make(hz.frame_of(index), action, reward, terminal, end))


@pytest.fixture(scope="module")
def stream():
    return hz.seeded_stream(seed=0)


@pytest.fixture(scope="module")
def filled(stream):
    """The real buffer after the whole stream (capacity above the element count: nothing evicted), flushed."""
    rb = _replay(8192)
    _feed(rb, stream)
    rb._flush()
    return rb


@pytest.fixture(scope="module")
def oracle_elements(stream):
    """For every m in 1..N_MAX: the oracle replay at update_horizon = m after the stream, as {state bytes: [element, ...]}."""
    out = {}
    for m in range(1, N_MAX + 1):
        orb = OracleRB(OracleUniform(0), 8, 8192, stack_size=STACK, update_horizon=m, gamma=GAMMA)
        _feed(orb, stream, make=OT)
        by_state = {}
        for e in orb._memory.values():
            by_state.setdefault(np.ascontiguousarray(e.state).tobytes(), []).append(e)
        out[m] = (orb.add_count, by_state)
    return out


def _tables(rb):
    """The buffer's host tables of its live elements in slot order, windows as observation indices (through its CPU frame store)."""
    n = min(rb.add_count, rb._max_capacity)
    store = np.concatenate([rb._frames.numpy(), np.zeros((1, 4), np.uint8)])  # (slot -1 reads the zero frame appended here)
    window = hz.index_of(store[rb._h_elem_window[:n]])
    return dict(window=window, steps=rb._h_elem_steps[:n], len=rb._h_elem_len[:n], action=rb._h_elem_action[:n], terminal=rb._h_elem_terminal[:n])


def _stacks(index_rows):
    """(rows, 2, 2, stack) uint8 stacks of rows of observation indices (-1: the zero frame), the oracle's layout."""
    rows = np.asarray(index_rows)
    out = np.zeros(rows.shape[:1] + (2, 2, rows.shape[1]), np.uint8)
    for i, row in enumerate(rows):
        for c, index in enumerate(row):
            if index >= 0:
                out[i, :, :, c] = hz.frame_of(int(index))
    return out


def _compare_with_oracle(t, oracle, m, variant=None):
    """Every element of the tables ``t``, cut at horizon m, against THE oracle element at m that has its state: matched exactly once,
    state / next state / action / terminal exact, the float64 return to 1e-12.  Returns the number of mismatching elements."""
    n = len(t["len"])
    ids, action, reward, terminal, discount = hz.gather(t["window"], t["steps"], t["len"], t["action"], t["terminal"], STACK, N_MAX, range(n), m,
                                                        GAMMA, variant=variant, reward_dtype=np.float64)
    _count, by_state = oracle[m]
    state, nxt = _stacks(ids[:, :STACK]), _stacks(ids[:, STACK:])
    bad, matched = 0, set()
    for i in range(n):
        found = by_state.get(state[i].tobytes(), [])
        assert len(found) == 1, "a state of the n_max buffer must be the state of exactly one element at m"
        e = found[0]
        assert id(e) not in matched
        matched.add(id(e))
        ok = (np.array_equal(nxt[i], e.next_state) and action[i] == e.action and bool(terminal[i]) == bool(e.is_terminal)
              and abs(float(reward[i]) - float(e.reward)) <= 1e-12)
        bad += not ok
    assert np.array_equal(discount, np.full(n, np.float32(GAMMA ** m)))
    return bad


# ------------------------------------------------------------------ 1. the oracle comparison
def test_tables_equal_the_restatement_from_trajectory_lists(stream, filled):
    want = hz.window_tables(stream, STACK, N_MAX)
    got = _tables(filled)
    assert filled.add_count == len(want["len"]) == hz.n_elements(stream, N_MAX)
    for name in ("window", "steps", "len", "action", "terminal"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    # the tables at n_max are still filled: the element table's ids are the window's two ends
    n = filled.add_count
    np.testing.assert_array_equal(filled._h_elem_frames[:n, :STACK], filled._h_elem_window[:n, :STACK])
    np.testing.assert_array_equal(filled._h_elem_frames[:n, STACK:], filled._h_elem_window[:n, N_MAX:])
    # and the flush carried the three tables to the (CPU) device copies
    np.testing.assert_array_equal(filled._d_elem_window.numpy()[:n], filled._h_elem_window[:n])
    np.testing.assert_array_equal(filled._d_elem_steps.numpy()[:n], filled._h_elem_steps[:n])
    np.testing.assert_array_equal(filled._d_elem_len.numpy()[:n], filled._h_elem_len[:n])


@pytest.mark.parametrize("m", range(1, N_MAX + 1))
def test_every_horizon_gives_the_oracle_elements(stream, filled, oracle_elements, m):
    t = _tables(filled)
    assert _compare_with_oracle(t, oracle_elements, m) == 0
    # the counts: the buffer at m holds more elements -- the states within n_max - m steps in front of a truncation, which the
    # n_max buffer never emits (the accepted loss)
    count_m, by_state = oracle_elements[m]
    assert count_m == hz.n_elements(stream, m) == sum(len(v) for v in by_state.values())
    assert filled.add_count == hz.n_elements(stream, N_MAX) <= count_m
    truncated_tail = sum(min(len(a), N_MAX) - min(len(a), m) for _f, a, _r, term in stream if not term)
    assert count_m - filled.add_count == truncated_tail
    if m < N_MAX:
        assert truncated_tail > 0


# ------------------------------------------------------------------ 2. eviction
def test_eviction_keeps_every_frame_a_live_window_names(stream):
    capacity = 97
    rb = _replay(capacity)
    want = hz.window_tables(stream, STACK, N_MAX)
    assert len(want["len"]) > 3 * capacity  # "three times as many adds"
    from slimdqn.sample_collection.replay_buffer import TransitionElement

    checks = 0
    for k, (index, action, reward, terminal, end) in enumerate(hz.transitions(stream)):
        rb.add(TransitionElement(hz.frame_of(index), action, reward, terminal, end))
        if k % 53 and not end and not terminal:
            continue
        checks += 1
        rb._flush()
        live = range(max(0, rb.add_count - capacity), rb.add_count)
        # the windows of the live elements, read through the frame store, are the restated ones: no frame was recycled or rewritten
        slots = [key % capacity for key in live]
        store = np.concatenate([rb._frames.numpy(), np.zeros((1, 4), np.uint8)])
        np.testing.assert_array_equal(hz.index_of(store[rb._h_elem_window[slots]]), want["window"][list(live)])
        np.testing.assert_array_equal(rb._h_elem_steps[slots], want["steps"][list(live)])
        np.testing.assert_array_equal(rb._h_elem_len[slots], want["len"][list(live)])
        # reference counts: the window ids of the live elements and the trajectories' frames, nothing else; free frames unheld
        held = np.zeros_like(rb._refcount)
        for s in slots:
            for f in rb._h_elem_window[s]:
                if f >= 0:
                    held[f] += 1
        for entry in rb._trajectory:
            held[entry[0]] += 1
        np.testing.assert_array_equal(held, rb._refcount)
        assert all(rb._refcount[f] == 0 for f in rb._free) and len(set(rb._free)) == len(rb._free)
        assert not set(rb._free) & {int(f) for s in slots for f in rb._h_elem_window[s] if f >= 0}
    assert checks > 100 and rb.add_count == len(want["len"])


# ------------------------------------------------------------------ 3. the schedule
def test_schedule_end_points_monotonicity_and_bbf_values():
    from slimdqn.networks._agent import horizon_schedule

    args = (10, 3, 0.97, 0.997, 10_000)
    assert horizon_schedule(*args, 0) == (10, np.float32(0.97)) and horizon_schedule(*args, 10_000) == (3, np.float32(0.997))
    assert horizon_schedule(*args, 10**9) == (3, np.float32(0.997))
    ns, gs = zip(*(horizon_schedule(*args, t) for t in range(0, 10_001, 7)))
    assert all(a >= b for a, b in zip(ns, ns[1:])) and set(ns) == set(range(3, 11))
    assert all(a <= b for a, b in zip(gs, gs[1:])) and all(g.dtype == np.float32 for g in gs)
    for t in (0, 1, 17, 4999, 5000, 9999, 10_000, 12_345):
        assert horizon_schedule(*args, t) == hz.schedule(*args, t)
    # half way: n = sqrt(10 * 3) = 5.48 -> 5; 1 - gamma = sqrt(0.03 * 0.003)
    n, g = horizon_schedule(*args, 5000)
    assert n == 5 and g == np.float32(1.0 - np.sqrt(0.03 * 0.003))
    # the other direction, and a constant one
    assert [horizon_schedule(1, 4, 0.9, 0.5, 3, t)[0] for t in range(5)] == [1, 2, 3, 4, 4]
    assert horizon_schedule(3, 3, 0.99, 0.99, 5, 2) == (3, np.float32(0.99))


def test_schedule_refusals():
    from slimdqn.networks._agent import EngineAgent

    agent = EngineAgent()
    agent._drop_graph = lambda: None
    for bad in [(3, 1, 0.9, 0.99, 0), (0, 1, 0.9, 0.99, 5), (3, 0, 0.9, 0.99, 5), (3, 1, 1.0, 0.99, 5), (3, 1, 0.9, -0.1, 5), (3, 1, float("nan"), 0.9, 5)]:
        with pytest.raises(ValueError):
            agent.set_horizon_schedule(*bad)
    with pytest.raises(ValueError, match="n_max >= 6"):
        agent.set_horizon_schedule(3, 6, 0.9, 0.99, 5, replay_buffer=_replay(16))
    with pytest.raises(ValueError, match="horizon_window=True"):
        agent.set_horizon_schedule(3, 1, 0.9, 0.99, 5, replay_buffer=_replay(16, horizon_window=False))
    agent.set_horizon_schedule(3, 1, 0.9, 0.99, 6, replay_buffer=_replay(16))
    ns, gs = agent._next_horizons(4)
    assert ns.dtype == np.int32 and gs.dtype == np.float32 and list(ns) == [hz.schedule(3, 1, 0.9, 0.99, 6, t)[0] for t in range(4)]
    assert agent._hz_step == 4 and agent._horizon_logs() == {"update_horizon": int(ns[-1]), "gamma": float(gs[-1])}


def test_replay_refusals():
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    for n in (0, 129):
        with pytest.raises(ValueError, match="1..128"):
            ReplayBuffer(UniformSamplingDistribution(0, device="cpu"), 8, 16, update_horizon=n, device="cpu", horizon_window=True)
    rb = _replay(16, horizon_window=False)
    rb.add_count = 1  # (the argument checks come first)
    with pytest.raises(ValueError, match="both or neither"):
        rb.gather(None, horizon=3)
    with pytest.raises(ValueError, match="horizon_window=True"):
        rb.gather(None, horizon=3, gamma=0.9)


# ------------------------------------------------------------------ 4. wrong readings of the definition
@pytest.mark.parametrize("variant", hz.VARIANTS)
def test_wrong_variants_fail_the_comparison(filled, oracle_elements, variant):
    """The tables hold zeros behind an element's end, which would hide a sum that runs over m steps: the comparison runs on a copy whose
    step rewards behind the end are poisoned -- the definition never reads them (the correct gather still matches everywhere), the wrong
    sum does."""
    t = _tables(filled)
    t["steps"] = t["steps"].copy()
    t["steps"][np.arange(N_MAX)[None] >= t["len"][:, None]] = 7.0
    failing = 0
    for m in range(1, N_MAX + 1):
        assert _compare_with_oracle(t, oracle_elements, m) == 0
        failing += _compare_with_oracle(t, oracle_elements, m, variant=variant)
    assert failing > 0


# ------------------------------------------------------------------ 5. off mode
def test_off_mode_is_the_buffer_it_was(stream):
    """horizon_window=False: no table, the host tables of a stream equal those of the n_max tables of an on buffer (which are filled as
    before), and a flush stages the sections it always did, in their order, with the same bytes."""
    off, on = _replay(97, horizon_window=False), _replay(97)
    short = stream[:60]
    _feed(off, short)
    _feed(on, short)
    for name in ("_h_elem_window", "_h_elem_steps", "_h_elem_len", "_d_elem_window", "_d_horizon"):
        assert not hasattr(off, name) and hasattr(on, name)
    for name in ("_h_elem_action", "_h_elem_reward64", "_h_elem_terminal", "_h_index_to_slot"):
        np.testing.assert_array_equal(getattr(off, name), getattr(on, name), err_msg=name)
    # (the frame SLOTS differ -- a window holds its frames longer, so the free list hands them out in another order -- the frames do not)
    off._flush()
    on._flush()
    content = lambda rb: hz.index_of(np.concatenate([rb._frames.numpy(), np.zeros((1, 4), np.uint8)])[rb._h_elem_frames])
    np.testing.assert_array_equal(content(off), content(on))
    _feed(off, stream[60:70])
    _feed(on, stream[60:70])
    assert off.add_count == on.add_count and list(off._memory.keys()) == list(on._memory.keys())

    def staged(rb):
        r = np.unique(np.asarray(rb._dirty_rows, dtype=np.int64))
        rows = (r.astype(np.int32), rb._h_elem_frames[r], rb._h_elem_action[r], rb._h_elem_reward64[r].astype(np.float32), rb._h_elem_terminal[r])
        hrows = (rb._h_elem_window[r], rb._h_elem_steps[r], rb._h_elem_len[r]) if rb._horizon_window else None
        u, sections = rb._staged_sections(None, rows, None, hrows)
        return u, [(name, np.ascontiguousarray(a).tobytes()) for name, a in sections]

    u_off, s_off = staged(off)
    u_on, s_on = staged(on)
    assert [n for n, _ in s_off] == ["off_rows", "off_row_frames", "off_row_action", "off_row_reward", "off_row_terminal"]
    r = np.unique(np.asarray(off._dirty_rows, dtype=np.int64))
    assert [b for _, b in s_off] == [r.astype(np.int32).tobytes(), off._h_elem_frames[r].tobytes(), off._h_elem_action[r].tobytes(),
                                     off._h_elem_reward64[r].astype(np.float32).tobytes(), off._h_elem_terminal[r].tobytes()]
    assert [n for n, _ in s_on] == [n for n, _ in s_off] + ["horizon_window", "horizon_steps", "horizon_len"]  # behind everything else
    assert [b for _, b in s_on[-3:]] == [on._h_elem_window[r].tobytes(), on._h_elem_steps[r].tobytes(), on._h_elem_len[r].tobytes()]
    assert (u_off.n_rows, u_off.stack2, u_off.n_frames, u_off.n_index) == (u_on.n_rows, u_on.stack2, 0, 0)
    # the flush itself, on the CPU storage: the same element tables either way
    off._flush()
    on._flush()
    for name in ("_d_elem_action", "_d_elem_reward", "_d_elem_terminal", "_d_index_to_slot"):
        assert np.array_equal(getattr(off, name).numpy(), getattr(on, name).numpy()), name
    np.testing.assert_array_equal(off._d_elem_frames.numpy(), off._h_elem_frames)


def test_flags_and_their_refusals():
    from experiments.base import parser_argument as pa

    base = dict(update_horizon=10, gamma=0.97, anneal_period=0, update_horizon_end=None, gamma_end=None)
    pa.check_anneal(base)
    assert pa.replay_horizon_kwargs(base) == dict(update_horizon=10)
    for bad in (dict(update_horizon_end=3), dict(gamma_end=0.997), dict(anneal_period=-1), dict(anneal_period=5, update_horizon_end=0),
                dict(anneal_period=5, update_horizon_end=129), dict(anneal_period=5, gamma_end=1.0)):
        with pytest.raises(ValueError):
            pa.check_anneal({**base, **bad})
    bbf = {**base, "anneal_period": 10_000, "update_horizon_end": 3, "gamma_end": 0.997}
    pa.check_anneal(bbf)
    assert pa.anneal_schedule(bbf) == (10, 3, 0.97, 0.997, 10_000)
    assert pa.replay_horizon_kwargs(bbf) == dict(update_horizon=10, horizon_window=True)
    assert pa.replay_horizon_kwargs({**bbf, "update_horizon": 2, "update_horizon_end": 6})["update_horizon"] == 6
    assert pa.anneal_schedule({**base, "anneal_period": 7}) == (10, 10, 0.97, 0.97, 7)
