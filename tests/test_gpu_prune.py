"""Gradual magnitude pruning on the device (include/isdqn_hip.h, isdqn_net_prune_*) against the numpy restatement of
tests/helpers/prune.py, bit for bit -- nothing here is floating-point arithmetic --, and through the engine and the agents.

Shapes (tests/helpers/prune.py): fc on 8 observations with features [20, 14] -- tensors smaller than a workgroup, Dense_0's rows and
Dense_1's input lanes padded -- and [256, 256] -- Dense_1 spans 17 chunks of the selection and 64 workgroups of the apply pass; cnn 84x84x4
with features [8, 8, 8, 16] and LayerNorm -- Conv_0's [out][plane][ky][kx] form, kernels whose offsets are no multiple of 32, so that a
mask word is shared between a kernel and its neighbours.  The parameters are written by the test: every float of the buffer that is no
real prunable element holds a sentinel that must survive.

tests/test_prune_host.py shows that the wrong variants of the oracle (ties to the higher index, pruned elements not ranked first, padding
counted) differ from it on these inputs: a device result that equals the oracle equals none of them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from slimdqn import _hip
from tests.helpers import prune as hp

pytestmark = pytest.mark.gpu

CONFIGS = {"fc-20-14": hp.FC_SMALL, "fc-256-256": hp.FC_WIDE, "cnn": hp.CNN}


def _bits(t):
    return hp.bits(t.detach().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _engine(name):
    eng = hp.make_engine(CONFIGS[name], gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4)
    assert eng.set_pruning() == hp.real_counts(eng)
    return eng


def _mirror(eng, workspace=None):
    """The workspace's weight-mirror region as int32 words (a view)."""
    off, size = ctypes.c_int64(), ctypes.c_int64()
    assert eng.lib.isdqn_net_workspace_region(ctypes.byref(eng.cfg), b"wsplit", ctypes.byref(off), ctypes.byref(size)) == 0
    ws = eng.workspace if workspace is None else workspace
    return ws[off.value // 4 : (off.value + size.value) // 4].view(torch.int32)


def _mirror_of(eng, master: np.ndarray):
    """What isdqn_net_refresh_mirror makes of ``master`` in a second workspace."""
    second = torch.zeros_like(eng.workspace)
    dev = torch.from_numpy(np.ascontiguousarray(master)).to(eng.device)
    assert eng.lib.isdqn_net_refresh_mirror(ctypes.byref(eng.cfg), dev.data_ptr(), second.data_ptr(), _hip.stream_ptr(eng.device)) == 0
    torch.cuda.synchronize()
    return _mirror(eng, second).clone()


def _load(eng, params: np.ndarray, mask: np.ndarray):
    """``params`` and ``mask`` into the engine's buffers, recognisable moments, a current mirror."""
    eng.params.copy_(torch.from_numpy(params))
    eng.prune_mask.copy_(torch.from_numpy(mask.view(np.int32)))
    eng.adam_m.fill_(3.25)
    eng.adam_v.fill_(1.5)
    eng.adam_count.fill_(7)
    eng.rebuild_mirror()


def _check(eng, want_mask, want_params, what):
    got_mask, got = _bits(eng.prune_mask), _bits(eng.params)
    assert np.array_equal(got_mask, want_mask), f"{what}: {(got_mask != want_mask).sum()} mask words differ"
    assert np.array_equal(got, hp.bits(want_params)), f"{what}: {(got != hp.bits(want_params)).sum()} parameters differ"
    ref, mir = _mirror_of(eng, want_params), _mirror(eng)
    assert torch.equal(mir, ref), f"{what}: {(mir != ref).sum().item()} mirror words differ from a rebuild on the expected parameters"
    assert bool((eng.adam_m == 3.25).all()) and bool((eng.adam_v == 1.5).all()) and eng.adam_count.item() == 7


# ---------------------------------------------------------------------------------------------------------------- select and apply
@pytest.mark.parametrize("case", ["normal", "equal", "levels"])
@pytest.mark.parametrize("name", ["fc-20-14", "fc-256-256"])
def test_update_matches_the_oracle_and_a_second_update_nests(name, case):
    """An update at 30 % from a full mask, then one at 70 % on top of it: mask words, master and mirror equal the oracle's; the second
    mask keeps everything the first pruned; on a copy with a NULL workspace the master alone is written."""
    eng = _engine(name)
    n = hp.real_counts(eng)
    p0 = hp.case_params(eng, case)
    _load(eng, p0, hp.full_mask(eng))
    k1, k2 = [int(0.3 * x) for x in n], [int(0.7 * x) for x in n]
    m1, p1 = hp.update(eng, p0, hp.full_mask(eng), k1)
    assert hp.popcount_pruned(eng, m1) == k1 and not np.array_equal(hp.bits(p1), hp.bits(p0))
    eng.prune_update(k1)
    _check(eng, m1, p1, f"{name}/{case}: first update")
    m2, p2 = hp.update(eng, p1, m1, k2)
    assert hp.popcount_pruned(eng, m2) == k2 and not (m2 & ~m1).any()  # nested: no bit comes back
    eng.prune_update(k2)
    _check(eng, m2, p2, f"{name}/{case}: second update")
    # another buffer of the layout: the master alone, the engine's own parameters and mirror untouched
    copy = torch.from_numpy(p0).to(eng.device)
    before = _mirror(eng).clone()
    eng.prune_apply(params=copy)
    assert np.array_equal(_bits(copy), hp.bits(hp.apply(eng, p0, m2)))
    assert np.array_equal(_bits(eng.params), hp.bits(p2)) and torch.equal(_mirror(eng), before)


@pytest.mark.parametrize("name", ["fc-20-14", "fc-256-256"])
def test_counts_at_the_ends(name):
    """k = 0 (nothing changes), k = 1 (the first of the smallest), k = n (every real element, no padding lane) and k = 0 again: the
    result is a function of (params, old mask, k), so the bits come back and the zeros stay."""
    eng = _engine(name)
    n = hp.real_counts(eng)
    p = hp.case_params(eng, "levels", seed=3)
    mask = hp.full_mask(eng)
    _load(eng, p, mask)
    for k in ([0] * len(n), [1] * len(n), n, [0] * len(n)):
        mask, p = hp.update(eng, p, mask, k)
        eng.prune_update(k)
        _check(eng, mask, p, f"{name}: k = {k}")
    assert np.array_equal(mask, hp.full_mask(eng))
    assert (p[np.concatenate([hp.real_index(eng, i) for i in hp.prunable(eng)])] == 0).all() and (p == hp.SENTINEL).any()


def test_cnn_kernels_and_their_padded_lanes():
    """One update at sparsity 0.5 on the cnn torso: Conv_0's [out][plane][ky][kx] form, the [out][tap][in padded to 8] kernels and the first
    Dense's [pixel][c padded to 8] columns agree with the oracle."""
    eng = _engine("cnn")
    n = hp.real_counts(eng)
    for case in ("normal", "equal"):
        p0 = hp.case_params(eng, case, seed=5)
        _load(eng, p0, hp.full_mask(eng))
        k = [x // 2 for x in n]
        m, p = hp.update(eng, p0, hp.full_mask(eng), k)
        eng.prune_update(k)
        _check(eng, m, p, f"cnn/{case}")


def test_refusals_on_live_buffers_launch_nothing():
    eng = _engine("fc-20-14")
    p0 = hp.case_params(eng, "normal")
    _load(eng, p0, hp.full_mask(eng))
    n = hp.real_counts(eng)
    with pytest.raises(ValueError):
        eng.prune_update([n[0] + 1, 0])
    with pytest.raises(ValueError):
        eng.prune_update([1])
    k = (ctypes.c_int32 * 2)(n[0] + 1, 0)
    args = (ctypes.byref(eng.cfg), _hip.ptr(eng.params), k, _hip.ptr(eng.prune_mask), _hip.ptr(eng.prune_scratch), None, None)
    assert eng.lib.isdqn_net_prune_update(*args) == _hip.ERR_ARG
    assert eng.lib.isdqn_net_prune_apply(ctypes.byref(eng.cfg), eng.params.data_ptr() + 4, _hip.ptr(eng.prune_mask), None, None) == _hip.ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(_bits(eng.params), hp.bits(p0)) and np.array_equal(_bits(eng.prune_mask), hp.full_mask(eng))


# ---------------------------------------------------------------------------------------------------------------- the learn step
def _fields(eng, seed=17):
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    B, A = int(eng.cfg.batch_size), int(eng.cfg.n_actions)
    return dict(action=dev(rng.integers(0, A, B).astype(np.int32)), reward=dev(rng.normal(size=B).astype(np.float32)),
                terminal=dev((rng.random(B) < 0.3).astype(np.uint8)), state=dev(rng.normal(size=(B, 8)).astype(np.float32)),
                next_state=dev(rng.normal(size=(B, 8)).astype(np.float32)))


@pytest.mark.parametrize("trusted", [False, True])
def test_learn_step_then_apply(trusted):
    """From masked parameters: learn_on_batch + prune_apply equals learn_on_batch alone at every kept position and is +0.0 at every
    pruned one, in the master and in the mirror -- which a trusted engine (trust_mirror = True) goes on reading without a rebuild."""
    eng = hp.make_engine(hp.FC_SMALL, gamma_n=0.99, learning_rate=1e-2, adam_eps=1.5e-4)
    eng.trust_mirror = trusted
    n = eng.set_pruning()
    eng.init_params(5)
    start = eng.params.clone()
    fields = _fields(eng)
    k = [x // 2 for x in n]
    eng.prune_update(k)
    mask = _bits(eng.prune_mask)
    assert hp.popcount_pruned(eng, mask) == k
    masked = eng.params.clone()
    assert np.array_equal(_bits(masked), hp.bits(hp.apply(eng, start.cpu().numpy(), mask)))
    if trusted:
        eng.refresh_mirror()
        assert eng._mirror_is_current(None)
    eng.learn_on_batch(eng.make_batch(mirror_current=eng._mirror_is_current(None), **fields))
    learnt = eng.params.cpu().numpy().copy()
    pruned = hp.pruned_index(eng, mask)
    assert (learnt[pruned] != 0).any()  # (dense gradients: Adam moved the pruned positions)
    eng.prune_apply()
    want = hp.apply(eng, learnt, mask)
    assert np.array_equal(_bits(eng.params), hp.bits(want))
    assert (want[pruned] == 0).all() and not np.signbit(want[pruned]).any()
    if trusted:
        assert eng._mirror_is_current(None)  # (the apply launch kept the mirror the learn step left current)
    assert torch.equal(_mirror(eng), _mirror_of(eng, want))
    # a trusted engine's next reader uses the mirror as it is: the loss equals that of an engine that rebuilds
    loss = eng.loss_on_batch(eng.make_batch(mirror_current=eng._mirror_is_current(None), **fields)).clone()
    eng.invalidate_mirror()
    again = eng.loss_on_batch(eng.make_batch(**fields)).clone()
    assert torch.equal(loss.view(torch.int32), again.view(torch.int32))
    # prune_update on a trusted engine: still coherent
    k2 = [(3 * x) // 4 for x in n]
    eng.refresh_mirror()
    eng.prune_update(k2)
    m2, p2 = hp.update(eng, want, mask, k2)
    assert np.array_equal(_bits(eng.prune_mask), m2) and np.array_equal(_bits(eng.params), hp.bits(p2))
    assert torch.equal(_mirror(eng), _mirror_of(eng, p2))
    # the engine's own params handed in as a foreign buffer: master alone, and the mirror is marked stale
    eng.prune_apply(params=eng.params)
    assert not eng._mirror_is_current(None)


# ---------------------------------------------------------------------------------------------------------------- agents
A, B = 3, 8
BUFFERS = ("params", "adam_m", "adam_v", "adam_count", "losses_accum")
PRUNE = dict(prune_sparsity=0.5, prune_start=0, prune_end=4, prune_period=1000)


def _agent_and_replay(kind, use_graph, **kw):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    if kind == "isdqn":
        agent = iSDQN(0, (8,), A, 3, [20, 14], False, False, "fc", 1e-2, 0.99, 1, 1, 1000, adam_eps=1.5e-4, batch_size=B, use_graph=use_graph, **kw)
    else:
        agent = DQN(0, (8,), A, [20, 14], False, "fc", 1e-2, 0.99, 1, 1, 1000, adam_eps=1.5e-4, batch_size=B, use_graph=use_graph, **kw)
    rb = ReplayBuffer(UniformSamplingDistribution(5), B, 64, stack_size=1, update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(0)
    for _ in range(48):
        obs = rng.normal(size=8).astype(np.float32)
        term = bool(rng.random() < 0.08)
        rb.add(TransitionElement(obs, int(rng.integers(0, A)), float(rng.normal()), term, term))
    return agent, rb


def _state(agent):
    out = {n: getattr(agent._engine, n).clone() for n in BUFFERS}
    out["mask"] = agent._engine.prune_mask.clone()
    if getattr(agent, "target_params", None) is not None:
        out["target"] = agent.target_params.tensor.clone()
    return out


def _same(a, b, what):
    for n in a:
        x, y = a[n], b[n]
        same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)
        assert same, f"{n} differs between {what}"


def _start_pruning(agent):
    """A mask update as the training loop makes it at a target update, at a clock behind the schedule's end: sparsity 0.5."""
    assert not agent.prune_active
    agent._prune_t = 10
    logs = agent.prune_target_update(1000)
    assert agent.prune_active and logs == {"sparsity": agent._prune.sparsity} and 0.49 < logs["sparsity"] <= 0.5
    eng = agent._engine
    mask = _bits(eng.prune_mask)
    assert hp.popcount_pruned(eng, mask) == agent._prune.counts == [x // 2 for x in hp.real_counts(eng)]
    return mask


def _pruned_are_zero(eng, tensor, mask):
    return not _bits(tensor)[hp.pruned_index(eng, mask)].any()


@pytest.mark.parametrize("kind,kw,steps", [("isdqn", {}, 1), ("isdqn", dict(soft_shift_tau=0.25), 1), ("isdqn", {}, 2),
                                          ("dqn", dict(ema_tau=0.25), 1)])
def test_eager_and_captured_steps_are_bit_identical(kind, kw, steps):
    """Three gradient steps (``steps`` = 2: four, as two learn_steps(2) replays) from the same state, eager and captured, with the mask at
    sparsity 0.5: parameters, moments, count, loss accumulator, mask and target end in the same bits; every pruned position of the
    online parameters -- and of DQN's EMA target -- is +0.0; the captured step carries the apply node (its key says so) and an agent
    without the option, stepped the same way, ends elsewhere."""
    eager, rb_e = _agent_and_replay(kind, False, **PRUNE, **kw)
    graph, rb_g = _agent_and_replay(kind, True, **PRUNE, **kw)
    plain, rb_p = _agent_and_replay(kind, False, **kw)
    # until the schedule starts the captured step is the one without the option
    graph.update_online_params(0, rb_g)
    eager.update_online_params(0, rb_e)
    plain.update_online_params(0, rb_p)
    assert graph._graphed is not None and "prune" not in repr(graph._graphed.key) and graph._captures == 1
    _same({n: v for n, v in _state(graph).items() if n != "mask"}, {n: getattr(plain._engine, n) for n in BUFFERS} | (
        {"target": plain.target_params.tensor} if kind == "dqn" else {}), "the captured step before the schedule starts and an agent without the option")
    mask = _start_pruning(eager)
    assert np.array_equal(_start_pruning(graph), mask)
    n = 3 if steps == 1 else 4
    for step in range(n):
        eager.update_online_params(step, rb_e)
        plain.update_online_params(step, rb_p)
    if steps == 1:
        for step in range(n):
            graph.update_online_params(step, rb_g)
    else:
        graph.learn_steps(2, rb_g)
        graph.learn_steps(2, rb_g)
    assert eager._graphed is None and graph._graphed.S == steps and graph._captures == 2 and "prune" in repr(graph._graphed.key)
    assert eager._prune_t == graph._prune_t == 10 + n
    _same(_state(graph), _state(eager), f"{n} captured and {n} eager steps")
    assert not torch.equal(eager._engine.params, plain._engine.params)
    for agent in (eager, graph):
        eng = agent._engine
        assert eng.adam_count.item() == 1 + n and _pruned_are_zero(eng, eng.params, mask)
        if kind == "dqn":
            assert _pruned_are_zero(eng, agent.target_params.tensor, mask)
            agent.update_target_params(1000)
            assert _pruned_are_zero(eng, agent.target_params.tensor, mask)
    assert (_bits(plain._engine.params)[hp.pruned_index(eager._engine, mask)] != 0).any()


def test_training_run_logs_the_schedule_and_keeps_pruned_positions_zero(tmp_path):
    """The lunar-lander entry point on the seeded synthetic environment with -prune 0.5 between gradient steps 0 and 12, -prunef = -tuf = 3
    and -redo / -reset on the same steps: the logged sparsity is the schedule's at the run's own count of gradient steps (one per step
    past -nis), the device mask's popcount equals the host's counts, and no pruned position of the parameters is non-zero at the end."""
    from unittest import mock

    import experiments.lunar_lander.isdqn as entry

    seen = {}
    real_train = entry.train

    def train(key, p, agent, env, rb):
        seen.update(p=p, agent=agent)
        return real_train(key, p, agent, env, rb)

    argv = ["--experiment_name", "_test_prune", "--seed", "1", "--disable_wandb", "--features", "25", "15", "--replay_buffer_capacity", "100",
            "--batch_size", "3", "--update_horizon", "1", "--gamma", "0.99", "--learning_rate", "1e-3", "--horizon", "10", "--n_epochs", "1",
            "--n_training_steps_per_epoch", "24", "--data_to_update", "1", "--target_update_frequency", "3", "--n_initial_samples", "3",
            "--epsilon_end", "0.01", "--epsilon_duration", "4", "--architecture_type", "fc", "-env", "synthetic",
            "-prune", "0.5", "-prunes", "0", "-prunee", "12", "-prunef", "3", "-redo", "3", "-reset", "6"]
    with mock.patch.object(entry, "train", train):
        entry.run(argv, root=str(tmp_path))
    agent, history = seen["agent"], [h for h in seen["p"]["wandb"].history if "sparsity" in h]
    eng = agent._engine
    n_real = hp.real_counts(eng)
    assert n_real == [8 * 25, 25 * 15] and len(history) >= 6
    counts = [0, 0]
    for h in history:
        step = h["n_training_steps"]
        assert step % 3 == 0 and "recycled_neurons" in h and (("reset" in h) == (step % 6 == 0))
        counts = hp.counts_at(step - 3, 0.5, 0, 12, n_real, counts)  # (-nis 3, -utd 1: the gradient steps so far)
        assert h["sparsity"] == sum(counts) / sum(n_real), h
    assert history[-1]["sparsity"] == sum(int(0.5 * x) for x in n_real) / sum(n_real) and history[0]["sparsity"] < history[2]["sparsity"]
    mask = _bits(eng.prune_mask)
    assert hp.popcount_pruned(eng, mask) == agent._prune.counts == counts
    assert _pruned_are_zero(eng, eng.params, mask) and (_bits(eng.params)[hp.real_index(eng, hp.prunable(eng)[0])] != 0).any()
