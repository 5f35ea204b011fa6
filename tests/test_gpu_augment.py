"""The random-shift augmentation on the GPU (include/isdqn_hip.h, isdqn_replay_augment_shift; csrc/augment.h), bit for bit against the
numpy model of tests/helpers/augment.py: the kernel on the 16-byte path, the byte path and a pad larger than the frame; pad 0; the ramp
property test; the counter; every error case; a learn step on an augmented batch against the same step on the model's stacks through
the reference-layout path; eager against captured agents; augment_pad = 0 against an agent built without the argument."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import augment as am

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
FILL = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(frames, stride, h, w, stack, ids, n_rows, rps, pad, seed, count, pool, out_ids):
    from slimdqn import _hip

    p = lambda t: t if isinstance(t, int) else _hip.ptr(t)
    return _hip.lib().isdqn_replay_augment_shift(p(frames), stride, h, w, stack, p(ids), n_rows, rps, pad, seed, p(count), p(pool), p(out_ids),
                                                 _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device())))


class Case:
    """A frame store with more frames than are sampled, an id table with some -1, a pool and an out table pre-filled."""

    def __init__(self, h, w, stack, n_rows, stride=None, seed=0, frames=None, ids=None):
        rng = np.random.default_rng(seed)
        self.h, self.w, self.stack, self.n_rows = h, w, stack, n_rows
        self.stride = h * w if stride is None else stride
        n_frames = 2 * n_rows * 2 * stack + 5
        self.frames = rng.integers(0, 256, (n_frames, self.stride), dtype=np.uint8) if frames is None else frames
        if ids is None:
            ids = rng.integers(0, n_frames, (n_rows, 2 * stack)).astype(np.int32)
            ids[rng.random(ids.shape) < 0.25] = -1
            ids[0, 0], ids[-1, -1] = -1, 0
        self.ids = ids
        self.d_frames, self.d_ids = _dev(self.frames), _dev(self.ids)
        self.reset_outputs()

    def reset_outputs(self):
        self.pool = torch.full((self.n_rows * 2 * self.stack, self.stride), FILL, dtype=torch.uint8, device="cuda")
        self.out_ids = torch.full((self.n_rows, 2 * self.stack), 77777, dtype=torch.int32, device="cuda")

    def run(self, rps, pad, count, seed=SEED, rows=None):
        """One call on rows [rows[0], rows[1]) (default all) into the matching part of the pool; returns the status."""
        lo, hi = rows or (0, self.n_rows)
        s2 = 2 * self.stack
        return _call(self.d_frames, self.stride, self.h, self.w, self.stack, self.d_ids[lo:], hi - lo, rps, pad, seed, count,
                     self.pool[lo * s2:], self.out_ids[lo:])

    def model(self, rps, pad, count, seed=SEED):
        before = np.full((self.n_rows * 2 * self.stack, self.stride), FILL, np.uint8)
        return am.augment(self.frames, self.h, self.w, self.stack, self.ids, rps, pad, seed, count, pool=before)


def _counter(v=0):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


SHAPES = [
    # h, w, stack, n_rows, rows_per_step, pad, stride
    pytest.param(84, 84, 4, 3, 3, 4, 7056, id="84x84-stack4-16-byte-path"),
    pytest.param(21, 19, 2, 5, 1, 3, 401, id="21x19-stack2-odd-bases-byte-path"),
    pytest.param(4, 4, 1, 2, 2, 6, 16, id="4x4-pad6-larger-than-the-frame-16-byte-path"),
    pytest.param(4, 4, 1, 2, 1, 6, 19, id="4x4-pad6-larger-than-the-frame-byte-path"),
]


@pytest.mark.parametrize("h,w,stack,n_rows,rps,pad,stride", SHAPES)
def test_kernel_equals_the_model_and_writes_nothing_else(h, w, stack, n_rows, rps, pad, stride):
    c = Case(h, w, stack, n_rows, stride)
    start = (1 << 32) + 3  # (a count whose high word is not zero)
    count = _counter(start)
    assert c.run(rps, pad, count) == 0
    torch.cuda.synchronize()
    want_pool, want_ids, want_count = c.model(rps, pad, start)
    assert (c.ids < 0).any() and (c.ids >= 0).any()
    got_pool, got_ids = c.pool.cpu().numpy(), c.out_ids.cpu().numpy()
    assert np.array_equal(got_ids, want_ids)
    assert np.array_equal(got_pool, want_pool), f"{(got_pool != want_pool).sum()} bytes of the pool differ from the model"
    # said once more without the model: frames of -1 ids and the bytes between h*w and the stride keep the fill
    flat = c.ids.reshape(-1)
    assert (got_pool[flat < 0] == FILL).all() and (got_pool[:, h * w:] == FILL).all()
    assert int(count.item()) == want_count == start + n_rows // rps
    assert np.array_equal(c.d_frames.cpu().numpy(), c.frames) and np.array_equal(c.d_ids.cpu().numpy(), c.ids)  # the sources are unchanged


@pytest.mark.parametrize("h,w,stack,n_rows,stride", [(84, 84, 4, 2, 7056), (21, 19, 2, 3, 401)])
def test_pad_zero_is_the_gather_and_the_table_is_compact(h, w, stack, n_rows, stride):
    c = Case(h, w, stack, n_rows, stride, ids=np.random.default_rng(1).integers(0, 9, (n_rows, 2 * stack)).astype(np.int32))
    count = _counter(5)
    assert c.run(n_rows, 0, count) == 0
    torch.cuda.synchronize()
    got = c.pool.cpu().numpy()
    assert np.array_equal(got[:, : h * w], c.frames[c.ids.reshape(-1), : h * w]) and (got[:, h * w:] == FILL).all()
    assert np.array_equal(c.out_ids.cpu().numpy().reshape(-1), np.arange(n_rows * 2 * stack))
    assert int(count.item()) == 6


def test_ramp_frames_show_one_shift_per_stack_and_independent_halves():
    frames, ids, h, w, stack, pad = am.ramp_case()
    c = Case(h, w, stack, ids.shape[0], frames.shape[1], frames=frames, ids=ids)
    assert c.run(ids.shape[0], pad, _counter(2)) == 0
    torch.cuda.synchronize()
    pool, out_ids = c.pool.cpu().numpy(), c.out_ids.cpu().numpy()
    assert am.check_ramp_properties(pool, out_ids, ids, h, w, stack, pad) == []  # from the output alone
    dy, dx = am.draws(ids.shape[0], ids.shape[0], pad, SEED, 2)
    assert am.check_ramp_properties(pool, out_ids, ids, h, w, stack, pad, dy, dx) == []  # and they are the draws, sign and axis


def test_the_counter_selects_the_draws():
    S, B = 4, 3
    c = Case(21, 19, 2, S * B, 401)
    count = _counter(9)
    assert c.run(B, 3, count) == 0  # one launch over 4 x 3 rows
    torch.cuda.synchronize()
    one_pool, one_ids = c.pool.clone(), c.out_ids.clone()
    assert int(count.item()) == 9 + S
    c.reset_outputs()
    count4 = _counter(9)
    for s in range(S):  # four launches over 3 rows
        assert c.run(B, 3, count4, rows=(s * B, (s + 1) * B)) == 0
        assert int(count4.item()) == 10 + s
    torch.cuda.synchronize()
    assert torch.equal(c.pool, one_pool), "one launch over S*B rows is not S launches over B rows"
    base = (torch.arange(S, device="cuda") * B * 4).repeat_interleave(B)[:, None]  # the small launches count from their own base
    assert torch.equal(torch.where(c.out_ids >= 0, c.out_ids + base.to(torch.int32), c.out_ids), one_ids)
    assert torch.equal(count4, count)
    # with the counter reset between them two launches are equal; without, the second draws anew
    c.reset_outputs()
    count = _counter(9)
    assert c.run(B, 3, count) == 0
    assert torch.equal(c.pool, one_pool) and torch.equal(c.out_ids, one_ids)
    assert c.run(B, 3, count) == 0
    torch.cuda.synchronize()
    assert not torch.equal(c.pool, one_pool) and torch.equal(c.out_ids, one_ids) and int(count.item()) == 9 + 2 * S
    # another seed draws other shifts
    c.reset_outputs()
    assert c.run(B, 3, _counter(9), seed=SEED + 1) == 0
    assert not torch.equal(c.pool, one_pool)


def test_every_error_case_is_an_argument_error_and_launches_nothing():
    from slimdqn import _hip

    h, w, stack, n_rows = 6, 5, 2, 4
    c = Case(h, w, stack, n_rows, 32)
    count = _counter(3)
    ok = dict(frames=c.d_frames, stride=32, h=h, w=w, stack=stack, ids=c.d_ids, n_rows=n_rows, rps=2, pad=4, seed=SEED, count=count, pool=c.pool,
              out_ids=c.out_ids)
    inside = c.pool.reshape(-1)[32:]  # a store whose base lies inside the pool
    bad = [dict(pad=-1), dict(pad=128), dict(h=0), dict(w=0), dict(stack=0), dict(n_rows=0), dict(h=-3), dict(rps=0), dict(rps=3), dict(rps=-2),
           dict(stride=h * w - 1), dict(frames=0), dict(ids=0), dict(count=0), dict(pool=0), dict(out_ids=0),
           dict(pool=c.d_frames), dict(frames=inside), dict(pool=c.d_frames.reshape(-1)[7:]), dict(out_ids=c.d_ids)]
    for change in bad:
        assert _call(**{**ok, **change}) == _hip.ERR_ARG, change
        assert _hip.last_error()
    torch.cuda.synchronize()
    assert (c.pool == FILL).all() and (c.out_ids == 77777).all() and int(count.item()) == 3
    assert np.array_equal(c.d_frames.cpu().numpy(), c.frames) and np.array_equal(c.d_ids.cpu().numpy(), c.ids)
    assert _call(**ok) == 0  # and the unchanged call runs
    torch.cuda.synchronize()
    assert int(count.item()) == 5 and not (c.pool == FILL).all()
    # pad 0 and a pad far larger than the frame are legal
    assert _call(**{**ok, "pad": 0}) == 0 and _call(**{**ok, "pad": 127}) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the learn step and the agents
def _fill(rbs, n=40, A=5, prioritized=False):
    from slimdqn.sample_collection.replay_buffer import TransitionElement

    rng = np.random.default_rng(0)
    for _ in range(n):
        obs = rng.integers(0, 256, (84, 84), dtype=np.uint8)
        a, r, term = int(rng.integers(0, A)), float(rng.choice([-1.0, 0.0, 1.0])), bool(rng.random() < 0.08)
        for rb in rbs:
            kw = dict(priority=rb._sampling_distribution.MAX_PRIORITY) if prioritized else {}
            rb.add(TransitionElement(obs, a, r, term, term), **kw)


def _agent(arch="cnn", batch_norm=False, B=6, **kw):
    from slimdqn.networks.isdqn import iSDQN

    feats = [7, 9, 11, 13] if arch == "cnn" else [8, 16, 16, 24]
    return iSDQN(0, (84, 84, 4), 5, 3, feats, True, batch_norm, arch, 2e-4, 0.99, 3, 1, 6, adam_eps=1.5e-4, batch_size=B, **kw)


def _replay(B, prioritized=False):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

    sampler = PrioritizedSamplingDistribution(5, 64) if prioritized else UniformSamplingDistribution(5)
    return ReplayBuffer(sampler, B, 64, update_horizon=3, gamma=0.99)


STATE = ("params", "adam_m", "adam_v", "adam_count", "losses_accum")


@pytest.mark.parametrize("arch,batch_norm,B", [("cnn", False, 6), ("impala", True, 4)])
def test_learn_step_on_the_augmented_batch_equals_the_step_on_the_models_stacks(arch, batch_norm, B):
    """The engine is unchanged, so any difference is the new code's: parameters, moments, losses and priorities of learn_on_batch on
    ReplayBuffer.augment's DeviceBatch against learn_on_batch on the model's augmented stacks, handed over in the reference's
    (B, h, w, stack) layout (the de-interleave path)."""
    dev, ref = _agent(arch, batch_norm, B), _agent(arch, batch_norm, B)
    assert torch.equal(dev._engine.params, ref._engine.params)
    rb = _replay(B)
    _fill([rb])
    batch = rb.sample()
    ids = batch.frame_ids.cpu().numpy()
    if not (ids < 0).any():  # some stacks of the batch reach into the leading padding
        first = torch.zeros(1, dtype=torch.int32, device="cuda")
        batch = rb.gather(torch.cat((first, batch.indices[1:])))
        ids = batch.frame_ids.cpu().numpy()
    assert (ids < 0).any()
    count = _counter(17)
    aug = rb.augment(batch, 4, SEED, count)
    assert aug.frames is not rb._frames and aug.frames.shape == (B * 8, 84 * 84) and aug.action is batch.action and aug.indices is batch.indices
    _, _, losses_dev = dev.learn_on_batch(dev.params, dev.optimizer_state, aug)
    torch.cuda.synchronize()
    assert int(count.item()) == 18
    pool, out_ids, _ = am.augment(rb._frames.cpu().numpy(), 84, 84, 4, ids, B, 4, SEED, 17)
    assert np.array_equal(aug.frames.cpu().numpy(), pool) and np.array_equal(aug.frame_ids.cpu().numpy(), out_ids)
    st, nx = am.stacks(pool, out_ids, 84, 84, 4)
    assert not np.array_equal(st, batch.state.cpu().numpy())  # the batch did move
    samples = types.SimpleNamespace(state=st, next_state=nx, action=batch.action, reward=batch.reward, is_terminal=batch.is_terminal)
    _, _, losses_ref = ref.learn_on_batch(ref.params, ref.optimizer_state, samples)
    torch.cuda.synchronize()
    assert torch.equal(losses_dev, losses_ref)
    for name in STATE + ("priorities", "q_values", "targets"):
        a, b = getattr(dev._engine, name), getattr(ref._engine, name)
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} elements differ"
    # what the augmented batch materialises is the model's stacks (DeviceBatch.state reads the pool through the table)
    assert np.array_equal(aug.state.cpu().numpy(), st) and np.array_equal(aug.next_state.cpu().numpy(), nx)


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_captured_steps_equal_eager_steps_and_every_replay_draws_anew(prioritized):
    B, S = 8, 8
    eager, graphed = _agent(B=B, use_graph=False, augment_pad=4), _agent(B=B, use_graph=True, augment_pad=4)
    rbs = [_replay(B, prioritized) for _ in range(2)]
    _fill(rbs, prioritized=prioritized)
    if prioritized:
        eager.priority_writeback = graphed.priority_writeback = True
    for agent, rb in zip((eager, graphed), rbs):
        assert int(agent.aug_count.item()) == 0
        agent.learn_steps(S, rb)
    torch.cuda.synchronize()
    g = graphed._graphed
    assert eager._graphed is None and g is not None and g.S == S and g.augment_pad == 4
    # the capture's warm-up left the counter where it was: S steps, S draws
    assert int(eager.aug_count.item()) == S and torch.equal(eager.aug_count, graphed.aug_count)
    for name in STATE:
        a, b = getattr(eager._engine, name), getattr(graphed._engine, name)
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} elements differ between eager and captured augmented steps"
    if prioritized:
        ta, tb = rbs[0]._sampling_distribution._sum_tree, rbs[1]._sampling_distribution._sum_tree
        assert torch.equal(ta._nodes_dev, tb._nodes_dev)
    # the steps did train on shifted frames: an agent without the option ends elsewhere
    plain, rb_plain = _agent(B=B, use_graph=False), _replay(B, prioritized)
    _fill([rb_plain], prioritized=prioritized)
    plain.learn_steps(S, rb_plain)
    assert not torch.equal(plain._engine.params, eager._engine.params)
    # a second replay draws other shifts than the first: same rows, other pool
    first_pool, first_ids = g.aug_frames.clone(), g.frame_ids.clone()
    rows = g.block.clone()
    graphed.learn_steps(S, rbs[1])
    eager.learn_steps(S, rbs[0])
    torch.cuda.synchronize()
    assert int(graphed.aug_count.item()) == 2 * S and torch.equal(eager.aug_count, graphed.aug_count)
    assert torch.equal(eager._engine.params, graphed._engine.params)
    if not prioritized:
        g.block.copy_(rows)  # replay the first replay's rows once more: the same frames, shifted otherwise
        g.graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g.frame_ids, first_ids) and not torch.equal(g.aug_frames, first_pool)
        assert int(graphed.aug_count.item()) == 3 * S
    assert graphed._captures == 1  # one capture served all of it


def test_changing_augment_pad_captures_again():
    B = 8
    agent, rb = _agent(B=B, augment_pad=4), _replay(B)
    _fill([rb])
    agent.learn_steps(2, rb)
    assert agent._graphed.augment_pad == 4 and agent._captures == 1
    agent.augment_pad = 2
    agent.learn_steps(2, rb)
    torch.cuda.synchronize()
    assert agent._graphed.augment_pad == 2 and agent._captures == 2 and int(agent.aug_count.item()) == 4


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
def test_augment_pad_zero_is_the_agent_built_without_the_argument(use_graph):
    B = 8
    off, plain = _agent(B=B, use_graph=use_graph, augment_pad=0), _agent(B=B, use_graph=use_graph)
    rbs = [_replay(B) for _ in range(2)]
    _fill(rbs)
    for agent, rb in zip((off, plain), rbs):
        agent.learn_steps(3, rb)
        torch.cuda.synchronize()
        if use_graph:
            assert agent._graphed.augment is None and not hasattr(agent._graphed, "aug_frames")
        agent._drop_graph()  # (one live executable graph at a time)
    assert off.aug_count is None and rbs[0]._aug_pools == {}  # no counter, no pool, no launch
    for name in STATE:
        assert torch.equal(getattr(off._engine, name), getattr(plain._engine, name)), name


def test_acting_and_recycling_never_augment():
    B = 8
    agent, rb = _agent(B=B, use_graph=False, augment_pad=4), _replay(B)
    _fill([rb])
    state = np.random.default_rng(0).integers(0, 256, (84, 84, 4), dtype=np.uint8)
    agent.q_values(agent.params, state)
    agent.best_action(agent.params, state, key=1)
    agent.recycle_dormant(rb, 0.1)
    agent.loss_on_batch(agent.params, rb.sample())
    torch.cuda.synchronize()
    assert int(agent.aug_count.item()) == 0 and rb._aug_pools == {}
    agent.update_online_params(0, rb)
    assert int(agent.aug_count.item()) == 1 and list(rb._aug_pools) == [B]


def test_the_analysis_agents_augment_the_training_batch_once_per_update():
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN

    B = 6
    a = AnalysisDQN(0, (84, 84, 4), 5, 3, [7, 9, 11, 13], True, False, "cnn", 2e-4, 0.99, 3, 1, 6, adam_eps=1.5e-4, batch_size=B, augment_pad=4)
    t = AnalysisTFDQN(0, (84, 84, 4), 5, [7, 9, 11, 13], True, False, "cnn", 2e-4, 0.99, 3, 1, 6, adam_eps=1.5e-4, batch_size=B, augment_pad=4)
    for agent in (a, t):
        rb = _replay(B)
        _fill([rb])
        agent.update_online_params(0, rb)
        agent.update_online_params(1, rb)
        torch.cuda.synchronize()
        assert int(agent.aug_count.item()) == 2  # one draw per update, whatever the number of passes over the batch
