"""Annealed update horizon and discount on the GPU (include/isdqn_hip.h: isdqn_replay_gather_horizon,
isdqn_replay_apply_staged_horizon, isdqn_batch_discount::discount) against the numpy restatement of tests/helpers/horizon.py:

  * the gather: bit for bit against the helper on buffers filled through add(), every horizon (and the clamped ones), several discounts,
    with and without the index table; at m = n_max against the existing row gather;
  * the learn step: a discount tensor filled with gamma_n equals NULL bit for bit; a tensor of two values (and zeros) by row gives, row
    by row, the uniform runs at either value; the losses against float64 from the device's own q_values and targets;
  * the captured update under a schedule against eager steps, a reset in between, run-to-run identity; the entry point with -anneal."""
import json

import numpy as np
import pytest
import torch

from tests import test_gpu_per_weights as pwt
from tests.gpu_helpers import make_frame_batch
from tests.helpers import horizon as hz
from tests.helpers import per_weights as pw

pytestmark = pytest.mark.gpu

U32 = 2.0**-24
_d = pwt._d


# ===================================================================================== 1. the gather kernel
def _filled(stack, n_max, capacity=97, gamma=0.97, n_episodes=110, positive_rewards=False, seed=1):
    """A device replay with horizon windows after a stream of about eight times its capacity (wrap-around, evictions), flushed."""
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(0), 8, capacity, stack_size=stack, update_horizon=n_max, gamma=gamma, device="cuda:0",
                      horizon_window=True)
    for index, action, reward, terminal, end in hz.transitions(hz.seeded_stream(seed=seed, n_episodes=n_episodes)):
        rb.add(TransitionElement(hz.frame_of(index), action, abs(reward) if positive_rewards else reward, terminal, end))
    rb._flush()
    assert rb.add_count > 3 * capacity
    return rb


def _launch(rb, slots, use_index, horizon, gamma):
    """isdqn_replay_gather_horizon itself (index_to_slot given or NULL), device scalars made here."""
    from slimdqn import _hip

    B, s2 = int(slots.numel()), 2 * rb._stack_size
    out = [torch.full((B, s2), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda"),
           torch.full((B,), np.nan, dtype=torch.float32, device="cuda"), torch.full((B,), 9, dtype=torch.uint8, device="cuda"),
           torch.full((B,), np.nan, dtype=torch.float32, device="cuda")]
    h, g = _d(np.array([horizon], np.int32)), _d(np.array([gamma], np.float32))
    _hip.check(rb._lib.isdqn_replay_gather_horizon(
        _hip.ptr(rb._d_elem_window), _hip.ptr(rb._d_elem_steps), _hip.ptr(rb._d_elem_len), _hip.ptr(rb._d_elem_action),
        _hip.ptr(rb._d_elem_terminal), rb._stack_size, rb._update_horizon, _hip.ptr(rb._d_index_to_slot) if use_index else None,
        _hip.ptr(slots), B, _hip.ptr(h), _hip.ptr(g), *[_hip.ptr(t) for t in out], _hip.stream_ptr(rb.device)), "isdqn_replay_gather_horizon")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _expected(rb, slots, horizon, gamma):
    return hz.gather(rb._h_elem_window, rb._h_elem_steps, rb._h_elem_len, rb._h_elem_action, rb._h_elem_terminal, rb._stack_size,
                     rb._update_horizon, slots, horizon, gamma)


NAMES = ("frame ids", "action", "reward", "terminal", "discount")


@pytest.mark.parametrize("stack", [1, 4])
@pytest.mark.parametrize("n_max", [1, 3, 10])
def test_gather_equals_the_restatement_bit_for_bit(stack, n_max):
    rb = _filled(stack, n_max)
    C = rb._max_capacity
    # the tables went up through the staged scatter: the device copies are the host tables
    for name in ("window", "steps", "len"):
        assert np.array_equal(getattr(rb, "_d_elem_" + name).cpu().numpy(), getattr(rb, "_h_elem_" + name)), name
    rng = np.random.default_rng(stack * 100 + n_max)
    n_terminal_cut = 0
    for B in (1, 5, 64, 65, 257):
        idx = rng.integers(0, C, B).astype(np.int32)
        if B >= 5:
            idx[0], idx[-1] = 0, C - 1
        for use_index in (True, False):
            slots = rb._h_index_to_slot[idx] if use_index else idx
            for m in range(0, n_max + 2):  # (0 and n_max + 1: clamped)
                for gamma in (0.0, 0.5, 0.97, 0.997):
                    got = _launch(rb, _d(idx), use_index, m, gamma)
                    want = _expected(rb, slots, m, gamma)
                    for name, a, b in zip(NAMES, got, want):
                        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (
                            f"{name} differs: B {B}, index table {use_index}, m {m}, gamma {gamma}: "
                            f"{int((a != b).sum())} of {a.size} elements")
                    n_terminal_cut += int(((rb._h_elem_terminal[slots] != 0) & (got[3] == 0)).sum())
    if n_max > 1:
        assert n_terminal_cut > 0  # rows whose terminal flag at n_max is off at a shorter horizon were among them
    # the clamped horizons are the end points
    assert all(np.array_equal(a, b) for a, b in zip(_launch(rb, _d(idx), True, -5, 0.5), _launch(rb, _d(idx), True, 1, 0.5)))
    assert all(np.array_equal(a, b) for a, b in zip(_launch(rb, _d(idx), True, 1 << 30, 0.5), _launch(rb, _d(idx), True, n_max, 0.5)))


def test_sample_and_gather_of_the_buffer():
    rb = _filled(4, 3)
    with pytest.raises(ValueError, match="both or neither"):
        rb.sample(horizon=2)
    plain = rb.sample()
    assert plain.discount is None
    batch = rb.sample(horizon=2, gamma=0.5)
    idx = batch.indices.cpu().numpy()
    want = _expected(rb, rb._h_index_to_slot[idx], 2, 0.5)
    for name, a, b in zip(NAMES, (batch.frame_ids, batch.action, batch.reward, batch.is_terminal, batch.discount), want):
        assert a.cpu().numpy().tobytes() == b.tobytes(), name
    assert (batch.discount == 0.25).all()
    # device scalars are read where python numbers were: the same rows
    again = rb.gather(batch.indices, horizon=_d(np.array([2], np.int32)), gamma=_d(np.array([0.5], np.float32)))
    assert torch.equal(again.reward, batch.reward) and torch.equal(again.frame_ids, batch.frame_ids) and torch.equal(again.discount, batch.discount)
    # materialised stacks follow the cut window
    nxt = hz.index_of(batch.next_state.cpu().numpy().transpose(0, 3, 1, 2).reshape(len(idx), 4, 4))
    store = np.concatenate([rb._frames.cpu().numpy(), np.zeros((1, 4), np.uint8)])
    assert np.array_equal(nxt, hz.index_of(store[want[0][:, 4:]]))
    # the augmentation carries the discounts along
    big = _big_replay(8)
    b = big.sample(horizon=2, gamma=0.9)
    aug = big.augment(b, 4, 123, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert aug.discount is b.discount and aug.frames is not b.frames


def test_null_pointers_and_bad_shapes_are_refused():
    from slimdqn import _hip

    rb = _filled(4, 3)
    lib = rb._lib
    idx = _d(np.zeros(4, np.int32))
    h, g = _d(np.array([1], np.int32)), _d(np.array([0.5], np.float32))
    outs = [torch.zeros(4, 8, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"),
            torch.zeros(4, dtype=torch.float32, device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda"),
            torch.zeros(4, dtype=torch.float32, device="cuda")]

    def call(B=4, stack=4, n_max=3, horizon=h, gamma=g, window=rb._d_elem_window, out4=outs[4]):
        return lib.isdqn_replay_gather_horizon(
            _hip.ptr(window), _hip.ptr(rb._d_elem_steps), _hip.ptr(rb._d_elem_len), _hip.ptr(rb._d_elem_action), _hip.ptr(rb._d_elem_terminal),
            stack, n_max, None, _hip.ptr(idx), B, _hip.ptr(horizon), _hip.ptr(gamma), *[_hip.ptr(t) for t in outs[:4]], _hip.ptr(out4),
            _hip.stream_ptr(rb.device))

    assert call() == _hip.OK
    for kw in (dict(B=0), dict(B=-1), dict(stack=0), dict(n_max=0), dict(n_max=129), dict(horizon=None), dict(gamma=None), dict(window=None),
               dict(out4=None)):
        assert call(**kw) == _hip.ERR_ARG, kw
    staged = torch.zeros(256, dtype=torch.uint8, device="cuda")

    def scatter(n_rows=1, stack=4, n_max=3, staged=staged, window=rb._d_elem_window, off=16):
        return lib.isdqn_replay_apply_staged_horizon(_hip.ptr(staged), n_rows, 0, off, 64, 128, stack, n_max, _hip.ptr(window),
                                                     _hip.ptr(rb._d_elem_steps), _hip.ptr(rb._d_elem_len), _hip.stream_ptr(rb.device))

    before = rb._d_elem_window.clone()
    assert scatter(n_rows=0) == _hip.OK
    torch.cuda.synchronize()
    assert torch.equal(before, rb._d_elem_window)
    for kw in (dict(n_rows=-1), dict(stack=0), dict(n_max=0), dict(n_max=129), dict(staged=None), dict(window=None), dict(off=-16)):
        assert scatter(**kw) == _hip.ERR_ARG, kw
    torch.cuda.synchronize()


def test_at_n_max_the_gather_is_the_existing_row_gather():
    """ids, action and terminal bit for bit; the rewards (non-negative here, so nothing cancels) the same float32 or its neighbour: the
    host accumulator weighs with gamma ** k (pow), the kernel with the running product, both in float64.  The buffer's gamma is a
    float32 value here, as the kernel reads one: a float64 0.97 and its float32 rounding are 2e-8 apart, three float32 steps by the
    ninth power."""
    for stack, n_max in ((4, 3), (1, 10), (4, 10)):
        rb = _filled(stack, n_max, positive_rewards=True, gamma=float(np.float32(0.97)))
        idx = _d(np.random.default_rng(0).integers(0, rb._max_capacity, 257).astype(np.int32))
        plain = rb.gather(idx)
        cut = rb.gather(idx, horizon=n_max, gamma=rb._gamma)
        torch.cuda.synchronize()
        assert torch.equal(plain.frame_ids, cut.frame_ids) and torch.equal(plain.action, cut.action) and torch.equal(plain.is_terminal, cut.is_terminal)
        a, b = plain.reward.cpu().numpy(), cut.reward.cpu().numpy()
        assert (a >= 0).all() and a.max() > 0
        steps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
        print(f"stack {stack} n_max {n_max}: {int((steps == 0).sum())} of {a.size} rewards equal, {int((steps == 1).sum())} adjacent")
        assert steps.max() <= 1


def test_prefill_synthetic_in_horizon_mode():
    rb = _big_replay(8, n_max=5, capacity=512, p_terminal=0.2)
    n, stack, n_max = 512, 4, 5
    w, steps, length, term = rb._h_elem_window[:n], rb._h_elem_steps[:n], rb._h_elem_len[:n], rb._h_elem_terminal[:n]
    base = np.arange(n)[:, None] + np.arange(stack + n_max)[None]
    behind = np.arange(stack + n_max)[None] > (stack - 1 + length)[:, None]
    assert np.array_equal(w, np.where(behind, -1, base)) and (length[term == 0] == n_max).all()
    assert term.sum() > 20 and set(length[term != 0]) == set(range(1, n_max + 1))
    assert set(np.unique(steps)) <= {-1.0, 0.0, 1.0} and (steps[np.arange(n_max)[None] >= length[:, None]] == 0).all()
    np.testing.assert_allclose(rb._h_elem_reward64[:n], (steps.astype(np.float64) * 0.99 ** np.arange(n_max)[None]).sum(1), rtol=0, atol=1e-15)
    assert np.array_equal(rb._h_elem_frames[:n, :stack], w[:, :stack]) and np.array_equal(rb._h_elem_frames[:n, stack:], w[:, n_max:])
    for name in ("window", "steps", "len"):
        assert np.array_equal(getattr(rb, "_d_elem_" + name).cpu().numpy(), getattr(rb, "_h_elem_" + name)), name
    held = np.bincount(w[w >= 0], minlength=len(rb._refcount))
    assert np.array_equal(held, rb._refcount)
    # off mode keeps its draws: the same call without the option gives the tables it always gave (bench.py's replay)
    off = _big_replay(8, n_max=5, capacity=512, p_terminal=0.2, horizon_window=False)
    rng = np.random.default_rng(5)
    assert np.array_equal(off._h_elem_action[:n], rng.integers(0, 5, n))
    assert np.array_equal(off._h_elem_reward64[:n], rng.choice([-1.0, 0.0, 1.0], size=n, p=[0.05, 0.9, 0.05]))
    assert np.array_equal(off._h_elem_terminal[:n], rng.random(n) < 0.2) and not hasattr(off, "_h_elem_window")


# ===================================================================================== engines and batches
NQ, NB65 = 65, 65
EXTRA = {
    # name: (feats, n_heads, A, B, arch, ln, extra engine keywords, target parameters) -- tests/test_gpu_per_weights.py's CONFIGS form
    "quantile": ((7, 9, 11, 13), 4, 5, 6, "cnn", True, dict(n_quantiles=NQ, huber_delta=1.0), False),
    "c51": ((7, 9, 11, 13), 4, 5, 6, "cnn", True, dict(n_bins=NB65, min_value=-10.0, max_value=10.0, categorical=True), False),
    "munchausen": ((7, 9, 11, 13), 4, 5, 6, "cnn", True, dict(munchausen_tau=0.03, munchausen_alpha=0.9, munchausen_clip=-1.0), False),
    "double-q": ((7, 9, 11, 13), 4, 5, 6, "cnn", True, dict(double_q=True), False),
    "dueling": ((7, 9, 11, 14), 4, 5, 6, "cnn", True, dict(dueling=True), False),
    "impala-tiny": ((8, 8, 8, 16), 3, 4, 5, "impala", True, {}, False),
}


class _Setup(pwt._Setup):
    """tests/test_gpu_per_weights.py's engine-and-batch setup, also for the EXTRA configurations (seeded initial parameters there).
    ``with_discount(t)`` puts a discount tensor into every batch the setup builds (None: takes it out)."""

    def __init__(self, name, seed=3, B=None):
        if name in pwt.CONFIGS:
            super().__init__(name, seed=seed, B=B)
            return
        from slimdqn._engine import QNetEngine

        feats, n_heads, A, B0, arch, ln, kw, target = EXTRA[name]
        B = B or B0
        self.name, self.A, self.B, self.arch, self.n_heads = name, A, B, arch, n_heads
        self.eng = eng = QNetEngine((84, 84, 4), A, n_heads, feats, arch, ln, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, **kw)
        eng.init_params(seed)
        self.target = None
        frames, ids, action, reward, terminal, _ = make_frame_batch(B, A, seed=seed)
        self.kw = dict(frames=_d(frames), frame_stride=frames.shape[1], frame_ids=_d(ids), action=_d(action), reward=_d(reward.astype(np.float32)),
                       terminal=_d(terminal))
        self.action = action
        self.K = eng.n_regressed
        self.oh = 1 if n_heads >= 2 else 0
        torch.cuda.synchronize()
        self.state0 = [t.clone() for t in self._state()]

    def with_discount(self, discount):
        self.kw.pop("discount", None)
        if discount is not None:
            self.kw["discount"] = discount
        return self

    def loss(self):
        return (self.eng.loss_on_batch_target(self.cb(), self.target) if self.target is not None else self.eng.loss_on_batch(self.cb())).clone()

    def dout(self):
        e = self.eng
        width = self.n_heads * self.A * max(e.n_bins, e.n_quantiles, 1)
        wp = (width + 7) // 8 * 8
        return e.region("dout")[: self.B * wp].reshape(self.B, wp).clone(), width


# ===================================================================================== 2. NULL == gamma_n everywhere
@pytest.mark.parametrize("name", list(pwt.CONFIGS) + list(EXTRA))
def test_null_discount_equals_gamma_n_everywhere_bit_for_bit(name):
    s = _Setup(name)
    full = torch.full((s.B,), float(np.float32(s.eng.cfg.gamma_n)), dtype=torch.float32, device="cuda")
    assert full[0].item() == s.eng.cfg.gamma_n
    runs = []
    for disc in (None, full):
        s.reset()
        s.with_discount(disc)
        per_step = []
        for _ in range(3):
            s.learn()
            per_step.append(s.outputs())
        runs.append((per_step, [t.clone() for t in s._state()]))
    (steps_a, state_a), (steps_b, state_b) = runs
    for i, (a, b) in enumerate(zip(steps_a, steps_b)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"step {i}: {k} differs between a NULL discount and gamma_n everywhere"
    for n, a, b in zip(("params", "adam_m", "adam_v", "adam_count", "losses_accum"), state_a, state_b):
        assert torch.equal(a, b), f"{n} differs between a NULL discount and gamma_n everywhere ({(a != b).sum().item()} elements)"
    assert int(state_a[3].item()) == 3 and not torch.equal(state_a[0], s.state0[0])
    s.reset()
    la = s.with_discount(None).loss()
    lb = s.with_discount(full).loss()
    assert torch.equal(la, lb) and torch.isfinite(la).all()
    # and the field is read: another value moves the targets
    s.with_discount(full * 0.5).loss()
    assert not torch.equal(s.outputs()["losses"], la)


# ===================================================================================== 3. row-local, 4. losses
ROW_LOCAL = [("c2-head-chain", 32), ("cnn-noln", None), ("fc", None), ("one-head-target", None), ("hl-gauss", None), ("quantile", None),
             ("c51", None), ("munchausen", None), ("batchnorm", None)]
SCALAR = ("c2-head-chain", "cnn-noln", "fc", "one-head-target", "munchausen", "batchnorm")
D1, D2 = np.float32(0.97**3), np.float32(0.5)


@pytest.mark.parametrize("name,B", ROW_LOCAL)
def test_discount_is_taken_row_by_row(name, B):
    """A tensor of D1, D2 and 0 by row against the uniform runs at gamma_n = D1, D2 and 0 with a NULL discount: q_values, targets,
    priorities and the rows of dL/d(head output) of every row equal those of the uniform run at the row's value, bit for bit; rows at 0
    have targets == reward (Munchausen: reward + bonus, the uniform run at 0).  Then the losses of the mixed run against float64 from
    the device's own q_values and targets, within tests/test_gpu_per_weights.py's bound for weighted losses (scalar heads)."""
    s = _Setup(name, B=B)
    B = s.B
    which = np.arange(B) % 3  # 0: D1, 1: D2, 2: zero
    values = np.array([D1, D2, 0.0], np.float32)
    mixed = _d(values[which])

    def run(gamma_n, discount):
        s.reset()
        s.eng.cfg.gamma_n = float(gamma_n)
        s.with_discount(discount)
        s.learn()
        out = s.outputs()
        out["dout"], _ = s.dout()
        return out

    uniform = [run(v, None) for v in values]
    got = run(0.123, mixed)  # (gamma_n is ignored once the tensor is there)
    s.eng.cfg.gamma_n = 0.99
    for v in range(3):
        rows = torch.from_numpy(which == v).cuda()
        assert int(rows.sum()) >= 1
        for k in ("q_values", "targets", "priorities", "dout"):
            assert torch.equal(got[k][rows], uniform[v][k][rows]), f"{k}: rows at discount {values[v]} differ from the uniform run at it"
    assert not torch.equal(uniform[0]["targets"], uniform[1]["targets"])
    zero_rows = torch.from_numpy(which == 2).cuda()
    if name != "munchausen":
        reward = s.kw["reward"][zero_rows]
        assert torch.equal(got["targets"][zero_rows], reward[:, None].expand(-1, s.K))
    assert float(got["dout"].abs().max()) > 0
    if name in SCALAR:
        ref = pw.weighted_td(got["q_values"].cpu().numpy(), got["targets"].cpu().numpy(), np.ones(B), float(s.eng.cfg.huber_delta))
        losses = got["losses"].double().cpu().numpy()
        lbound = (B + 4) * U32 * ref["abs_terms"]
        print(f"{name}: loss error / bound = {(np.abs(losses - ref['losses']) / lbound).max():.4f}")
        assert (np.abs(losses - ref["losses"]) <= lbound).all(), (losses, ref["losses"], lbound)


def test_targets_are_reward_plus_discount_times_bootstrap():
    """The mixed targets against float64 from the uniform run's own targets: (t - r) scales with the discount."""
    s = _Setup("cnn-noln")
    base = np.float32(0.75)
    s.eng.cfg.gamma_n = float(base)
    s.reset()
    s.learn()
    t0 = s.outputs()["targets"].double().cpu().numpy()
    s.eng.cfg.gamma_n = 0.99
    disc = np.linspace(0.0, 0.999, s.B).astype(np.float32)
    s.reset()
    s.with_discount(_d(disc)).learn()
    t1 = s.outputs()["targets"].double().cpu().numpy()
    r = s.kw["reward"].double().cpu().numpy()[:, None]
    want = r + (t0 - r) * (disc.astype(np.float64) / float(base))[:, None]
    assert np.abs(t1 - want).max() <= 8 * U32 * np.abs(want).max()


# ===================================================================================== 5. captured against eager
STATE = ("params", "adam_m", "adam_v", "adam_count", "losses_accum")


def _big_replay(B, n_max=3, capacity=2048, prioritized=False, seed=5, p_terminal=0.1, horizon_window=True):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

    sampler = PrioritizedSamplingDistribution(seed, capacity, device="cuda:0") if prioritized else UniformSamplingDistribution(seed)
    rb = ReplayBuffer(sampler, B, capacity, stack_size=4, update_horizon=n_max, gamma=0.99, device="cuda:0", horizon_window=horizon_window)
    pri = np.exp(np.random.default_rng(seed).uniform(np.log(0.05), np.log(5.0), capacity)) if prioritized else None
    rb.prefill_synthetic(capacity, (84, 84), 5, seed=seed, p_terminal=p_terminal, priorities=pri)
    return rb


SCHEDULE = (3, 1, 0.9, 0.99, 6)  # n 3 -> 1 and gamma 0.9 -> 0.99 over six steps


def _compare(eager, graphed, what):
    torch.cuda.synchronize()
    for name in STATE:
        x, y = getattr(eager._engine, name), getattr(graphed._engine, name)
        assert torch.equal(x, y), f"{what}: {name}: {(x != y).sum().item()} elements differ between eager and captured steps"


@pytest.mark.parametrize("extras", [False, True])
def test_graph_replay_equals_eager_steps_under_a_schedule_isdqn(extras):
    """Eight eager steps against two replays of one captured graph of four; with ``extras`` the replay is prioritized with write-back and
    importance sampling and the batches are augmented.  Then a reset, which restarts the schedule in both, and eight steps more."""
    from slimdqn.networks.isdqn import iSDQN

    K, A, B = 3, 5, 8

    def make(use_graph):
        agent = iSDQN(0, (84, 84, 4), A, K, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.9, 3, 1, 100, adam_eps=1.5e-4, batch_size=B,
                      use_graph=use_graph, **(dict(augment_pad=4) if extras else {}))
        rb = _big_replay(B, prioritized=extras)
        if extras:
            agent.priority_writeback = True
            agent.set_importance_sampling(0.4, 1.0, n_steps=6)
        agent.set_horizon_schedule(*SCHEDULE, replay_buffer=rb)
        return agent, rb

    (eager, rb_e), (graphed, rb_g) = make(False), make(True)
    fresh = eager._engine.params.clone()
    for step in range(8):
        eager.update_online_params(step, rb_e)
    graphed.learn_steps(4, rb_g)
    first = graphed._graphed
    exe = first.graph
    pairs_1 = (first.horizons.clone(), first.gammas.clone())
    graphed.learn_steps(4, rb_g)
    assert graphed._graphed is first and first.graph is exe and graphed._captures == 1 and first.horizon  # no re-capture for new pairs
    want = [hz.schedule(*SCHEDULE, t) for t in range(8)]
    assert pairs_1[0].tolist() == [n for n, _ in want[:4]] and first.horizons.tolist() == [n for n, _ in want[4:]]
    assert pairs_1[1].tolist() == [float(g) for _, g in want[:4]] and first.gammas.tolist() == [float(g) for _, g in want[4:]]
    assert [n for n, _ in want] == [3, 2, 2, 2, 1, 1, 1, 1] and want[7][1] == np.float32(0.99)
    assert eager._hz_step == graphed._hz_step == 8 and eager._horizon_logs() == graphed._horizon_logs() == {"update_horizon": 1, "gamma": float(np.float32(0.99))}
    _compare(eager, graphed, "first eight steps")
    assert eager._graphed is None and not torch.equal(fresh, eager._engine.params)
    # the discounts of the last replay's batches are gamma ** n of their steps
    if not extras:  # (uniform: one batch slot per step; n = 1 on the last four steps)
        for slot, (n, g) in enumerate(want[4:]):
            assert n == 1 and (first.discount[slot] == float(g)).all()
    if extras:
        ta, tb = rb_e._sampling_distribution._sum_tree, rb_g._sampling_distribution._sum_tree
        assert torch.equal(ta._nodes_dev, tb._nodes_dev) and torch.equal(eager.aug_count, graphed.aug_count)
    # a reset in between restarts the schedule in both; the live graph serves on
    for agent in (eager, graphed):
        agent.reset_parameters()
        assert agent._hz_step == 0
    for step in range(8):
        eager.update_online_params(step, rb_e)
    graphed.learn_steps(4, rb_g)
    assert first.horizons.tolist() == [n for n, _ in want[:4]]
    graphed.learn_steps(4, rb_g)
    assert graphed._graphed is first and first.graph is exe and graphed._captures == 1
    _compare(eager, graphed, "eight steps behind a reset")
    # the schedule is part of what a request has to match: an agent without it captures a step without the gather at a horizon
    plain = iSDQN(0, (84, 84, 4), A, K, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.9, 3, 1, 100, adam_eps=1.5e-4, batch_size=B)
    graphed._drop_graph()
    plain.learn_steps(4, rb_g)
    assert not plain._graphed.horizon and plain._graphed.discount is None
    torch.cuda.synchronize()


def test_graph_replay_equals_eager_steps_under_a_schedule_dqn():
    from slimdqn.networks.dqn import DQN

    A, B = 5, 8

    def make(use_graph):
        agent = DQN(0, (84, 84, 4), A, [8, 12, 16, 24], True, "cnn", 2e-4, 0.9, 3, 1, 100, adam_eps=1.5e-4, batch_size=B, use_graph=use_graph)
        agent.target_params.tensor.mul_(0.75)  # a target that is not the online network
        rb = _big_replay(B)
        agent.set_horizon_schedule(*SCHEDULE, replay_buffer=rb)
        return agent, rb

    (eager, rb_e), (graphed, rb_g) = make(False), make(True)
    for step in range(8):
        eager.update_online_params(step, rb_e)
    target = graphed._target_tensor(graphed.target_params)
    eng = graphed._engine
    g = graphed._graphed_update(rb_g, learn=lambda cb: eng.learn_on_batch_target(cb, target), key=target.data_ptr(), steps=4)
    exe = g.graph
    for _ in range(2):
        graphed._run_graph(g)
    assert graphed._graphed is g and g.graph is exe and graphed._captures == 1 and g.horizon
    _compare(eager, graphed, "DQN")
    assert eager._hz_step == graphed._hz_step == 8


def test_a_step_under_the_schedule_is_bit_identical_run_to_run():
    from slimdqn.networks.isdqn import iSDQN

    runs = []
    for _ in range(2):
        agent = iSDQN(0, (84, 84, 4), 5, 3, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.9, 3, 1, 100, adam_eps=1.5e-4, batch_size=8, use_graph=False)
        rb = _big_replay(8)
        agent.set_horizon_schedule(*SCHEDULE, replay_buffer=rb)
        for step in range(3):
            agent.update_online_params(step, rb)
        torch.cuda.synchronize()
        e = agent._engine
        runs.append([getattr(e, n).clone() for n in STATE] + [e.priorities.clone(), e.targets.clone()])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_the_analysis_agents_take_the_schedule():
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN

    B = 6
    a = AnalysisDQN(0, (84, 84, 4), 5, 3, [7, 9, 11, 13], True, False, "cnn", 2e-4, 0.9, 3, 1, 6, adam_eps=1.5e-4, batch_size=B)
    t = AnalysisTFDQN(0, (84, 84, 4), 5, [7, 9, 11, 13], True, False, "cnn", 2e-4, 0.9, 3, 1, 6, adam_eps=1.5e-4, batch_size=B)
    for agent in (a, t):
        rb = _big_replay(B)
        agent.set_horizon_schedule(*SCHEDULE, replay_buffer=rb)
        for step in range(3):
            agent.update_online_params(step, rb)
        torch.cuda.synchronize()
        assert agent._hz_step == 3 and agent._hz_last == hz.schedule(*SCHEDULE, 2)
        assert torch.isfinite(agent._engine.losses).all() and torch.isfinite(agent._engine.params).all()


# ===================================================================================== 6. the entry point
def test_entry_point_with_anneal(tmp_path):
    from experiments.atari import isdqn as entry
    from experiments.base import dqn as loop

    seen = {}
    train = loop.train

    def spy(key, p, agent, env, rb):
        seen["agent"], seen["rb"], seen["p"] = agent, rb, p
        return train(key, p, agent, env, rb)

    entry.train = spy
    try:
        argv = ["-en", "anneal_Synthetic", "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "200", "-bs", "8", "-n", "4", "-horizon", "50",
                "-at", "cnn", "-ne", "2", "-ntspe", "60", "-utd", "4", "-nis", "20", "-ed", "100", "-nbi", "2", "-ln", "-tuf", "16",
                "-env", "synthetic", "-anneal", "12", "-nend", "2", "-gamma", "0.9", "-gammaend", "0.99"]
        gathered = entry.run(argv, root=str(tmp_path))
    finally:
        entry.train = train
    assert len(gathered) == 2
    agent, rb, p = seen["agent"], seen["rb"], seen["p"]
    assert rb._horizon_window and rb._update_horizon == 4
    assert agent._hz_schedule == (4, 2, 0.9, 0.99, 12) and agent._hz_step >= 20
    logged = [h for h in p["wandb"].history if "update_horizon" in h]
    assert logged and logged[0]["update_horizon"] in (2, 3, 4) and logged[-1]["update_horizon"] == 2 and logged[-1]["gamma"] == float(np.float32(0.99))
    assert all(a["update_horizon"] >= b["update_horizon"] for a, b in zip(logged, logged[1:]))
    out = tmp_path / "atari" / "exp_output" / "anneal_Synthetic"
    res = json.load(open(out / "isdqn" / "episode_returns_and_lengths" / "1.json"))
    assert len(res["episode_returns"]) == 2
    import pickle

    model = pickle.load(open(out / "isdqn" / "models" / "1", "rb"))["params"]
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())
    assert torch.isfinite(agent._engine.losses).all() and torch.isfinite(agent._engine.losses_accum).all()
    # the larger of -n and -nend builds the replay
    for bad in (["-nend", "2"], ["-gammaend", "0.99"], ["-anneal", "5", "-nend", "0"], ["-anneal", "5", "-gammaend", "1.0"]):
        with pytest.raises(ValueError):
            entry.run(["-en", "bad_Synthetic", "-s", "1", "-dw", "-env", "synthetic"] + bad, root=str(tmp_path))
