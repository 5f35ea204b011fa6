"""The soft head shift on the device (include/isdqn_hip.h, isdqn_net_soft_shift) against the numpy float32 restatement of
tests/helpers/soft_shift.py, bit for bit, and through the engine and the agents.

The kernel sees the last Dense only, so every network is an fc torso on 8 observations (tests/helpers/soft_shift.py, CONFIGS): a padded
and an unpadded in_p, K in {1, 3}, scalar / histogram / quantile / dueling heads, tau in {0.005, 0.5}; "wide" spans 459 workgroups and
"stride" is the one size past the capped grid, where the stride loop takes a second turn.  The parameters are random normal numbers (the
kernel does not care where they come from), the Adam moments random too, so that a stray write anywhere shows.

tests/test_soft_shift_host.py shows that the contracted variant and the variant that reads already-shifted neighbours differ from the
restatement (at tau = 0.005; K = 3 for the second): a device result that equals the restatement equals neither."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from slimdqn import _hip
from tests.helpers import soft_shift as hs

pytestmark = pytest.mark.gpu

BUFFERS = ("params", "adam_m", "adam_v", "adam_count", "losses_accum")


def _bits(t):
    return hs.bits(t.detach().cpu().numpy())


def _randomise(eng, seed=0):
    """Random parameters and moments in the engine's own buffers; returns the host copy of the parameters."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = eng.n_param_floats
    host = torch.randn(n, generator=g)
    eng.params.copy_(host)
    eng.adam_m.copy_(torch.randn(n, generator=g))
    eng.adam_v.copy_(torch.rand(n, generator=g))
    eng.adam_count.fill_(7)
    return host.numpy().copy()


def _mirror(eng, workspace=None):
    """The workspace's weight-mirror region as int32 words (a view)."""
    off, size = ctypes.c_int64(), ctypes.c_int64()
    assert eng.lib.isdqn_net_workspace_region(ctypes.byref(eng.cfg), b"wsplit", ctypes.byref(off), ctypes.byref(size)) == 0
    assert off.value % 32 == 0 and size.value >= 4 * eng.n_param_floats  # (the region: the buffer's length rounded up)
    ws = eng.workspace if workspace is None else workspace
    return ws[off.value // 4 : (off.value + size.value) // 4].view(torch.int32)


def _call(eng, params, tau, workspace=None):
    return eng.lib.isdqn_net_soft_shift(ctypes.byref(eng.cfg), _hip.ptr(params), tau, _hip.ptr(workspace), _hip.stream_ptr(eng.device))


@functools.lru_cache(maxsize=None)
def _engine(name, **kw):
    return hs.make_engine(name, **kw)


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", list(hs.CONFIGS))
def test_kernel_matches_the_restated_definition_and_keeps_every_other_bit(name):
    """Master alone (NULL workspace) and master + mirror: the parameters equal the restatement bit for bit -- which holds heads 0 .. K-1
    blended and head K, the padding rows and every other tensor unchanged --, the moments and the count keep their bits, and with a
    workspace the mirror region equals what isdqn_net_refresh_mirror makes of the NEW parameters in a second workspace."""
    eng = _engine(name)
    for tau in hs.TAUS:
        p0 = _randomise(eng)
        m0, v0 = _bits(eng.adam_m), _bits(eng.adam_v)
        want = hs.soft_shift(eng, p0, tau)
        assert not np.array_equal(hs.bits(want), hs.bits(p0))
        # the master alone, on a copy
        copy = eng.params.clone()
        assert _call(eng, copy, tau) == 0
        assert np.array_equal(_bits(copy), hs.bits(want)), f"tau {tau}: {(_bits(copy) != hs.bits(want)).sum()} words differ (NULL workspace)"
        assert np.array_equal(_bits(eng.params), hs.bits(p0))
        # master and mirror, through the engine
        eng.rebuild_mirror()
        before = _mirror(eng).clone()
        eng.soft_shift(tau)
        assert np.array_equal(_bits(eng.params), hs.bits(want)), f"tau {tau}: {(_bits(eng.params) != hs.bits(want)).sum()} words differ"
        assert np.array_equal(_bits(eng.adam_m), m0) and np.array_equal(_bits(eng.adam_v), v0) and eng.adam_count.item() == 7
        second = torch.zeros_like(eng.workspace)
        assert eng.lib.isdqn_net_refresh_mirror(ctypes.byref(eng.cfg), eng.params.data_ptr(), second.data_ptr(), _hip.stream_ptr(eng.device)) == 0
        torch.cuda.synchronize()
        got, ref = _mirror(eng), _mirror(eng, second)
        assert torch.equal(got, ref), f"tau {tau}: {(got != ref).sum().item()} mirror words differ from a rebuild on the new parameters"
        assert not torch.equal(got, before)  # (a shift that wrote the master alone would have left the stale heads here)


def test_tau_one_is_the_hard_shift_and_tau_zero_is_nothing():
    """tau = 1 leaves the bits isdqn_net_shift_params leaves on a copy, NaN, infinity and -0 planted in head rows included, and with a
    workspace a current mirror; tau = 0 changes nothing."""
    eng = _engine("f20-K3-bins")
    p0 = _randomise(eng, seed=1)
    w, b = hs.head_views(eng, p0)
    w[1, 0, 0], w[2, 1, 3], w[3, 2, 5], w[0, 4, 4], b[1, 1], b[0, 0], b[3, 2] = np.nan, -0.0, np.inf, np.nan, -0.0, np.nan, -0.0
    eng.params.copy_(torch.from_numpy(p0))
    hard = eng.params.clone()
    eng.shift_params(params=hard)
    want = hs.soft_shift(eng, p0, 1.0)
    assert np.array_equal(_bits(hard), hs.bits(want)) and not np.array_equal(hs.bits(want), hs.bits(p0))
    copy = eng.params.clone()
    assert _call(eng, copy, 1.0) == 0 and np.array_equal(_bits(copy), _bits(hard))
    assert _call(eng, copy, 0.0) == 0 and np.array_equal(_bits(copy), _bits(hard))
    eng.rebuild_mirror()
    before = _mirror(eng).clone()
    eng.soft_shift(0.0)
    assert np.array_equal(_bits(eng.params), hs.bits(p0)) and torch.equal(_mirror(eng), before)
    eng.soft_shift(1.0)
    assert np.array_equal(_bits(eng.params), _bits(hard))
    second = torch.zeros_like(eng.workspace)
    assert eng.lib.isdqn_net_refresh_mirror(ctypes.byref(eng.cfg), eng.params.data_ptr(), second.data_ptr(), _hip.stream_ptr(eng.device)) == 0
    torch.cuda.synchronize()
    assert torch.equal(_mirror(eng), _mirror(eng, second))


def test_an_unaligned_view_is_refused_and_nothing_is_written():
    """The lanes are 16 bytes wide and there is no scalar path: a parameter view one float behind an aligned address is ISDQN_ERR_ARG."""
    eng = _engine("f24-K3-scalar")
    n = eng.n_param_floats
    buf = torch.randn(n + 8, device="cuda")
    keep = buf.clone()
    st = _hip.stream_ptr(eng.device)
    assert (buf.data_ptr() + 4) % 16 == 4
    for tau in (0.0, 0.005, 1.0):
        assert eng.lib.isdqn_net_soft_shift(ctypes.byref(eng.cfg), buf.data_ptr() + 4, tau, None, st) == _hip.ERR_ARG
        assert "aligned" in _hip.last_error()
    assert torch.equal(buf, keep)
    assert eng.lib.isdqn_net_soft_shift(ctypes.byref(eng.cfg), buf.data_ptr() + 16, 0.005, None, st) == _hip.OK  # four floats in: aligned again
    assert np.array_equal(_bits(buf[4 : 4 + n]), hs.bits(hs.soft_shift(eng, keep[4 : 4 + n].cpu().numpy(), 0.005)))
    assert torch.equal(buf[:4], keep[:4]) and torch.equal(buf[4 + n :], keep[4 + n :])


def test_refusals_with_their_codes_on_live_buffers():
    from slimdqn._engine import QNetEngine

    eng = _engine("f20-K1-scalar")
    p0 = _randomise(eng, seed=2)
    eng.rebuild_mirror()
    mirror = _mirror(eng).clone()
    assert _call(eng, None, 0.005, eng.workspace) == _hip.ERR_ARG
    for tau in (-1e-3, 1.001, float("nan"), float("inf")):
        assert _call(eng, eng.params, tau, eng.workspace) == _hip.ERR_ARG, tau
    with pytest.raises(RuntimeError):
        eng.soft_shift(1.5)
    single = QNetEngine((8,), 3, 1, (20,), "fc", False, 4)
    single.params.normal_()
    keep = single.params.clone()
    for tau in (0.0, 0.005, 1.0):
        assert _call(single, single.params, tau, single.workspace) == _hip.ERR_ARG and "n_heads" in _hip.last_error()
    with pytest.raises(RuntimeError):
        single.soft_shift(0.005)
    assert torch.equal(single.params, keep)
    assert np.array_equal(_bits(eng.params), hs.bits(p0)) and torch.equal(_mirror(eng), mirror)


def test_sigma_of_a_noisy_engine_follows_the_rule():
    """One engine call shifts mu and sigma alike, the masters alone; the bookkeeping says the mirror no longer holds what a step may
    trust, and the next compose equals a compose on the restated buffers."""
    eng = hs.make_engine("f20-K3-scalar", noisy=True, noisy_seed=7)
    eng.init_params(3)
    mu0 = _randomise(eng, seed=3)
    sigma0 = eng.sigma.cpu().numpy().copy()
    live = sigma0 != 0
    sigma0[live] = np.random.default_rng(4).uniform(0.01, 0.5, int(live.sum())).astype(np.float32)  # (the other positions stay +0)
    eng.sigma.copy_(torch.from_numpy(sigma0))
    sm, sv = _bits(eng.sigma_m), _bits(eng.sigma_v)
    eng.resample_noise()
    eng.compose()
    eng.soft_shift(0.25)
    want_mu, want_sigma = hs.soft_shift(eng, mu0, 0.25), hs.soft_shift(eng, sigma0, 0.25)
    assert not np.array_equal(want_sigma, sigma0)
    assert np.array_equal(_bits(eng.params), hs.bits(want_mu)) and np.array_equal(_bits(eng.sigma), hs.bits(want_sigma))
    assert np.array_equal(_bits(eng.sigma_m), sm) and np.array_equal(_bits(eng.sigma_v), sv)
    assert not hs.bits(want_sigma)[~live].any()  # +0 stays +0 where sigma means nothing
    assert eng._mirror_version is None
    eff = eng.compose().clone()
    other = eng.compose(mu=torch.from_numpy(want_mu).cuda(), sigma=torch.from_numpy(want_sigma).cuda(), eff=torch.empty_like(eng.params), mirror=False)
    assert torch.equal(eff.view(torch.int32), other.view(torch.int32))
    # another buffer of the layout: that buffer alone
    copy = torch.from_numpy(mu0).cuda()
    sigma_now = _bits(eng.sigma)
    eng.soft_shift(0.25, params=copy)
    assert np.array_equal(_bits(copy), hs.bits(want_mu)) and np.array_equal(_bits(eng.sigma), sigma_now)


# ---------------------------------------------------------------------------------------------------------------- agents
TAU, K, B = 0.25, 3, 8


def _agent_and_replay(use_graph, prioritized=False, **kw):
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

    agent = iSDQN(0, (8,), hs.A, K, [20], False, False, "fc", 1e-3, 0.99, 1, 1, 1000, adam_eps=1.5e-4, batch_size=B, use_graph=use_graph, **kw)
    sampler = PrioritizedSamplingDistribution(5, 64) if prioritized else UniformSamplingDistribution(5)
    rb = ReplayBuffer(sampler, B, 64, stack_size=1, update_horizon=1, gamma=0.99)
    agent.priority_writeback = prioritized
    rng = np.random.default_rng(0)
    for _ in range(48):
        obs = rng.normal(size=8).astype(np.float32)
        term = bool(rng.random() < 0.08)
        extra = dict(priority=float(rng.uniform(0.1, 2.0))) if prioritized else {}
        rb.add(TransitionElement(obs, int(rng.integers(0, hs.A)), float(rng.normal()), term, term), **extra)
    return agent, rb


def _state(agent):
    return {n: getattr(agent._engine, n).clone() for n in BUFFERS}


def _same(a, b, what):
    for n in BUFFERS:
        x, y = a[n], b[n]
        same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)
        assert same, f"{n} differs between {what}"


@pytest.mark.parametrize("prioritized", [False, True])
def test_eager_captured_and_multi_step_updates_equal_the_hand_sequenced_loop(prioritized):
    """soft_shift_tau = 0.25, K = 3: three eager steps, three single-step captured steps and one learn_steps(3) capture end in
    bit-identical parameters, moments, step count and loss accumulator, and all equal learn_on_batch -> engine.soft_shift (-> priority
    write-back) sequenced by hand on an agent built without the option."""
    hand, rb_h = _agent_and_replay(False, prioritized)
    start = hand._engine.params.clone()
    for _ in range(3):
        batch = hand._sample(rb_h)
        hand.learn_on_batch(hand.params, hand.optimizer_state, batch)
        hand._engine.soft_shift(TAU)
        if prioritized:
            rb_h.update_device(batch, hand._engine.priorities)
    want = _state(hand)
    plain, rb_p = _agent_and_replay(False, prioritized)  # the same three steps without any shift: the shift is not a no-op
    for step in range(3):
        plain.update_online_params(step, rb_p)
    assert not torch.equal(want["params"], _state(plain)["params"]) and not torch.equal(want["params"], start)

    eager, rb_e = _agent_and_replay(False, prioritized, soft_shift_tau=TAU)
    single, rb_s = _agent_and_replay(True, prioritized, soft_shift_tau=TAU)
    multi, rb_m = _agent_and_replay(True, prioritized, soft_shift_tau=TAU)
    for step in range(3):
        eager.update_online_params(step, rb_e)
        single.update_online_params(step, rb_s)
    multi.learn_steps(3, rb_m)
    assert eager._graphed is None
    assert single._graphed is not None and single._graphed.S == 1 and single._captures == 1 and single._graphed.key == ("soft_shift", TAU)
    assert multi._graphed is not None and multi._graphed.S == 3 and multi._captures == 1 and multi._graphed.key == ("soft_shift", TAU)
    for agent, what in ((eager, "the eager steps"), (single, "the single-step captures"), (multi, "the learn_steps(3) capture")):
        assert agent._engine.adam_count.item() == 3
        _same(_state(agent), want, f"{what} and the hand-sequenced loop")
    if prioritized:
        trees = [rb._sampling_distribution._sum_tree._nodes_dev for rb in (rb_h, rb_e, rb_s, rb_m)]
        assert all(torch.equal(trees[0], t) for t in trees[1:])
    # a second replay of the multi-step capture against three more eager steps: steps 2 .. S trusted the mirror the shift kept current
    for step in range(3, 6):
        eager.update_online_params(step, rb_e)
    multi.learn_steps(3, rb_m)
    assert multi._captures == 1
    _same(_state(multi), _state(eager), "two learn_steps(3) replays and six eager steps")


def test_tau_zero_is_the_agent_without_the_option():
    off, rb_o = _agent_and_replay(True, soft_shift_tau=0.0)
    default, rb_d = _agent_and_replay(True)
    for agent, rb in ((off, rb_o), (default, rb_d)):
        for step in range(3):
            agent.update_online_params(step, rb)
        assert agent._graphed.key is None
        updated, _ = agent.update_target_params(1000)  # the hard shift
        assert updated
    _same(_state(off), _state(default), "soft_shift_tau = 0 and the default agent")


def test_update_target_params_shifts_nothing_under_a_soft_shift():
    agent, rb = _agent_and_replay(False, soft_shift_tau=TAU)
    agent.update_online_params(0, rb)
    before = agent._engine.params.clone()
    assert agent.update_target_params(999) == (False, {})
    updated, logs = agent.update_target_params(1000)
    assert updated and "loss" in logs and "networks/0_loss" in logs
    assert torch.equal(agent._engine.params.view(torch.int32), before.view(torch.int32))
    hard, rb_h = _agent_and_replay(False)
    hard.update_online_params(0, rb_h)
    before = hard._engine.params.clone()
    hard.update_target_params(1000)
    assert not torch.equal(hard._engine.params, before)


def test_analysis_agent_shifts_behind_its_step():
    from slimdqn.networks.analysisdqn import AnalysisDQN

    _, rb = _agent_and_replay(False)
    _, rb2 = _agent_and_replay(False)
    make = lambda **kw: AnalysisDQN(0, (8,), hs.A, K, [20], False, False, "fc", 1e-3, 0.99, 1, 1, 1000, adam_eps=1.5e-4, batch_size=B, **kw)
    soft, plain = make(soft_shift_tau=TAU), make()
    soft.update_online_params(0, rb)
    plain.update_online_params(0, rb2)
    want = hs.soft_shift(plain._engine, plain._engine.params.cpu().numpy(), TAU)
    assert np.array_equal(_bits(soft._engine.params), hs.bits(want)) and not np.array_equal(hs.bits(want), _bits(plain._engine.params))
