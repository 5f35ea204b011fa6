"""Periodic resets and EMA targets on the device (include/isdqn_hip.h, isdqn_net_reset / isdqn_net_ema) against the numpy float32
restatements of tests/helpers/reset.py, bit for bit.

Shapes, the smallest that still have padding lanes and every tensor kind: cnn (8, 12, 16, 24) on (84, 84, 4) with and without LayerNorm
(12 channels pad to 16), fc (40, 24) on (11,), impala (8, 16, 16, 24) on (44, 44, 3) with LayerNorm, and the BatchNorm cnn (8, 16, 8, 32)
on (44, 44, 2) of tests/test_gpu_batchnorm.py, and its impala + BatchNorm network (16, 8, 16, 24) on (36, 36, 2), whose 70 tensors do not
fit one launch's table; B = 4, A = 5, K = 2.  The starting state of every case is the state after three learn
steps (moments and step count non-trivial), made once per case and restored in front of every call; subnormal parameters, should a
step ever leave one, are flushed to zero on the host first (the definitions are stated for normal numbers and zeros).

tests/test_reset_host.py shows that every wrong variant of the helper differs from the definition on one of the factor sets used here;
a device result that equals the definition on all of them equals none of the variants."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.helpers import reset as hr

pytestmark = pytest.mark.gpu

A, K, B = 5, 2, 4
CASES = {
    "cnn": dict(arch="cnn", obs=(84, 84, 4), feats=(8, 12, 16, 24), ln=False),
    "cnn-ln": dict(arch="cnn", obs=(84, 84, 4), feats=(8, 12, 16, 24), ln=True),
    "fc": dict(arch="fc", obs=(11,), feats=(40, 24), ln=False),
    "impala-ln": dict(arch="impala", obs=(44, 44, 3), feats=(8, 16, 16, 24), ln=True),
    "cnn-bn": dict(arch="cnn", obs=(44, 44, 2), feats=(8, 16, 8, 32), ln=True, batch_norm=True),
    "impala-bn": dict(arch="impala", obs=(36, 36, 2), feats=(16, 8, 16, 24), ln=False, batch_norm=True),  # 70 tensors: the table is split
}
FACTORS = (((0.5, 0.5), (0.0, 1.0)), ((0.8, 0.2), (0.3, 0.7)), ((1.0, 0.0), (0.0, 1.0)))  # (lower, upper) pairs of (shrink, perturb)
BUFFERS = ("params", "adam_m", "adam_v", "adam_count")


def _engine(name, **kw):
    from slimdqn._engine import QNetEngine

    c = CASES[name]
    return QNetEngine(c["obs"], A, 1 + K, c["feats"], c["arch"], c["ln"], B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4,
                      batch_norm=c.get("batch_norm", False), **kw)


def _batch(eng, name, mirror_current=False, seed=0):
    c = CASES[name]
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    common = dict(action=dev(rng.integers(0, A, B).astype(np.int32)), reward=dev(rng.normal(size=B).astype(np.float32)),
                  terminal=dev((rng.random(B) < 0.3).astype(np.uint8)), mirror_current=mirror_current)
    if c["arch"] == "fc":
        d = int(np.prod(c["obs"]))
        return eng.make_batch(state=dev(rng.normal(size=(B, d)).astype(np.float32)), next_state=dev(rng.normal(size=(B, d)).astype(np.float32)), **common)
    h, w, stack = c["obs"]
    n_frames = 3 * B + 8
    ids = rng.integers(0, n_frames, (B, 2 * stack)).astype(np.int32)
    ids[rng.random(ids.shape) < 0.1] = -1
    return eng.make_batch(frames=dev(rng.integers(0, 256, (n_frames, h * w), dtype=np.uint8)), frame_stride=h * w, frame_ids=dev(ids), **common)


def _host(eng, names=BUFFERS):
    return {n: getattr(eng, n).cpu().numpy().copy() for n in names}


def _restore(eng, state):
    for n, a in state.items():
        getattr(eng, n).copy_(torch.from_numpy(a))


@functools.lru_cache(maxsize=None)
def _trained(name, **kw):
    """(engine, its state after three learn steps on the host, fresh parameters on the device and on the host).  Shared by the tests of a
    case; every test restores the state first and leaves the host copies alone."""
    eng = _engine(name, **kw)
    eng.init_params(3)
    batch = _batch(eng, name)
    if eng.noisy:
        eng.resample_noise()  # (under zero noise sigma has no gradient)
    for _ in range(3):
        eng.learn_on_batch(batch)
    state = _host(eng)
    p = state["params"]
    p[(np.abs(p) < np.finfo(np.float32).tiny) & (p != 0)] = 0
    assert state["adam_count"].tolist() == [3] and np.abs(state["adam_m"]).max() > 0 and np.isfinite(p).all()
    fresh = eng.fresh_params(12345)
    return eng, state, fresh, fresh.cpu().numpy()


def _assert_state(eng, want, what=""):
    for n, w in zip(BUFFERS, want):
        got = getattr(eng, n).cpu().numpy()
        assert np.array_equal(hr.bits(got), hr.bits(w)), f"{what}{n}: {(hr.bits(got) != hr.bits(w)).sum()} words differ from the restated definition"


def _splits(eng):
    n_layers, first = eng.reset_layout()
    assert (n_layers, first) == hr.layout_numbers(eng)
    return [0, first, n_layers - 1, n_layers]


@pytest.mark.parametrize("name", list(CASES))
def test_reset_matches_the_restated_definition(name):
    """1: params, adam_m, adam_v and adam_count bit for bit, for every split layer and every factor set."""
    eng, state, fresh, fresh_h = _trained(name)
    args = [state[n] for n in BUFFERS]
    changed = 0
    for split in _splits(eng):
        for lower, upper in FACTORS:
            _restore(eng, state)
            eng.reset(fresh, split, *lower, *upper)
            want = hr.reset(eng, *args, fresh_h, split, lower, upper)
            _assert_state(eng, want, f"split {split}, factors {lower} | {upper}: ")
            changed += int(not np.array_equal(want[0], state["params"]))
    assert changed >= 8  # (the factor sets do write: only (1, 0 | 0, 1) at split = n_layers leaves the parameters alone)


def test_reset_of_unaligned_buffers_takes_the_scalar_path():
    """1, the path without 16-byte accesses: the four buffers start one float behind an aligned address; the floats around them stay."""
    from slimdqn import _hip

    name = "fc"
    eng, state, fresh, fresh_h = _trained(name)
    n, G, SENT = eng.n_param_floats, 5, -7.25
    bufs = [torch.full((n + 2 * G,), SENT, device="cuda") for _ in range(4)]
    for b, a in zip(bufs, (state["params"], state["adam_m"], state["adam_v"], fresh_h)):
        b[G : G + n].copy_(torch.from_numpy(a))
    assert all((b.data_ptr() + 4 * G) % 16 == 4 for b in bufs)
    at = lambda t: t.data_ptr() + 4 * G
    split, (lower, upper) = 1, FACTORS[1]
    _hip.check(eng.lib.isdqn_net_reset(ctypes.byref(eng.cfg), at(bufs[0]), at(bufs[1]), at(bufs[2]), None, at(bufs[3]), split, *lower, *upper, None,
                                       _hip.stream_ptr(eng.device)), "isdqn_net_reset")
    want = hr.reset(eng, state["params"], state["adam_m"], state["adam_v"], None, fresh_h, split, lower, upper)
    for b, w in zip(bufs, want[:3] + (fresh_h,)):
        got = b.cpu().numpy()
        assert np.array_equal(hr.bits(got[G : G + n]), hr.bits(w)) and (got[:G] == SENT).all() and (got[G + n :] == SENT).all()


@pytest.mark.parametrize("name", list(CASES))
def test_identity_factors_keep_every_bit(name):
    """2: (1, 0 | 1, 0) without a count pointer."""
    eng, state, fresh, _ = _trained(name)
    _restore(eng, state)
    eng.reset(fresh, 1, 1.0, 0.0, 1.0, 0.0, count=False)
    _assert_state(eng, [state[n] for n in BUFFERS])


@pytest.mark.parametrize("name", ["cnn-ln", "fc"])
def test_reset_recovers_from_nan_and_inf(name):
    """3: the upper class holds NaN and Inf; (0, 1) replaces it with the fresh parameters bit for bit, the lower class keeps its bits."""
    eng, state, fresh, fresh_h = _trained(name)
    split = eng.reset_layout()[1] if name != "fc" else 1
    broken = dict(state, params=state["params"].copy())
    upper = np.zeros(eng.n_param_floats, bool)
    for info in eng.infos:
        if info.layer >= split:
            upper[info.offset : info.offset + info.size] = True
    broken["params"][upper] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(upper.sum()))
    _restore(eng, broken)
    eng.reset(fresh, split, 1.0, 0.0, 0.0, 1.0)
    got = eng.params.cpu().numpy()
    assert 0 < upper.sum() < upper.size and np.isfinite(got).all()
    assert np.array_equal(hr.bits(got[upper]), hr.bits(fresh_h[upper])) and np.array_equal(hr.bits(got[~upper]), hr.bits(state["params"][~upper]))
    _assert_state(eng, hr.reset(eng, *[broken[n] for n in BUFFERS], fresh_h, split, (1.0, 0.0), (0.0, 1.0)))


@pytest.mark.parametrize("name", list(CASES))
def test_a_full_reset_then_a_step_equals_a_first_step_from_the_fresh_parameters(name):
    """4: engine A starts from `fresh` and takes one learn step; engine B trains three steps, is reset with (0, 1) in both classes and
    takes the same step on the weight mirror the reset left (ISDQN_BATCH_MIRROR_CURRENT).  Parameters, moments, count and losses agree
    bit for bit: the moments were cleared, the count restarted and the mirror rebuilt."""
    eng_b, state, fresh, fresh_h = _trained(name)
    eng_a = _engine(name)
    eng_a.params.copy_(fresh)
    loss_a = eng_a.learn_on_batch(_batch(eng_a, name, seed=1)).cpu().numpy().copy()
    _restore(eng_b, state)
    eng_b.reset(fresh, eng_b.reset_layout()[1], 0.0, 1.0, 0.0, 1.0)
    loss_b = eng_b.learn_on_batch(_batch(eng_b, name, mirror_current=True, seed=1)).cpu().numpy().copy()
    assert np.array_equal(hr.bits(loss_a), hr.bits(loss_b)) and np.isfinite(loss_a).all()
    _assert_state(eng_b, [getattr(eng_a, n).cpu().numpy() for n in BUFFERS])
    assert eng_a.adam_count.item() == 1 and not np.array_equal(eng_a.params.cpu().numpy(), fresh_h)


def test_dueling_zeros_and_padding_lanes_stay_positive_zero():
    """5: on a dueling engine the structural zeros of the head and every padding lane are +0.0f by bit pattern in all three buffers
    after a reset, and the buffers follow the definition."""
    name = "cnn-ln"
    eng, state, fresh, fresh_h = _trained(name, dueling=True)
    dead = np.zeros(eng.n_param_floats, bool)
    head = eng.head_kernel_info()
    for info in eng.infos:
        real = np.ones(tuple(info.flax_shape[: info.ndim]), np.float32)
        if info.offset == head.offset:
            real = eng.dueling_live_mask().astype(np.float32)
        dead[info.offset : info.offset + info.size] = eng._to_internal(info, real).reshape(-1) == 0
    assert dead.sum() > 500 and not hr.bits(state["params"])[dead].any() and not hr.bits(fresh_h)[dead].any()
    for lower, upper in FACTORS[:2]:
        _restore(eng, state)
        eng.reset(fresh, None, *lower, *upper)
        _assert_state(eng, hr.reset(eng, *[state[n] for n in BUFFERS], fresh_h, eng.reset_layout()[1], lower, upper))
        for n in BUFFERS[:3]:
            assert not hr.bits(getattr(eng, n).cpu().numpy())[dead].any(), n


def test_sigma_of_a_noisy_engine_follows_the_rule():
    """6: sigma and its moments against the definition (towards the initial sigma); the next compose equals a compose on the restated
    sigma; mu, its moments and the count are not this call's."""
    name = "fc"
    eng, state, fresh, fresh_h = _trained(name, noisy=True, noisy_seed=7)
    sig = _host(eng, ("sigma", "sigma_m", "sigma_v"))
    assert np.abs(sig["sigma_m"]).max() > 0
    fresh_sigma = eng.fresh_sigma()
    split, (lower, upper) = 1, FACTORS[1]
    _restore(eng, state)
    eng.reset(fresh_sigma, split, *lower, *upper, params=eng.sigma)
    want = hr.reset(eng, sig["sigma"], sig["sigma_m"], sig["sigma_v"], None, fresh_sigma.cpu().numpy(), split, lower, upper)
    for n, w in zip(("sigma", "sigma_m", "sigma_v"), want):
        assert np.array_equal(hr.bits(getattr(eng, n).cpu().numpy()), hr.bits(w)), n
    assert not np.array_equal(want[0], sig["sigma"])
    _assert_state(eng, [state[n] for n in BUFFERS])
    eng.resample_noise()
    eff = eng.compose().clone()
    restated = torch.from_numpy(want[0]).cuda()
    other = eng.compose(sigma=restated, eff=torch.empty_like(eng.params), mirror=False)
    assert np.array_equal(hr.bits(eff.cpu().numpy()), hr.bits(other.cpu().numpy())) and not torch.equal(eff, eng.params)
    _restore(eng, dict(sig))


# ---------------------------------------------------------------------------------------------------------------- agents
def _agent_and_replay(cls, use_graph, n_fill=80, **kw):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    Bs, C = 8, 128
    isdqn = cls.__name__ == "iSDQN"
    args = (0, (84, 84, 4), A) + ((K,) if isdqn else ()) + ([8, 12, 16, 24], False) + ((False,) if isdqn else ())
    agent = cls(*args, "cnn", 2e-4, 0.99, 1, 1, 1000, adam_eps=1.5e-4, batch_size=Bs, use_graph=use_graph, **kw)
    rb = ReplayBuffer(UniformSamplingDistribution(5), Bs, C, update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(0)
    for _ in range(n_fill):
        obs = rng.integers(0, 256, (84, 84), dtype=np.uint8)
        term = bool(rng.random() < 0.08)
        rb.add(TransitionElement(obs, int(rng.integers(0, A)), float(rng.choice([-1.0, 0.0, 1.0])), term, term))
    return agent, rb


def test_dqn_resets_online_and_target_towards_the_same_fresh_parameters():
    """7: the online parameters with moments and count, the target copy with the same fresh parameters and factors and no moments."""
    from slimdqn.networks._agent import reset_seed
    from slimdqn.networks.dqn import DQN

    agent, rb = _agent_and_replay(DQN, use_graph=False)
    agent.learn_steps(3, rb)
    eng = agent._engine
    before = _host(eng)
    target = agent.target_params.tensor.cpu().numpy().copy()
    assert not np.array_equal(target, before["params"])
    ptrs = (eng.params.data_ptr(), agent.target_params.tensor.data_ptr())
    agent.reset_parameters(shrink=0.8)
    fresh_h = eng.fresh_params(reset_seed(agent._seed, 0)).cpu().numpy()
    split = eng.reset_layout()[1]
    s = np.float32(0.8)
    lower, upper = (float(s), float(np.float32(1) - s)), (0.0, 1.0)
    _assert_state(eng, hr.reset(eng, *[before[n] for n in BUFFERS], fresh_h, split, lower, upper))
    want_target = hr.reset(eng, target, None, None, None, fresh_h, split, lower, upper)[0]
    assert np.array_equal(hr.bits(agent.target_params.tensor.cpu().numpy()), hr.bits(want_target))
    assert ptrs == (eng.params.data_ptr(), agent.target_params.tensor.data_ptr()) and agent._resets == 1
    # the second reset draws other parameters; n_top_layers = 1 re-initialises the last Dense alone, shrink = 1 keeps the rest
    mid = _host(eng)
    agent.reset_parameters(shrink=1.0, n_top_layers=1)
    fresh2 = eng.fresh_params(reset_seed(agent._seed, 1)).cpu().numpy()
    assert not np.array_equal(fresh2, fresh_h)
    _assert_state(eng, hr.reset(eng, *[mid[n] for n in BUFFERS], fresh2, eng.reset_layout()[0] - 1, (1.0, 0.0), (0.0, 1.0)))


def test_isdqn_resets_all_heads_together():
    """7: the 1 + K heads share the last Dense: after a reset its kernel and bias are the fresh ones in every head, the target head 0
    included, and the torso is the blend."""
    from slimdqn.networks._agent import reset_seed
    from slimdqn.networks.isdqn import iSDQN

    agent, rb = _agent_and_replay(iSDQN, use_graph=False)
    agent.learn_steps(2, rb)
    eng = agent._engine
    before = _host(eng)
    agent.reset_parameters()
    fresh_h = eng.fresh_params(reset_seed(agent._seed, 0)).cpu().numpy()
    got = eng.params.cpu().numpy()
    n_layers, first = eng.reset_layout()
    for info in eng.infos:
        sl = slice(info.offset, info.offset + info.size)
        if info.layer == n_layers - 1:
            assert info.flax_shape[info.ndim - 1] == (1 + K) * A
            assert np.array_equal(hr.bits(got[sl]), hr.bits(fresh_h[sl])) and not np.array_equal(before["params"][sl], fresh_h[sl])
    _assert_state(eng, hr.reset(eng, *[before[n] for n in BUFFERS], fresh_h, first, (0.5, 0.5), (0.0, 1.0)))


@pytest.mark.parametrize("agent_name", ["iSDQN", "DQN"])
def test_captured_update_stays_valid_across_a_reset(agent_name):
    """7: learn_steps(3), reset_parameters, learn_steps(3) through the captured graph ends with the bits of the same sequence run
    eagerly, and nothing is captured again."""
    import importlib

    cls = getattr(importlib.import_module(f"slimdqn.networks.{agent_name.lower()}"), agent_name)
    (eager, rb_e), (graphed, rb_g) = _agent_and_replay(cls, False), _agent_and_replay(cls, True)
    for agent, rb in ((eager, rb_e), (graphed, rb_g)):
        agent.trust_mirror = True  # as the trainer declares it: the replay behind the reset takes the mirror the reset left
        agent.learn_steps(3, rb)
        captures = getattr(agent, "_captures", 0)
        agent.reset_parameters()
        assert agent._engine.adam_count.item() == 0
        agent.learn_steps(3, rb)
        assert getattr(agent, "_captures", 0) == captures
    assert eager._graphed is None and graphed._graphed is not None and graphed._captures == 1
    for n in BUFFERS + ("losses_accum",):
        assert torch.equal(getattr(eager._engine, n), getattr(graphed._engine, n)), f"{n} differs between the eager and the captured sequence"
    if agent_name == "DQN":
        assert torch.equal(eager.target_params.tensor, graphed.target_params.tensor)
    assert eager._engine.adam_count.item() == 3


# ---------------------------------------------------------------------------------------------------------------- EMA
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("name", ["cnn", "fc"])
def test_ema_matches_the_restated_definition(name, aligned):
    """8: tau in {0, 0.005, 0.5, 1} bit for bit; tau = 1 is a copy (the sign of a zero and a NaN target included), tau = 0 leaves the
    target.  Every plan's buffer length is a multiple of 8 floats, so the path without 16-byte accesses is reached the way a caller can
    reach it: buffers that start one float behind an aligned address (all elements then take it).  The floats around stay."""
    from slimdqn import _hip

    eng, _, _, _ = _trained(name)
    n, G, SENT = eng.n_param_floats, 4 if aligned else 5, -7.25
    rng = np.random.default_rng(5)
    t0, p0 = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    t0[:3], p0[:3] = [0.0, np.nan, -1.0], [-0.0, 2.0, np.inf]
    online = torch.full((n + 2 * G,), SENT, device="cuda")
    online[G : G + n].copy_(torch.from_numpy(p0))
    for tau in (0.0, 0.005, 0.5, 1.0):
        t_in = t0.copy()
        if 0.0 < tau < 1.0:
            t_in[1] = 3.0  # (a NaN operand: the payload of the result is not part of the definition)
        target = torch.full((n + 2 * G,), SENT, device="cuda")
        target[G : G + n].copy_(torch.from_numpy(t_in))
        assert (target.data_ptr() + 4 * G) % 16 == (0 if aligned else 4)
        if aligned:
            eng.ema(target[G : G + n], tau, online=online[G : G + n])
        else:
            _hip.check(eng.lib.isdqn_net_ema(ctypes.byref(eng.cfg), target.data_ptr() + 4 * G, online.data_ptr() + 4 * G, tau, _hip.stream_ptr(eng.device)))
        got = target.cpu().numpy()
        want = hr.ema(t_in, p0, tau)
        assert np.array_equal(hr.bits(got[G : G + n]), hr.bits(want)), f"tau {tau}: {(hr.bits(got[G : G + n]) != hr.bits(want)).sum()} words differ"
        assert (got[:G] == SENT).all() and (got[G + n :] == SENT).all()
        if tau == 1.0:
            assert np.array_equal(hr.bits(got[G : G + n]), hr.bits(p0))
        if tau == 0.0:
            assert np.array_equal(hr.bits(got[G : G + n]), hr.bits(t_in))
    assert np.array_equal(hr.bits(online.cpu().numpy()[G : G + n]), hr.bits(p0))


def test_dqn_with_an_ema_target():
    """9: ema_tau = 0.005 -- eager and captured twins hold the same online and target bits after 5 steps; after step 1 the target is the
    definition applied to the recorded online parameters; update_target_params copies nothing."""
    from slimdqn.networks.dqn import DQN

    (eager, rb_e), (graphed, rb_g) = _agent_and_replay(DQN, False, ema_tau=0.005), _agent_and_replay(DQN, True, ema_tau=0.005)
    t0 = eager.target_params.tensor.cpu().numpy().copy()
    assert torch.equal(eager.target_params.tensor, graphed.target_params.tensor)
    eager.update_online_params(0, rb_e)
    graphed.update_online_params(0, rb_g)
    online1 = eager.params.tensor.cpu().numpy()
    want = hr.ema(t0, online1, 0.005)
    assert not np.array_equal(online1, t0) and not np.array_equal(want, t0)
    for agent in (eager, graphed):
        assert np.array_equal(hr.bits(agent.target_params.tensor.cpu().numpy()), hr.bits(want))
    for agent, rb in ((eager, rb_e), (graphed, rb_g)):
        for step in range(1, 5):
            agent.update_online_params(step, rb)
    assert eager._graphed is None and graphed._graphed is not None and graphed._captures == 1
    assert torch.equal(eager.params.tensor, graphed.params.tensor) and torch.equal(eager.target_params.tensor, graphed.target_params.tensor)
    assert torch.equal(eager._engine.adam_count, graphed._engine.adam_count) and eager._engine.adam_count.item() == 5
    for agent in (eager, graphed):
        target = agent.target_params.tensor.clone()
        updated, logs = agent.update_target_params(1000)
        assert updated and "loss" in logs and torch.equal(agent.target_params.tensor, target) and not torch.equal(target, agent.params.tensor)


@pytest.mark.parametrize("use_graph", [False, True])
def test_dqn_with_ema_tau_one_tracks_the_online_parameters(use_graph):
    """9: with ema_tau = 1 the target equals the online parameters after every step."""
    from slimdqn.networks.dqn import DQN

    agent, rb = _agent_and_replay(DQN, use_graph, ema_tau=1.0)
    start = agent.params.tensor.clone()
    for step in range(3):
        agent.update_online_params(step, rb)
        assert torch.equal(agent.target_params.tensor, agent.params.tensor)
    assert not torch.equal(agent.params.tensor, start)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_with_their_codes_on_live_buffers():
    """10: every ISDQN_ERR_ARG of the two calls on device pointers; no refused call writes anything."""
    from slimdqn import _hip

    eng, state, fresh, _ = _trained("fc")
    _restore(eng, state)
    other = eng.params.clone()
    st = _hip.stream_ptr(eng.device)

    def reset(params=eng.params, m=eng.adam_m, v=eng.adam_v, count=eng.adam_count, fresh=fresh, split=1, f=(0.5, 0.5, 0.0, 1.0), ws=eng.workspace):
        at = lambda t: t if isinstance(t, int) else _hip.ptr(t)
        return eng.lib.isdqn_net_reset(ctypes.byref(eng.cfg), at(params), at(m), at(v), at(count), at(fresh), split, *f, at(ws), st)

    assert reset(params=None) == _hip.ERR_ARG and reset(fresh=None) == _hip.ERR_ARG
    assert reset(m=None) == _hip.ERR_ARG and reset(v=None) == _hip.ERR_ARG
    for bad in (-0.5, float("nan"), float("inf")):
        for k in range(4):
            f = [0.5, 0.5, 0.0, 1.0]
            f[k] = bad
            assert reset(f=tuple(f)) == _hip.ERR_ARG, (bad, k)
    n_layers = eng.reset_layout()[0]
    assert reset(split=-1) == _hip.ERR_ARG and reset(split=n_layers + 1) == _hip.ERR_ARG
    assert reset(fresh=eng.params) == _hip.ERR_ARG and reset(fresh=eng.params.data_ptr() + 4 * (eng.n_param_floats - 1)) == _hip.ERR_ARG
    ema = lambda target=other, online=eng.params, tau=0.005: eng.lib.isdqn_net_ema(ctypes.byref(eng.cfg), _hip.ptr(target), _hip.ptr(online), tau, st)
    assert ema(target=None) == _hip.ERR_ARG and ema(online=None) == _hip.ERR_ARG and ema(target=eng.params) == _hip.ERR_ARG
    for tau in (-1e-3, 1.001, float("nan")):
        assert ema(tau=tau) == _hip.ERR_ARG
    with pytest.raises(RuntimeError):
        eng.reset(fresh, 1, shrink_lower=-1.0)
    with pytest.raises(RuntimeError):
        eng.ema(other, 2.0)
    torch.cuda.synchronize()
    _assert_state(eng, [state[n] for n in BUFFERS])
    assert torch.equal(other, eng.params)
    assert reset() == _hip.OK and reset(m=None, v=None, count=None, ws=None) == _hip.OK and ema() == _hip.OK
