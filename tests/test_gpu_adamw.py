"""AdamW's decoupled weight decay on the device (include/isdqn_hip.h, isdqn_batch_decay) against the numpy restatement of
tests/helpers/adamw.py, bit for bit, in every kernel that runs Adam and through every layer up to the agents.

Which kernel updates which tensor (tests/test_gpu_optimizer.py; learn_step.h weight_gradient and clipped_adam):
  fc       8 -> 100 -> 100, A = 4, K = 1, B = 32, LayerNorm: Dense_1 -> the fused epilogue of the weight-gradient GEMM, the rest -> adam_kernel
  cnn      (32, 64, 64, 512), K = 9, A = 9, B = 32: the conv kernels -> adam_kernel over their slabs, Dense_0 -> the fused epilogue
  fc-clip  the fc site with max_grad_norm = 10: every tensor -> adam_flat_kernel
  cnn-bn   84 x 84 x 4, (8, 8, 8, 16), B = 4, BatchNorm and LayerNorm: batchnorm.h's own optimizer list (tensor kinds 0 .. 8)
  impala   84 x 84 x 4, (8, 8, 8, 16), B = 4, LayerNorm: impala.h's optimizer list for the torso, learn_step.h's for the Dense layers
  fc-duel  8 -> 20 -> 14 with dueling heads: the head kernel's structural zeros
Every site: plant moments and a step count, run one learn step without decay (p1, m1, v1, ...), restore, run it with the decay behind
the batch, and hold the result to the restatement from (p1, p0).  lr = 1e-3 and wd = 0.1 take 1e-4 of every element: some 2^11
spacings of it, so the restatement differs from p1 wherever p0 != 0 -- checked on the restatement alone, per decayed tensor, so a site
that ignores the decay cannot pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.helpers import adamw as hw

pytestmark = pytest.mark.gpu

LR, WD = 1e-3, 0.1
SITES = {
    "fc": dict(obs=(8,), feats=(100, 100), arch="fc", K=1, A=4, B=32, eps=1e-8),
    "cnn": dict(obs=(84, 84, 4), feats=(32, 64, 64, 512), arch="cnn", K=9, A=9, B=32, eps=1.5e-4),
    "fc-clip": dict(obs=(8,), feats=(100, 100), arch="fc", K=1, A=4, B=32, eps=1e-8, kw=dict(max_grad_norm=10.0)),
    "cnn-bn": dict(obs=(84, 84, 4), feats=(8, 8, 8, 16), arch="cnn", K=2, A=5, B=4, eps=1.5e-4, kw=dict(batch_norm=True)),
    "impala": dict(obs=(84, 84, 4), feats=(8, 8, 8, 16), arch="impala", K=2, A=5, B=4, eps=1.5e-4),
    "fc-duel": dict(obs=(8,), feats=(20, 14), arch="fc", K=2, A=4, B=32, eps=1e-8, kw=dict(dueling=True)),
}
STATE = ("params", "adam_m", "adam_v", "adam_count", "losses_accum")
OUTPUTS = ("adam_m", "adam_v", "adam_count", "losses", "losses_accum", "q_values", "targets", "priorities")


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).reshape(-1).view(np.int64 if a.dtype.itemsize == 8 else np.int32 if a.dtype.itemsize == 4 else np.uint8)


def _with_decay(batch, weight_decay, decay_kinds):
    """The caller's side of the C ABI, written out: an isdqn_batch_decay around the fields of ``batch``, the flag set."""
    from slimdqn import _hip

    b = _hip.BatchDecay()
    for name, _ in _hip.Batch._fields_:
        setattr(b, name, getattr(batch, name))
    if isinstance(batch, _hip.BatchDiscount):
        b.discount = batch.discount
    b.flags = batch.flags | _hip.BATCH_WEIGHT_DECAY
    b.weight_decay, b.decay_kinds = weight_decay, decay_kinds
    b._keep = batch  # (and with it the tensors it points to)
    return b


def _real(eng):
    """True where an internal parameter element is a real Flax element: not padding, not a structural zero of a dueling head."""
    mask = np.zeros(eng.n_param_floats, bool)
    head = eng.head_kernel_info() if eng.dueling else None
    for info in eng.infos:
        shape = tuple(info.flax_shape[: info.ndim])
        ones = eng.dueling_live_mask().astype(np.float32) if head is not None and info.offset == head.offset else np.ones(shape, np.float32)
        mask[info.offset : info.offset + info.size] = eng._to_internal(info, ones) != 0
    return mask


@functools.lru_cache(maxsize=None)
def _site(name):
    """(engine, batch, real-element mask) of a site, made once: parameters of init_params(3) with the biases and the normalisation
    scales and biases moved off their trivial initial values (a bias of 0 has nothing to decay), on real elements only."""
    from slimdqn._engine import QNetEngine

    c = SITES[name]
    A, B = c["A"], c["B"]
    eng = QNetEngine(c["obs"], A, 1 + c["K"], c["feats"], c["arch"], True, B, gamma_n=0.99, learning_rate=LR, adam_eps=c["eps"], **c.get("kw", {}))
    eng.init_params(3)
    real = _real(eng)
    rng = np.random.default_rng(17)
    p = eng.params.cpu().numpy()
    for info in eng.infos:
        if 2 <= info.kind <= 6:
            sl = slice(info.offset, info.offset + info.size)
            p[sl] = np.where(real[sl], p[sl] + rng.normal(0, 0.1, info.size).astype(np.float32), p[sl])
    eng.params.copy_(torch.from_numpy(p))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    common = dict(action=dev(rng.integers(0, A, B).astype(np.int32)), reward=dev(rng.normal(size=B).astype(np.float32)),
                  terminal=dev((rng.random(B) < 0.3).astype(np.uint8)))
    if c["arch"] == "fc":
        d = c["obs"][0]
        batch = eng.make_batch(state=dev(rng.normal(size=(B, d)).astype(np.float32)), next_state=dev(rng.normal(size=(B, d)).astype(np.float32)), **common)
    else:
        h, w, stack = c["obs"]
        n_frames = 3 * B + 8
        ids = rng.integers(0, n_frames, (B, 2 * stack)).astype(np.int32)
        ids[rng.random(ids.shape) < 0.1] = -1
        batch = eng.make_batch(frames=dev(rng.integers(0, 256, (n_frames, h * w), dtype=np.uint8)), frame_stride=h * w, frame_ids=dev(ids), **common)
    assert type(batch).__name__ == "Batch" and eng.weight_decay == 0.0
    return eng, batch, real


def _planted(name, t0):
    """The site's engine with moments planted (tests/test_gpu_optimizer.py _plant: six classes of (m, v) per element) and the count
    t0; returns (engine, batch, real, the state on the host)."""
    from tests.test_gpu_optimizer import _plant

    eng, batch, real = _site(name)
    g_pre = torch.zeros_like(eng.params)
    eng.grad_on_batch(batch, g_pre)
    m0, v0 = _plant(g_pre.cpu().numpy(), real, t0 + 1, SITES[name]["eps"], np.random.default_rng(11 + t0))
    eng.adam_m.copy_(torch.from_numpy(m0))
    eng.adam_v.copy_(torch.from_numpy(v0))
    eng.adam_count.fill_(t0)
    eng.losses_accum.zero_()
    return eng, batch, real, {n: getattr(eng, n).cpu().numpy().copy() for n in STATE}


def _restore(eng, state):
    for n, a in state.items():
        getattr(eng, n).copy_(torch.from_numpy(a))


def _step(eng, batch, state, learn=None):
    """Restore, one learn step (the debug form: the reduced gradient comes back), and everything the step wrote, on the host."""
    _restore(eng, state)
    grad = torch.zeros_like(eng.params)
    (learn or (lambda b: eng.learn_on_batch(b, grad_out=grad)))(batch)
    torch.cuda.synchronize()
    out = {n: getattr(eng, n).cpu().numpy().copy() for n in OUTPUTS + ("params",)}
    out["grad_out"] = grad.cpu().numpy()
    out["mirror"] = _bits(eng.region("wsplit")).copy()
    eng.rebuild_mirror()
    out["fresh_mirror"] = _bits(eng.region("wsplit")).copy()
    return out


def _hold_to_the_restatement(eng, real, p0, plain, got, kinds, what):
    mask = hw.decay_mask(eng.infos, eng.n_param_floats, kinds)
    restated = hw.decay32(plain["params"], p0, LR, WD)
    for info in eng.infos:  # the restatement alone: it moves most of every decayed tensor
        if (kinds >> info.kind) & 1:
            sl = slice(info.offset, info.offset + info.size)
            moved = np.count_nonzero((_bits(restated[sl]) != _bits(plain["params"][sl])) & real[sl])
            assert moved > 0.5 * real[sl].sum() > 0, f"{what} {info.name.decode()}: the restatement differs from p1 on {moved} of {real[sl].sum()} real elements"
    want = np.where(mask, restated, plain["params"])
    bad = np.flatnonzero(_bits(got["params"]) != _bits(want))
    if bad.size:
        i = int(bad[0])
        name = next(t.name.decode() for t in eng.infos if t.offset <= i < t.offset + t.size)
        raise AssertionError(f"{what}: {bad.size} parameter words differ from the restatement, first at {i} ({name}, decays: {bool(mask[i])}): p0 "
                             f"{p0[i]!r} p1 {plain['params'][i]!r} want {want[i]!r} got {got['params'][i]!r}")
    for n in OUTPUTS + ("grad_out",):
        assert np.array_equal(_bits(got[n]), _bits(plain[n])), f"{what}: {n} is not what it is without decay"
    # the mirror: a fresh split of the new parameters over everything the optimizer owns.  (The running statistics sit in one block behind
    # it, are written by the step's own kernel in fp32 only and are read by no MFMA stage: that part of the mirror is the plain step's)
    stats = [t.offset for t in eng.infos if t.kind >= 7]
    lo = min(stats) if stats else eng.n_param_floats
    assert lo % 8 == 0 and all(t.offset + t.size <= lo for t in eng.infos if t.kind < 7)
    assert np.array_equal(got["mirror"][:lo], got["fresh_mirror"][:lo]), f"{what}: the mirror is not a fresh split of the new parameters"
    assert np.array_equal(got["mirror"][lo:], plain["mirror"][lo:])
    assert not np.array_equal(got["mirror"], plain["mirror"])


@pytest.mark.parametrize("t0", [0, 9])
@pytest.mark.parametrize("name", list(SITES))
def test_decay_is_the_restatement_at_every_adam_site(name, t0):
    """Kernels only (the default mask), then all kinds: decayed tensors equal the restatement from (p1, p0) bit for bit, the other
    tensors p1 -- the running statistics of the BatchNorm site among them, under either mask; moments, count, losses, q_values, targets,
    priorities and the reduced gradient are the plain step's; the mirror is a fresh split of the new parameters.  Padding lanes and the
    dueling head's structural zeros hold +0 before and after."""
    from slimdqn import _hip

    eng, batch, real, state = _planted(name, t0)
    p0 = state["params"]
    plain = _step(eng, batch, state)
    assert plain["adam_count"].tolist() == [t0 + 1] and np.isfinite(plain["params"]).all() and np.abs(plain["grad_out"]).max() > 0
    assert np.count_nonzero(plain["params"][real] != p0[real]) > 0.5 * real.sum()
    kinds_here = {int(i.kind) for i in eng.infos}
    assert {1, 2, 3, 4} <= kinds_here and (SITES[name]["arch"] == "fc" or 0 in kinds_here) and (name != "cnn-bn" or {5, 6, 7, 8} <= kinds_here)
    for kinds in (_hip.DECAY_KINDS_KERNELS, _hip.DECAY_KINDS_ALL):
        got = _step(eng, _with_decay(batch, WD, kinds), state)
        _hold_to_the_restatement(eng, real, p0, plain, got, kinds, f"{name} t0={t0} kinds={kinds:#x}")
        assert not _bits(got["params"][~real]).any(), "a padding element or a structural zero left +0"
        for info in eng.infos:
            if info.kind >= 7:  # running statistics: written by the step, never by the optimizer
                sl = slice(info.offset, info.offset + info.size)
                assert np.array_equal(_bits(got["params"][sl]), _bits(plain["params"][sl])) and not np.array_equal(plain["params"][sl], p0[sl])
    assert not _bits(p0[~real]).any()


def test_fc_site_within_the_float64_bound():
    """The device's float32 AdamW step against float64 AdamW (adamw64, optax's form) on the gradient the update consumed.  The bound:
    tests.gpu_helpers.adam_bounds' bound on p1 -- the float32 Adam step against float64 Adam, its own final rounding included -- plus
    what the definition adds on a decayed element.  The float64 step subtracts lr wd p0 exactly; the device forms fl32(wd p0), then
    fl32(lr .): each within u = 2^-24 of its value (or one denormal spacing), together (2 u + u^2) lr wd |p0|; and it rounds p1 - t
    once more: half a spacing of p_new.  Nothing else differs: p1 enters the subtraction as the float32 the plain step stores."""
    from slimdqn import _hip
    from tests.gpu_helpers import adam_bounds

    t0 = 9
    eng, batch, real, state = _planted("fc", t0)
    got = _step(eng, _with_decay(batch, WD, _hip.DECAY_KINDS_KERNELS), state)
    p0, m0, v0, g = state["params"], state["adam_m"], state["adam_v"], got["grad_out"]
    mask = hw.decay_mask(eng.infos, eng.n_param_floats, _hip.DECAY_KINDS_KERNELS)
    (_, m, v, _), (ep, em, ev) = adam_bounds(p0, m0, v0, g, t0 + 1, LR, SITES["fc"]["eps"])
    want = hw.adamw64(p0, m0, v0, g, t0 + 1, LR, SITES["fc"]["eps"], np.where(mask, WD, 0.0))[0]
    bound = ep + np.where(mask, hw.decay_bound(p0, got["params"], LR, WD), 0.0)
    r = np.abs(got["params"].astype(np.float64) - want) / bound
    i = int(np.argmax(r))
    print(f"fc t0={t0}: worst |p - p64| / bound = {r[i]:.3f} at {i} (decays: {bool(mask[i])}); decayed elements: {int((mask & real).sum())}")
    assert r[i] <= 1.0, (i, got["params"][i], want[i], bound[i])
    assert np.all(np.abs(got["adam_m"] - m) <= em) and np.all(np.abs(got["adam_v"] - v) <= ev)
    # and the decay is far outside the bound: the plain float64 step is not within it on the decayed elements
    plain64 = hw.adamw64(p0, m0, v0, g, t0 + 1, LR, SITES["fc"]["eps"], 0.0)[0]
    far = np.abs(got["params"].astype(np.float64) - plain64) > bound
    assert far[mask & real].mean() > 0.99


@pytest.mark.parametrize("name", ["fc", "fc-clip", "cnn-bn"])
def test_the_flag_with_zero_decay_is_a_call_without_the_flag(name):
    from slimdqn import _hip

    eng, batch, real, state = _planted(name, 9)
    plain = _step(eng, batch, state)
    for kinds in (_hip.DECAY_KINDS_KERNELS, _hip.DECAY_KINDS_ALL, 0):
        got = _step(eng, _with_decay(batch, 0.0, kinds), state)
        for n in plain:
            assert np.array_equal(_bits(got[n]), _bits(plain[n])), (kinds, n)


def test_make_batch_builds_the_struct_only_when_the_decay_is_on():
    from slimdqn import _hip

    eng, batch, real, state = _planted("fc", 0)
    fields = dict(state=torch.zeros(32, 8, device="cuda"), next_state=torch.zeros(32, 8, device="cuda"), action=torch.zeros(32, dtype=torch.int32, device="cuda"),
                  reward=torch.zeros(32, device="cuda"), terminal=torch.zeros(32, dtype=torch.uint8, device="cuda"))
    disc = torch.ones(32, device="cuda")
    try:
        assert type(eng.make_batch(**fields)) is _hip.Batch and type(eng.make_batch(discount=disc, **fields)) is _hip.BatchDiscount
        eng.set_weight_decay(WD)
        assert (eng.weight_decay, eng.decay_kinds) == (WD, _hip.DECAY_KINDS_KERNELS)
        b = eng.make_batch(mirror_current=True, **fields)
        assert type(b) is _hip.BatchDecay and b.flags == _hip.BATCH_WEIGHT_DECAY | _hip.BATCH_MIRROR_CURRENT and b.discount is None
        assert (b.weight_decay, b.decay_kinds) == (np.float32(WD), 0x03)
        b = eng.make_batch(discount=disc, **fields)
        assert b.flags == _hip.BATCH_WEIGHT_DECAY | _hip.BATCH_DISCOUNT and b.discount == disc.data_ptr()
        eng.set_weight_decay(0.25, all_kinds=True)
        assert (eng.weight_decay, eng.decay_kinds) == (0.25, 0x7F)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                eng.set_weight_decay(bad)
        assert eng.weight_decay == 0.25
        # the engine's own batch runs the step of the hand-written struct
        eng.set_weight_decay(WD, all_kinds=True)
        _, _, st, nx, action, reward, terminal = batch._keep[:7]
        own = _step(eng, eng.make_batch(state=st, next_state=nx, action=action, reward=reward, terminal=terminal), state)
        hand = _step(eng, _with_decay(batch, WD, _hip.DECAY_KINDS_ALL), state)
        for n in own:
            assert np.array_equal(_bits(own[n]), _bits(hand[n])), n
    finally:
        eng.set_weight_decay(0.0)
    assert type(eng.make_batch(**fields)) is _hip.Batch and eng.decay_kinds == 0


def test_refusals_leave_everything_untouched():
    """Each ISDQN_ERR_ARG case, through the learn entry point and its _target and debug forms: nothing is launched, parameters, moments
    and count keep their bits.  The loss-only and the gradient-only entry points ignore the decay, a malformed one included."""
    from slimdqn import _hip

    eng, batch, real, state = _planted("fc", 9)
    _restore(eng, state)
    torch.cuda.synchronize()
    before = {n: _bits(getattr(eng, n)).copy() for n in STATE}
    target = eng.params.clone()
    grad = torch.zeros_like(eng.params)
    cases = [(-0.1, 0x03), (float("nan"), 0x03), (float("inf"), 0x03), (float("-inf"), 0x03), (WD, 0x80), (WD, 0x103), (WD, -1), (WD, 0), (0.0, 0x80)]
    for wd, kinds in cases:
        b = _with_decay(batch, wd, kinds)
        common = [_hip.ptr(eng.adam_m), _hip.ptr(eng.adam_v), _hip.ptr(eng.adam_count), ctypes.byref(b), _hip.ptr(eng.losses), _hip.ptr(eng.losses_accum),
                  _hip.ptr(eng.q_values), _hip.ptr(eng.targets), _hip.ptr(eng.priorities), _hip.ptr(eng.workspace), _hip.stream_ptr(eng.device)]
        cfg, p = ctypes.byref(eng.cfg), _hip.ptr(eng.params)
        assert eng.lib.isdqn_net_learn_on_batch(cfg, p, *common) == _hip.ERR_ARG, (wd, kinds)
        assert "weight_decay" in _hip.last_error() or "decay_kinds" in _hip.last_error()
        assert eng.lib.isdqn_net_learn_on_batch_debug(cfg, p, *common, _hip.ptr(grad)) == _hip.ERR_ARG, (wd, kinds)
        assert eng.lib.isdqn_net_learn_on_batch_target(cfg, p, _hip.ptr(target), *common) == _hip.ERR_ARG, (wd, kinds)
        torch.cuda.synchronize()
        for n in STATE:
            assert np.array_equal(_bits(getattr(eng, n)), before[n]), (wd, kinds, n)
    assert not grad.any()
    # loss only and gradient only: what they return without the flag, and nothing moves
    loss_plain = eng.loss_on_batch(batch).clone()
    loss_target_plain = eng.loss_on_batch_target(batch, target).clone()
    eng.grad_on_batch(batch, grad)
    grad_plain = grad.clone()
    for wd, kinds in [(WD, 0x7F), (float("nan"), -1)]:
        b = _with_decay(batch, wd, kinds)
        assert torch.equal(eng.loss_on_batch(b), loss_plain)
        assert torch.equal(eng.loss_on_batch_target(b, target), loss_target_plain)
        grad.zero_()
        eng.grad_on_batch(b, grad)
        assert torch.equal(grad, grad_plain)
        torch.cuda.synchronize()
        for n in STATE:
            assert np.array_equal(_bits(getattr(eng, n)), before[n]), (wd, kinds, n)


def test_the_noisy_learn_step_refuses_a_decay():
    from slimdqn import _hip, _optimizer
    from slimdqn._engine import QNetEngine

    A, B = 4, 8
    eng = QNetEngine((8,), A, 3, (20, 14), "fc", True, B, gamma_n=0.99, learning_rate=LR, adam_eps=1e-8, noisy=True)
    eng.init_params(3)
    with pytest.raises(ValueError) as e:
        eng.set_weight_decay(WD)
    assert str(e.value) == _optimizer.WEIGHT_DECAY_NOISY_REFUSED and eng.weight_decay == 0.0
    eng.set_weight_decay(0.0)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(a).cuda()
    batch = eng.make_batch(state=dev(rng.normal(size=(B, 8)).astype(np.float32)), next_state=dev(rng.normal(size=(B, 8)).astype(np.float32)),
                           action=dev(rng.integers(0, A, B).astype(np.int32)), reward=dev(rng.normal(size=B).astype(np.float32)),
                           terminal=dev((rng.random(B) < 0.3).astype(np.uint8)))
    eng.resample_noise()
    names = ("params", "sigma", "adam_m", "adam_v", "sigma_m", "sigma_v", "adam_count")
    before = {n: _bits(getattr(eng, n)).copy() for n in names}
    with pytest.raises(NotImplementedError):  # ISDQN_ERR_UNSUPPORTED
        eng._noisy_learn(_with_decay(batch, WD, _hip.DECAY_KINDS_KERNELS), None)
    with pytest.raises(RuntimeError):  # ISDQN_ERR_ARG: a malformed decay is malformed here too
        eng._noisy_learn(_with_decay(batch, -1.0, _hip.DECAY_KINDS_KERNELS), None)
    torch.cuda.synchronize()
    for n in names:
        assert np.array_equal(_bits(getattr(eng, n)), before[n]), n
    # the flag with zero decay is the step without the flag
    snap = {n: getattr(eng, n).clone() for n in names}
    eng._noisy_learn(batch, None)
    plain = {n: getattr(eng, n).clone() for n in names}
    for n in names:
        getattr(eng, n).copy_(snap[n])
    eng._noisy_learn(_with_decay(batch, 0.0, _hip.DECAY_KINDS_KERNELS), None)
    for n in names:
        assert torch.equal(getattr(eng, n), plain[n]), n
    assert not torch.equal(plain["params"], snap["params"])


# ---------------------------------------------------------------------------------------------------------------- agents
def _agents(cls, use_graph, **kw):
    from tests.test_gpu_reset import _agent_and_replay

    return _agent_and_replay(cls, use_graph, **kw)


def _agent_want(eng, p0, p1, lr, wd, kinds):
    return np.where(hw.decay_mask(eng.infos, eng.n_param_floats, kinds), hw.decay32(p1, p0, lr, wd), p1)


@pytest.mark.parametrize("agent_name", ["iSDQN", "DQN"])
def test_agents_with_weight_decay(agent_name):
    """One update_online_params of an agent built with weight_decay = 0.1 (the captured single step of the product path) leaves the
    parameters of the same agent without decay plus the restatement, the moments and the count of that agent; DQN's target parameters
    keep their bits."""
    import importlib

    from slimdqn import _hip

    cls = getattr(importlib.import_module(f"slimdqn.networks.{agent_name.lower()}"), agent_name)
    (plain, rb_p), (decayed, rb_d) = _agents(cls, True), _agents(cls, True, weight_decay=WD)
    assert (decayed._engine.weight_decay, decayed._engine.decay_kinds) == (WD, _hip.DECAY_KINDS_KERNELS) and plain._engine.weight_decay == 0.0
    p0 = plain._engine.params.cpu().numpy().copy()
    assert np.array_equal(_bits(decayed._engine.params), _bits(p0))
    targets = [a.target_params.tensor.clone() for a in (plain, decayed)] if agent_name == "DQN" else None
    for agent, rb in ((plain, rb_p), (decayed, rb_d)):
        agent.update_online_params(0, rb)
    torch.cuda.synchronize()
    assert decayed._graphed is not None and type(decayed._graphed.chained[0]) is _hip.BatchDecay and type(plain._graphed.chained[0]) is _hip.Batch
    eng = decayed._engine
    p1 = plain._engine.params.cpu().numpy()
    want = _agent_want(eng, p0, p1, decayed.learning_rate, WD, _hip.DECAY_KINDS_KERNELS)
    assert np.count_nonzero(_bits(want) != _bits(p1)) > 0.25 * p1.size
    assert np.array_equal(_bits(eng.params), _bits(want))
    for n in ("adam_m", "adam_v", "adam_count", "losses_accum"):
        assert torch.equal(getattr(eng, n), getattr(plain._engine, n)), n
    if targets is not None:
        for agent, t in zip((plain, decayed), targets):
            assert torch.equal(agent.target_params.tensor, t) and agent.target_params.tensor.data_ptr() != agent._engine.params.data_ptr()
    # a batch of another size: the engine the agent builds for it decays too
    decayed._engine_for(4)
    assert (decayed._engine.weight_decay, decayed._engine.decay_kinds, decayed._engine.batch_size) == (WD, _hip.DECAY_KINDS_KERNELS, 4)


def test_noisy_agents_refuse_weight_decay_before_building_anything():
    from slimdqn import _optimizer
    from slimdqn.networks.dqn import DQN

    with pytest.raises(ValueError) as e:
        DQN(0, (84, 84, 4), 5, [8, 12, 16, 24], False, "cnn", 2e-4, 0.99, 1, 1, 1000, noisy=True, weight_decay=WD)
    assert str(e.value) == _optimizer.WEIGHT_DECAY_NOISY_REFUSED


def test_two_captured_steps_with_decay_are_two_eager_steps():
    """A two-step GraphedUpdate (iSDQN.learn_steps(2)) of an agent with weight decay ends on the bits of two eager steps, and not on
    those of an agent without; another decay set on the engine drops the captured steps, which are captured again with it."""
    from slimdqn.networks.isdqn import iSDQN

    (eager, rb_e), (graphed, rb_g), (plain, rb_p) = _agents(iSDQN, False, weight_decay=WD, weight_decay_all=True), \
        _agents(iSDQN, True, weight_decay=WD, weight_decay_all=True), _agents(iSDQN, False)
    for agent, rb in ((eager, rb_e), (graphed, rb_g), (plain, rb_p)):
        agent.learn_steps(2, rb)
    assert eager._graphed is None and graphed._graphed is not None and graphed._graphed.S == 2
    for n in ("params", "adam_m", "adam_v", "adam_count", "losses_accum"):
        assert torch.equal(getattr(eager._engine, n), getattr(graphed._engine, n)), f"{n} differs between the eager and the captured steps"
    assert not torch.equal(eager._engine.params, plain._engine.params) and eager._engine.adam_count.item() == 2
    g = graphed._graphed
    for agent in (eager, graphed):
        agent._engine.set_weight_decay(0.05)
    assert g.graph is None  # dropped by the engine
    for agent, rb in ((eager, rb_e), (graphed, rb_g)):
        agent.learn_steps(2, rb)
    assert graphed._graphed is g and g.graph is not None and g.chained[0].weight_decay == np.float32(0.05) and g.chained[0].decay_kinds == 0x03
    for n in ("params", "adam_m", "adam_v", "adam_count", "losses_accum"):
        assert torch.equal(getattr(eager._engine, n), getattr(graphed._engine, n)), f"{n} differs after the decay changed"
