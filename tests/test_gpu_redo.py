"""ReDo on the device (Sokar et al. 2023; include/isdqn_hip.h, isdqn_net_redo) against the CPU reference of tests/helpers/redo.py:
float64 scores from the oracle's AnalysisNet, the recycle restated in numpy on the internal layout.

Shapes: cnn (8, 12, 16, 24) on (84, 84, 4) with 37 rows (12 channels pad to 16; 37 is ragged against the 8 row lanes of the
per-position sums), fc (40, 24) on (11,) with 50 rows; B = 32, A = 5, K = 3.  Every reference is computed once per case and shared.

Where device and reference can only agree away from a threshold, the test first asserts the distance on the float64 reference:
  * tau = 0: every neuron that is not dormant by construction has a_c >= 1e-3 * mean_l (the forward's 1e-3 bar);
  * tau = 0.1: every neuron has |a_c - tau * mean_l| >= 1e-2, ten times that bar (in normalised units: |a_c / mean_l - tau| >=
    10 * 1e-3 / mean_l).  Seeds and bias spreads of the cases were picked on the CPU so that this holds for all neurons.
"""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from tests.helpers import redo as hr

A, K, B = 5, 3, 32
CASES = {
    "cnn": dict(arch="cnn", obs=(84, 84, 4), feats=(8, 12, 16, 24), n_rows=37,
                chosen=[[0, 7], [0, 9, 11], [0, 8, 15], [0, 13, 23]]),   # channel 0, the last real one, one at index >= 8
    "fc": dict(arch="fc", obs=(11,), feats=(40, 24), n_rows=50, chosen=[[0, 17, 39], [0, 5, 23]]),
}


@functools.lru_cache(maxsize=None)
def _states(name):
    c = CASES[name]
    rng = np.random.default_rng(3)
    if c["arch"] == "fc":
        return rng.normal(size=(c["n_rows"],) + c["obs"]).astype(np.float32)
    return rng.integers(0, 256, (c["n_rows"],) + c["obs"], dtype=np.uint8)


def _hidden_modules(name, ln):
    c = CASES[name]
    n_conv = 0 if c["arch"] == "fc" else 3
    mods = [f"Conv_{i}" for i in range(n_conv)] + [f"Dense_{i}" for i in range(len(c["feats"]) - n_conv)]
    return [(m, f"LayerNorm_{i}" if ln else None) for i, m in enumerate(mods)]


LIFT_LN, LIFT_PLAIN = (3.0, 3.0), {"cnn": (1.0, 30.0), "fc": (0.0, 0.5)}  # (conv layers, Dense layers)


def _base_params(name, ln, seed, final_feature=(1 + K) * A, lift=(0.0, 0.0)):
    """perturbed_params; `lift` (conv layers, Dense layers) is added to the biases in front of every ReLU (the LayerNorm's with -ln).
    The synthetic states give a neuron nearly the same input on every row and at every position, so without a lift a good part of
    the neurons is silent everywhere: a LayerNorm output lies within +-sqrt(C - 1) and is lifted by 3; without a LayerNorm the
    cnn's Dense pre-activations are sums over ~2000 inputs with a spread of several units and are lifted by 30, the fc network's
    (11 and 40 inputs) by 0.5."""
    from tests.gpu_helpers import perturbed_params

    c = CASES[name]
    p = perturbed_params(seed, c["obs"], c["feats"], c["arch"], final_feature, ln)
    for mod, ln_mod in _hidden_modules(name, ln):
        tensor = p[ln_mod if ln else mod]
        tensor["bias"] = (tensor["bias"] + lift[0 if mod.startswith("Conv") else 1]).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def _constructed(name, ln, final_feature=(1 + K) * A):
    """Test 1's network: the chosen neurons' pre-ReLU values are far negative on every row (bias -1e3: the layer's own without a
    LayerNorm, the LayerNorm's with one), everything else alive.  Returns (params, float64 scores, chosen masks)."""
    c = CASES[name]
    p = _base_params(name, ln, seed=11, final_feature=final_feature, lift=LIFT_LN if ln else LIFT_PLAIN[name])
    for (mod, ln_mod), chosen in zip(_hidden_modules(name, ln), c["chosen"]):
        p[ln_mod if ln else mod]["bias"][chosen] = -1e3
    scores = hr.reference_scores(p, _states(name), c["feats"], c["arch"], ln)
    masks = [np.isin(np.arange(w), ch) for w, ch in zip(c["feats"], c["chosen"])]
    return p, scores, masks


@functools.lru_cache(maxsize=None)
def _alive(name):
    """Test 4's network (with LayerNorm): nothing dormant."""
    c = CASES[name]
    p = _base_params(name, True, seed=11, lift=LIFT_LN)
    return p, hr.reference_scores(p, _states(name), c["feats"], c["arch"], True)


TAU_CASES = {"cnn": dict(seed=13, spread=1.0), "fc": dict(seed=15, spread=1.5)}


@functools.lru_cache(maxsize=None)
def _spread(name):
    """Test 2's network (with LayerNorm): LayerNorm biases spread with a normal of the case's width, so that some neurons fall below
    tau = 0.1 of their layer's mean."""
    c, t = CASES[name], TAU_CASES[name]
    p = _base_params(name, True, seed=t["seed"])
    rng = np.random.default_rng(t["seed"] + 100)
    for _, ln_mod in _hidden_modules(name, True):
        p[ln_mod]["bias"] = rng.normal(0.0, t["spread"], p[ln_mod]["bias"].shape).astype(np.float32)
    return p, hr.reference_scores(p, _states(name), c["feats"], c["arch"], True)


def _assert_alive_away_from_zero(scores, masks):
    for a, m in zip(scores, masks):
        assert (a[m] == 0).all() and (a[~m] >= 1e-3 * a.mean()).all(), (a, m)


# ---------------------------------------------------------------------------------------------------------------- device side
def _engine(name, ln, precision="bf16x3", n_heads=1 + K, **kw):
    from slimdqn._engine import QNetEngine

    c = CASES[name]
    return QNetEngine(c["obs"], A, n_heads, c["feats"], c["arch"], ln, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, precision=precision, **kw)


def _inputs(name):
    c, states = CASES[name], _states(name)
    if c["arch"] == "fc":
        return dict(obs=torch.from_numpy(states).cuda(), n_rows=c["n_rows"])
    h, w, s = c["obs"]
    planes = torch.from_numpy(np.ascontiguousarray(np.moveaxis(states, -1, 1)).reshape(c["n_rows"] * s, h * w)).cuda()
    return dict(frames=planes, frame_stride=h * w, frame_ids=torch.arange(c["n_rows"] * s, dtype=torch.int32, device="cuda"), n_rows=c["n_rows"])


def _load(eng, params, seed=5):
    """Parameters in, seeded non-zero noise in both moments (padding lanes included).  Returns the three host copies."""
    eng.import_flax(params)
    rng = np.random.default_rng(seed)
    m = rng.normal(0, 1, eng.n_param_floats).astype(np.float32)
    v = rng.uniform(0.5, 2.0, eng.n_param_floats).astype(np.float32)
    eng.adam_m.copy_(torch.from_numpy(m))
    eng.adam_v.copy_(torch.from_numpy(v))
    return eng.params.cpu().numpy(), m, v


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)


def _assert_buffers(eng, expected):
    for name, want in zip(("params", "adam_m", "adam_v"), expected):
        got = getattr(eng, name)
        assert np.array_equal(_bits(got), _bits(want)), f"{name}: {(_bits(got) != _bits(want)).sum()} words differ from the CPU reference"


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("name", ["cnn", "fc"])
def test_constructed_dormancy_is_recycled_exactly(name, ln, precision):
    """1: tau = 0.  The mask is the chosen set, the counts match, and params / adam_m / adam_v equal the CPU reference bit for bit over
    the whole buffers (padding lanes and every untouched tensor included)."""
    params, scores, masks = _constructed(name, ln)
    _assert_alive_away_from_zero(scores, masks)
    eng = _engine(name, ln, precision)
    p0, m0, v0 = _load(eng, params)
    fresh = eng.fresh_params(12345)
    dev_scores, dev_mask, n_recycled = eng.redo(tau=0.0, fresh=fresh, **_inputs(name))
    for l, (mask, got) in enumerate(zip(masks, dev_mask)):
        assert np.array_equal(got.cpu().numpy(), mask.astype(np.int32)), f"layer {l}"
        assert (dev_scores[l].cpu().numpy()[mask] == 0).all()
    assert n_recycled.cpu().tolist() == [len(ch) for ch in CASES[name]["chosen"]]
    expected = hr.recycle(eng, p0, m0, v0, fresh.cpu().numpy(), masks)
    assert not np.array_equal(expected[0], p0)
    _assert_buffers(eng, expected)


@pytest.mark.parametrize("name", ["cnn", "fc"])
def test_tau_above_zero_matches_the_reference_away_from_the_threshold(name):
    """2: tau = 0.1 on LayerNorm networks whose LayerNorm biases are spread."""
    tau = 0.1
    params, scores = _spread(name)
    for a, d in zip(scores, hr.threshold_margins(scores, tau)):
        assert (d >= 10 * 1e-3 / a.mean()).all(), (a / a.mean(), d)
    masks = hr.dormant_masks(scores, tau)
    assert sum(int(m.sum()) for m in masks) > 0 and all(not m.all() for m in masks)
    eng = _engine(name, True)
    p0, m0, v0 = _load(eng, params)
    fresh = eng.fresh_params(999)
    dev_scores, dev_mask, n_recycled = eng.redo(tau=tau, fresh=fresh, **_inputs(name))
    for l, (a, mask) in enumerate(zip(scores, masks)):
        err = np.abs(dev_scores[l].cpu().numpy().astype(np.float64) - a).max()
        print(f"{name} layer {l}: max |score - reference| = {err:.3e}, dormant {int(mask.sum())} of {mask.size}")
        assert err <= 1e-3
        assert np.array_equal(dev_mask[l].cpu().numpy(), mask.astype(np.int32)), f"layer {l}"
    assert n_recycled.cpu().tolist() == [int(m.sum()) for m in masks]
    _assert_buffers(eng, hr.recycle(eng, p0, m0, v0, fresh.cpu().numpy(), masks))


@pytest.mark.parametrize("name", ["cnn", "fc"])
def test_function_is_preserved_without_layer_norm(name):
    """3: tau = 0, no LayerNorm: the forward on the scoring rows is bit-identical before and after, although neurons were recycled in
    every layer and the parameters differ."""
    params, scores, masks = _constructed(name, False)
    _assert_alive_away_from_zero(scores, masks)
    eng = _engine(name, False)
    p0, _, _ = _load(eng, params)
    q0 = eng.forward(**_inputs(name)).clone()
    _, _, n_recycled = eng.redo(tau=0.0, fresh=eng.fresh_params(4242), **_inputs(name))
    q1 = eng.forward(**_inputs(name))
    assert all(n > 0 for n in n_recycled.cpu().tolist())
    assert not np.array_equal(_bits(eng.params), _bits(p0))
    assert np.array_equal(_bits(q0), _bits(q1)) and np.isfinite(q0.cpu().numpy()).all() and float(q0.abs().max()) > 0


@pytest.mark.parametrize("name", ["cnn", "fc"])
def test_nothing_dormant_changes_nothing(name):
    """4: tau = 0 and every neuron alive on the reference: the three buffers keep their bits, the counts are 0."""
    params, scores = _alive(name)
    _assert_alive_away_from_zero(scores, [np.zeros(a.size, bool) for a in scores])
    eng = _engine(name, True)
    before = _load(eng, params)
    _, mask, n_recycled = eng.redo(tau=0.0, fresh=eng.fresh_params(1), **_inputs(name))
    assert n_recycled.cpu().tolist() == [0] * len(scores) and all(int(m.sum()) == 0 for m in mask)
    _assert_buffers(eng, before)


@pytest.mark.parametrize("name", ["cnn", "fc"])
def test_guard_bands_around_every_buffer_stay_intact(name):
    """5: the C ABI directly, params / adam_m / adam_v (and the three outputs) inside larger tensors with 4096 sentinel floats on each
    side."""
    from slimdqn import _hip

    G, SENT = 4096, -7.25
    params, _, masks = _constructed(name, True)
    eng = _engine(name, True)
    src = _load(eng, params)
    n = eng.n_param_floats
    widths = eng.redo_layout()

    def guarded(size, dtype=torch.float32, fill=None):
        big = torch.full((size + 2 * G,), SENT, dtype=torch.float32, device="cuda").view(dtype) if dtype != torch.float32 else \
            torch.full((size + 2 * G,), SENT, dtype=torch.float32, device="cuda")
        if fill is not None:
            big[G : G + size].copy_(torch.from_numpy(fill))
        return big

    bufs = [guarded(n, fill=a) for a in src]
    scores, mask, count = guarded(sum(widths)), guarded(sum(widths), torch.int32), guarded(len(widths), torch.int32)
    fresh = eng.fresh_params(77)
    inp = _inputs(name)
    at = lambda t: t.data_ptr() + 4 * G
    torch.cuda.synchronize()
    _hip.check(eng.lib.isdqn_net_redo(
        ctypes.byref(eng.cfg), at(bufs[0]), at(bufs[1]), at(bufs[2]), _hip.ptr(fresh), _hip.ptr(inp.get("frames")), int(inp.get("frame_stride", 0)),
        _hip.ptr(inp.get("frame_ids")), _hip.ptr(inp.get("obs")), inp["n_rows"], 0.0, at(scores), at(mask), at(count), _hip.ptr(eng.workspace),
        _hip.stream_ptr(eng.device)), "isdqn_net_redo")
    torch.cuda.synchronize()
    sentinel = _bits(np.full(G, SENT, np.float32))
    for t, size in [(b, n) for b in bufs] + [(scores, sum(widths)), (mask, sum(widths)), (count, len(widths))]:
        words = _bits(t.view(torch.float32))
        assert np.array_equal(words[:G], sentinel) and np.array_equal(words[G + size :], sentinel)
    assert count[G : G + len(widths)].cpu().tolist() == [int(m.sum()) for m in masks]
    expected = hr.recycle(eng, *src, fresh.cpu().numpy(), masks)
    for b, want in zip(bufs, expected):
        assert np.array_equal(_bits(b[G : G + n]), _bits(want))
    # the engine's own buffers were not the call's
    for own, was in zip((eng.params, eng.adam_m, eng.adam_v), src):
        assert np.array_equal(_bits(own), _bits(was))
    # moments may be left out together
    p2 = guarded(n, fill=src[0])
    _hip.check(eng.lib.isdqn_net_redo(
        ctypes.byref(eng.cfg), at(p2), None, None, _hip.ptr(fresh), _hip.ptr(inp.get("frames")), int(inp.get("frame_stride", 0)),
        _hip.ptr(inp.get("frame_ids")), _hip.ptr(inp.get("obs")), inp["n_rows"], 0.0, at(scores), at(mask), at(count), _hip.ptr(eng.workspace),
        _hip.stream_ptr(eng.device)), "isdqn_net_redo")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(p2[G : G + n]), _bits(expected[0]))


@pytest.mark.parametrize("heads", [dict(n_bins=5, min_value=-10.0, max_value=10.0, sigma=0.75), dict(n_quantiles=4, huber_delta=1.0), dict(n_heads=1)])
def test_outgoing_zeroing_covers_every_head_output(heads):
    """6: histogram heads (5 bins), quantile heads (4 quantiles) and the one-head DQN form: column c of the last Dense is zeroed in
    every head, action, bin or quantile; a DQN's target parameters keep their bits."""
    name = "fc"
    kw = dict(heads)
    n_heads = kw.pop("n_heads", 1 + K)
    width = n_heads * A * max(kw.get("n_bins", 0), kw.get("n_quantiles", 0), 1)
    params, scores, masks = _constructed(name, True, final_feature=width)
    _assert_alive_away_from_zero(scores, masks)
    eng = _engine(name, True, n_heads=n_heads, **kw)
    p0, m0, v0 = _load(eng, params)
    target = eng.params.clone()
    target_bits = _bits(target)
    fresh = eng.fresh_params(31)
    _, dev_mask, _ = eng.redo(tau=0.0, fresh=fresh, **_inputs(name))
    assert all(np.array_equal(g.cpu().numpy(), m.astype(np.int32)) for g, m in zip(dev_mask, masks))
    last = eng.export_flax()[f"Dense_{len(CASES[name]['feats'])}"]["kernel"]
    assert last.shape == (CASES[name]["feats"][-1], width)
    dormant = masks[-1]
    assert (last[dormant] == 0).all() and (last[~dormant] != 0).all()
    assert np.array_equal(last[~dormant], params[f"Dense_{len(CASES[name]['feats'])}"]["kernel"][~dormant])
    _assert_buffers(eng, hr.recycle(eng, p0, m0, v0, fresh.cpu().numpy(), masks))
    assert np.array_equal(_bits(target), target_bits)


def test_dqn_agent_recycles_online_parameters_only():
    """6, agent level: DQN.recycle_dormant on a device replay leaves target_params alone and counts per hidden layer."""
    from slimdqn.networks.dqn import DQN

    agent, rb = _agent_and_replay(DQN, use_graph=True)
    agent.learn_steps(2, rb)
    target = _bits(agent.target_params.tensor)
    online = _bits(agent.params.tensor)
    counts = agent.recycle_dormant(rb, 2.0)  # (tau = 2: everything at or below twice the layer mean, so that something is recycled)
    assert len(counts) == 4 and all(isinstance(c, int) for c in counts) and sum(counts) > 0
    assert np.array_equal(_bits(agent.target_params.tensor), target) and not np.array_equal(_bits(agent.params.tensor), online)


@pytest.mark.parametrize("name", ["cnn", "fc"])
def test_mirror_is_current_after_redo_under_trust_mirror(name):
    """7: with trust_mirror = True a forward after redo skips the rebuild; it must be bit-identical to the forward of a second engine
    that imports export_flax() of the first."""
    params, _, _ = _constructed(name, True)
    eng = _engine(name, True)
    eng.trust_mirror = True
    _load(eng, params)
    eng.forward(**_inputs(name))
    eng.redo(tau=0.0, fresh=eng.fresh_params(8), **_inputs(name))
    assert eng._mirror_is_current(None)
    heads = torch.zeros(CASES[name]["n_rows"], dtype=torch.int32, device="cuda")
    inp = {k: v for k, v in _inputs(name).items() if k != "n_rows"}
    acts = eng.best_actions(idx_networks=heads, **inp)  # (takes the mirror as it is when the bookkeeping says current)
    rows = CASES[name]["n_rows"] * 24  # (the rows of this forward: (1 + K) * A = 20 values padded to 24)
    q = eng.region("q")[:rows].clone()
    other = _engine(name, True)
    other.import_flax(eng.export_flax())
    acts2 = other.best_actions(idx_networks=heads, **inp)
    assert np.array_equal(_bits(q), _bits(other.region("q")[:rows])) and torch.equal(acts, acts2) and float(q.abs().max()) > 0
    assert np.array_equal(_bits(eng.forward(**_inputs(name))), _bits(other.forward(**_inputs(name))))


def _agent_and_replay(cls, use_graph, n_fill=80, **kw):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    Bs, C = 8, 128
    args = (0, (84, 84, 4), A) + ((K,) if cls.__name__ == "iSDQN" else ()) + ([8, 12, 16, 24], False) + ((False,) if cls.__name__ == "iSDQN" else ())
    agent = cls(*args, "cnn", 2e-4, 0.99, 1, 1, 1000, adam_eps=1.5e-4, batch_size=Bs, use_graph=use_graph, **kw)
    rb = ReplayBuffer(UniformSamplingDistribution(5), Bs, C, update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(0)
    for _ in range(n_fill):
        obs = rng.integers(0, 256, (84, 84), dtype=np.uint8)
        term = bool(rng.random() < 0.08)
        rb.add(TransitionElement(obs, int(rng.integers(0, A)), float(rng.choice([-1.0, 0.0, 1.0])), term, term))
    return agent, rb


def test_captured_update_stays_valid_across_a_recycle():
    """8: iS-DQN, learn_steps(3), recycle_dormant, learn_steps(3) through the captured graph ends with the parameter bits of the same
    sequence run eagerly, and nothing is captured again."""
    from slimdqn.networks.isdqn import iSDQN

    (eager, rb_e), (graphed, rb_g) = _agent_and_replay(iSDQN, False), _agent_and_replay(iSDQN, True)
    assert torch.equal(eager._engine.params, graphed._engine.params)
    for agent in (eager, graphed):
        agent.trust_mirror = True  # as the trainer declares it: the replay behind the recycle takes the mirror redo left
    counts = []
    for agent, rb in ((eager, rb_e), (graphed, rb_g)):
        agent.learn_steps(3, rb)
        captures = getattr(agent, "_captures", 0)
        counts.append(agent.recycle_dormant(rb, 2.0))
        agent.learn_steps(3, rb)
        assert getattr(agent, "_captures", 0) == captures
    assert counts[0] == counts[1] and sum(counts[0]) > 0
    assert eager._graphed is None and graphed._graphed is not None and graphed._captures == 1
    for name in ("params", "adam_m", "adam_v", "adam_count", "losses_accum"):
        x, y = getattr(eager._engine, name), getattr(graphed._engine, name)
        assert torch.equal(x, y), f"{name} differs between the eager and the captured sequence"


@pytest.mark.parametrize("name", ["cnn", "fc"])
def test_scores_are_run_to_run_identical(name):
    """9: two calls from identical state give identical score bits (and masks)."""
    params, _ = _spread(name)
    out = []
    for _ in range(2):
        eng = _engine(name, True)
        _load(eng, params)
        scores, mask, _ = eng.redo(tau=0.1, fresh=eng.fresh_params(2), **_inputs(name))
        out.append((_bits(torch.cat(scores)), _bits(torch.cat(mask).view(torch.float32)), _bits(eng.params)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_refusals_with_their_codes():
    """10: every refusal of the header on live device pointers, through the engine's exception mapping and as raw codes."""
    from slimdqn import _hip
    from slimdqn._engine import QNetEngine

    name = "fc"
    eng = _engine(name, True)
    eng.init_params(0)
    fresh = eng.fresh_params(1)
    inp = _inputs(name)
    before = _bits(eng.params)
    scores = torch.zeros(64, device="cuda")
    mask = torch.zeros(64, dtype=torch.int32, device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(cfg=None, params=eng.params, m=eng.adam_m, v=eng.adam_v, fresh=fresh, obs=inp["obs"], n_rows=50, tau=0.1, scores=scores, mask=mask,
             count=count, ws=eng.workspace):
        return eng.lib.isdqn_net_redo(ctypes.byref(cfg or eng.cfg), _hip.ptr(params), _hip.ptr(m), _hip.ptr(v), _hip.ptr(fresh), None, 0, None,
                                      _hip.ptr(obs), n_rows, tau, _hip.ptr(scores), _hip.ptr(mask), _hip.ptr(count), _hip.ptr(ws), _hip.stream_ptr(eng.device))

    for null in ("params", "fresh", "scores", "mask", "count", "ws"):
        assert call(**{null: None}) == _hip.ERR_ARG, null
    assert call(m=None) == _hip.ERR_ARG and call(v=None) == _hip.ERR_ARG
    for tau in (-1e-3, float("nan"), float("inf")):
        assert call(tau=tau) == _hip.ERR_ARG
    for n_rows in (0, 2 * B + 1):
        assert call(n_rows=n_rows) == _hip.ERR_SHAPE
    with pytest.raises(AssertionError):
        eng.redo(tau=0.1, fresh=fresh, obs=inp["obs"], n_rows=2 * B + 1)
    with pytest.raises(RuntimeError):
        eng.redo(tau=-0.5, fresh=fresh, **inp)
    for kw, word in ((dict(arch="impala"), "impala"), (dict(batch_norm=True), "BatchNorm")):
        other = QNetEngine((84, 84, 4), A, 1 + K, (8, 16, 8, 24), kw.get("arch", "cnn"), True, 4, batch_norm=kw.get("batch_norm", False))
        other.init_params(0)
        f2 = other.fresh_params(1)
        states = torch.zeros(4 * 84 * 84, dtype=torch.uint8, device="cuda").reshape(4, 84 * 84)
        with pytest.raises(NotImplementedError, match=word):
            other.redo(frames=states, frame_stride=84 * 84, frame_ids=torch.arange(4, dtype=torch.int32, device="cuda"), n_rows=1, tau=0.1, fresh=f2)
        with pytest.raises(NotImplementedError, match=word):
            other.redo_layout()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(eng.params), before)  # no refused call wrote anything
    assert call() == _hip.OK


@pytest.mark.parametrize("analysis", [True, False])
def test_redo_flag_of_the_trainer(tmp_path, analysis):
    """11: -redo 16 -redot 0.1 -tuf 16 on test_analysis_flag_of_the_trainer's run, with and without -a: one per-layer list of recycle
    counts for every target update at a multiple of 16."""
    from experiments.atari.isdqn import run

    name = "redo_Synthetic"
    argv = ["-en", name, "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "300", "-bs", "8", "-horizon", "40", "-at", "cnn",
            "-ne", "1", "-ntspe", "80", "-utd", "4", "-nis", "30", "-ed", "100", "-nbi", "2", "-ln", "-tuf", "16", "-env", "synthetic",
            "-redo", "16", "-redot", "0.1"] + (["-a"] if analysis else [])
    run(argv, root=str(tmp_path))
    out = tmp_path / "atari" / "exp_output" / name / "isdqn"
    logs = json.load(open(out / "analysis" / "1.json"))
    assert set(logs) == ({"srank", "dead_neurons", "recycled_neurons"} if analysis else {"recycled_neurons"})
    n_steps = sum(sum(epoch) for epoch in json.load(open(out / "episode_returns_and_lengths" / "1.json"))["episode_lengths"])
    updates = [s for s in range(31, n_steps + 1) if s % 16 == 0]
    assert len(updates) >= 2 and len(logs["recycled_neurons"]) == len(updates)
    assert all(len(r) == 4 and all(isinstance(c, int) and 0 <= c <= w for c, w in zip(r, (8, 8, 8, 16))) for r in logs["recycled_neurons"])
    if analysis:
        assert len(logs["srank"]) == len(logs["dead_neurons"]) == len(updates)
    stored = json.load(open(tmp_path / "atari" / "exp_output" / name / "parameters.json"))
    assert not any("redo" in k for section in stored.values() for k in section)
