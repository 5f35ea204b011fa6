"""Normalize-and-Project on the device (include/isdqn_hip.h, isdqn_net_project_*) against the float64 restatement of
tests/helpers/nap.py, in three tiers with derived bounds, and through the engine and the agents.

Shapes (tests/helpers/prune.py): fc on 8 observations with features [20, 14] -- tensors smaller than a workgroup, Dense_0's rows and
Dense_1's input lanes padded -- and [256, 256] -- Dense_1 spans 17 chunks, so the sum across chunks and the same scale in every workgroup
are exercised; cnn 84x84x4 with features [8, 8, 8, 16] and LayerNorm -- Conv_0's [out][plane][ky][kx] form, kernels whose offsets are no
multiple of 32, so that chunks are shared with neighbours.  The parameters are written by the test: every float of the buffer that is no
real projected element holds a sentinel that must survive.

  tier 1  norms[i] against the fsum reference: relative difference <= N_i * 2^-53.  Any order of N float64 additions of exact
          non-negative terms is within (N - 1) * 2^-53 of the exact sum, a square root halves a relative error and adds its own 2^-53, as
          does the reference's: (N / 2 + 2) * 2^-53 <= N * 2^-53 for the N >= 160 here.  The float32-accumulation variant is far outside.
  tier 2  scales[i] bitwise equal to float32(rho_i / norms_dev[i]): IEEE float64 division, one rounding.
  tier 3  master bitwise equal to float32(w) * scales_dev[i] on real elements, every other float, both moments and the count unchanged,
          mirror bitwise equal to a rebuild from the expected master in a second workspace.
tests/test_nap_host.py shows that the wrong variants of the oracle (padding counted, last Dense included, biases scaled, norm per row,
float32 sum) each move a scale by 16 ulps or more on these inputs: a device result that passes tier 2 and tier 3 is none of them."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from slimdqn import _hip
from tests.helpers import nap
from tests.helpers import prune as hp

pytestmark = pytest.mark.gpu

CONFIGS = {"fc-20-14": hp.FC_SMALL, "fc-256-256": hp.FC_WIDE, "cnn": hp.CNN}
ONE = np.float32(1.0)
AFTER = 2.0 ** -22  # |norm / rho - 1| after a projection: (1 + 2^-24)^2 - 1 < 2^-23 + 2^-48 for the rounding of s and of each product;
#                     the factor two covers products that round into the denormal range


def _bits(t):
    return hp.bits(t.detach().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _engine(name):
    eng = hp.make_engine(CONFIGS[name], gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4)
    assert eng.project_target is None
    eng.set_weight_projection(nap.case_targets(eng))
    assert [i[3] for i in eng.project_infos] == hp.real_counts(eng)
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


def _load(eng, params: np.ndarray, rho):
    """``params`` and the target norms into the engine's buffers, recognisable moments and outputs, a current mirror."""
    eng.params.copy_(torch.from_numpy(params))
    eng.project_target.copy_(torch.tensor(rho, dtype=torch.float64))
    eng.project_norms_out.fill_(-7.0)
    eng.project_scales.fill_(-7.0)
    eng.adam_m.fill_(3.25)
    eng.adam_v.fill_(1.5)
    eng.adam_count.fill_(7)
    eng.rebuild_mirror()


def _tier1(got, want, n_real, what):
    for i, (g, w, n) in enumerate(zip(got, want, n_real)):
        if math.isnan(w) or math.isinf(w) or w == 0.0:
            assert (math.isnan(g) if math.isnan(w) else g == w), f"{what}: norm {i} is {g}, expected {w}"
            continue
        err = abs(g / w - 1.0)
        print(f"{what}: tensor {i}: N = {n}, norm {g!r}, fsum {w!r}, relative difference {err:.3e}, bound {n * 2.0 ** -53:.3e}")
        assert err <= n * 2.0 ** -53, f"{what}: norm {i} is {err:.3e} off, above N * 2^-53 = {n * 2.0 ** -53:.3e}"


def _apply_and_check(eng, p0: np.ndarray, rho, what):
    """project_weights on loaded buffers through the three tiers; returns (norms, scales, expected master)."""
    eng.project_weights()
    torch.cuda.synchronize()
    k = len(eng.project_infos)
    n_dev = [float(x) for x in eng.project_norms_out.cpu().numpy()[:k]]
    s_dev = eng.project_scales.cpu().numpy()[:k].copy()
    _tier1(n_dev, nap.norms(eng, p0), hp.real_counts(eng), what)
    for i in range(k):  # tier 2
        want = nap.scale_of(rho[i], n_dev[i])
        assert hp.bits(s_dev[i : i + 1])[0] == hp.bits(np.array([want], np.float32))[0], f"{what}: scale {i} is {s_dev[i]!r}, expected {want!r}"
    want = nap.scaled(eng, p0, s_dev)  # tier 3
    got = _bits(eng.params)
    assert np.array_equal(got, hp.bits(want)), f"{what}: {(got != hp.bits(want)).sum()} parameters differ"
    keep = nap.not_projected(eng)
    assert np.array_equal(got[keep], hp.bits(p0)[keep])  # (implied by the line above; said once more for the sentinels)
    ref, mir = _mirror_of(eng, want), _mirror(eng)
    assert torch.equal(mir, ref), f"{what}: {(mir != ref).sum().item()} mirror words differ from a rebuild on the expected parameters"
    assert bool((eng.adam_m == 3.25).all()) and bool((eng.adam_v == 1.5).all()) and eng.adam_count.item() == 7
    return n_dev, s_dev, want


# ---------------------------------------------------------------------------------------------------------------- the three tiers
@pytest.mark.parametrize("name", list(CONFIGS))
def test_random_weights_through_the_three_tiers_and_a_second_apply(name):
    eng = _engine(name)
    rho = nap.case_targets(eng)
    p0 = nap.case_params(eng, "normal")
    _load(eng, p0, rho)
    measured = eng.project_norms()
    assert np.array_equal(_bits(eng.params), hp.bits(p0))  # (measuring writes no parameter)
    n_dev, s_dev, p1 = _apply_and_check(eng, p0, rho, f"{name}/normal")
    assert measured == n_dev  # isdqn_net_project_norms: the bits the apply reports for the same buffer
    assert all(s != ONE for s in s_dev) and not np.array_equal(hp.bits(p1), hp.bits(p0))
    # the float32-accumulation variant is far outside tier 1
    _, n32, _ = nap.project(eng, p0, rho, "fp32")
    assert any(abs(a / b - 1.0) > 64 * n * 2.0 ** -53 for a, b, n in zip(n32, n_dev, hp.real_counts(eng)))
    # the projected tensors have their target norms
    for i, (n, r) in enumerate(zip(nap.norms(eng, p1), rho)):
        print(f"{name}: tensor {i}: |norm / rho - 1| = {abs(n / r - 1.0):.3e}, bound {AFTER:.3e}")
        assert abs(n / r - 1.0) < AFTER
    # a second apply on the result: every scale within one float32 ulp of 1
    _, s2, _ = _apply_and_check(eng, p1, rho, f"{name}/second apply")
    assert all(nap.ulps(s, ONE) <= 1 for s in s2), s2
    # another buffer of the layout: the master alone, the engine's own parameters and mirror untouched
    copy = torch.from_numpy(p0).to(eng.device)
    before_p, before_m = eng.params.clone(), _mirror(eng).clone()
    eng.project_weights(params=copy)
    s3 = eng.project_scales.cpu().numpy()[: len(rho)]
    assert np.array_equal(hp.bits(s3), hp.bits(s_dev)) and np.array_equal(_bits(copy), hp.bits(p1))
    assert torch.equal(eng.params, before_p) and torch.equal(_mirror(eng), before_m)


@pytest.mark.parametrize("case", ["zero", "nonfinite", "denormal"])
@pytest.mark.parametrize("name", ["fc-20-14", "cnn"])
def test_special_tensors(name, case):
    """An all-zero tensor: untouched, scale 1, norm 0.  A tensor holding one inf and one holding a NaN: untouched, scale 1.  Denormals:
    counted and scaled without a flush."""
    eng = _engine(name)
    rho = nap.case_targets(eng)
    p0 = nap.case_params(eng, case, seed=2)
    _load(eng, p0, rho)
    n_dev, s_dev, p1 = _apply_and_check(eng, p0, rho, f"{name}/{case}")
    first = hp.real_index(eng, nap.projected(eng)[0])
    if case == "zero":
        assert n_dev[0] == 0.0 and s_dev[0] == ONE and np.array_equal(hp.bits(p1[first]), hp.bits(p0[first])) and all(s != ONE for s in s_dev[1:])
    elif case == "nonfinite":
        assert n_dev[0] == math.inf and math.isnan(n_dev[1]) and s_dev[0] == ONE and s_dev[1] == ONE and all(s != ONE for s in s_dev[2:])
        second = hp.real_index(eng, nap.projected(eng)[1])
        assert np.array_equal(hp.bits(p1[first]), hp.bits(p0[first])) and np.array_equal(hp.bits(p1[second]), hp.bits(p0[second]))
    else:
        tiny = first[np.abs(p0[first]) < np.float32(1e-38)]
        assert tiny.size > 0 and (p1[tiny] != 0).all()
        for n, r in zip(nap.norms(eng, p1), rho):
            assert abs(n / r - 1.0) < AFTER


@pytest.mark.parametrize("bad", [0.0, -1.0, math.inf, math.nan])
def test_a_target_norm_that_is_not_positive_and_finite_leaves_its_tensor_alone(bad):
    eng = _engine("fc-256-256")
    rho = nap.case_targets(eng)
    p0 = nap.case_params(eng, "normal", seed=4)
    for which in range(len(rho)):
        r = list(rho)
        r[which] = bad
        _load(eng, p0, r)
        _, s_dev, p1 = _apply_and_check(eng, p0, r, f"rho[{which}] = {bad}")
        idx = hp.real_index(eng, nap.projected(eng)[which])
        assert s_dev[which] == ONE and np.array_equal(hp.bits(p1[idx]), hp.bits(p0[idx]))
        assert all(s != ONE for i, s in enumerate(s_dev) if i != which)


def test_refusals_on_live_buffers_launch_nothing():
    eng = _engine("fc-20-14")
    rho = nap.case_targets(eng)
    p0 = nap.case_params(eng, "normal")
    _load(eng, p0, rho)
    ptrs = [_hip.ptr(t) for t in (eng.project_target, eng.project_norms_out, eng.project_scales, eng.project_scratch)]
    cfg = ctypes.byref(eng.cfg)
    assert eng.lib.isdqn_net_project_apply(cfg, eng.params.data_ptr() + 4, *ptrs, None, None) == _hip.ERR_ARG
    assert eng.lib.isdqn_net_project_apply(cfg, _hip.ptr(eng.params), ptrs[0], eng.project_norms_out.data_ptr() + 4, ptrs[2], ptrs[3], None, None) == _hip.ERR_ARG
    assert eng.lib.isdqn_net_project_norms(cfg, _hip.ptr(eng.params), None, ptrs[3], None) == _hip.ERR_ARG
    with pytest.raises(ValueError):
        eng.set_weight_projection([1.0])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(eng.params), hp.bits(p0)) and bool((eng.project_scales == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- the learn step
def _fields(eng, seed=17):
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    B, A = int(eng.cfg.batch_size), int(eng.cfg.n_actions)
    return dict(action=dev(rng.integers(0, A, B).astype(np.int32)), reward=dev(rng.normal(size=B).astype(np.float32)),
                terminal=dev((rng.random(B) < 0.3).astype(np.uint8)), state=dev(rng.normal(size=(B, 8)).astype(np.float32)),
                next_state=dev(rng.normal(size=(B, 8)).astype(np.float32)))


@pytest.mark.parametrize("trusted", [False, True])
def test_learn_step_then_projection(trusted):
    """set_weight_projection() measures the initial parameters; learn_on_batch + project_weights equals learn_on_batch alone scaled by
    the reported scales, in the master and in the mirror -- which a trusted engine (trust_mirror = True) goes on reading without a
    rebuild."""
    eng = hp.make_engine(hp.FC_SMALL, gamma_n=0.99, learning_rate=1e-2, adam_eps=1.5e-4)
    eng.trust_mirror = trusted
    eng.init_params(5)
    start = eng.params.cpu().numpy().copy()
    rho = eng.set_weight_projection()
    _tier1(rho, nap.norms(eng, start), hp.real_counts(eng), "initial norms")
    assert np.array_equal(_bits(eng.params), hp.bits(start)) and bool((eng.project_scales == 1.0).all())
    fields = _fields(eng)
    if trusted:
        eng.refresh_mirror()
        assert eng._mirror_is_current(None)
    eng.learn_on_batch(eng.make_batch(mirror_current=eng._mirror_is_current(None), **fields))
    learnt = eng.params.cpu().numpy().copy()
    eng.project_weights()
    k = len(rho)
    n_dev, s_dev = eng.project_norms_out.cpu().numpy()[:k], eng.project_scales.cpu().numpy()[:k]
    _tier1([float(x) for x in n_dev], nap.norms(eng, learnt), hp.real_counts(eng), "norms behind the learn step")
    assert all(hp.bits(s_dev[i : i + 1])[0] == hp.bits(np.array([nap.scale_of(rho[i], float(n_dev[i]))], np.float32))[0] for i in range(k))
    assert all(s != ONE for s in s_dev)  # (Adam at 1e-2 moved every kernel's norm)
    want = nap.scaled(eng, learnt, s_dev)
    assert np.array_equal(_bits(eng.params), hp.bits(want))
    for n, r in zip(nap.norms(eng, want), rho):
        assert abs(n / r - 1.0) < AFTER
    if trusted:
        assert eng._mirror_is_current(None)  # (the projection kept the mirror the learn step left current)
    assert torch.equal(_mirror(eng), _mirror_of(eng, want))
    # a trusted engine's next reader uses the mirror as it is: the loss equals that of an engine that rebuilds
    loss = eng.loss_on_batch(eng.make_batch(mirror_current=eng._mirror_is_current(None), **fields)).clone()
    eng.invalidate_mirror()
    again = eng.loss_on_batch(eng.make_batch(**fields)).clone()
    assert torch.equal(loss.view(torch.int32), again.view(torch.int32))
    # the engine's own params handed in as a foreign buffer: master alone, and the mirror is marked stale
    eng.refresh_mirror()
    eng.project_weights(params=eng.params)
    assert not eng._mirror_is_current(None)


# ---------------------------------------------------------------------------------------------------------------- agents
A, B = 4, 4
OBS, FEATURES = hp.CNN["observation_dim"], list(hp.CNN["features"])
BUFFERS = ("params", "adam_m", "adam_v", "adam_count", "losses_accum")
PRUNE = dict(prune_sparsity=0.5, prune_start=0, prune_end=4, prune_period=1000)


def _agent_and_replay(kind, use_graph, **kw):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    common = dict(adam_eps=1.5e-4, batch_size=B, use_graph=use_graph, **kw)
    if kind == "isdqn":
        agent = iSDQN(0, OBS, A, 2, FEATURES, True, False, "cnn", 1e-2, 0.99, 1, 1, 1000, **common)
    elif kind == "dqn":
        agent = DQN(0, OBS, A, FEATURES, True, "cnn", 1e-2, 0.99, 1, 1, 1000, **common)
    else:
        agent = TFDQN(0, OBS, A, FEATURES, True, False, "cnn", 1e-2, 0.99, 1, 1, 1000, **common)
    rb = ReplayBuffer(UniformSamplingDistribution(5), B, 64, stack_size=OBS[2], update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(0)
    for _ in range(40):
        term = bool(rng.random() < 0.08)
        rb.add(TransitionElement(rng.integers(0, 256, OBS[:2], dtype=np.uint8), int(rng.integers(0, A)), float(rng.normal()), term, term))
    return agent, rb


def _state(agent):
    out = {n: getattr(agent._engine, n).clone() for n in BUFFERS}
    if getattr(agent, "target_params", None) is not None:
        out["target"] = agent.target_params.tensor.clone()
    return out


def _same(a, b, what):
    for n in a:
        x, y = a[n], b[n]
        same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)
        assert same, f"{n} differs between {what}"


def _last_dense_norm(eng, params: np.ndarray):
    last = [i for i in eng.infos if int(i.kind) == 1][-1]
    return math.sqrt(nap.sumsq(params[hp.real_index(eng, last)]))


@pytest.mark.parametrize("kind,kw,steps", [("isdqn", {}, 1), ("isdqn", dict(soft_shift_tau=0.25), 1), ("isdqn", {}, 2),
                                          ("dqn", dict(ema_tau=0.25), 1), ("tfdqn", {}, 1), ("isdqn", PRUNE, 1)])
def test_eager_and_captured_steps_are_bit_identical(kind, kw, steps):
    """Three gradient steps (``steps`` = 2: four, as two learn_steps(2) replays) from the same state, eager and captured, on the cnn with
    LayerNorm: parameters, moments, count, loss accumulator and DQN's target end in the same bits; the captured step carries the
    projection (its key says so); every projected tensor's norm is within 2^-22 of its initial norm while the last Dense's has moved;
    an agent without the option, stepped the same way, ends elsewhere.  With pruning on, the norm that comes out right pins the order:
    a projection in front of the prune apply would leave the masked tensor short of its target."""
    eager, rb_e = _agent_and_replay(kind, False, weight_projection=True, **kw)
    graph, rb_g = _agent_and_replay(kind, True, weight_projection=True, **kw)
    plain, rb_p = _agent_and_replay(kind, False, **kw)
    assert plain._engine.project_target is None and not plain.weight_projection
    start = eager._engine.params.cpu().numpy().copy()
    rho = eager._nap_targets
    assert rho == graph._nap_targets and len(rho) == 4
    _tier1(rho, nap.norms(eager._engine, start), hp.real_counts(eager._engine), "the agent's initial norms")
    if "prune_sparsity" in kw:  # a mask update as the training loop makes it at a target update, behind the schedule's end
        for agent in (eager, graph, plain):
            agent._prune_t = 10
            assert agent.prune_target_update(1000)["sparsity"] > 0.49 and agent.prune_active
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
    assert eager._graphed is None and graph._graphed.S == steps and graph._captures == 1 and "nap" in repr(graph._graphed.key)
    assert ("prune" in repr(graph._graphed.key)) == ("prune_sparsity" in kw)
    _same(_state(graph), _state(eager), f"{n} captured and {n} eager steps")
    assert not torch.equal(eager._engine.params, plain._engine.params)
    eng = eager._engine
    assert eng.adam_count.item() == n
    end = eng.params.cpu().numpy()
    for i, (norm, r) in enumerate(zip(nap.norms(eng, end), rho)):
        print(f"{kind} {kw}: tensor {i}: |norm / initial norm - 1| = {abs(norm / r - 1.0):.3e}")
        assert abs(norm / r - 1.0) < AFTER
    moved = abs(_last_dense_norm(eng, end) / _last_dense_norm(eng, start) - 1.0)
    assert moved > 2.0 ** -16, moved  # (the last Dense is left to Adam)
    assert any(abs(norm / r - 1.0) > 2.0 ** -16 for norm, r in zip(nap.norms(eng, plain._engine.params.cpu().numpy()), rho))
    logs = eager.nap_target_update(1000)
    assert set(logs) == {"weight_scale_min", "weight_scale_max"} and 0.5 < logs["weight_scale_min"] <= logs["weight_scale_max"] < 2.0
    assert logs == graph.nap_target_update(1000) and plain.nap_target_update(1000) == {}
    if kind == "dqn":  # the target is never projected itself: an EMA of projected parameters
        assert eager.target_params.tensor is not eng.params


def test_the_option_switched_off_is_the_agent_without_the_keyword():
    off, rb_o = _agent_and_replay("isdqn", True, weight_projection=False)
    plain, rb_p = _agent_and_replay("isdqn", True)
    for step in range(3):
        off.update_online_params(step, rb_o)
        plain.update_online_params(step, rb_p)
    _same(_state(off), _state(plain), "weight_projection=False and no keyword")
    for agent in (off, plain):
        eng = agent._engine
        assert not agent.weight_projection and agent._nap_targets is None and "nap" not in repr(agent._graphed.key)
        assert eng.project_target is None and eng.project_scratch is None and eng.project_scales is None and eng.project_norms_out is None


def test_an_engine_for_another_batch_size_receives_the_same_target_norms():
    agent, _ = _agent_and_replay("tfdqn", False, weight_projection=True)
    first = agent._engine
    rho = list(agent._nap_targets)
    first.params.mul_(1.5)  # (norms that are no longer the initial ones: a re-measurement would show)
    eng = agent._engine_for(2 * B)
    assert eng is not first and agent._nap_targets == rho
    assert [float(x) for x in eng.project_target.cpu().numpy()[: len(rho)]] == rho


def test_training_run_logs_the_scales_and_keeps_the_initial_norms_through_a_reset(tmp_path):
    """The lunar-lander entry point on the seeded synthetic environment with -ln -nap and -reset: weight_scale_min / weight_scale_max are
    logged at every target update, the target norms are still those measured at the start, and at the end -- two resets later -- every
    projected kernel has its initial norm."""
    from unittest import mock

    import experiments.lunar_lander.isdqn as entry

    seen = {}
    real_train = entry.train

    def train(key, p, agent, env, rb):
        seen.update(p=p, agent=agent, rho=list(agent._nap_targets))
        return real_train(key, p, agent, env, rb)

    argv = ["--experiment_name", "_test_nap", "--seed", "1", "--disable_wandb", "--features", "25", "15", "--replay_buffer_capacity", "100",
            "--batch_size", "3", "--update_horizon", "1", "--gamma", "0.99", "--learning_rate", "1e-3", "--horizon", "10", "--n_epochs", "1",
            "--n_training_steps_per_epoch", "24", "--data_to_update", "1", "--target_update_frequency", "3", "--n_initial_samples", "3",
            "--epsilon_end", "0.01", "--epsilon_duration", "4", "--architecture_type", "fc", "-env", "synthetic",
            "-ln", "-nap", "-reset", "9"]
    with mock.patch.object(entry, "train", train):
        entry.run(argv, root=str(tmp_path))
    agent, history = seen["agent"], [h for h in seen["p"]["wandb"].history if "weight_scale_min" in h]
    assert agent.weight_projection and len(history) >= 6
    assert sum("reset" in h for h in history) == sum(h["n_training_steps"] % 9 == 0 for h in history) >= 2 and "reset" not in history[-1]
    for h in history:
        assert h["n_training_steps"] % 3 == 0 and 0.0 < h["weight_scale_min"] <= h["weight_scale_max"] < math.inf
    eng = agent._engine
    assert agent._nap_targets == seen["rho"] == [float(x) for x in eng.project_target.cpu().numpy()[: len(seen["rho"])]]
    for norm, r in zip(nap.norms(eng, eng.params.cpu().numpy()), seen["rho"]):
        assert abs(norm / r - 1.0) < AFTER
