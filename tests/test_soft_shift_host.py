"""Host side of the soft head shift (include/isdqn_hip.h, isdqn_net_soft_shift) and of the replay ratio, no GPU: the numpy restatement
of tests/helpers/soft_shift.py against float64, the wrong variants shown to differ from it, the two flags with their refusals on the
entry points, the gradient-step count of a run, the trainer's cadence under -rr with a recording agent, the agents' constructor refusals
and the C ABI's refusals, which come before any launch.  The device side is tests/test_gpu_soft_shift.py."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.helpers import redo as hredo
from tests.helpers import soft_shift as hs

F32 = np.float32
ENTRY_POINTS = [("atari", a) for a in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn")] + [("lunar_lander", a) for a in ("isdqn", "dqn", "tfdqn")]
SOFT_SHIFT_ENTRY_POINTS = [("atari", "isdqn"), ("atari", "analysisdqn"), ("lunar_lander", "isdqn")]


# ------------------------------------------------------------------------------------------------ the restatement
def _layout(K=3, **kw):
    return hredo.HostLayout((8,), 3, 1 + K, (20,), "fc", False, **kw)


def test_geometry_of_the_head_blocks():
    lay = _layout()
    w_off, b_off, in_p, out_p, R, K = hs.head_geometry(lay)
    assert (in_p, out_p, R, K) == (24, 16, 3, 3) and w_off % 8 == 0 and b_off % 8 == 0  # 20 -> 24 columns, 12 -> 16 rows
    assert hs.head_geometry(_layout(K=1, n_bins=5))[3:] == (32, 15, 1)  # 2 * 3 * 5 = 30 -> 32 rows
    assert hs.head_geometry(_layout(K=3, n_quantiles=4))[3:] == (48, 12, 3)


def test_hand_written_shift():
    """K = 2, tau = 1/4 on small integers (every operation exact): head 0 <- 3/4 h0 + 1/4 h1, head 1 <- 3/4 h1 + 1/4 h2 with the OLD
    h1; head 2, the padding rows and every other tensor keep their bits."""
    lay = hredo.HostLayout((8,), 3, 3, (20,), "fc", False)
    w_off, b_off, in_p, out_p, R, K = hs.head_geometry(lay)
    n = lay.n_param_floats
    p = np.arange(n, dtype=F32) * F32(4)
    out = hs.soft_shift(lay, p, 0.25)
    w, b = hs.head_views(lay, p)
    wn, bn = hs.head_views(lay, out)
    for k in range(K):
        assert np.array_equal(wn[k], 0.75 * w[k] + 0.25 * w[k + 1]) and np.array_equal(bn[k], 0.75 * b[k] + 0.25 * b[k + 1])
    assert np.array_equal(wn[K], w[K]) and np.array_equal(bn[K], b[K])
    touched = np.zeros(n, bool)
    touched[w_off : w_off + K * R * in_p] = True
    touched[b_off : b_off + K * R] = True
    assert np.array_equal(hs.bits(out)[~touched], hs.bits(p)[~touched]) and (out[touched] != p[touched]).all()
    assert p[1] == 4  # the input is not modified
    assert np.array_equal(hs.bits(hs.soft_shift(lay, p, 0.0)), hs.bits(p))


def test_tau_one_is_the_hard_shift_bit_for_bit():
    lay = _layout()
    rng = np.random.default_rng(0)
    p = rng.standard_normal(lay.n_param_floats).astype(F32)
    w, b = hs.head_views(lay, p)
    w[1, 0, 0], w[2, 1, 3], w[3, 2, 5], b[1, 1], b[0, 0] = np.nan, -0.0, np.inf, -0.0, np.nan
    out = hs.soft_shift(lay, p, 1.0)
    wn, bn = hs.head_views(lay, out)
    assert np.array_equal(hs.bits(wn[:3]), hs.bits(w[1:])) and np.array_equal(hs.bits(bn[:3]), hs.bits(b[1:]))
    assert np.array_equal(hs.bits(wn[3]), hs.bits(w[3]))
    # the blend at tau -> 1 would not: (1 - tau) * NaN stays NaN where the hard shift replaces it
    assert np.isnan(hs.soft_shift(lay, p, 0.5)[hs.head_geometry(lay)[1]])


@pytest.mark.parametrize("tau", [0.005, 0.3, 0.9])  # (at a power of two both products are exact and a contraction changes nothing)
def test_restatement_against_float64_and_the_wrong_variants(tau):
    """Float64 holds the product of two float32 exactly and their sum to within 2^-53: rounding each of the three float64 results to
    float32 once is the definition's value (53 >= 2 * 24 + 2: double rounding is innocuous), so the restatement must equal it bit for
    bit, and it lies within three float32 roundings of the unrounded float64 value.  The contracted variant differs from it in bits
    (it skips one rounding, so it stays inside the bound: only the bits tell it apart); the variant that reads already-shifted
    neighbours leaves the bound."""
    lay = _layout(K=3)
    rng = np.random.default_rng(7)
    p = (rng.standard_normal(lay.n_param_floats) * 3).astype(F32)
    got = hs.soft_shift(lay, p, tau)
    t32 = F32(tau)
    omt = np.float64(F32(1.0) - t32)
    ref, exact, bound = p.copy(), p.astype(np.float64), np.zeros(p.size)
    eps = 2.0 ** -24
    for src, dst, ex, bd in zip(*(hs.head_views(lay, a) for a in (p.copy(), ref, exact, bound))):  # weights, then biases
        lo, up = src[:3].astype(np.float64), src[1:].astype(np.float64)
        a, b = (omt * lo).astype(F32), (np.float64(t32) * up).astype(F32)
        dst[:3] = (a.astype(np.float64) + b.astype(np.float64)).astype(F32)
        ex[:3] = omt * lo + np.float64(t32) * up
        bd[:3] = eps * (np.abs(omt * lo) + np.abs(np.float64(t32) * up)) * (1 + eps) + eps * np.abs(ex[:3]) + 1e-45
    assert np.array_equal(hs.bits(got), hs.bits(ref))
    assert (np.abs(got.astype(np.float64) - exact) <= bound).all()
    fma = hs.soft_shift(lay, p, tau, fma=True)
    assert not np.array_equal(hs.bits(fma), hs.bits(ref)) and (np.abs(fma.astype(np.float64) - exact) <= bound).all()
    shifted = hs.soft_shift(lay, p, tau, shifted_neighbours=True)
    assert not np.array_equal(hs.bits(shifted), hs.bits(ref)) and not (np.abs(shifted.astype(np.float64) - exact) <= bound).all()
    # with one head to write there is no neighbour that could have been shifted: the two orders agree (K = 1 cannot show the mistake)
    one = _layout(K=1)
    q = p[: one.n_param_floats]
    assert np.array_equal(hs.bits(hs.soft_shift(one, q, tau)), hs.bits(hs.soft_shift(one, q, tau, shifted_neighbours=True)))


# ------------------------------------------------------------------------------------------------ flags
def _base(env):
    return ["-en", "sst_Synthetic", "-s", "1", "-dw", "-tuf", "16"] + (["-f", "8", "8", "8", "16", "-at", "cnn"] if env == "atari" else [])


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_flags_parse_and_stay_out_of_parameters_json(tmp_path, env, algo):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    p = prepare_logs(env, algo, _base(env), root=str(tmp_path))
    assert (p["soft_shift_tau"], p["replay_ratio"]) == (0.0, 1)
    assert pa.soft_shift_kwargs(p) == {}  # without the flag the agents receive the keywords they received before it existed
    p = prepare_logs(env, algo, _base(env) + ["-s", "2", "-rr", "4"], root=str(tmp_path))
    assert p["replay_ratio"] == 4 and pa.soft_shift_kwargs(p) == {}
    p = prepare_logs(env, algo, _base(env) + ["-s", "3", "--replay_ratio", "16"], root=str(tmp_path))
    assert p["replay_ratio"] == 16
    stored = json.load(open(tmp_path / env / "exp_output" / "sst_Synthetic" / "parameters.json"))
    assert not any("soft_shift" in k or "replay_ratio" in k for section in stored.values() for k in section)


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_soft_shift_is_for_the_three_isdqn_entry_points(tmp_path, env, algo):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs
    from slimdqn.networks._agent import SOFT_SHIFT_REFUSED

    argv = _base(env) + ["-sst", "0.005"]
    if (env, algo) in SOFT_SHIFT_ENTRY_POINTS:
        p = prepare_logs(env, algo, argv, root=str(tmp_path))
        assert pa.soft_shift_kwargs(p) == dict(soft_shift_tau=0.005)
        assert prepare_logs(env, algo, _base(env) + ["-s", "2", "--soft_shift_tau", "1"], root=str(tmp_path))["soft_shift_tau"] == 1.0
        stored = json.load(open(tmp_path / env / "exp_output" / "sst_Synthetic" / "parameters.json"))
        assert not any("soft_shift" in k for section in stored.values() for k in section)
    else:
        with pytest.raises(ValueError) as e:
            prepare_logs(env, algo, argv, root=str(tmp_path))
        assert str(e.value) == SOFT_SHIFT_REFUSED
        assert not os.path.exists(tmp_path / env)


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
@pytest.mark.parametrize("extra,message", [
    (["-sst", "-0.1"], "SOFT_SHIFT_TAU_REFUSED"),
    (["-sst", "1.5"], "SOFT_SHIFT_TAU_REFUSED"),
    (["-sst", "nan"], "SOFT_SHIFT_TAU_REFUSED"),
    (["-rr", "0"], "REPLAY_RATIO_REFUSED"),
    (["-rr", "-2"], "REPLAY_RATIO_REFUSED"),
    (["-rr", "2", "-utd", "4"], "REPLAY_RATIO_UTD_REFUSED"),
    (["-rr", "2", "-utd", "0.5"], "REPLAY_RATIO_UTD_REFUSED"),
    (["-rr", "2", "-offline", "nowhere"], "REPLAY_RATIO_OFFLINE_REFUSED"),
    (["-rr", "3"], "REPLAY_RATIO_TUF_REFUSED"),   # -tuf 16
    (["-rr", "32"], "REPLAY_RATIO_TUF_REFUSED"),
])
def test_refusals_come_before_anything_is_written(tmp_path, env, algo, extra, message):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, _base(env) + extra, root=str(tmp_path))
    assert str(e.value) == getattr(pa, message)
    assert not os.path.exists(tmp_path / env)


def test_a_replay_ratio_of_one_refuses_nothing_new(tmp_path):
    """-rr 1 with -utd 4, and -offline without -rr, are today's runs."""
    from experiments.base.utils import prepare_logs

    assert prepare_logs("atari", "isdqn", _base("atari") + ["-rr", "1", "-utd", "4"], root=str(tmp_path))["replay_ratio"] == 1
    assert prepare_logs("atari", "dqn", _base("atari") + ["-s", "2", "-offline", "nowhere"], root=str(tmp_path / "offline"))["replay_ratio"] == 1


def test_gradient_steps_of_a_run_carry_the_replay_ratio():
    from experiments.base.parser_argument import n_gradient_steps

    p = dict(n_epochs=3, n_training_steps_per_epoch=1000, n_initial_samples=200, data_to_update=1)
    assert n_gradient_steps(p) == 2800  # (a p from before the flag: no key)
    assert n_gradient_steps(dict(p, replay_ratio=1)) == 2800 and n_gradient_steps(dict(p, replay_ratio=4)) == 11200
    assert n_gradient_steps(dict(p, data_to_update=4)) == 700 and n_gradient_steps(dict(p, data_to_update=4, replay_ratio=1)) == 700
    assert n_gradient_steps(dict(p, n_initial_samples=5000, replay_ratio=8)) == 1


# ------------------------------------------------------------------------------------------------ the trainer's cadence
class _Env:
    n_actions, state, observation = 2, None, np.zeros((2, 2), np.uint8)

    def __init__(self):
        self.n_steps = 0

    def reset(self):
        self.n_steps = 0

    def step(self, action):
        self.n_steps += 1
        return 0.0, False


class _Replay:
    _clipping = None

    def add(self, *a, **k):
        pass


class _Agent:
    """Records every call the trainer makes, in order."""
    data_to_update, params = 1, None

    def __init__(self, tuf=8):
        self.target_update_frequency = tuf
        self.calls = []

    def best_action(self, params, state, **kw):
        return 0

    def update_online_params(self, step, rb):
        self.calls.append(("online", step))

    def learn_steps(self, n, rb):
        self.calls.append(("learn_steps", n))

    def update_target_params(self, step):
        self.calls.append(("target", step))
        return (True, {"loss": 0.0}) if step % self.target_update_frequency == 0 else (False, {})

    def recycle_dormant(self, rb, tau):
        self.calls.append(("redo", tau))
        return [0]

    def reset_parameters(self, **kw):
        self.calls.append(("reset", kw))

    def get_model(self):
        return {}


def _p(tmp_path, name, **kw):
    from experiments.base.utils import _NullLogger

    p = dict(epsilon_end=0.1, epsilon_duration=10, n_epochs=1, n_training_steps_per_epoch=30, n_initial_samples=10, horizon=10,
             reset_frequency=0, reset_shrink=0.25, reset_top_layers=2, redo_frequency=0, redo_tau=0.1, save_path=str(tmp_path / name), seed=1,
             wandb=_NullLogger())
    p.update(kw)
    return p


def test_a_replay_ratio_of_one_is_the_loop_without_the_flag(tmp_path):
    from experiments.base.dqn import train

    runs = []
    for name, extra in (("none", {}), ("one", dict(replay_ratio=1))):
        p = _p(tmp_path, name, reset_frequency=16, redo_frequency=8, **extra)
        agent = _Agent()
        train(np.random.default_rng(0), p, agent, _Env(), _Replay())
        runs.append((agent.calls, [dict(h) for h in p["wandb"].history]))
    assert runs[0] == runs[1] and not any(c[0] == "learn_steps" for c in runs[0][0])
    assert [c for c in runs[0][0] if c[0] in ("online", "target")][:4] == [("online", 11), ("target", 11), ("online", 12), ("target", 12)]


def test_a_replay_ratio_counts_target_updates_and_their_hooks_in_gradient_steps(tmp_path):
    """-rr 4 -tuf 8, 10 initial samples, 30 environment steps: 20 of them train, each with learn_steps(4); update_target_params sees the
    gradient counts 4, 8, .., 80; updates are logged at 8, 16, ..; -redo 16 and -reset 32 fire at their gradient-step multiples, the
    reset behind the recycle of the same step."""
    from experiments.base.dqn import train

    p = _p(tmp_path, "rr4", replay_ratio=4, redo_frequency=16, reset_frequency=32)
    agent = _Agent(tuf=8)
    train(np.random.default_rng(0), p, agent, _Env(), _Replay())
    assert not any(c[0] == "online" for c in agent.calls)
    assert [c for c in agent.calls if c[0] == "learn_steps"] == [("learn_steps", 4)] * 20
    assert [c[1] for c in agent.calls if c[0] == "target"] == list(range(4, 84, 4))
    # every environment step: its gradient steps, then the target update at their count
    pairs = [c for c in agent.calls if c[0] in ("learn_steps", "target")]
    assert all(a[0] == "learn_steps" and b[0] == "target" for a, b in zip(pairs[::2], pairs[1::2]))
    updates = [h for h in p["wandb"].history if "loss" in h]
    assert [h["n_training_steps"] for h in updates] == list(range(8, 88, 8))
    assert [h["n_training_steps"] for h in updates if "recycled_neurons" in h] == [16, 32, 48, 64, 80]
    assert [h["n_training_steps"] for h in updates if h.get("reset") == 1] == [32, 64]
    hooks = [c[0] for c in agent.calls if c[0] in ("redo", "reset")]
    assert hooks == ["redo", "redo", "reset", "redo", "redo", "reset", "redo"]  # 16, 32, 32, 48, 64, 64, 80


class _VectorEnv:
    """Four environments in lockstep: what collect_vector_samples needs of a VectorEnv is replaced with it below."""
    envs = [None] * 4

    def __len__(self):
        return 4

    def reset(self):
        pass


def test_the_vector_round_owes_the_ratio_per_step(tmp_path, monkeypatch):
    """Rounds of 4 environment steps, -rr 2 -tuf 8, 10 initial samples: steps 11 and 12 of the third round owe 2 each; from then on a
    round owes 8, and the target update in its middle (the gradient count reaches 8 at step 14, 16 at step 18, ..) splits it into the
    steps owed in front of the update and those behind it; the counts handed to the target update are gradient counts."""
    from experiments.base import dqn as trainer

    def collect(rng, env, agent, rb, p, schedule, n_training_steps, between):
        res = [(0.0, n_training_steps + i + 1 == 32) for i in range(4)]
        between(res)
        return res

    monkeypatch.setattr(trainer, "collect_vector_samples", collect)
    p = _p(tmp_path, "vec", replay_ratio=2, n_training_steps_per_epoch=32)
    agent = _Agent(tuf=8)
    trainer.train(np.random.default_rng(0), p, agent, _VectorEnv(), _Replay())
    assert not any(c[0] == "online" for c in agent.calls)
    # rounds 1, 2: nothing owed; round 3 (steps 9..12): 4 owed, no update; rounds 4..8 (steps 13..32): 8 each; the count reaches 12, 20, ..
    assert [c for c in agent.calls if c[0] != "target"][:3] == [("learn_steps", 0), ("learn_steps", 0), ("learn_steps", 4)]
    assert sum(c[1] for c in agent.calls if c[0] == "learn_steps") == 2 * 22
    assert [c[1] for c in agent.calls if c[0] == "target"] == [8, 16, 24, 32, 40]
    # the steps owed before an update are issued in front of it: gradient steps 5..8 of round 4, then the update at 8, then the rest
    i = agent.calls.index(("target", 8))
    assert agent.calls[i - 1] == ("learn_steps", 4) and agent.calls[i + 1] == ("learn_steps", 4)
    assert [h["n_training_steps"] for h in p["wandb"].history if "loss" in h] == [8, 16, 24, 32, 40]
    # without the flag the same rounds take the old path: one step owed per environment step, updates at environment steps
    q = _p(tmp_path, "vec1", n_training_steps_per_epoch=32)
    plain = _Agent(tuf=8)
    trainer.train(np.random.default_rng(0), q, plain, _VectorEnv(), _Replay())
    assert sum(c[1] for c in plain.calls if c[0] == "learn_steps") == 22 and [c[1] for c in plain.calls if c[0] == "target"] == [16, 24, 32]


# ------------------------------------------------------------------------------------------------ agents and the C ABI
def test_the_agents_own_soft_shift_check():
    from slimdqn.networks._agent import SOFT_SHIFT_REFUSED, check_soft_shift_tau

    assert check_soft_shift_tau(0) == 0.0 and check_soft_shift_tau(0.0, supported=True) == 0.0 and check_soft_shift_tau(0.25, supported=True) == 0.25
    assert check_soft_shift_tau(1, supported=True) == 1.0
    with pytest.raises(ValueError) as e:
        check_soft_shift_tau(0.005)
    assert str(e.value) == SOFT_SHIFT_REFUSED
    for bad in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            check_soft_shift_tau(bad, supported=True)


def test_the_single_head_agents_refuse_a_soft_shift_and_isdqn_still_refuses_an_ema_target():
    """Before an engine is built: no GPU is needed to be refused."""
    import inspect

    from slimdqn.networks._agent import EMA_REFUSED, SOFT_SHIFT_REFUSED
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    with pytest.raises(ValueError) as e:
        DQN(0, (11,), 5, [40, 24], False, "fc", 1e-3, 0.99, 1, 1, 8, batch_size=4, soft_shift_tau=0.005)
    assert str(e.value) == SOFT_SHIFT_REFUSED
    for cls in (TFDQN, AnalysisTFDQN):
        with pytest.raises(ValueError) as e:
            cls(0, (11,), 5, [40, 24], False, False, "fc", 1e-3, 0.99, 1, 1, 8, batch_size=4, soft_shift_tau=0.005)
        assert str(e.value) == SOFT_SHIFT_REFUSED
    for cls in (iSDQN, AnalysisDQN):
        with pytest.raises(ValueError) as e:
            cls(0, (11,), 5, 2, [40, 24], False, False, "fc", 1e-3, 0.99, 1, 1, 8, batch_size=4, ema_tau=0.005, soft_shift_tau=0.005)
        assert str(e.value) == EMA_REFUSED
        with pytest.raises(ValueError, match=r"soft_shift_tau must be in \[0, 1\]"):
            cls(0, (11,), 5, 2, [40, 24], False, False, "fc", 1e-3, 0.99, 1, 1, 8, batch_size=4, soft_shift_tau=1.5)
    for cls in (iSDQN, DQN, TFDQN):
        par = inspect.signature(cls.__init__).parameters["soft_shift_tau"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == 0.0


def test_the_c_abi_refuses_without_touching_a_device():
    """Every ISDQN_ERR_ARG of the call comes before any launch: stand-in pointers are never read."""
    from slimdqn import _hip

    lay = _layout(K=3)
    lib, cfg = lay.lib, lay.cfg
    one = 1 << 20

    def shift(cfg=cfg, params=one, tau=0.005):
        return lib.isdqn_net_soft_shift(ctypes.byref(cfg), params, tau, None, None)

    assert "isdqn_net_soft_shift" in _hip.PUBLIC_SYMBOLS
    assert shift(params=None) == _hip.ERR_ARG
    for tau in (-1e-3, 1.001, float("nan"), float("inf")):
        assert shift(tau=tau) == _hip.ERR_ARG, tau
        assert "[0, 1]" in _hip.last_error()
    single = hredo.HostLayout((8,), 3, 1, (20,), "fc", False)
    assert shift(cfg=single.cfg) == _hip.ERR_ARG and "n_heads" in _hip.last_error()
    assert shift(cfg=single.cfg, tau=0.0) == _hip.ERR_ARG  # (a refusal does not depend on the tau)
    assert shift(params=one + 4) == _hip.ERR_ARG and "aligned" in _hip.last_error()  # a view at an odd offset: the lanes are 16 bytes wide
    assert shift(tau=0.0) == _hip.OK  # launches nothing: the stand-in pointer is not touched
    assert lib.isdqn_net_soft_shift(None, one, 0.005, None, None) == _hip.ERR_ARG


def test_the_kernel_lives_in_a_source_of_its_own_and_passes_the_lint():
    """The four pinned sources and the conservative term's keep their kernels (tests/golden/kernel_order.txt and
    tests/test_conservative_host.py hold them): soft_shift_kernel is built from build.SIDE_SOURCES into every variant, its two
    instantiations are the only kernels of that object, no other object has them, and scripts/isa_lint.py is clean on it."""
    import importlib.util
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(root, "is-dqn_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SIDE_SOURCES == ["soft_shift_kernels.hip"] and not set(build.SIDE_SOURCES) & set(build.SOURCES + build.EXTRA_SOURCES)
    assert "__global__" not in open(os.path.join(build.CSRC, "soft_shift.h")).read()
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    side = build.emit_side_asm()
    assert [os.path.basename(a) for a in side] == ["soft_shift_kernels.s"]
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(side[0]).read(), re.M)
    assert len(kernels) == 2 and all("soft_shift_kernel" in k for k in kernels), kernels
    for other in build.emit_asm():
        assert "soft_shift_kernel" not in open(other).read(), other
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "isa_lint.py")] + side, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert re.search(r"soft_shift_kernels\.s: 2 functions", r.stdout), r.stdout[:500]
