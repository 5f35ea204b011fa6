"""Host side of the periodic resets and the EMA targets (include/isdqn_hip.h, isdqn_net_reset / isdqn_net_ema), no GPU: the numpy
restatements of tests/helpers/reset.py on arrays small enough to write the expected buffers by hand, the wrong variants shown to differ
from them, the seeds, the flags with their refusals on all eight entry points, the trainer's cadence with a stub agent, and the
host-only layout call.  The device side is tests/test_gpu_reset.py."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.helpers import redo as hredo
from tests.helpers import reset as hr

F32 = np.float32
FACTORS = (((0.5, 0.5), (0.0, 1.0)), ((0.8, 0.2), (0.3, 0.7)), ((1.0, 0.0), (0.0, 1.0)))  # (lower, upper) pairs of (shrink, perturb)
ENTRY_POINTS = [("atari", a) for a in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn")] + [("lunar_lander", a) for a in ("isdqn", "dqn", "tfdqn")]


def _fc_layout():
    """obs 2 -> Dense_0 (3) -> Dense_1 (2 outputs): kernels [8][8], vectors 8 floats, layers 0 and 1."""
    lay = hredo.HostLayout((2,), 2, 1, (3,), "fc", False)
    assert [(i.name.decode(), int(i.layer), int(i.offset), int(i.size)) for i in lay.infos] == [
        ("Dense_0/kernel", 0, 0, 64), ("Dense_0/bias", 0, 64, 8), ("Dense_1/kernel", 1, 72, 64), ("Dense_1/bias", 1, 136, 8)]
    return lay


def test_reset_on_hand_written_arrays():
    lay = _fc_layout()
    n = lay.n_param_floats
    p = np.arange(1, n + 1, dtype=F32)
    f = -np.arange(1, n + 1, dtype=F32) * F32(0.25)
    m, v = np.full(n, 3, F32), np.full(n, 5, F32)
    # split at layer 1: Dense_0 is lower (0.5, 0.5), Dense_1 upper (0, 1)
    p2, m2, v2, c2 = hr.reset(lay, p, m, v, np.array([7], np.int32), f, 1, (0.5, 0.5), (0.0, 1.0))
    assert np.array_equal(p2[:72], F32(0.5) * p[:72] + F32(0.5) * f[:72])  # (exact: halves and quarters of small integers)
    assert p2[0] == 0.5 * 1 - 0.125 and p2[71] == 36 - 9
    assert np.array_equal(p2[72:], f[72:])
    assert not m2.any() and not v2.any() and c2.tolist() == [0]
    assert p[0] == 1 and m[0] == 3  # the inputs are not modified
    # identity on the lower class: parameters and moments of Dense_0 keep their bits, Dense_1 is replaced; the count may be left alone
    p3, m3, v3, c3 = hr.reset(lay, p, m, v, None, f, 1, (1.0, 0.0), (0.0, 1.0))
    assert np.array_equal(p3[:72], p[:72]) and np.array_equal(p3[72:], f[72:]) and c3 is None
    assert (m3[:72] == 3).all() and not m3[72:].any() and (v3[:72] == 5).all() and not v3[72:].any()
    # split 0: everything upper; split n_layers: nothing is; no moments given
    assert np.array_equal(hr.reset(lay, p, None, None, None, f, 0, (1.0, 0.0), (0.0, 2.0))[0], 2 * f)
    out = hr.reset(lay, p, None, None, None, f, 2, (1.0, 0.0), (0.0, 2.0))
    assert np.array_equal(out[0], p) and out[1] is None and out[2] is None
    # s == 0 does not read p: NaN and Inf are replaced; a general blend propagates them
    bad = p.copy()
    bad[72], bad[73] = np.nan, np.inf
    assert np.array_equal(hr.reset(lay, bad, None, None, None, f, 1, (0.5, 0.5), (0.0, 1.0))[0], p2)
    assert np.isnan(hr.reset(lay, bad, None, None, None, f, 1, (0.5, 0.5), (0.25, 1.0))[0][72])
    # +0 in both buffers stays +0 by bit pattern
    z = hr.reset(lay, np.zeros(n, F32), None, None, None, np.zeros(n, F32), 1, (0.8, 0.2), (0.0, 1.0))[0]
    assert not hr.bits(z).any()
    assert hr.layout_numbers(lay) == (2, 0)


def test_each_wrong_reset_differs_from_the_definition():
    """On a LayerNorm network (a LayerNorm tensor of an upper layer is where 'class by kind' goes wrong) with factors that are not
    dyadic (so that the contracted sum rounds differently somewhere) and a NaN in the upper class."""
    lay = hredo.HostLayout((11,), 5, 3, (40, 24), "fc", True)
    rng = np.random.default_rng(0)
    n = lay.n_param_floats
    p, f = rng.normal(size=n).astype(F32), rng.normal(size=n).astype(F32)
    m, v = rng.normal(size=n).astype(F32), rng.uniform(0.5, 2, n).astype(F32)
    n_layers, first = hr.layout_numbers(lay)
    assert (n_layers, first) == (3, 0)
    args = (lay, p, m, v, np.array([3], np.int32), f, 1)
    told_apart = {name: [] for name in hr.WRONG_RESETS}
    for lower, upper in FACTORS:
        right = hr.reset(*args, lower, upper)
        for name, kw in hr.WRONG_RESETS.items():
            wrong = hr.reset(*args, lower, upper, **kw)
            if any(not np.array_equal(hr.bits(a), hr.bits(b)) for a, b in zip(right[:3], wrong[:3])):
                told_apart[name].append((lower, upper))
    # every variant but the NaN one (finite parameters: 0 * p == 0; shown below) is told apart by at least one factor set
    assert all(told_apart[name] for name in hr.WRONG_RESETS if name != "p read when s == 0"), told_apart
    assert ((0.8, 0.2), (0.3, 0.7)) in told_apart["fma-contracted sum"] and ((1.0, 0.0), (0.0, 1.0)) in told_apart["moments cleared everywhere"]
    bad = p.copy()
    bad[lay.infos[-1].offset] = np.nan
    right = hr.reset(lay, bad, m, v, None, f, 1, (0.5, 0.5), (0.0, 1.0))[0]
    wrong = hr.reset(lay, bad, m, v, None, f, 1, (0.5, 0.5), (0.0, 1.0), read_p_when_s_is_zero=True)[0]
    assert np.isfinite(right).all() and np.isnan(wrong).sum() == 1


def test_ema_on_hand_written_arrays_and_its_wrong_variant():
    t, p = np.array([1.0, -2.0, 0.0, 8.0], F32), np.array([3.0, 2.0, -0.0, 8.0], F32)
    assert np.array_equal(hr.ema(t, p, 0.5), [2.0, 0.0, 0.0, 8.0])
    assert np.array_equal(hr.bits(hr.ema(t, p, 0.0)), hr.bits(t)) and np.array_equal(hr.bits(hr.ema(t, p, 1.0)), hr.bits(p))
    assert hr.bits(hr.ema(t, p, 1.0))[2] == 0x80000000  # the sign of the zero is copied
    omt, tau = F32(1) - F32(0.005), F32(0.005)
    assert hr.ema(t, p, 0.005)[0] == F32(omt * F32(1.0)) + F32(tau * F32(3.0))
    nan = hr.ema(np.array([np.nan], F32), np.array([1.0], F32), 0.005)
    assert np.isnan(nan[0]) and hr.ema(np.array([np.nan], F32), np.array([1.0], F32), 1.0)[0] == 1.0
    rng = np.random.default_rng(1)
    t, p = rng.normal(size=4096).astype(F32), rng.normal(size=4096).astype(F32)
    for tau in (0.005, 0.5):
        assert not np.array_equal(hr.bits(hr.ema(t, p, tau)), hr.bits(hr.ema(t, p, tau, lerp=True))), tau
        assert np.allclose(hr.ema(t, p, tau), hr.ema(t, p, tau, lerp=True), atol=1e-6)


def test_reset_seeds_are_distinct_from_recycle_seeds_and_from_the_seed():
    from slimdqn.networks._agent import augment_seed, recycle_seed, reset_seed

    resets = [reset_seed(s, k) for s in (0, 1, 7) for k in range(50)]
    recycles = [recycle_seed(s, k) for s in (0, 1, 7) for k in range(50)]
    assert len(set(resets)) == len(resets) and not set(resets) & set(recycles) and not set(resets) & {0, 1, 7}
    assert not set(resets) & {augment_seed(s) for s in (0, 1, 7)}
    assert resets == [reset_seed(s, k) for s in (0, 1, 7) for k in range(50)]
    state = np.random.SeedSequence(entropy=7, spawn_key=(3, 4)).generate_state(4)
    assert reset_seed(7, 4) == int.from_bytes(state.tobytes(), "little")
    first = lambda s: np.random.default_rng(s).uniform(size=4).tolist()
    inits = [first(s) for s in range(64)]
    assert all(first(reset_seed(s, k)) not in inits for s in (0, 1, 7) for k in range(4))


def _base(env):
    return ["-en", "reset_Synthetic", "-s", "1", "-dw", "-tuf", "16"] + (["-f", "8", "8", "8", "16", "-at", "cnn"] if env == "atari" else [])


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_flags_parse_and_stay_out_of_parameters_json(tmp_path, env, algo):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    p = prepare_logs(env, algo, _base(env), root=str(tmp_path))
    assert (p["reset_frequency"], p["reset_shrink"], p["reset_top_layers"], p["ema_tau"]) == (0, 0.5, 0, 0.0)
    # without the flags the agents receive exactly the keywords they received before the flags existed
    assert pa.ema_kwargs(p) == {}
    p = prepare_logs(env, algo, _base(env) + ["-s", "2", "-reset", "32", "-resets", "0.8", "-resetl", "1"], root=str(tmp_path))
    assert pa.reset_kwargs(p) == dict(shrink=0.8, n_top_layers=1) and p["reset_frequency"] == 32 and pa.ema_kwargs(p) == {}
    stored = json.load(open(tmp_path / env / "exp_output" / "reset_Synthetic" / "parameters.json"))
    assert not any("reset" in k or "ema" in k for section in stored.values() for k in section)
    # the two modifiers mean nothing without -reset
    prepare_logs(env, algo, _base(env) + ["-s", "3", "-resets", "7", "-resetl", "-2"], root=str(tmp_path))


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
@pytest.mark.parametrize("extra,message", [
    (["-reset", "24"], "RESET_FREQUENCY_REFUSED"),  # not a multiple of -tuf 16
    (["-reset", "8"], "RESET_FREQUENCY_REFUSED"),
    (["-reset", "-16"], "RESET_FREQUENCY_REFUSED"),
    (["-reset", "16", "-resets", "-0.1"], "RESET_SHRINK_REFUSED"),
    (["-reset", "16", "-resets", "1.5"], "RESET_SHRINK_REFUSED"),
    (["-reset", "16", "-resets", "nan"], "RESET_SHRINK_REFUSED"),
    (["-reset", "16", "-resetl", "-1"], "RESET_TOP_LAYERS_REFUSED"),
    (["-ema", "-0.1"], "EMA_TAU_REFUSED"),
    (["-ema", "1.5"], "EMA_TAU_REFUSED"),
    (["-ema", "nan"], "EMA_TAU_REFUSED"),
])
def test_refusals_come_before_anything_is_written(tmp_path, env, algo, extra, message):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, _base(env) + extra, root=str(tmp_path))
    assert getattr(pa, message) in str(e.value)
    assert not os.path.exists(tmp_path / env)


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_ema_is_for_the_two_dqn_entry_points(tmp_path, env, algo):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs
    from slimdqn.networks._agent import EMA_REFUSED

    argv = _base(env) + ["-ema", "0.005"]
    if algo == "dqn":
        p = prepare_logs(env, algo, argv, root=str(tmp_path))
        assert pa.ema_kwargs(p) == dict(ema_tau=0.005)
        stored = json.load(open(tmp_path / env / "exp_output" / "reset_Synthetic" / "parameters.json"))
        assert not any("ema" in k for section in stored.values() for k in section)
    else:
        with pytest.raises(ValueError) as e:
            prepare_logs(env, algo, argv, root=str(tmp_path))
        assert str(e.value) == EMA_REFUSED
        assert not os.path.exists(tmp_path / env)


def test_the_agents_own_ema_check():
    from slimdqn.networks._agent import EMA_REFUSED, check_ema_tau

    assert check_ema_tau(0) == 0.0 and check_ema_tau(0.0, supported=True) == 0.0 and check_ema_tau(0.25, supported=True) == 0.25
    with pytest.raises(ValueError) as e:
        check_ema_tau(0.005)
    assert str(e.value) == EMA_REFUSED
    for bad in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            check_ema_tau(bad, supported=True)


def test_the_other_agents_refuse_an_ema_target():
    """Before an engine is built: no GPU is needed to be refused."""
    from slimdqn.networks._agent import EMA_REFUSED
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    for cls in (iSDQN, AnalysisDQN):
        with pytest.raises(ValueError) as e:
            cls(0, (11,), 5, 2, [40, 24], False, False, "fc", 1e-3, 0.99, 1, 1, 8, batch_size=4, ema_tau=0.005)
        assert str(e.value) == EMA_REFUSED
    for cls in (TFDQN, AnalysisTFDQN):
        with pytest.raises(ValueError) as e:
            cls(0, (11,), 5, [40, 24], False, False, "fc", 1e-3, 0.99, 1, 1, 8, batch_size=4, ema_tau=0.005)
        assert str(e.value) == EMA_REFUSED


class _StubEnv:
    n_actions, state, observation = 2, None, np.zeros((2, 2), np.uint8)

    def __init__(self):
        self.n_steps = 0

    def reset(self):
        self.n_steps = 0

    def step(self, action):
        self.n_steps += 1
        return 0.0, False


class _StubReplay:
    _clipping = None

    def add(self, *a, **k):
        pass


class _StubAgent:
    data_to_update, target_update_frequency, params = 1, 8, None

    def __init__(self):
        self.calls = []

    def best_action(self, params, state, **kw):
        return 0

    def update_online_params(self, step, rb):
        pass

    def update_target_params(self, step):
        return (True, {"loss": 0.0}) if step % self.target_update_frequency == 0 else (False, {})

    def recycle_dormant(self, rb, tau):
        self.calls.append(("redo", tau))
        return [0]

    def reset_parameters(self, **kw):
        self.calls.append(("reset", kw))

    def get_model(self):
        return {}


@pytest.mark.parametrize("redo", [0, 8])
def test_trainer_resets_at_exact_multiples_behind_redo(tmp_path, redo):
    """-tuf 8, -reset 16 [-redo 8] over 60 steps with 10 initial samples: resets at steps 16, 32, 48 and nowhere else, with the flags'
    keywords, behind the recycle of the same step, and logs["reset"] = 1 on exactly those target updates."""
    from experiments.base.dqn import train
    from experiments.base.utils import _NullLogger

    p = dict(epsilon_end=0.1, epsilon_duration=10, n_epochs=1, n_training_steps_per_epoch=60, n_initial_samples=10, horizon=20,
             reset_frequency=16, reset_shrink=0.25, reset_top_layers=2, redo_frequency=redo, redo_tau=0.1, save_path=str(tmp_path / "out"), seed=1,
             wandb=_NullLogger())
    agent = _StubAgent()
    train(np.random.default_rng(0), p, agent, _StubEnv(), _StubReplay())
    updates = [h for h in p["wandb"].history if "loss" in h]
    assert [h["n_training_steps"] for h in updates] == [16, 24, 32, 40, 48, 56]
    assert [h["n_training_steps"] for h in updates if h.get("reset") == 1] == [16, 32, 48]
    assert all("reset" not in h for h in updates if h["n_training_steps"] % 16)
    resets = [c for c in agent.calls if c[0] == "reset"]
    assert resets == [("reset", dict(shrink=0.25, n_top_layers=2))] * 3
    if redo:
        kinds = [c[0] for c in agent.calls]
        assert kinds == ["redo", "reset", "redo", "redo", "reset", "redo", "redo", "reset", "redo"]  # steps 16, 24, 32, 40, 48, 56
    # without -reset nothing is called and nothing is logged
    p2 = dict(p, reset_frequency=0, wandb=_NullLogger(), save_path=str(tmp_path / "out2"))
    quiet = _StubAgent()
    train(np.random.default_rng(0), p2, quiet, _StubEnv(), _StubReplay())
    assert not [c for c in quiet.calls if c[0] == "reset"] and all("reset" not in h for h in p2["wandb"].history)


def test_reset_layout_of_the_three_torsos():
    """isdqn_net_reset_layout is host arithmetic on the plan: the cnn plan has three conv layers in front of its Dense layers, the
    impala torso is ONE entry of the layer list, fc starts with a Dense; and it agrees with what the tensor table says."""
    from slimdqn import _hip

    def numbers(lay):
        n, first = ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert lay.lib.isdqn_net_reset_layout(ctypes.byref(lay.cfg), ctypes.byref(n), ctypes.byref(first)) == _hip.OK
        assert lay.lib.isdqn_net_reset_layout(ctypes.byref(lay.cfg), None, None) == _hip.OK
        return n.value, first.value

    cnn = hredo.HostLayout((84, 84, 4), 5, 3, (8, 12, 16, 24), "cnn", True)
    imp = hredo.HostLayout((44, 44, 3), 5, 3, (8, 16, 16, 24), "impala", True)
    fc = hredo.HostLayout((11,), 5, 3, (40, 24), "fc", False)
    assert numbers(cnn) == (5, 3) and numbers(imp) == (3, 1) and numbers(fc) == (3, 0)
    for lay in (cnn, imp, fc):
        assert numbers(lay) == hr.layout_numbers(lay)
    assert {"isdqn_net_reset_layout", "isdqn_net_reset", "isdqn_net_ema"} <= set(_hip.PUBLIC_SYMBOLS)
    assert fc.lib.isdqn_net_reset_layout(None, None, None) == _hip.ERR_ARG


def test_the_c_abi_refuses_without_touching_a_device():
    """Every ISDQN_ERR_ARG of the two calls comes before any launch: stand-in pointers are never read."""
    from slimdqn import _hip

    lay = hredo.HostLayout((11,), 5, 3, (40, 24), "fc", True)
    lib, cfg, n = lay.lib, lay.cfg, lay.n_param_floats
    one, far = 1 << 20, 1 << 30  # stand for two buffers that do not overlap

    def reset(params=one, m=one + (1 << 24), v=one + (1 << 25), count=None, fresh=far, split=1, f=(0.5, 0.5, 0.0, 1.0)):
        return lib.isdqn_net_reset(ctypes.byref(cfg), params, m, v, count, fresh, split, *f, None, None)

    assert reset(params=None) == _hip.ERR_ARG and reset(fresh=None) == _hip.ERR_ARG
    assert reset(m=None) == _hip.ERR_ARG and "both" in _hip.last_error() and reset(v=None) == _hip.ERR_ARG
    for bad in (-0.5, float("nan"), float("inf")):
        for k in range(4):
            f = [0.5, 0.5, 0.0, 1.0]
            f[k] = bad
            assert reset(f=tuple(f)) == _hip.ERR_ARG, (bad, k)
    assert reset(split=-1) == _hip.ERR_ARG and reset(split=4) == _hip.ERR_ARG
    assert reset(fresh=one) == _hip.ERR_ARG and reset(fresh=one + 4 * (n - 1)) == _hip.ERR_ARG and reset(fresh=one - 4 * (n - 1)) == _hip.ERR_ARG
    assert "overlap" in _hip.last_error()

    def ema(target=one, online=far, tau=0.005):
        return lib.isdqn_net_ema(ctypes.byref(cfg), target, online, tau, None)

    assert ema(target=None) == _hip.ERR_ARG and ema(online=None) == _hip.ERR_ARG and ema(online=one) == _hip.ERR_ARG
    for tau in (-1e-3, 1.001, float("nan"), float("inf")):
        assert ema(tau=tau) == _hip.ERR_ARG, tau
    assert ema(tau=0.0) == _hip.OK  # launches nothing: the stand-in pointers are not touched
