"""Host side of AdamW's decoupled weight decay (include/isdqn_hip.h, isdqn_batch_decay), no GPU: the numpy restatement of
tests/helpers/adamw.py against hand-written numbers and against torch.optim.AdamW in float64, the kind mask, the flags with their
refusals on all eight entry points, what the agents hand to every engine they build, and the ctypes layout of the struct that carries
the decay against the C compiler's.  The device side is tests/test_gpu_adamw.py."""
import ctypes
import json
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from tests.helpers import adamw as hw

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = [("atari", a) for a in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn")] + [("lunar_lander", a) for a in ("isdqn", "dqn", "tfdqn")]


# ------------------------------------------------------------------ the restatement
def test_the_three_roundings_on_hand_written_numbers():
    lr, wd = F32(1e-3), F32(0.1)
    p0 = np.array([1.0, -2.0, 0.0, -0.0, 3.0e-39, 1.0e30], F32)
    p1 = np.array([0.5, -2.5, 0.0, -0.0, 3.0e-39, 1.0e30], F32)
    got = hw.decay32(p1, p0, lr, wd)
    want = np.array([F32(p1[i]) - F32(lr * F32(wd * p0[i])) for i in range(p0.size)], F32)  # scalar float32 arithmetic, one rounding each
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert got[0] == F32(0.5) - F32(F32(1e-3) * F32(0.1)) and got[0] < 0.5
    # zeros keep their sign bit patterns as the definition says: +0 - (+0) = +0, and -0 - lr * (-0) = -0 - (-0) = +0 is NOT -0 - (+0) = -0
    assert got[2].view(np.int32) == 0
    assert hw.decay32(F32(-0.0), F32(0.0), lr, wd).view(np.int32) == F32(-0.0).view(np.int32)
    assert hw.decay32(F32(-0.0), F32(-0.0), lr, wd).view(np.int32) == 0
    # it is not the once-rounded form: where p1 does not hide the term (p1 = 0), the two roundings of the products show
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=4096).astype(F32), rng.normal(size=4096).astype(F32)
    once = (-float(lr) * float(wd) * a.astype(np.float64)).astype(F32)
    assert np.count_nonzero(hw.decay32(np.zeros_like(a), a, lr, wd) != once) > 100
    # wd = 0 in the restatement subtracts +-0: the values are p1's (the kernels do not even run the subtraction: tests/test_gpu_adamw.py)
    assert np.array_equal(hw.decay32(b, a, lr, 0.0), b)


def test_the_kind_mask():
    info = lambda off, size, kind: types.SimpleNamespace(offset=off, size=size, kind=kind)
    infos = [info(0, 4, 0), info(4, 2, 2), info(6, 4, 1), info(10, 2, 3), info(12, 2, 4), info(14, 2, 5), info(16, 2, 6), info(18, 2, 7), info(20, 2, 8)]
    kernels = hw.decay_mask(infos, 22, hw.KINDS_KERNELS)
    assert kernels.tolist() == [True] * 4 + [False] * 2 + [True] * 4 + [False] * 12
    everything = hw.decay_mask(infos, 22, hw.KINDS_ALL)
    assert everything[:18].all() and not everything[18:].any()  # the running statistics (kinds 7, 8) never
    assert not hw.decay_mask(infos, 22, 0).any()
    from slimdqn import _hip, _optimizer

    assert (_hip.DECAY_KINDS_KERNELS, _hip.DECAY_KINDS_ALL) == (hw.KINDS_KERNELS, hw.KINDS_ALL) == (0x03, 0x7F)
    assert _optimizer.decay_kinds() == 0x03 and _optimizer.decay_kinds(True) == 0x7F and _hip.BATCH_WEIGHT_DECAY == 4


@pytest.mark.parametrize("eps", [1.5e-4, 1e-8])
@pytest.mark.parametrize("wd", [0.1, 0.0])
def test_float64_step_against_torch_adamw(wd, eps):
    """Ten steps of adamw64 against torch.optim.AdamW on CPU in float64, random gradients, the same b1, b2.  Both sides are float64 and
    differ by operation order only (torch: p *= 1 - lr wd, then p -= (lr / c1) m / (sqrt(v) / sqrt(c2) + eps); here optax's
    p - lr (m_hat / (sqrt(v_hat) + eps) + wd p)).  The bound, with e = 2^-53:
      * a side goes from (p, m, v, g) to the new p in at most 8 rounded operations, each within e of a quantity that is at most
        S = |p| + lr U, U = (M / c1) / den with M = b1 M' + (1 - b1) |g| the magnitude sum behind m (M >= |m|: what a rounding of m is
        relative to when its two terms cancel): 16 e S per step for the two sides;
      * the moments themselves differ: m by at most 3 e M and v by at most 4 e v per step taken, accumulating linearly, so in step j by
        3 j e and 4 j e; they enter the step lr u to first order with factors 1 and 1/2 (the square root): 5 j e lr U <= 5 j e S;
      * so step j adds (16 + 5 j) e S, and after k steps the two parameters differ by at most (16 k + 5 k (k + 1) / 2) e S_max, S_max the
        largest S of the steps so far, element by element.  k = 10: 435 e S_max ~ 4.8e-14 S_max."""
    rng = np.random.default_rng(5)
    n, lr = 257, 1e-3
    p = rng.normal(size=n)
    m, v = np.zeros(n), np.zeros(n)
    tp = torch.tensor(p.copy(), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(hw.B1, hw.B2), eps=eps, weight_decay=wd)
    e = 2.0**-53
    M, s_max = np.zeros(n), np.zeros(n)
    for k in range(1, 11):
        g = rng.normal(size=n) * 10.0 ** rng.integers(-6, 2, size=n)
        tp.grad = torch.tensor(g.copy(), dtype=torch.float64)
        opt.step()
        p, m, v = hw.adamw64(p, m, v, g, k, lr, eps, wd)
        M = hw.B1 * M + (1 - hw.B1) * np.abs(g)
        U = (M / (1.0 - hw.B1**k)) / (np.sqrt(v / (1.0 - hw.B2**k)) + eps)
        s_max = np.maximum(s_max, np.abs(p) + lr * U)
        bound = (16 * k + 5 * k * (k + 1) / 2) * e * s_max
        d = np.abs(tp.detach().numpy() - p)
        i = int(np.argmax(d / bound))
        print(f"wd={wd} eps={eps} step {k}: max |d| / bound = {d[i] / bound[i]:.3f}")
        assert d[i] <= bound[i], (k, i, d[i], bound[i])
    if wd:  # and the decay is really in it: without it the parameters are somewhere else
        q = rng.normal(size=3)
        assert np.all(hw.adamw64(q, 0 * q, 0 * q, q, 1, lr, eps, wd)[0] != hw.adamw64(q, 0 * q, 0 * q, q, 1, lr, eps, 0.0)[0])


# ------------------------------------------------------------------ flags
def _base(env):
    return ["-en", "adamw_Synthetic", "-s", "1", "-dw", "-tuf", "16"] + (["-f", "8", "8", "8", "16", "-at", "cnn"] if env == "atari" else [])


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_flags_parse_and_stay_out_of_parameters_json(tmp_path, env, algo):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    p = prepare_logs(env, algo, _base(env), root=str(tmp_path))
    assert (p["weight_decay"], p["weight_decay_all"]) == (0.0, False)
    assert pa.weight_decay_kwargs(p) == {}  # no flag: no agent keyword
    p = prepare_logs(env, algo, _base(env) + ["-s", "2", "-wdall"], root=str(tmp_path))
    assert p["weight_decay_all"] is True and pa.weight_decay_kwargs(p) == {}  # -wdall without -wd changes nothing
    p = prepare_logs(env, algo, _base(env) + ["-s", "3", "-wd", "0.1"], root=str(tmp_path))
    assert pa.weight_decay_kwargs(p) == dict(weight_decay=0.1, weight_decay_all=False)
    p = prepare_logs(env, algo, _base(env) + ["-s", "4", "--weight_decay", "0.05", "--weight_decay_all"], root=str(tmp_path))
    assert pa.weight_decay_kwargs(p) == dict(weight_decay=0.05, weight_decay_all=True)
    stored = json.load(open(tmp_path / env / "exp_output" / "adamw_Synthetic" / "parameters.json"))
    assert not any("weight_decay" in k for section in stored.values() for k in section)


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
@pytest.mark.parametrize("extra,message", [
    (["-wd", "-1"], "WEIGHT_DECAY_REFUSED"),
    (["-wd", "nan"], "WEIGHT_DECAY_REFUSED"),
    (["-wd", "inf"], "WEIGHT_DECAY_REFUSED"),
    (["-wd", "0.1", "-noisy"], "WEIGHT_DECAY_NOISY_REFUSED"),
])
def test_refusals_come_before_anything_is_written(tmp_path, env, algo, extra, message):
    from experiments.base.utils import prepare_logs
    from slimdqn import _optimizer

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, _base(env) + extra, root=str(tmp_path))
    assert str(e.value) == getattr(_optimizer, message)
    assert not os.path.exists(tmp_path / env)


def test_every_entry_point_hands_the_keywords_to_its_agent():
    for env, algo in ENTRY_POINTS:
        text = open(os.path.join(ROOT, "is-dqn_amd", "experiments", env, algo + ".py")).read()
        assert text.count("**weight_decay_kwargs(p),") == 1, (env, algo)


# ------------------------------------------------------------------ agents
class _StubEngine:
    """Stands where QNetEngine stands: records what the agent asks of every engine it builds."""

    built = []

    def __init__(self, *args, **kwargs):
        self.batch_size = args[6]
        self.noisy = kwargs.get("noisy", False)
        self.params, self.adam_m, self.adam_v = (torch.zeros(8) for _ in range(3))
        self.adam_count = torch.zeros(1, dtype=torch.int32)
        self.trust_mirror = False
        self.decay_calls = []
        _StubEngine.built.append(self)

    def init_params(self, seed):
        pass

    def copy_state_from(self, old):
        pass

    def set_weight_decay(self, weight_decay, all_kinds=False):
        self.decay_calls.append((weight_decay, all_kinds))


def _build(cls_name, **kw):
    from unittest import mock

    from slimdqn.networks import _agent
    from tests.helpers import options_grid as og

    _StubEngine.built = []
    with mock.patch.object(_agent, "QNetEngine", _StubEngine):
        agent = og.build_agent(cls_name, "fc", kw)
        agent._engine_for(og.BATCH + 1)  # a batch of another size arrives: the agent builds a second engine
    return agent, list(_StubEngine.built)


@pytest.mark.parametrize("cls_name", ["iSDQN", "DQN", "TFDQN", "AnalysisDQN", "AnalysisTFDQN"])
def test_agents_set_the_decay_on_every_engine_they_build(cls_name):
    from slimdqn import _optimizer

    agent, engines = _build(cls_name)
    assert len(engines) == 2 and all(e.decay_calls == [] for e in engines) and agent.weight_decay == 0.0  # off: the engines never hear of it
    agent, engines = _build(cls_name, weight_decay=0.1)
    assert len(engines) == 2 and all(e.decay_calls == [(0.1, False)] for e in engines)
    agent, engines = _build(cls_name, weight_decay=0.25, weight_decay_all=True)
    assert all(e.decay_calls == [(0.25, True)] for e in engines)
    _, engines = _build(cls_name, weight_decay_all=True)
    assert all(e.decay_calls == [] for e in engines)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError) as e:
            _build(cls_name, weight_decay=bad)
        assert str(e.value) == _optimizer.WEIGHT_DECAY_REFUSED and _StubEngine.built == []
    with pytest.raises(ValueError) as e:
        _build(cls_name, weight_decay=0.1, noisy=True)
    assert str(e.value) == _optimizer.WEIGHT_DECAY_NOISY_REFUSED and _StubEngine.built == []  # before anything is built
    import inspect

    from tests.helpers import options_grid as og

    cls = og._agent_classes()[cls_name]
    owner = next(c for c in cls.__mro__ if "weight_decay" in inspect.signature(c.__init__).parameters)  # (the analysis agents take **kwargs)
    params = inspect.signature(owner.__init__).parameters
    assert params["weight_decay"].kind is params["weight_decay_all"].kind is inspect.Parameter.KEYWORD_ONLY
    assert (params["weight_decay"].default, params["weight_decay_all"].default) == (0.0, False)


def test_the_engines_messages_live_outside_the_engine_module():
    from slimdqn import _engine, _optimizer

    assert _engine._optimizer is _optimizer and not hasattr(_engine, "WEIGHT_DECAY_REFUSED")
    assert _optimizer.check_weight_decay(0) == 0.0 and _optimizer.check_weight_decay("0.1") == 0.1
    assert _optimizer.check_weight_decay(0.0, noisy=True) == 0.0  # off is off, noisy or not


# ------------------------------------------------------------------ the struct
def test_batch_decay_layout_is_the_c_compilers(tmp_path):
    from slimdqn import _hip

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses, here as a host C compiler
    exe = str(tmp_path / "batch_decay_layout")
    subprocess.run([hipcc, "-x", "c", "-std=c11", "-O0", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "helpers", "batch_decay_layout.c"), "-o", exe], check=True)
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    c = {k: int(v) for k, v in out.items()}
    B = _hip.BatchDecay
    assert ctypes.sizeof(B) == c["sizeof"] and ctypes.sizeof(_hip.Batch) == c["sizeof_batch"] and ctypes.sizeof(_hip.BatchDiscount) == c["sizeof_discount"]
    for field in ("flags", "loss_weights", "discount", "weight_decay", "decay_kinds"):
        assert getattr(B, field).offset == c[field], field
    assert B.weight_decay.size == 4 and B.decay_kinds.size == 4
    assert (_hip.BATCH_WEIGHT_DECAY, _hip.DECAY_KINDS_KERNELS, _hip.DECAY_KINDS_ALL) == (
        c["ISDQN_BATCH_WEIGHT_DECAY"], c["ISDQN_DECAY_KINDS_KERNELS"], c["ISDQN_DECAY_KINDS_ALL"])
    # a BatchDecay IS a batch for every entry point: the batch sits at offset 0 and byref() of the whole hands &x.base.batch
    assert B.B.offset == 0 and issubclass(B, _hip.BatchDiscount) and issubclass(_hip.BatchDiscount, _hip.Batch)
