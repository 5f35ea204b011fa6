"""Importance-sampling weights of prioritized replay, the parts that need no GPU: the float64 restatement against itself
(tests/helpers/per_weights.py), the layout of isdqn_batch with its new field, the argument checks of
isdqn_tree_query_weighted, the three command-line flags and the beta schedule."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import per_weights as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = (0.0, 0.4, 0.5, 1.0)


# ------------------------------------------------------------------ 1. the helper against itself
def test_explicit_n_and_r_form_equals_the_short_form():
    """(N p_i / R)^-beta / max_j (...) against (p_min / p_i)^beta: two pow, one division and beta times the three roundings of the
    argument (N p / R), i.e. within 8 float64 ulp; rounded to float32 the two never lie more than one float32 ulp apart."""
    rng = np.random.default_rng(20161116)
    worst, worst32 = 0.0, 0
    for trial in range(2000):
        n = int(rng.integers(1, 4097))
        leaves = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), n))
        N = int(np.exp(rng.uniform(np.log(2), np.log(1e6))))
        R = float(leaves.sum() * rng.uniform(1.0, 50.0))
        beta = BETAS[trial % 4]
        a, b = pw.weights(leaves, beta, n_keys=N, root=R), pw.weights_short(leaves, beta)
        ulp = np.abs(a - b) / np.spacing(b)
        worst = max(worst, float(ulp.max()))
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        steps = np.abs(a32.view(np.int32).astype(np.int64) - b32.view(np.int32).astype(np.int64))
        worst32 = max(worst32, int(steps.max()))
        assert a.max() == 1.0 and b.max() == 1.0
        if beta == 0.0:
            assert (a == 1.0).all() and (b == 1.0).all()
    print(f"worst distance: {worst} float64 ulp, {worst32} float32 ulp")
    assert worst <= 8.0, worst
    assert worst32 <= 1, worst32


def test_non_positive_leaves_stay_out_of_the_minimum():
    leaves = np.array([0.0, 2.0, 0.5, -0.0, 8.0])
    for f in (lambda l, b: pw.weights(l, b, n_keys=77, root=123.0), pw.weights_short):
        w = f(leaves, 0.5)
        assert w[0] == 1.0 and w[3] == 1.0 and w[2] == 1.0
        np.testing.assert_allclose(w[[1, 4]], [0.5, 0.25], rtol=1e-15)
        assert (f(np.zeros(7), 0.7) == 1.0).all()
    ones = pw.weighted_td(np.ones((4, 2)), np.zeros((4, 2)), np.ones(4))
    assert np.array_equal(ones["losses"], [1.0, 1.0]) and np.array_equal(ones["dq"], np.full((4, 2), 0.5))
    hub = pw.weighted_td(np.array([[3.0], [0.25]]), np.zeros((2, 1)), np.array([0.5, 1.0]), huber_delta=1.0)
    np.testing.assert_allclose(hub["dq"][:, 0], [0.5 * 1.0 / 2, 0.25 / 2])
    np.testing.assert_allclose(hub["losses"], [(0.5 * 2.5 + 0.5 * 0.0625) / 2])


# ------------------------------------------------------------------ 2. ABI layout
def test_batch_layout_matches_the_header(tmp_path):
    from slimdqn import _hip

    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "isdqn_hip.h"\n'
        "int main(void) {\n"
        '    printf("%zu %zu %zu\\n", sizeof(isdqn_batch), offsetof(isdqn_batch, loss_weights), offsetof(isdqn_batch, priorities_ready));\n'
        "    return 0;\n}\n"
    )
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses
    exe = tmp_path / "layout"
    subprocess.check_call([hipcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_w, off_ev = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == ctypes.sizeof(_hip.Batch)
    assert off_w == _hip.Batch.loss_weights.offset
    assert off_ev == _hip.Batch.priorities_ready.offset
    assert off_w + ctypes.sizeof(ctypes.c_void_p) == size  # the trailing field
    assert _hip.Batch().loss_weights is None  # a batch built without it carries NULL: weight 1


# ------------------------------------------------------------------ 3. argument checks in front of the launch
@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


def test_tree_query_weighted_argument_errors_without_a_device(lib):
    from slimdqn import _hip

    assert "isdqn_tree_query_weighted" in _hip.PUBLIC_SYMBOLS
    x = 0x1000  # any non-null value: the checks come before anything is dereferenced or launched
    ok = dict(nodes=x, depth=5, targets=x, n=8, unit=1, beta=x, out=x, leaf=None, w=x, status=x, stream=None)

    def call(**kw):
        a = {**ok, **kw}
        return lib.isdqn_tree_query_weighted(a["nodes"], a["depth"], a["targets"], a["n"], a["unit"], a["beta"], a["out"], a["leaf"], a["w"],
                                             a["status"], a["stream"])

    for name in ("nodes", "targets", "beta", "out", "w", "status"):
        assert call(**{name: None}) == _hip.ERR_ARG, name
    assert call(depth=0) == _hip.ERR_ARG and call(depth=31) == _hip.ERR_ARG
    assert call(n=_hip.TREE_MAX_BATCH + 1) == _hip.ERR_SHAPE
    assert call(n=-1) == _hip.ERR_SHAPE
    assert call(n=0) == _hip.OK          # nothing to do: no launch
    assert call(n=0, leaf=None) == _hip.OK
    assert b"0.2" in lib.isdqn_version()


# ------------------------------------------------------------------ 4. flags and the beta schedule
def _parse(argv):
    import argparse

    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    pa.add_isdqn_arguments(parser)
    names = pa.add_engine_arguments(parser)
    return vars(parser.parse_args(["-en", "x_Game", "-s", "1"] + argv)), names


def test_flags_and_defaults(tmp_path, monkeypatch):
    from experiments.atari import common
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    p, names = _parse([])
    assert {"priority_exponent", "is_beta", "is_beta_end"} <= set(names)
    assert p["priority_exponent"] == 1.0 and p["is_beta"] == 0.0 and p["is_beta_end"] is None
    p, _ = _parse(["-per", "-pe", "0.6", "-isb", "0.4", "-isbe", "1.0"])
    assert (p["priority_exponent"], p["is_beta"], p["is_beta_end"]) == (0.6, 0.4, 1.0)
    p, _ = _parse(["--prioritized", "--priority_exponent", "0.5", "--is_beta", "0.25", "--is_beta_end", "0.75"])
    assert (p["priority_exponent"], p["is_beta"], p["is_beta_end"]) == (0.5, 0.25, 0.75)
    for short, long, kw in pa._ENGINE:
        if long in ("--priority_exponent", "--is_beta", "--is_beta_end"):
            assert "-per" in kw["help"]  # they mean nothing without it, and say so

    # a default run builds the sampler with alpha 1.0 and leaves importance sampling off
    built = []

    class FakeSampler:
        def __init__(self, seed, max_capacity, priority_exponent=1.0, device=None):
            built.append(priority_exponent)

    monkeypatch.setattr(common, "PrioritizedSamplingDistribution", FakeSampler)
    monkeypatch.setattr(common, "ReplayBuffer", lambda **kw: kw["sampling_distribution"])
    base = ["-en", "flags_Game", "-dw"]
    p = prepare_logs("atari", "isdqn", base + ["-s", "1", "-per"], root=str(tmp_path))
    common.make_replay(p, prioritized=True)
    p2 = prepare_logs("atari", "isdqn", ["-en", "flags2_Game", "-dw", "-s", "1", "-per", "-pe", "0.6", "-isb", "0.4"], root=str(tmp_path))
    common.make_replay(p2, prioritized=True)
    assert built == [1.0, 0.6]

    class FakeAgent:
        calls = []

        def set_importance_sampling(self, *a, **kw):
            self.calls.append((a, kw))

    class FakeReplay:
        _sampling_distribution = FakeSampler(0, 1)

        def add(self, *a, **kw):
            pass

    from experiments.atari import analysisdqn, isdqn

    for mod in (isdqn, analysisdqn):
        FakeAgent.calls = []
        agent = FakeAgent()
        mod._wire_prioritized(agent, FakeReplay(), p)
        assert agent.priority_writeback and agent.calls == []  # default: off
        mod._wire_prioritized(agent, FakeReplay(), p2)
        assert agent.calls == [((0.4, None), dict(n_steps=pa.n_gradient_steps(p2)))]
    assert pa.n_gradient_steps(dict(n_epochs=2, n_training_steps_per_epoch=60, n_initial_samples=20, data_to_update=4)) == 25

    with pytest.raises(ValueError):  # -isb weighs prioritized samples
        prepare_logs("atari", "isdqn", ["-en", "flags3_Game", "-dw", "-s", "1", "-isb", "0.4"], root=str(tmp_path))


def test_parameters_json_holds_the_prioritized_flags_only_under_per(tmp_path):
    import json

    from experiments.base.utils import prepare_logs

    prepare_logs("atari", "isdqn", ["-en", "a_Game", "-dw", "-s", "1"], root=str(tmp_path))
    plain = json.load(open(tmp_path / "atari" / "exp_output" / "a_Game" / "parameters.json"))
    assert "is_beta" not in plain["isdqn"] and "priority_exponent" not in plain["isdqn"]
    prepare_logs("atari", "isdqn", ["-en", "b_Game", "-dw", "-s", "1", "-per", "-pe", "0.6", "-isb", "0.4", "-isbe", "1.0"], root=str(tmp_path))
    per = json.load(open(tmp_path / "atari" / "exp_output" / "b_Game" / "parameters.json"))
    assert (per["isdqn"]["priority_exponent"], per["isdqn"]["is_beta"], per["isdqn"]["is_beta_end"]) == (0.6, 0.4, 1.0)


def test_beta_schedule():
    from slimdqn.networks._agent import EngineAgent, importance_beta

    f32 = np.float32
    assert importance_beta(0.4, 1.0, 1000, 0) == f32(0.4) and importance_beta(0.4, 1.0, 1000, 1000) == f32(1.0)  # endpoints exact
    assert importance_beta(0.4, 1.0, 1000, 5000) == f32(1.0)  # constant past n_steps
    assert importance_beta(0.4, None, 1000, 123) == f32(0.4) and importance_beta(0.4, None, 0, 10**9) == f32(0.4)
    assert importance_beta(0.4, 1.0, 0, 0) == f32(1.0)
    for t in range(0, 1001, 7):
        want = f32(np.float64(0.4) + (np.float64(1.0) - np.float64(0.4)) * (t / 1000.0))
        got = importance_beta(0.4, 1.0, 1000, t)
        assert got.dtype == np.float32 and got == want
    vals = [float(importance_beta(0.4, 1.0, 1000, t)) for t in range(1001)]
    assert all(b >= a for a, b in zip(vals, vals[1:]))
    assert abs(vals[500] - 0.7) < 1e-7

    class Bare(EngineAgent):
        def _drop_graph(self):
            self.dropped = True

    a = Bare()
    assert not a.importance_sampling and a._next_betas(3) is None
    a.set_importance_sampling(0.5, 1.0, n_steps=4)
    assert a.importance_sampling and a.dropped
    assert np.array_equal(a._next_betas(1), f32([0.5]))
    assert np.array_equal(a._next_betas(4), f32([0.625, 0.75, 0.875, 1.0]))  # a captured replay of 4 steps continues the count
    assert np.array_equal(a._next_betas(2), f32([1.0, 1.0]))
