"""Host side of the conservative (CQL) term and of offline training: the float64 restatement of tests/helpers/conservative.py against
torch autograd (and against three wrong variants it must be able to tell apart), the ctypes layout of the struct that carries the
weight against the C compiler's, flag and setter refusals, where the new source and the new messages live, and the transition log's
round trip through the host replay.  The device side is tests/test_gpu_conservative.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import conservative as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = [("atari", a) for a in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn")] + [("lunar_lander", a) for a in ("isdqn", "dqn", "tfdqn")]
ALPHA = 0.7


# ---------------------------------------------------------------------------------------------------------------- (a) the restatement
def _case(kind, seed=0):
    rng = np.random.default_rng(seed)
    B, K, A = 6, 3, 5
    W = {"scalar": 1, "quantile": 7, "histogram": 9}[kind]
    rows = rng.normal(size=(B, K, A, W)) * 1.5
    action, w = rng.integers(0, A, B), rng.uniform(0.0, 2.0, B)
    w[0] = 0.0
    z = hc.support(W, -3.0, 4.0) if kind == "histogram" else None
    return rows, action, w, z


def _autograd(rows, action, w, z, kind):
    """d/d(rows) of sum_k alpha mean_b w_b c_bk, and c, in torch float64."""
    t = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
    q = t[..., 0] if kind == "scalar" else t.mean(-1) if kind == "quantile" else (torch.softmax(t, -1) * torch.tensor(z)).sum(-1)
    B, K, A = q.shape
    qa = q.gather(2, torch.tensor(action)[:, None, None].expand(B, K, 1))[..., 0]
    c = torch.logsumexp(q, -1) - qa
    per_head = ALPHA * (torch.tensor(w)[:, None] * c).mean(0)
    per_head.sum().backward()
    return t.grad.numpy(), c.detach().numpy(), per_head.detach().numpy()


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("kind", hc.KINDS)
def test_restatement_is_the_autograd_gradient(kind):
    rows, action, w, z = _case(kind)
    grad, c, loss = _autograd(rows, action, w, z, kind)
    r = hc.restate(rows, action, w, ALPHA, kind, z)
    assert _rel(r["dout"], grad) < 1e-10 and _rel(r["c"], c) < 1e-10 and _rel(r["loss"], loss) < 1e-10
    assert _rel(r["dbh"], grad.sum(0)) < 1e-10
    assert (r["c"] >= 0).all()  # logsumexp dominates every action value
    assert not r["dout"][0].any()  # the row of weight 0


@pytest.mark.parametrize("kind,wrong", [("quantile", "no_inv_n"), ("histogram", "no_centre"), ("scalar", "no_indicator"), ("quantile", "no_indicator"),
                                        ("histogram", "no_indicator")])
def test_wrong_variants_fail_the_same_check(kind, wrong):
    rows, action, w, z = _case(kind, 1)
    grad, _, _ = _autograd(rows, action, w, z, kind)
    assert _rel(hc.restate(rows, action, w, ALPHA, kind, z)["dout"], grad) < 1e-10
    assert _rel(hc.restate(rows, action, w, ALPHA, kind, z, wrong=wrong)["dout"], grad) > 1e-2


# ---------------------------------------------------------------------------------------------------------------- (b) the ABI
def test_batch_conservative_layout_is_the_c_compilers(tmp_path):
    from slimdqn import _hip

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses, here as a host C compiler
    exe = str(tmp_path / "batch_conservative_layout")
    subprocess.run([hipcc, "-x", "c", "-std=c11", "-O0", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "helpers", "batch_conservative_layout.c"), "-o", exe], check=True)
    c = {k: int(v) for k, v in (line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())}
    S = _hip.BatchConservative
    import ctypes

    assert ctypes.sizeof(S) == c["sizeof"] and ctypes.sizeof(_hip.Batch) == c["sizeof_batch"] and ctypes.sizeof(_hip.BatchDecay) == c["sizeof_decay"]
    for name in ("flags", "loss_weights", "discount", "weight_decay", "decay_kinds", "cql_alpha", "reserved"):
        assert getattr(S, name).offset == c[name], name
    assert S.cql_alpha.offset == c["sizeof_decay"] and c["sizeof"] == c["sizeof_decay"] + 8
    assert (_hip.BATCH_CONSERVATIVE, _hip.BATCH_WEIGHT_DECAY) == (c["ISDQN_BATCH_CONSERVATIVE"], c["ISDQN_BATCH_WEIGHT_DECAY"]) == (8, 4)
    assert len({_hip.BATCH_MIRROR_CURRENT, _hip.BATCH_DISCOUNT, _hip.BATCH_WEIGHT_DECAY, _hip.BATCH_CONSERVATIVE}) == 4


# ---------------------------------------------------------------------------------------------------------------- (c) refusals and routing
BASE = ["-s", "1", "-dw", "-f", "8", "8", "8", "16", "-at", "cnn", "-tuf", "16", "-ln"]


def _argv(env, name, extra):
    return ["-en", name] + (BASE if env == "atari" else ["-s", "1", "-dw", "-f", "20", "14", "-at", "fc", "-tuf", "16", "-ln"]) + extra


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_flags_parse_and_stay_out_of_parameters_json(tmp_path, env, algo):
    import json

    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    p = prepare_logs(env, algo, _argv(env, "cql_Synthetic", ["-cql", "1.5", "-logrb", str(tmp_path / "log")]), root=str(tmp_path))
    assert p["cql_alpha"] == 1.5 and pa.conservative_kwargs(p) == dict(cql_alpha=1.5) and p["log_replay"] == str(tmp_path / "log")
    assert p["offline_dir"] is None and p["evaluation_steps"] == 0
    stored = json.load(open(tmp_path / env / "exp_output" / "cql_Synthetic" / "parameters.json"))
    for section in stored.values():
        assert not {"cql_alpha", "log_replay", "offline_dir", "evaluation_steps"} & set(section)
    q = prepare_logs(env, algo, _argv(env, "plain_Synthetic", []), root=str(tmp_path))
    assert q["cql_alpha"] == 0.0 and pa.conservative_kwargs(q) == {}
    text = open(os.path.join(ROOT, "is-dqn_amd", "experiments", env, algo + ".py")).read()
    assert text.count("**conservative_kwargs(p),") == 1 and text.count("environment_for(p, make_environment)") == 1


def _refusals():
    from experiments.base import offline
    from slimdqn import _conservative

    return [(["-cql", "-0.5"], _conservative.CQL_ALPHA_REFUSED), (["-cql", "nan"], _conservative.CQL_ALPHA_REFUSED),
            (["-cql", "inf"], _conservative.CQL_ALPHA_REFUSED), (["-logrb", "somewhere", "-nenvs", "2"], offline.LOGRB_VECTOR_REFUSED),
            (["-offline", "somewhere", "-utd", "2"], offline.OFFLINE_UTD_REFUSED), (["-offline", "somewhere", "-logrb", "elsewhere"], offline.OFFLINE_LOGRB_REFUSED),
            (["-evals", "10"], offline.EVALS_REFUSED), (["-offline", "somewhere", "-evals", "-1"], offline.EVALS_REFUSED)]


@pytest.mark.parametrize("env,algo", [("atari", "dqn"), ("lunar_lander", "isdqn")])
def test_refusals_come_before_anything_is_written(tmp_path, env, algo):
    from experiments.base.utils import prepare_logs

    for extra, message in _refusals():
        with pytest.raises(ValueError) as e:
            prepare_logs(env, algo, _argv(env, "bad_Synthetic", extra), root=str(tmp_path))
        assert str(e.value) == message, extra
    assert not os.path.exists(tmp_path / env)


def test_setter_refusals_and_where_the_messages_live():
    from slimdqn import _conservative, _engine
    from slimdqn._engine import QNetEngine

    assert _engine._conservative is _conservative and not hasattr(_engine, "CQL_ALPHA_REFUSED")
    text = open(os.path.join(ROOT, "is-dqn_amd", "slimdqn", "_engine.py")).read()
    assert len(re.findall(r"^[A-Z_]*(?:REFUSED|NEEDS)[A-Z_]* = ", text, re.M)) == 22  # (tests/test_options_snapshot_host.py pins the count)
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError) as e:
            _conservative.check_cql_alpha(bad)
        assert str(e.value) == _conservative.CQL_ALPHA_REFUSED
    assert _conservative.check_cql_alpha(0) == 0.0 and _conservative.check_cql_alpha("1.5") == 1.5
    assert QNetEngine.cql_alpha == 0.0 and callable(QNetEngine.set_conservative)


def test_the_kernels_live_in_a_source_of_their_own():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES == ["api.hip", "tree_kernels.hip", "replay_kernels.hip", "net_kernels.hip"]
    assert build.EXTRA_SOURCES == ["conservative_kernels.hip"]
    asm = build.emit_asm()
    assert [os.path.basename(a) for a in asm] == [s.replace(".hip", ".s") for s in build.SOURCES + build.EXTRA_SOURCES]
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(asm[-1]).read(), re.M)
    assert len(kernels) == 3 and all("cql_" in k for k in kernels), kernels
    for other in asm[:-1]:
        assert "cql_" not in open(other).read()
    assert "__global__" not in open(os.path.join(build.CSRC, "conservative.h")).read()


# ---------------------------------------------------------------------------------------------------------------- (d) log and offline
def _stream(n_steps, seed=3):
    rng = np.random.default_rng(seed)
    for _ in range(n_steps):
        terminal = bool(rng.random() < 0.06)
        yield (rng.integers(0, 256, (6, 5), dtype=np.uint8), int(rng.integers(0, 5)), float(rng.normal()), terminal, terminal or bool(rng.random() < 0.05))


def _host_replay(n, capacity=400):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    return ReplayBuffer(UniformSamplingDistribution(0, device="cpu"), 8, capacity, stack_size=4, update_horizon=n, gamma=0.9, device="cpu")


@pytest.mark.parametrize("n", [1, 3])
def test_log_then_fill_is_feeding_the_replay_directly(tmp_path, n):
    """A 300-step stream with terminals and truncations: direct rb.add; the same stream through a logging replay (-logrb) into shards of
    128; fill_replay of a third replay from those shards.  The three element tables are equal."""
    from experiments.base import offline
    from slimdqn.sample_collection.replay_buffer import TransitionElement

    direct, logged, filled = _host_replay(n), _host_replay(n), _host_replay(n)
    log = offline.TransitionLog(tmp_path / "log", shard_size=128, n_actions=5)
    offline.log_replay_adds(logged, log)
    stream = list(_stream(300))
    assert sum(t[3] for t in stream) >= 5 and sum(t[4] and not t[3] for t in stream) >= 5
    for t in stream:
        direct.add(TransitionElement(*t))
        logged.add(TransitionElement(*t))
    log.close()
    assert [os.path.basename(s) for s in offline.shard_paths(tmp_path / "log")] == ["shard_000000.npz", "shard_000001.npz", "shard_000002.npz"]
    with np.load(offline.shard_paths(tmp_path / "log")[2]) as shard:
        assert shard["observation"].shape == (44, 6, 5) and shard["observation"].dtype == np.uint8 and shard["action"].dtype == np.int32
        assert shard["reward"].dtype == np.float32 and shard["terminal"].dtype == np.uint8 and shard["episode_end"].dtype == np.uint8
    assert offline.dataset_size(tmp_path / "log") == 300 and offline.fill_replay(filled, tmp_path / "log") == 300
    shapes = offline.DatasetShapes(tmp_path / "log")
    assert (shapes.n_actions, shapes.state_height, shapes.state_width, shapes.n_stacked_frames) == (5, 6, 5, 4)
    assert direct.add_count == logged.add_count == filled.add_count > 250
    C = direct.add_count
    for other in (logged, filled):
        for table in ("_h_elem_frames", "_h_elem_action", "_h_elem_terminal"):
            np.testing.assert_array_equal(getattr(other, table)[:C], getattr(direct, table)[:C], err_msg=table)
        # (rewards went through float32 in the shards: the stream's are float64 draws)
        np.testing.assert_allclose(other._h_elem_reward64[:C], direct._h_elem_reward64[:C], rtol=0 if other is logged else 1e-6, atol=0 if other is logged else 1e-7)
    small = _host_replay(n, capacity=100)
    with pytest.raises(ValueError, match="more than the replay's capacity"):
        offline.fill_replay(small, tmp_path / "log")
    assert small.add_count == 0


def test_float_observations_round_trip(tmp_path):
    from experiments.base import offline

    log = offline.TransitionLog(tmp_path / "log", shard_size=50)
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(70, 8)).astype(np.float32)
    for i in range(70):
        log.append(obs[i], i % 4, 0.5 * i, i % 17 == 16, i % 17 == 16 or i % 23 == 22)
    log.close()
    got = np.concatenate([np.load(s)["observation"] for s in offline.shard_paths(tmp_path / "log")])
    assert got.dtype == np.float32 and np.array_equal(got, obs)
    shapes = offline.DatasetShapes(tmp_path / "log")
    assert shapes.observation_shape == (8,) and shapes.n_actions == 4  # (no n_actions in the log: the largest action taken)
