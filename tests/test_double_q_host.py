"""Double Q-learning targets (include/isdqn_hip.h, isdqn_net_config::double_q), host side: the float64 restatement of
tests/helpers/double_q.py against a plain loop, the tie rule, the single-head identity with the max form, the configuration struct,
the workspace plan, the flag and the agents that refuse it.  No GPU."""
import argparse
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))

from tests.helpers import double_q as dq
from tests.helpers import hl_gauss as hl
from tests.helpers import per_weights as pw


def _rows(seed, B, heads, A, scale=1.0):
    rng = np.random.default_rng(seed)
    rows = rng.normal(size=(2 * B, heads * A)) * scale
    action = rng.integers(0, A, B)
    reward = rng.normal(size=B)
    terminal = (rng.random(B) < 0.3).astype(np.uint8)
    terminal[0], terminal[1] = 1, 0  # both kinds in every batch
    return rows, action, reward, terminal


# ------------------------------------------------------------------ 1. the helper
@pytest.mark.parametrize("value_rows", [False, True])
@pytest.mark.parametrize("shape", [(11, 4, 5, 3, 1, 0), (6, 10, 9, 9, 1, 0), (7, 3, 4, 1, 2, 1), (5, 1, 6, 1, 0, 0)])
def test_helper_equals_a_plain_triple_loop(shape, value_rows):
    B, heads, A, K, on0, tg0 = shape
    rows, action, reward, terminal = _rows(3, B, heads, A)
    vr = np.random.default_rng(9).normal(size=(B, heads * A)) if value_rows else None
    got = dq.double_q(rows, action, reward, terminal, 0.97, K, on0, tg0, A, value_rows=vr)
    a_star, tg = dq.triple_loop(rows, action, reward, terminal, 0.97, K, on0, tg0, A, value_rows=vr)
    assert np.array_equal(got["a_star"], a_star)
    assert np.array_equal(got["targets"], tg)  # the same float64 operations in the same order
    # everything behind the target is the existing loss on these targets
    q = np.stack([rows[np.arange(B), (on0 + k) * A + action] for k in range(K)], axis=1)
    assert np.array_equal(got["q"], q)
    ref = pw.weighted_td(q, tg, np.ones(B))
    np.testing.assert_allclose(got["losses"], ref["losses"], rtol=1e-14)
    np.testing.assert_allclose(got["priorities"], np.sqrt(((q - tg) ** 2).mean(1) + 1e-10), rtol=1e-14)
    dense = np.zeros((B, heads, A))
    for k in range(K):
        dense[np.arange(B), on0 + k, action] = ref["dq"][:, k]
    assert np.array_equal(got["dq"], dense.reshape(B, -1))
    np.testing.assert_allclose(got["loss_t"].numpy(), got["losses"], rtol=1e-14)
    assert (terminal == 1).any() and (got["targets"][terminal == 1] == reward[terminal == 1][:, None]).all()
    # Double Q never exceeds the max form on the same value rows, and differs from it where the heads disagree
    assert (got["targets"] <= got["max_targets"]).all()
    if not (on0 == tg0 and vr is None):
        assert (got["a_star"] != got["greedy"]).any() and (got["targets"] < got["max_targets"]).any()


def test_weights_and_huber_go_through_the_existing_loss():
    B, heads, A, K = 9, 3, 4, 2
    rows, action, reward, terminal = _rows(5, B, heads, A, scale=3.0)
    w = np.random.default_rng(1).uniform(0.1, 1.0, B)
    got = dq.double_q(rows, action, reward, terminal, 0.99, K, 1, 0, A, weights=w, huber_delta=1.0)
    ref = pw.weighted_td(got["q"], got["targets"], w, 1.0)
    assert np.array_equal(got["losses"], ref["losses"])
    assert (np.abs(got["q"] - got["targets"]) > 1.0).any() and (np.abs(got["q"] - got["targets"]) < 1.0).any()
    np.testing.assert_allclose(got["loss_t"].numpy(), ref["losses"], rtol=1e-14)
    np.testing.assert_allclose(got["priorities"], np.sqrt(ref["l"].mean(1) + 1e-10), rtol=1e-14)  # unweighted


def test_an_exact_tie_selects_the_first_index():
    B, heads, A, K = 4, 2, 5, 1
    rows, action, reward, terminal = _rows(7, B, heads, A)
    terminal[:] = 0
    sel = rows[B:, A : 2 * A]  # selector head 1
    sel[:] = np.array([0.0, 2.0, -1.0, 2.0, 1.0])  # entries 1 and 3 tie exactly
    rows[B:, :A] = np.array([10.0, 20.0, 30.0, 40.0, 50.0])  # the value head tells the two apart
    got = dq.double_q(rows, action, reward, terminal, 0.5, K, 1, 0, A)
    assert (got["a_star"] == 1).all()
    assert np.array_equal(got["targets"][:, 0], reward + 0.5 * 20.0)
    assert np.array_equal(dq.triple_loop(rows, action, reward, terminal, 0.5, K, 1, 0, A)[0], got["a_star"])
    sel[:, 0] = 2.0  # a three-way tie that starts at index 0
    assert (dq.double_q(rows, action, reward, terminal, 0.5, K, 1, 0, A)["a_star"] == 0).all()
    assert np.array_equal(dq.first_argmax([[1.0, 3.0, 3.0], [-0.0, 0.0, -1.0]]), [1, 0])  # (-0.0 == 0.0: not a strict >)


def test_single_head_with_selector_equal_to_value_is_the_max_form():
    B, A = 13, 6
    rows, action, reward, terminal = _rows(11, B, 1, A)
    got = dq.double_q(rows, action, reward, terminal, 0.99, 1, 0, 0, A)
    assert np.array_equal(got["targets"], got["max_targets"])
    assert np.array_equal(got["a_star"], got["greedy"])
    want = reward + (1.0 - terminal) * 0.99 * rows[B:].max(1)
    assert np.array_equal(got["targets"][:, 0], want)


def test_histogram_heads_select_and_value_on_expectations():
    B, heads, A, K, nb = 5, 3, 4, 2, 11
    hist = dict(nb=nb, vmin=-5.0, vmax=5.0, sigma=0.75 * 10.0 / nb)
    rng = np.random.default_rng(2)
    logits = rng.normal(size=(2 * B, heads * A * nb)) * 2.0
    action, reward, terminal = rng.integers(0, A, B), rng.normal(size=B) * 4, (rng.random(B) < 0.3).astype(np.uint8)
    got = dq.double_q(logits, action, reward, terminal, 0.9, K, 1, 0, A, hist=hist)
    ex = hl.expectations(logits, nb, -5.0, 5.0).numpy()  # [2B, heads * A]
    a_star, tg = dq.triple_loop(ex, action, reward, terminal, 0.9, K, 1, 0, A)
    assert np.array_equal(got["a_star"], a_star)
    np.testing.assert_allclose(got["targets"], tg, rtol=1e-14)
    # behind the target: the cross-entropy of hl_gauss.py against the projection of THESE targets
    same = hl.hl_loss(logits, action, reward, terminal, 0.9, K, 1, 0, A, nb, -5.0, 5.0, hist["sigma"])
    np.testing.assert_allclose(got["q"], same["q"].numpy(), rtol=1e-14)
    assert not np.allclose(got["targets"], same["targets"].numpy())
    import torch

    la = torch.as_tensor(logits[:B]).reshape(B, heads, A, nb)[torch.arange(B)[:, None], torch.arange(1, 1 + K)[None, :], torch.as_tensor(action)[:, None]]
    p = hl.projection(torch.as_tensor(tg), nb, -5.0, 5.0, hist["sigma"])
    ce = (torch.logsumexp(la, -1) - (p * la).sum(-1)).mean(0)
    np.testing.assert_allclose(got["losses"], ce.numpy(), rtol=1e-13)


# ------------------------------------------------------------------ 2. the C ABI's configuration
def test_config_struct_ends_in_double_q_and_the_header_names_it(tmp_path):
    import subprocess

    from slimdqn import _hip

    names = [f[0] for f in _hip.NetConfig._fields_]
    assert names[-1] == "double_q" and names[-2] == "hl_sigma"
    assert _hip.NetConfig().double_q == 0  # a configuration built without it: off
    header = open(os.path.join(ROOT, "include", "isdqn_hip.h")).read()
    body = header[header.index("typedef struct isdqn_net_config") : header.index("} isdqn_net_config;")]
    fields = re.findall(r"^\s+(?:int32_t|float)\s+([^;]+);", body, flags=re.M)
    assert fields[-1].strip() == "double_q"
    assert "FIRST index" in body and "ISDQN_ERR_UNSUPPORTED" in body
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "isdqn_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(isdqn_net_config), offsetof(isdqn_net_config, double_q)); return 0; }\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses
    exe = tmp_path / "layout"
    subprocess.check_call([hipcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == ctypes.sizeof(_hip.NetConfig) and off == _hip.NetConfig.double_q.offset and off + 4 == size


@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


def _cfg(double_q=0, n_bins=0, n_heads=4, batch_norm=0):
    from slimdqn import _hip

    c = _hip.NetConfig()
    c.arch = _hip.ARCH_CNN
    c.obs_h, c.obs_w, c.obs_c = 84, 84, 4
    c.n_features = 4
    for i, f in enumerate((32, 64, 64, 512)):
        c.features[i] = f
    c.n_actions, c.n_heads, c.layer_norm, c.batch_size = 9, n_heads, 1, 32
    c.precision = _hip.PRECISION_BF16X3
    c.gamma_n, c.learning_rate, c.adam_b1, c.adam_b2, c.adam_eps = 0.99, 1e-4, 0.9, 0.999, 1e-8
    c.batch_norm = batch_norm
    c.n_bins = n_bins
    if n_bins:
        c.hl_min, c.hl_max, c.hl_sigma = -10.0, 10.0, 0.3
    c.double_q = double_q
    return c


def _regions(lib, cfg, names):
    out = {}
    for n in names:
        off, size = ctypes.c_int64(), ctypes.c_int64()
        rc = lib.isdqn_net_workspace_region(ctypes.byref(cfg), n.encode(), ctypes.byref(off), ctypes.byref(size))
        out[n] = (off.value, size.value) if rc == 0 else None
    return out


@pytest.mark.parametrize("n_bins", [0, 51])
def test_workspace_plan_appends_the_target_rows_only_with_the_option(lib, n_bins):
    from slimdqn import _hip

    names = ["q", "dout", "da", "slab", "q_values", "targets", "loss_partials", "wsplit", "act/Conv_0", "gw/Dense_1"] + (["logits"] if n_bins else [])
    off_cfg, on_cfg = _cfg(0, n_bins), _cfg(1, n_bins)
    b0, b1 = ctypes.c_int64(), ctypes.c_int64()
    assert lib.isdqn_net_workspace_bytes(ctypes.byref(off_cfg), ctypes.byref(b0)) == _hip.OK
    assert lib.isdqn_net_workspace_bytes(ctypes.byref(on_cfg), ctypes.byref(b1)) == _hip.OK
    r0, r1 = _regions(lib, off_cfg, names), _regions(lib, on_cfg, names)
    assert r0 == r1 and all(v is not None for v in r0.values())  # no existing region moves
    new = ["q_target"] + (["logits_target"] if n_bins else [])
    assert all(v is None for v in _regions(lib, off_cfg, ["q_target", "logits_target"]).values())
    t = _regions(lib, on_cfg, new)
    nha_p = (4 * 9 + 7) // 8 * 8
    assert t["q_target"][0] == b0.value  # appended behind everything a configuration without the option has
    assert t["q_target"][1] >= 32 * nha_p * 4
    end = t["q_target"][0] + t["q_target"][1]
    if n_bins:
        assert t["logits_target"][0] == end and t["logits_target"][1] >= 32 * (4 * 9 * n_bins) * 4
        end += t["logits_target"][1]
    else:
        assert _regions(lib, on_cfg, ["logits_target"])["logits_target"] is None
    assert b1.value == end


def test_values_other_than_0_and_1_are_argument_errors(lib):
    from slimdqn import _hip

    for bad in (2, -1, 256):
        c = _cfg(bad)
        b = ctypes.c_int64()
        assert lib.isdqn_net_workspace_bytes(ctypes.byref(c), ctypes.byref(b)) == _hip.ERR_ARG
        assert b"double_q" in lib.isdqn_last_error()
    for ok in (0, 1):
        c = _cfg(ok, n_heads=1)  # (a single head: accepted by the C ABI)
        assert lib.isdqn_net_workspace_bytes(ctypes.byref(c), ctypes.byref(ctypes.c_int64())) == _hip.OK


# ------------------------------------------------------------------ 3. the flag
def _parse(argv, algo="isdqn"):
    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    getattr(pa, f"add_{algo}_arguments")(parser)
    names = pa.add_engine_arguments(parser)
    return vars(parser.parse_args(["-en", "x_Game", "-s", "1"] + argv)), names


def test_the_flag_short_and_long_default_off():
    p, names = _parse([])
    assert "double_q" in names and p["double_q"] is False
    assert _parse(["-dq"])[0]["double_q"] is True
    assert _parse(["--double_q"])[0]["double_q"] is True
    assert _parse(["-dq"], algo="dqn")[0]["double_q"] is True


def test_parameters_json_holds_the_flag_only_under_dq(tmp_path):
    from experiments.base.utils import prepare_logs

    for algo in ("isdqn", "dqn", "analysisdqn"):
        p = prepare_logs("atari", algo, ["-en", f"a{algo}_Game", "-dw", "-s", "1"], root=str(tmp_path))
        assert p["double_q"] is False
        plain = json.load(open(tmp_path / "atari" / "exp_output" / f"a{algo}_Game" / "parameters.json"))
        assert "double_q" not in plain[algo] and "double_q" not in plain["shared_parameters"]
        p = prepare_logs("atari", algo, ["-en", f"b{algo}_Game", "-dw", "-s", "1", "-dq"], root=str(tmp_path))
        assert p["double_q"] is True
        on = json.load(open(tmp_path / "atari" / "exp_output" / f"b{algo}_Game" / "parameters.json"))
        assert on[algo]["double_q"] is True and "double_q" not in on["shared_parameters"]
    # a second seed of the same experiment without the flag is another agent: refused like any changed agent parameter
    with pytest.raises(AssertionError):
        prepare_logs("atari", "isdqn", ["-en", "bisdqn_Game", "-dw", "-s", "2"], root=str(tmp_path))


@pytest.mark.parametrize("env,algo", [("atari", "tfdqn"), ("atari", "analysistfdqn"), ("lunar_lander", "tfdqn")])
def test_target_free_entry_points_fail_early_with_the_agents_message(tmp_path, env, algo):
    from experiments.base.utils import prepare_logs
    from slimdqn.networks.tfdqn import DOUBLE_Q_REFUSED

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, ["-en", "tf_Game", "-dw", "-s", "1", "-dq"], root=str(tmp_path))
    assert str(e.value) == DOUBLE_Q_REFUSED
    assert not (tmp_path / env).exists()  # before anything is written
    prepare_logs(env, algo, ["-en", "tf_Game", "-dw", "-s", "1"], root=str(tmp_path))  # without the flag: as before


def test_entry_points_pass_the_flag_to_their_agents():
    base = os.path.join(ROOT, "is-dqn_amd", "experiments")
    for rel in ("atari/isdqn.py", "atari/dqn.py", "atari/analysisdqn.py", "lunar_lander/isdqn.py", "lunar_lander/dqn.py",
                "atari/tfdqn.py", "atari/analysistfdqn.py", "lunar_lander/tfdqn.py"):
        assert 'double_q=p["double_q"]' in open(os.path.join(base, rel)).read(), rel


def test_target_free_agents_refuse_the_option_and_say_why():
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.tfdqn import DOUBLE_Q_REFUSED, TFDQN

    for cls in (TFDQN, AnalysisTFDQN):
        with pytest.raises(ValueError) as e:  # (raised before the engine is built: no GPU needed)
            cls(0, (84, 84, 4), 4, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, double_q=True)
        assert str(e.value) == DOUBLE_Q_REFUSED
    assert "selects and values" in DOUBLE_Q_REFUSED and "max Q" in DOUBLE_Q_REFUSED


def test_analysis_agent_refuses_batch_norm_with_the_option_before_it_builds_an_engine():
    from slimdqn.networks.analysisdqn import AnalysisDQN

    for args, kw in (((0, (84, 84, 4), 4, 2, [8, 8, 8, 16], True, True, "cnn", 1e-3, 0.99, 1, 1, 4), dict(double_q=True)),
                     ((0, (84, 84, 4), 4, 2, [8, 8, 8, 16], True), dict(batch_norm=True, architecture_type="cnn", learning_rate=1e-3, gamma=0.99,
                                                                     update_horizon=1, data_to_update=1, target_update_frequency=4, double_q=True))):
        with pytest.raises(NotImplementedError) as e:  # (no GPU here: building the engine would raise something else)
            AnalysisDQN(*args, batch_size=4, **kw)
        assert "double_q" in str(e.value) and "batch_norm" in str(e.value)


def test_agents_take_the_keyword():
    import inspect

    from slimdqn._engine import QNetEngine
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN

    for f in (QNetEngine.__init__, DQN.__init__, iSDQN.__init__):
        par = inspect.signature(f).parameters["double_q"]
        assert par.default is False
