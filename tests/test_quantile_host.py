"""QR-DQN quantile-regression heads (include/isdqn_hip.h, isdqn_net_config::n_quantiles) without a GPU: the float64 restatement of
tests/helpers/quantile.py against a plain loop and torch autograd, the struct layout and the header's definition, the workspace plan
with the option off, the C ABI's refusals, the flags, the agents' refusals and the entry points."""
import argparse
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from tests.helpers import quantile as qr


def _case(seed, B, n_heads, A, N, scale=1.0, f32=True):
    rng = np.random.default_rng(seed)
    rows = rng.normal(0, scale, (2 * B, n_heads * A * N))
    if f32:
        rows = rows.astype(np.float32).astype(np.float64)
    return (rows, rng.integers(0, A, B), rng.normal(size=B).astype(np.float32), (rng.random(B) < 0.3).astype(np.uint8),
            rng.uniform(0.2, 1.0, B).astype(np.float32))


# ------------------------------------------------------------------ 1. the helper against a plain loop
@pytest.mark.parametrize("kappa", [1.0, 0.3, 0.0])
@pytest.mark.parametrize("shape", [(5, 3, 4, 2), (4, 2, 3, 7), (3, 1, 5, 33)])
def test_vectorised_helper_equals_the_triple_loop(shape, kappa):
    B, K, A, N = shape
    n_heads = 1 + K if K > 1 else 1
    on0 = 1 if n_heads > 1 else 0
    rows, a, r, t, w = _case(B + N, B, n_heads, A, N)
    g = float(np.float32(0.99))
    for extra in (dict(), dict(weights=w), dict(selector_rows=rows[B:][::-1].copy()), dict(value_rows=rows[:B] * 0.5)):
        v = qr.qr_loss(rows, a, r, t, g, K, on0, 0, A, N, kappa, **extra)
        l = qr.qr_loss_loops(rows, a, r, t, g, K, on0, 0, A, N, kappa, **extra)
        assert np.array_equal(v["a_star"].numpy(), l["a_star"])
        for name in ("q", "targets", "losses", "priorities", "dtheta", "l"):
            np.testing.assert_allclose(v[name].detach().numpy(), l[name], rtol=1e-12, atol=1e-14, err_msg=name)
    assert t.any() and not t.all()
    np.testing.assert_allclose(qr.means(rows, N).numpy(), rows.reshape(2 * B, -1, N).mean(-1), rtol=1e-15)


def test_targets_equal_the_mean_of_the_atoms_and_selector_rows_decide():
    B, K, A, N = 6, 2, 4, 9
    rows, a, r, t, _ = _case(1, B, 1 + K, A, N)
    ref = qr.qr_loss(rows, a, r, t, 0.97, K, 1, 0, A, N, 1.0)
    val = rows[B:].reshape(B, 1 + K, A, N)
    for b in range(B):
        for k in range(K):
            m = val[b, k].mean(-1)
            assert int(ref["a_star"][b, k]) == int(np.argmax(m))
            atoms = float(r[b]) + (1.0 - t[b]) * 0.97 * val[b, k, int(np.argmax(m))]
            assert abs(float(ref["targets"][b, k]) - atoms.mean()) < 1e-12
    # double_q: head on0 + k of the selector rows decides; an exact tie resolves to the lowest index
    sel = np.zeros_like(rows[B:]).reshape(B, 1 + K, A, N)
    sel[:, :, 1] = 1.0
    sel[:, :, 3] = 1.0
    dq = qr.qr_loss(rows, a, r, t, 0.97, K, 1, 0, A, N, 1.0, selector_rows=sel.reshape(B, -1))
    assert (dq["a_star"] == 1).all()


# ------------------------------------------------------------------ 2. the helper's gradient against torch autograd
@pytest.mark.parametrize("kappa", [1.0, 0.0])
def test_gradient_equals_autograd_and_no_gradient_flows_through_target_atoms(kappa):
    B, K, A, N, heads = 7, 3, 4, 6, 4
    rows_np, a, r, t, w = _case(11, B, heads, A, N)
    rows = torch.tensor(rows_np, requires_grad=True)
    ref = qr.qr_loss(rows, a, r, t, float(np.float32(0.99)), K, 1, 0, A, N, kappa, weights=w)
    # (kappa = 0: the pinball loss has a kink at u = 0; these inputs have no u_ij = 0 -- the test below)
    assert 0.1 < ref["neg_share"] < 0.9
    ref["losses"].sum().backward()
    g = rows.grad.numpy()
    # heads 1 and 2 supply the atoms of pairs 1 and 2 and are learned in pairs 0 and 1: still nothing in the next-state rows, and one
    # block of N non-zeros per (transition, pair) at (1 + k, a_b)
    assert (g[B:] == 0).all()
    np.testing.assert_allclose(g[:B], ref["dtheta"].numpy(), rtol=1e-12, atol=1e-16)
    nz = (g[:B].reshape(B, heads, A, N) != 0).any(-1)
    assert nz.sum() == B * K and not nz[:, 0].any()
    for k in range(K):
        assert nz[np.arange(B), 1 + k, a].all()


def test_no_difference_is_exactly_zero_in_the_pinball_case():
    B, K, A, N = 7, 3, 4, 6
    rows, a, r, t, _ = _case(11, B, 1 + K, A, N)
    g = float(np.float32(0.99))
    val = rows[B:].reshape(B, 1 + K, A, N)
    ref = qr.qr_loss(rows, a, r, t, g, K, 1, 0, A, N, 0.0)
    bi, ki = np.arange(B)[:, None], np.arange(K)[None, :]
    atoms = qr.target_atoms_f32(r, t, g, val[bi, ki, ref["a_star"].numpy()]).numpy()
    th = rows[:B].reshape(B, 1 + K, A, N)[bi, 1 + ki, a[:, None]]
    assert ((atoms[:, :, None, :] - th[:, :, :, None]) != 0).all()


# ------------------------------------------------------------------ 3. the C ABI's configuration
def test_config_struct_gains_n_quantiles_between_n_bins_and_hl_min_and_the_header_defines_it(tmp_path):
    import subprocess

    from slimdqn import _hip

    names = [f[0] for f in _hip.NetConfig._fields_]
    i = names.index("n_bins")
    assert names[i : i + 3] == ["n_bins", "n_quantiles", "hl_min"] and names[-2:] == ["hl_sigma", "double_q"]
    assert _hip.NetConfig().n_quantiles == 0  # built without it: off
    header = open(os.path.join(ROOT, "include", "isdqn_hip.h")).read()
    body = header[header.index("typedef struct isdqn_net_config") : header.index("} isdqn_net_config;")]
    fields = re.findall(r"^\s+(?:int32_t|float)\s+([^;]+);", body, flags=re.M)
    flat = [re.sub(r"\[.*\]", "", x).strip() for f in fields for x in f.split(",")]
    assert flat == names
    for phrase in ("n_quantiles = N", "0: off", "2..256: on", "n_heads * n_actions * N outputs", "((h * A) + a) * N + i", "(i + 1/2) / N",
                   "Q_h(s, a) = (1 / N) sum_i theta_i", "the FIRST index attaining max_a", "t_j    = r + ((1 - terminal) * gamma^n) * theta^val_j",
                   "u_ij   = t_j - theta^on_i(s, a_b)", "|tau_i - 1{u_ij < 0}| * h_kappa(u_ij)", "kappa = huber_delta", "Dopamine's form",
                   "the plain pinball loss", "-(w_b / (B N))", "clip(u, -kappa, kappa) / kappa", "sign(0) = 0", "No gradient flows through any target atom",
                   "the online mean", "sqrt(mean_k (q - target)^2 +", "Quantile crossing is not prevented", "ISDQN_ERR_ARG", "ISDQN_ERR_UNSUPPORTED",
                   "5456"):
        assert phrase in body, phrase
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "isdqn_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(isdqn_net_config), offsetof(isdqn_net_config, n_bins),'
                   ' offsetof(isdqn_net_config, n_quantiles), offsetof(isdqn_net_config, hl_min)); return 0; }\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses
    exe = tmp_path / "layout"
    subprocess.check_call([hipcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_b, o_q, o_m = (int(x) for x in subprocess.check_output([str(exe)]).split())
    N = _hip.NetConfig
    assert size == ctypes.sizeof(N) and (o_b, o_q, o_m) == (N.n_bins.offset, N.n_quantiles.offset, N.hl_min.offset)
    assert o_q == o_b + 4 and o_m == o_q + 4 and N.double_q.offset + 4 == size


@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


def _fill(c, n_bins=0, double_q=0, n_heads=4, n_actions=9, batch_norm=0, tau=0.0, huber=0.0):
    from slimdqn import _hip

    c.arch = _hip.ARCH_CNN
    c.obs_h, c.obs_w, c.obs_c = 84, 84, 4
    c.n_features = 4
    for i, f in enumerate((32, 64, 64, 512)):
        c.features[i] = f
    c.n_actions, c.n_heads, c.layer_norm, c.batch_size = n_actions, n_heads, 1, 32
    c.precision = _hip.PRECISION_BF16X3
    c.gamma_n, c.learning_rate, c.adam_b1, c.adam_b2, c.adam_eps = 0.99, 1e-4, 0.9, 0.999, 1e-8
    c.huber_delta = huber
    c.batch_norm = batch_norm
    c.n_bins = n_bins
    if n_bins:
        c.hl_min, c.hl_max, c.hl_sigma = -10.0, 10.0, 0.3
    c.double_q = double_q
    c.munchausen_tau, c.munchausen_alpha, c.munchausen_clip = tau, 0.9, -1.0
    return c


def _cfg(n_quantiles=0, **kw):
    from slimdqn import _hip

    c = _fill(_hip.NetConfig(), **kw)
    c.n_quantiles = n_quantiles
    return c


def _region_table(lib, cfg, names):
    out = {}
    for n in names:
        off, size = ctypes.c_int64(), ctypes.c_int64()
        rc = lib.isdqn_net_workspace_region(ctypes.byref(cfg), n.encode(), ctypes.byref(off), ctypes.byref(size))
        out[n] = (off.value, size.value) if rc == 0 else None
    return out


def _bytes(lib, cfg):
    b = ctypes.c_int64()
    return lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)), b.value


REGIONS = ["q", "logits", "dout", "da", "slab", "q_values", "targets", "dbh", "adam_consts", "loss_partials", "wsplit", "q_target", "logits_target",
           "act/Conv_0", "z/Conv_1", "dz/Conv_2", "act/Dense_0", "red/Dense_0", "part/Dense_0", "gw/Conv_0", "gw/Dense_0", "gw/Dense_1"]


@pytest.mark.parametrize("kw", [dict(), dict(n_bins=51), dict(double_q=1), dict(n_bins=51, double_q=1), dict(tau=0.03), dict(n_heads=1, huber=1.0)])
def test_workspace_plan_with_the_option_off_is_the_plan_without_the_field(lib, kw):
    from slimdqn import _hip

    never = _fill(_hip.NetConfig(), **kw)  # a configuration that never set the field
    off = _cfg(0, **kw)
    (rc0, b0), (rc1, b1) = _bytes(lib, never), _bytes(lib, off)
    assert rc0 == rc1 == _hip.OK and b0 == b1
    r0, r1 = _region_table(lib, never, REGIONS), _region_table(lib, off, REGIONS)
    assert r0 == r1 and r0["q"] is not None and (r0["logits"] is None) == ("n_bins" not in kw)
    n0, n1 = ctypes.c_int64(), ctypes.c_int64()
    cnt = ctypes.c_int32()
    assert lib.isdqn_net_param_layout(ctypes.byref(never), ctypes.byref(n0), None, 0, ctypes.byref(cnt)) == _hip.OK
    assert lib.isdqn_net_param_layout(ctypes.byref(off), ctypes.byref(n1), None, 0, ctypes.byref(cnt)) == _hip.OK
    assert n0.value == n1.value


def test_workspace_plan_with_quantile_heads_has_the_histogram_regions_at_the_quantile_width(lib):
    from slimdqn import _hip

    N = 51
    hist, quant = _cfg(0, n_bins=N, double_q=1), _cfg(N, double_q=1, huber=1.0)
    (rc0, b0), (rc1, b1) = _bytes(lib, hist), _bytes(lib, quant)
    assert rc0 == rc1 == _hip.OK and b0 == b1  # the same block width: the same plan
    assert _region_table(lib, hist, REGIONS) == _region_table(lib, quant, REGIONS)
    r = _region_table(lib, quant, ["logits", "logits_target", "q_target"])
    assert r["logits"][1] >= 2 * 32 * 4 * 9 * N * 4 and r["logits_target"][1] >= 32 * 4 * 9 * N * 4 and r["q_target"] is not None
    n = ctypes.c_int64()
    cnt = ctypes.c_int32()
    assert lib.isdqn_net_param_layout(ctypes.byref(quant), ctypes.byref(n), None, 0, ctypes.byref(cnt)) == _hip.OK
    infos = (_hip.TensorInfo * cnt.value)()
    assert lib.isdqn_net_param_layout(ctypes.byref(quant), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)) == _hip.OK
    head = [i for i in infos if i.name == b"Dense_1/kernel"][0]
    assert tuple(head.flax_shape[:2]) == (512, 4 * 9 * N)


def test_every_refusal_returns_its_code_and_names_the_field(lib):
    from slimdqn import _hip

    table = [
        (dict(n_quantiles=1), _hip.ERR_ARG),
        (dict(n_quantiles=-3), _hip.ERR_ARG),
        (dict(n_quantiles=257), _hip.ERR_ARG),
        (dict(n_quantiles=32, n_bins=51), _hip.ERR_ARG),
        (dict(n_quantiles=32, n_bins=51, huber=1.0), _hip.ERR_ARG),
        (dict(n_quantiles=32, tau=0.03), _hip.ERR_UNSUPPORTED),
        (dict(n_quantiles=32, batch_norm=1), _hip.ERR_UNSUPPORTED),
        (dict(n_quantiles=2, n_heads=66, n_actions=2), _hip.ERR_UNSUPPORTED),  # K = 65 regressed heads
        (dict(n_quantiles=32, n_heads=10, n_actions=18), _hip.ERR_UNSUPPORTED),  # 5760 outputs > 5456
    ]
    for kw, code in table:
        rc, _ = _bytes(lib, _cfg(**kw))
        assert rc == code, (kw, rc)
        assert b"n_quantiles" in lib.isdqn_last_error(), (kw, lib.isdqn_last_error())
    ok = [dict(n_quantiles=2), dict(n_quantiles=256, n_heads=2, n_actions=9), dict(n_quantiles=32, huber=1.0), dict(n_quantiles=32, huber=0.0),
          dict(n_quantiles=32, double_q=1), dict(n_quantiles=200, n_heads=1), dict(n_quantiles=2, n_heads=65, n_actions=2),
          dict(n_quantiles=31, n_heads=4, n_actions=44)]  # 5456 outputs
    for kw in ok:
        assert _bytes(lib, _cfg(**kw))[0] == _hip.OK, kw


# ------------------------------------------------------------------ 4. the flags
def _parse(argv, algo="isdqn"):
    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    getattr(pa, f"add_{algo}_arguments")(parser)
    names = pa.add_engine_arguments(parser)
    return vars(parser.parse_args(["-en", "x_Game", "-s", "1"] + argv)), names, parser


def test_the_flags_their_defaults_and_quantile_kwargs():
    from experiments.base import parser_argument as pa

    p, names, parser = _parse([])
    assert {"quantile_regression", "n_quantiles"} <= set(names)
    assert p["quantile_regression"] is False and p["n_quantiles"] == 32 and p["huber_delta"] == 0.0
    assert pa.quantile_kwargs(p) == dict(n_quantiles=0)  # without -qr: off, whatever -nq says
    assert pa.quantile_kwargs(_parse(["-nq", "64"])[0]) == dict(n_quantiles=0)
    for algo in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn"):
        assert pa.quantile_kwargs(_parse(["-qr"], algo=algo)[0]) == dict(n_quantiles=32)
    p = _parse(["--quantile_regression", "--n_quantiles", "51", "-hd", "1"])[0]
    assert pa.quantile_kwargs(p) == dict(n_quantiles=51) and p["huber_delta"] == 1.0
    help_text = parser.format_help()
    hd = help_text[help_text.index("--huber_delta"):]
    assert "kappa" in hd[:400] and "usual value is 1" in " ".join(hd[:400].split())
    # kappa for the agents whose entry points never took -hd
    assert pa.quantile_kappa(_parse(["-hd", "1"])[0]) == 0.0 and pa.quantile_kappa(_parse(["-qr", "-hd", "1"])[0]) == 1.0


def test_parameters_json_keeps_the_reference_groups(tmp_path):
    """Like the other engine flags (-hl, -hd, -prec), -qr and -nq stay out of parameters.json, with and without -qr."""
    from experiments.base.utils import prepare_logs

    for env, algo in (("atari", "isdqn"), ("atari", "dqn"), ("lunar_lander", "tfdqn")):
        p = prepare_logs(env, algo, ["-en", f"b{algo}_Game", "-dw", "-s", "1", "-qr", "-nq", "16", "-hd", "1"], root=str(tmp_path))
        assert p["quantile_regression"] is True and p["n_quantiles"] == 16 and p["huber_delta"] == 1.0
        on = json.load(open(tmp_path / env / "exp_output" / f"b{algo}_Game" / "parameters.json"))
        plain_p = prepare_logs(env, algo, ["-en", f"a{algo}_Game", "-dw", "-s", "1"], root=str(tmp_path))
        plain = json.load(open(tmp_path / env / "exp_output" / f"a{algo}_Game" / "parameters.json"))
        assert plain_p["quantile_regression"] is False
        for stored in (on, plain):
            assert not any("quantile" in k or k == "huber_delta" for k in list(stored[algo]) + list(stored["shared_parameters"]))
        assert set(on[algo]) == set(plain[algo]) and set(on["shared_parameters"]) == set(plain["shared_parameters"])


@pytest.mark.parametrize("env,algo,extra", [("atari", "isdqn", ["-mq"]), ("atari", "isdqn", ["-hl"]), ("atari", "dqn", ["-hl"]),
                                            ("atari", "tfdqn", ["-bn"]), ("lunar_lander", "dqn", ["-mq"]), ("atari", "analysisdqn", ["-bn"])])
def test_qr_with_mq_hl_or_bn_is_refused_before_anything_is_written(tmp_path, env, algo, extra):
    from experiments.base.utils import prepare_logs

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, ["-en", "q_Game", "-dw", "-s", "1", "-qr"] + extra, root=str(tmp_path))
    assert "n_quantiles" in str(e.value)
    assert not (tmp_path / env).exists()  # before the output directory is created
    prepare_logs(env, algo, ["-en", "q_Game", "-dw", "-s", "1", "-nq", "16"] + extra, root=str(tmp_path))  # -nq alone means nothing


def test_entry_points_pass_the_keyword_to_their_agents():
    base = os.path.join(ROOT, "is-dqn_amd", "experiments")
    for rel in ("atari/isdqn.py", "atari/dqn.py", "atari/analysisdqn.py", "lunar_lander/isdqn.py", "lunar_lander/dqn.py",
                "atari/tfdqn.py", "atari/analysistfdqn.py", "lunar_lander/tfdqn.py"):
        src = open(os.path.join(base, rel)).read()
        assert "**quantile_kwargs(p)" in src, rel
        assert 'huber_delta=p["huber_delta"]' in src or "huber_delta=quantile_kappa(p)" in src, rel  # -hd is kappa for every agent


# ------------------------------------------------------------------ 5. the agents
def test_agents_take_the_keyword_and_refuse_the_three_combinations_before_an_engine_is_built():
    from slimdqn import _engine
    from slimdqn._engine import QNetEngine
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    for f in (QNetEngine.__init__, DQN.__init__, iSDQN.__init__, TFDQN.__init__):
        assert inspect.signature(f).parameters["n_quantiles"].default == 0
    for f in (DQN.__init__, iSDQN.__init__, TFDQN.__init__):
        assert inspect.signature(f).parameters["huber_delta"].default == 0.0
    isd = lambda **kw: iSDQN(0, (84, 84, 4), 4, 2, [8, 8, 8, 16], True, kw.pop("batch_norm", False), "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    ana = lambda **kw: AnalysisDQN(0, (84, 84, 4), 4, 2, [8, 8, 8, 16], True, kw.pop("batch_norm", False), "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    dqn = lambda **kw: DQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    tf = lambda **kw: TFDQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, kw.pop("batch_norm", False), "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    atf = lambda **kw: AnalysisTFDQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, kw.pop("batch_norm", False), "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    eng = lambda **kw: QNetEngine((84, 84, 4), 4, 3, [8, 8, 8, 16], "cnn", True, 4, **kw)
    # raised before an engine is built (no GPU here: building one would raise something else)
    for make in (isd, ana, dqn, tf, atf, eng):
        with pytest.raises(ValueError) as e:
            make(n_quantiles=16, n_bins=51)
        assert str(e.value) == _engine.QUANTILE_HISTOGRAM_REFUSED
        with pytest.raises(ValueError) as e:
            make(n_quantiles=16, munchausen_tau=0.03)
        assert str(e.value) == _engine.QUANTILE_MUNCHAUSEN_REFUSED
    for make in (isd, ana, tf, atf, eng):
        with pytest.raises(ValueError) as e:
            make(n_quantiles=16, batch_norm=True)
        assert str(e.value) == _engine.QUANTILE_BATCH_NORM_REFUSED
    for msg in (_engine.QUANTILE_HISTOGRAM_REFUSED, _engine.QUANTILE_MUNCHAUSEN_REFUSED, _engine.QUANTILE_BATCH_NORM_REFUSED):
        assert "n_quantiles" in msg
