"""Noisy Dense layers, the part that needs no GPU (include/isdqn_hip.h, isdqn_noisy_layout):

1. the numpy reference of tests/helpers/noisy.py: Philox4x32-10 against known answers, the statistics of the draws, compose and the
   sigma gradients against torch autograd, and the named wrong readings against those checks;
2. the host side of the C ABI: the noise layout of the plan and the refusals of the noisy entry points, in their order;
3. the flags, check_noisy, noisy_kwargs, the entry points and the agents' refusals before an engine is built."""
import argparse
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import noisy as nz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    got = nz.philox4x32_10(ctr, key)
    assert " ".join(f"{int(x[0]):08x}" for x in got) == want


def test_philox_is_elementwise_and_the_counter_words_are_what_the_header_says():
    x0, x1 = nz.words(5, layer=3, vec=1, seed=(7 << 32) | 9, count=(2 << 32) | 11, stream_id=1)
    for j in range(5):
        one = nz.philox4x32_10((j, (1 << 16) | 7, 11, 2), (9, 7))
        assert int(one[0][0]) == int(x0[j]) and int(one[1][0]) == int(x1[j])


def test_statistics_of_the_draws():
    n = 2**17
    x0, x1 = nz.words(n, 0, 0, seed=12345, count=0, stream_id=0)
    u1, u2 = nz.uniforms(x0, x1)
    assert u1.min() > 0 and u1.max() < 1 and u2.min() >= 0 and u2.max() < 1
    z, _ = nz.normal(x0, x1)
    se = lambda a: a.std(ddof=1) / np.sqrt(a.size)
    assert abs(z.mean()) <= 4 * se(z)
    assert abs((z * z - 1).mean()) <= 4 * se(z * z - 1)
    f2 = nz.f(z) ** 2  # |z|: E|z| = sqrt(2 / pi)
    assert abs((f2 - np.sqrt(2 / np.pi)).mean()) <= 4 * se(f2)
    assert np.array_equal(np.sign(nz.f(z)), np.sign(z))


def _mlp_case(seed=0, d_in=7, d_h=7, d_out=5, B=6):
    """Two noisy layers (square first layer so that the swapped reading is well-formed) with their fp32 operands."""
    rng = np.random.default_rng(seed)
    L = []
    for l, (i, o) in enumerate(((d_in, d_h), (d_h, d_out))):
        ein, _, _ = nz.sample_vector(i, l, 0, 5, 3, 0)
        eout, _, _ = nz.sample_vector(o, l, 1, 5, 3, 0)
        L.append(dict(mu=rng.normal(size=(o, i)).astype(np.float32), sigma=rng.uniform(0.1, 0.5, (o, i)).astype(np.float32),
                      mu_b=rng.normal(size=o).astype(np.float32), sigma_b=rng.uniform(0.1, 0.5, o).astype(np.float32),
                      ein=ein.astype(np.float32), eout=eout.astype(np.float32)))
    x = rng.normal(size=(B, d_in))
    y = rng.normal(size=(B, d_out))
    return L, x, y


def _autograd(L, x, y):
    """float64 torch: w = mu + sigma * outer(eout, ein), b = mu_b + sigma_b * eout; gradients w.r.t. w (= g), sigma, sigma_b."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    h = torch.tensor(x)
    leaves = []
    for k, l in enumerate(L):
        sigma, sigma_b = t(l["sigma"]), t(l["sigma_b"])
        ein, eout = torch.tensor(l["ein"].astype(np.float64)), torch.tensor(l["eout"].astype(np.float64))
        w = torch.tensor(l["mu"].astype(np.float64)) + sigma * torch.outer(eout, ein)
        b = torch.tensor(l["mu_b"].astype(np.float64)) + sigma_b * eout
        w.retain_grad(); b.retain_grad()
        h = h @ w.T + b
        if k == 0:
            h = torch.relu(h)
        leaves.append((w, b, sigma, sigma_b))
    ((h - torch.tensor(y)) ** 2).mean().backward()
    return [tuple(v.grad.numpy() for v in leaf) for leaf in leaves]


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def test_sigma_gradients_equal_autograd():
    L, x, y = _mlp_case()
    for l, (g_w, g_b, g_sigma, g_sigma_b) in zip(L, _autograd(L, x, y)):
        n64 = l["eout"].astype(np.float64)[:, None] * l["ein"].astype(np.float64)[None, :]
        assert _rel(g_w * n64, g_sigma) <= 1e-12 and _rel(g_b * l["eout"].astype(np.float64), g_sigma_b) <= 1e-12
        # the helper forms the same products in fp32 (the device's g_sigma): one rounding of n, one of g * n
        g32 = g_w.astype(np.float32)
        assert _rel(nz.g_sigma_kernel(g32, l["ein"], l["eout"]), g32.astype(np.float64) * n64) <= 2.0**-22
        assert _rel(nz.g_sigma_bias(g_b.astype(np.float32), l["eout"]), g_b.astype(np.float32).astype(np.float64) * l["eout"]) <= 2.0**-23


def test_compose_is_the_three_rounded_steps_and_zero_noise_gives_mu():
    L, _, _ = _mlp_case(1)
    l = L[0]
    eff = nz.compose_kernel(l["mu"], l["sigma"], l["ein"], l["eout"])
    assert eff.dtype == np.float32
    exact = l["mu"].astype(np.float64) + l["sigma"].astype(np.float64) * (l["eout"].astype(np.float64)[:, None] * l["ein"].astype(np.float64)[None, :])
    assert np.all(np.abs(eff - exact) <= 2.0**-23 * (np.abs(exact) + 2 * np.abs(exact - l["mu"])))  # three roundings
    n = np.float32(l["eout"])[:, None] * np.float32(l["ein"])[None, :]
    assert np.array_equal(eff, l["mu"] + (l["sigma"] * n).astype(np.float32))
    zero_in, zero_out = np.zeros_like(l["ein"]), np.zeros_like(l["eout"])
    assert np.array_equal(nz.compose_kernel(l["mu"], l["sigma"], zero_in, zero_out).view(np.uint32), l["mu"].view(np.uint32))
    assert np.array_equal(nz.compose_bias(l["mu_b"], l["sigma_b"], zero_out).view(np.uint32), l["mu_b"].view(np.uint32))


def test_wrong_readings_miss_the_checks():
    L, x, y = _mlp_case(2)
    l = L[0]
    (g_w, g_b, g_sigma, g_sigma_b) = _autograd(L, x, y)[0]
    right = nz.compose_kernel(l["mu"], l["sigma"], l["ein"], l["eout"])
    # f not applied: the raw normals behind the same vectors
    _, zin, _ = nz.sample_vector(l["ein"].size, 0, 0, 5, 3, 0)
    _, zout, _ = nz.sample_vector(l["eout"].size, 0, 1, 5, 3, 0)
    assert not np.array_equal(nz.compose_kernel_no_f(l["mu"], l["sigma"], zin, zout), right)
    assert _rel(nz.compose_kernel_no_f(l["mu"], l["sigma"], zin, zout), right.astype(np.float64)) > 1e-3
    # ein / eout swapped
    assert _rel(nz.compose_kernel_swapped(l["mu"], l["sigma"], l["ein"], l["eout"]), right.astype(np.float64)) > 1e-3
    # bias scaled by ein
    assert _rel(nz.compose_bias_by_ein(l["mu_b"], l["sigma_b"], l["ein"]), nz.compose_bias(l["mu_b"], l["sigma_b"], l["eout"]).astype(np.float64)) > 1e-3
    # sigma updated with g instead of g * n: misses the autograd check by far more than its 1e-12
    assert _rel(nz.g_sigma_plain(g_w.astype(np.float32), l["ein"], l["eout"]), g_sigma) > 1e-3


def test_adam_on_both_buffers_from_one_gradient():
    rng = np.random.default_rng(3)
    mu, sigma, g, n = (rng.normal(size=9).astype(np.float32) for _ in range(4))
    z = np.zeros(9)
    mu1, s1, st = nz.noisy_step64(mu, sigma, (z, z, z, z), g, n, 1, 1e-3, 1e-8)
    # first step of Adam: p - lr * sign(g) up to eps
    assert np.allclose(mu1, mu - 1e-3 * np.sign(g), atol=1e-9) and np.allclose(s1, sigma - 1e-3 * np.sign(g * n), atol=1e-9)
    mu2, s2, _ = nz.noisy_step64(mu1, s1, st, g, n, 2, 1e-3, 1e-8)
    assert np.all(np.abs(mu2 - mu1) > 0) and np.all(np.abs(s2 - s1) > 0)


# ------------------------------------------------------------------ 2. the host side of the C ABI
@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


def _cfg(arch="cnn", feats=(32, 64, 64, 512), n_heads=10, n_actions=9, batch_norm=0, dueling=0, max_grad_norm=0.0, B=32, obs=8):
    from slimdqn import _hip

    cfg = _hip.NetConfig()
    cfg.arch = {"cnn": _hip.ARCH_CNN, "fc": _hip.ARCH_FC, "impala": _hip.ARCH_IMPALA}[arch]
    cfg.obs_h, cfg.obs_w, cfg.obs_c = (84, 84, 4) if arch != "fc" else (1, 1, obs)
    cfg.n_features = len(feats)
    for i, f in enumerate(feats):
        cfg.features[i] = f
    cfg.n_actions, cfg.n_heads, cfg.layer_norm, cfg.batch_size = n_actions, n_heads, 1, B
    cfg.precision = _hip.PRECISION_BF16X3
    cfg.gamma_n, cfg.learning_rate, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps = 0.99, 1e-4, 0.9, 0.999, 1e-8
    cfg.batch_norm, cfg.dueling, cfg.max_grad_norm = batch_norm, dueling, max_grad_norm
    cfg.munchausen_alpha, cfg.munchausen_clip = 0.9, -1.0
    return cfg


def _layout(lib, cfg):
    nl, total = ctypes.c_int32(), ctypes.c_int64()
    offs, wi, wo = (ctypes.c_int64 * 8)(), (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)()
    rc = lib.isdqn_noisy_layout(ctypes.byref(cfg), ctypes.byref(nl), offs, wi, wo, 8, ctypes.byref(total))
    return rc, [(offs[i], wi[i], wo[i]) for i in range(nl.value)], total.value


def test_noise_layout_is_the_dense_layers_internal_widths(lib):
    from slimdqn import _hip

    rc, lay, total = _layout(lib, _cfg())
    assert rc == _hip.OK
    # headline: Dense_0 reads 11 * 11 pixels (SAME padding: 84 -> 21 -> 11 -> 11) of 64 channels, the head writes 90 rows padded to 96
    assert lay == [(0, 7744, 512), (8256, 512, 96)] and total == 8256 + 608
    rc, lay, total = _layout(lib, _cfg(arch="fc", feats=(100, 100), n_heads=4, n_actions=4))
    assert rc == _hip.OK and lay == [(0, 8, 104), (112, 104, 104), (320, 104, 16)] and total == 440
    rc, lay, _ = _layout(lib, _cfg(arch="fc", feats=(100, 100), n_heads=4, n_actions=4, dueling=1))
    assert rc == _hip.OK and lay[-1] == (320, 104, 24)  # 4 heads of 4 advantages + 1 value
    # the tensor table agrees: every Dense kernel is [out_p][in_p]
    cfg = _cfg()
    n, cnt = ctypes.c_int64(), ctypes.c_int32()
    assert lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), None, 0, ctypes.byref(cnt)) == _hip.OK
    infos = (_hip.TensorInfo * cnt.value)()
    assert lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)) == _hip.OK
    dense = [(i.dims[1], i.dims[0]) for i in infos if i.kind == 1]
    assert dense == [(w_in, w_out) for _, w_in, w_out in _layout(lib, cfg)[1]]


def _entry_points(lib, cfg):
    """The four noisy entry points on `cfg` with null pointers everywhere else: the refusals answer before any pointer is looked at."""
    return {
        "layout": lambda: _layout(lib, cfg)[0],
        "sample": lambda: lib.isdqn_noisy_sample(ctypes.byref(cfg), 0, 0, None, None, None),
        "compose": lambda: lib.isdqn_noisy_compose(ctypes.byref(cfg), None, None, None, None, None, None),
        "learn": lambda: lib.isdqn_noisy_learn_on_batch(ctypes.byref(cfg), *([None] * 11), None, *([None] * 7)),
    }


REFUSED = [  # (configuration, words of the message) -- in the order the header states: batch_norm, impala, max_grad_norm > 0
    (dict(batch_norm=1, arch="impala", feats=(8, 8, 8, 16)), ("noisy", "BatchNorm")),
    (dict(batch_norm=1), ("noisy", "BatchNorm")),
    (dict(arch="impala", feats=(8, 8, 8, 16)), ("noisy", "impala")),
    (dict(max_grad_norm=10.0), ("noisy", "max_grad_norm", "follow-up")),
    (dict(max_grad_norm=float("inf")), ("noisy", "max_grad_norm", "follow-up")),
    # the plan's own refusals answer first (gradient clipping on a BatchNorm network or on the impala torso is the plan's)
    (dict(max_grad_norm=10.0, batch_norm=1), ("gradient clipping",)),
    (dict(max_grad_norm=10.0, arch="impala", feats=(8, 8, 8, 16)), ("gradient clipping",)),
]


@pytest.mark.parametrize("entry", ["layout", "sample", "compose", "learn"])
@pytest.mark.parametrize("kw,words", REFUSED)
def test_refusals_of_the_noisy_entry_points_in_their_order(lib, entry, kw, words):
    from slimdqn import _hip

    assert _entry_points(lib, _cfg(**kw))[entry]() == _hip.ERR_UNSUPPORTED
    msg = lib.isdqn_last_error().decode()
    assert all(w in msg for w in words), msg


def test_behind_the_refusals_null_pointers_and_a_short_layout_array_are_argument_errors(lib):
    from slimdqn import _hip

    calls = _entry_points(lib, _cfg())
    assert calls["layout"]() == _hip.OK
    for entry in ("sample", "compose", "learn"):
        assert calls[entry]() == _hip.ERR_ARG, entry
    # the layout call: NULL arrays query the count and the total; arrays that cannot hold every layer are refused, never truncated
    cfg = _cfg(arch="fc", feats=(100, 100), n_heads=4, n_actions=4)
    nl, total = ctypes.c_int32(), ctypes.c_int64()
    assert lib.isdqn_noisy_layout(ctypes.byref(cfg), ctypes.byref(nl), None, None, None, 0, ctypes.byref(total)) == _hip.OK
    assert (nl.value, total.value) == (3, 440)
    offs, wi, wo = (ctypes.c_int64 * 3)(*[-1] * 3), (ctypes.c_int32 * 3)(*[-1] * 3), (ctypes.c_int32 * 3)(*[-1] * 3)
    nl.value, total.value = 0, 0
    assert lib.isdqn_noisy_layout(ctypes.byref(cfg), ctypes.byref(nl), offs, wi, wo, 2, ctypes.byref(total)) == _hip.ERR_ARG
    assert "max_layers" in lib.isdqn_last_error().decode() and (nl.value, total.value) == (3, 440) and list(offs) == [-1] * 3
    assert lib.isdqn_noisy_layout(ctypes.byref(cfg), ctypes.byref(nl), offs, None, None, 3, None) == _hip.OK and list(offs) == [0, 112, 320]


# ------------------------------------------------------------------ 3. flags, check_noisy, agents, entry points
def _parse(argv, algo="isdqn"):
    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    getattr(pa, f"add_{algo}_arguments")(parser)
    names = pa.add_engine_arguments(parser)
    return vars(parser.parse_args(["-en", "x_Game", "-s", "1"] + argv)), names, parser


def test_the_flags_their_defaults_and_noisy_kwargs():
    from experiments.base import parser_argument as pa

    p, names, parser = _parse([])
    assert "noisy_nets" in names and "noisy_sigma0" in names and p["noisy_nets"] is False and p["noisy_sigma0"] == 0.5
    assert pa.noisy_kwargs(p) == {}  # without -noisy: the keywords of before the flag
    assert pa.noisy_kwargs(_parse(["-noisys", "0.1"])[0]) == {}  # -noisys means nothing without -noisy
    for algo in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn"):
        assert pa.noisy_kwargs(_parse(["-noisy"], algo=algo)[0]) == dict(noisy=True, noisy_sigma0=0.5)
    assert pa.noisy_kwargs(_parse(["--noisy_nets", "--noisy_sigma0", "0.25"])[0]) == dict(noisy=True, noisy_sigma0=0.25)
    # the README's Rainbow line parses, and the epsilon flags keep their own values
    rainbow = "-noisy -duel -dq -per -pe 0.5 -isb 0.4 -isbe 1 -n 3 -hl -cat -nb 51 -minn -10.2 -maxn 10.2 -ee 0 -ed 1".split()
    p = _parse(rainbow)[0]
    assert p["noisy_nets"] and p["epsilon_end"] == 0 and p["epsilon_duration"] == 1 and p["dueling"] and p["categorical"]
    assert _parse(["-noisy"])[0]["epsilon_end"] == 0.01


def test_check_noisy_says_every_refusal_in_the_librarys_order():
    from slimdqn import _engine

    check = _engine.check_noisy
    check(False, "impala", True, 10.0, True)  # off: nothing to refuse
    check(True, "cnn")
    check(True, "fc", False, 0.0, False)
    for args, msg in (((True, "impala", True, 10.0, True), _engine.NOISY_BATCH_NORM_REFUSED), ((True, "impala", False, 10.0, True), _engine.NOISY_IMPALA_REFUSED),
                      ((True, "cnn", False, 10.0, True), _engine.NOISY_GRAD_CLIP_REFUSED), ((True, "cnn", False, float("inf")), _engine.NOISY_GRAD_CLIP_REFUSED),
                      ((True, "cnn", False, 0.0, True), _engine.NOISY_REDO_REFUSED)):
        with pytest.raises(ValueError) as e:
            check(*args)
        assert str(e.value) == msg


@pytest.mark.parametrize("env,algo,extra", [("atari", "isdqn", ["-noisy", "-bn"]), ("atari", "tfdqn", ["-noisy", "-bn"]),
                                            ("atari", "dqn", ["-noisy", "-at", "impala", "-f", "8", "8", "8", "16"]),
                                            ("atari", "analysisdqn", ["-noisy", "-gc", "10", "-at", "cnn", "-f", "8", "8", "8", "16"]),
                                            ("lunar_lander", "dqn", ["-noisy", "-redo", "200"]), ("lunar_lander", "isdqn", ["-noisy", "-gc", "inf"])])
def test_noisy_on_what_it_is_not_built_for_is_refused_before_anything_is_written(tmp_path, env, algo, extra):
    from experiments.base.utils import prepare_logs

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, ["-en", "g_Game", "-dw", "-s", "1"] + extra, root=str(tmp_path))
    assert "noisy layers" in str(e.value)
    assert not (tmp_path / env).exists()  # before the output directory is created
    prepare_logs(env, algo, ["-en", "g_Game", "-dw", "-s", "1"] + [a for a in extra if a != "-noisy"], root=str(tmp_path))  # without -noisy they pass


def test_parameters_json_keeps_the_reference_groups(tmp_path):
    """Like the other engine flags (-hl, -qr, -duel, -gc), -noisy and -noisys stay out of parameters.json."""
    from experiments.base.utils import prepare_logs

    for env, algo in (("atari", "isdqn"), ("lunar_lander", "dqn")):
        p = prepare_logs(env, algo, ["-en", f"b{algo}_Game", "-dw", "-s", "1", "-noisy", "-noisys", "0.3"], root=str(tmp_path))
        assert p["noisy_nets"] and p["noisy_sigma0"] == 0.3
        on = json.load(open(tmp_path / env / "exp_output" / f"b{algo}_Game" / "parameters.json"))
        prepare_logs(env, algo, ["-en", f"a{algo}_Game", "-dw", "-s", "1"], root=str(tmp_path))
        plain = json.load(open(tmp_path / env / "exp_output" / f"a{algo}_Game" / "parameters.json"))
        assert not any("noisy" in k for k in list(on[algo]) + list(on["shared_parameters"]))
        assert set(on[algo]) == set(plain[algo]) and set(on["shared_parameters"]) == set(plain["shared_parameters"])


def test_entry_points_pass_the_keywords_to_their_agents():
    base = os.path.join(ROOT, "is-dqn_amd", "experiments")
    for rel in ("atari/isdqn.py", "atari/dqn.py", "atari/analysisdqn.py", "lunar_lander/isdqn.py", "lunar_lander/dqn.py",
                "atari/tfdqn.py", "atari/analysistfdqn.py", "lunar_lander/tfdqn.py"):
        assert "**noisy_kwargs(p)" in open(os.path.join(base, rel)).read(), rel


def test_agents_take_the_keywords_and_refuse_before_an_engine_is_built():
    from slimdqn import _engine
    from slimdqn._engine import QNetEngine
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    for f in (QNetEngine.__init__, DQN.__init__, iSDQN.__init__, TFDQN.__init__):
        assert inspect.signature(f).parameters["noisy"].default is False and inspect.signature(f).parameters["noisy_sigma0"].default == 0.5
    assert inspect.signature(QNetEngine.__init__).parameters["noisy_seed"].default == 0
    feats = [8, 8, 8, 16]
    isd = lambda **kw: iSDQN(0, (84, 84, 4), 4, 2, feats, True, kw.pop("batch_norm", False), kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    ana = lambda **kw: AnalysisDQN(0, (84, 84, 4), 4, 2, feats, True, kw.pop("batch_norm", False), kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    dqn = lambda **kw: DQN(0, (84, 84, 4), 4, feats, True, kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    tf = lambda **kw: TFDQN(0, (84, 84, 4), 4, feats, True, kw.pop("batch_norm", False), kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    atf = lambda **kw: AnalysisTFDQN(0, (84, 84, 4), 4, feats, True, kw.pop("batch_norm", False), kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    eng = lambda **kw: QNetEngine((84, 84, 4), 4, 3, feats, kw.pop("arch", "cnn"), True, 4, **kw)
    # raised before an engine is built (no GPU here: building one would raise something else)
    for make in (isd, ana, dqn, tf, atf, eng):
        with pytest.raises(ValueError) as e:
            make(noisy=True, arch="impala")
        assert str(e.value) == _engine.NOISY_IMPALA_REFUSED
        with pytest.raises(ValueError) as e:
            make(noisy=True, max_grad_norm=10.0)
        assert str(e.value) == _engine.NOISY_GRAD_CLIP_REFUSED
    for make in (isd, ana, tf, atf, eng):
        with pytest.raises(ValueError) as e:
            make(noisy=True, batch_norm=True)
        assert str(e.value) == _engine.NOISY_BATCH_NORM_REFUSED
