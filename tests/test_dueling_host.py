"""Dueling value / advantage heads (include/isdqn_hip.h, isdqn_net_config::dueling) without a GPU: the float64 restatement of
tests/helpers/dueling.py against a plain loop, torch autograd and five wrong readings of the header; the structural-zero indices of
the internal layout; the struct layout; the workspace plan with the option off and on; the C ABI's refusals; the flag, the agents'
refusals and the entry points."""
import argparse
import ctypes
import inspect
import json
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from tests.helpers import dueling as du

SHAPES = [(1, 1, 1), (1, 3, 1), (4, 18, 1), (2, 3, 2), (3, 5, 51), (1, 2, 200)]  # (H, A, w)


# ------------------------------------------------------------------ 1. the helper: loops, autograd, wrong readings
@pytest.mark.parametrize("shape", SHAPES)
def test_combine_equals_the_plain_loop(shape):
    H, A, w = shape
    raw = np.random.default_rng(H + A + w).normal(size=(5, du.raw_width(H, A, w)))
    np.testing.assert_allclose(du.combine(raw, H, A, w).numpy(), du.combine_loops(raw, H, A, w), rtol=0, atol=1e-14)


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_is_the_transpose_of_combine_by_autograd(shape):
    H, A, w = shape
    rng = np.random.default_rng(7 * H + A + w)
    raw = torch.tensor(rng.normal(size=(4, du.raw_width(H, A, w))), dtype=torch.float64, requires_grad=True)
    d = rng.normal(size=(4, H * A * w))
    (du.combine(raw, H, A, w) * torch.from_numpy(d)).sum().backward()
    np.testing.assert_allclose(du.backward(d, H, A, w), raw.grad.numpy(), rtol=0, atol=1e-13)
    # a vector (the reduced head-bias gradient) takes the same map
    np.testing.assert_array_equal(du.backward(d[0], H, A, w), du.backward(d[:1], H, A, w)[0])


def test_one_nonzero_per_row_head_and_component_reaches_the_value_row_unchanged():
    H, A, w = 3, 5, 4
    rng = np.random.default_rng(2)
    d = np.zeros((6, H, A, w))
    for n in range(6):
        for h in range(H):
            for j in range(w):
                d[n, h, rng.integers(A), j] = rng.normal()
    draw = du.backward(d.reshape(6, -1), H, A, w).reshape(6, H, A + 1, w)
    assert np.array_equal(draw[:, :, A], d.sum(2))  # adding zeros is exact: bit for bit
    assert np.array_equal(np.sort(np.abs(draw[:, :, A]), axis=None), np.sort(np.abs(d[d != 0])))


def _hand_example():
    """One row, one head, A = 3, w = 2, worked by hand: adv = [[1, 10], [2, 20], [6, 60]], value = [100, 1000].
    mean = [3, 30]; out[a][j] = value[j] + adv[a][j] - mean[j]."""
    raw = np.array([[1.0, 10.0, 2.0, 20.0, 6.0, 60.0, 100.0, 1000.0]])
    want = np.array([[98.0, 980.0, 99.0, 990.0, 103.0, 1030.0]])
    return raw, want


WRONG = {
    "no mean subtraction": lambda adv, val, A: val + adv,
    "sum instead of mean": lambda adv, val, A: val + (adv - adv.sum(2, keepdims=True)),
    "mean over A + 1": lambda adv, val, A: val + (adv - adv.sum(2, keepdims=True) / (A + 1)),
}


def test_helper_is_the_hand_example_and_tells_the_wrong_readings_apart():
    raw, want = _hand_example()
    H, A, w = 1, 3, 2
    assert np.array_equal(du.combine(raw, H, A, w).numpy(), want)
    assert np.array_equal(du.combine_loops(raw, H, A, w), want)
    r = raw.reshape(1, H, A + 1, w)
    for name, f in WRONG.items():
        got = f(r[:, :, :A], r[:, :, A:], A).reshape(1, -1)
        assert not np.allclose(got, want), name
    # value row first: the same numbers read as [value, adv_0 .. adv_{A-1}]
    first = r[:, :, 1:] + 0.0
    got = (r[:, :, :1] + (first - first.sum(2, keepdims=True) / A)).reshape(1, -1)
    assert not np.allclose(got, want), "value row first"
    assert du.raw_index(0, A, 0, A, w) == A * w and du.raw_index(1, 0, 1, A, w) == (A + 1) * w + 1  # the value row is the LAST of a head


def test_live_mask_puts_the_value_stream_on_the_first_half():
    F, H, A, w = 6, 2, 2, 2
    m = du.live_mask(F, H, A, w)
    assert m.shape == (F, H * (A + 1) * w) and m.sum(0).tolist() == [F // 2] * m.shape[1]
    for h in range(H):
        for j in range(w):
            assert m[:3, du.raw_index(h, A, j, A, w)].all() and not m[3:, du.raw_index(h, A, j, A, w)].any()
            for a in range(A):
                assert m[3:, du.raw_index(h, a, j, A, w)].all() and not m[:3, du.raw_index(h, a, j, A, w)].any()
    swapped = ~m  # mask halves swapped: a different network
    assert not np.array_equal(swapped, m) and (swapped != m).all()
    # through the network: a kernel that is live only where the swapped mask is gives another raw row
    rng = np.random.default_rng(0)
    x, k = rng.normal(size=(1, F)), rng.normal(size=m.shape)
    assert not np.allclose(x @ (k * m), x @ (k * swapped))


@pytest.mark.parametrize("F", [14, 20, 2, 512])  # halves 7 and 10: no multiple of 8, a group of 8 straddles the two streams
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 1), (2, 3, 5)])
def test_structural_indices_of_the_internal_layout(F, shape):
    from slimdqn import _engine

    H, A, w = shape
    R, in_p = du.raw_width(H, A, w), (F + 7) // 8 * 8
    R_p = (R + 7) // 8 * 8
    live = du.live_mask(F, H, A, w)
    assert np.array_equal(live, _engine.dueling_live_mask(F, H, A, w))  # the engine's own mask is the helper's
    internal = np.zeros((R_p, in_p))  # the engine's [out padded][in padded] form of an all-ones kernel with the zeros written
    internal[:R, :F] = live.T
    idx = du.structural_indices(F, in_p, H, A, w)
    assert idx.size == R * (F // 2) and np.all(np.diff(idx) > 0)
    flat = internal.reshape(-1)
    assert (flat[idx] == 0).all()
    rest = np.ones(flat.size, bool)
    rest[idx] = False
    pad = np.ones((R_p, in_p), bool)
    pad[:R, :F] = False
    assert np.array_equal(flat[rest] == 0, pad.reshape(-1)[rest])  # every other zero is padding


@pytest.mark.parametrize("shape", SHAPES)
def test_bounds_hold_for_a_float32_evaluation_in_the_header_order(shape):
    H, A, w = shape
    rng = np.random.default_rng(11 + A)
    raw = rng.normal(0, 3, (7, du.raw_width(H, A, w))).astype(np.float32)
    r = raw.reshape(7, H, A + 1, w)
    s = np.zeros((7, H, w), np.float32)
    for a in range(A):
        s = (s + r[:, :, a]).astype(np.float32)
    mean = (s / np.float32(A)).astype(np.float32)
    out = (r[:, :, A:] + (r[:, :, :A] - mean[:, :, None]).astype(np.float32)).astype(np.float32).reshape(7, -1)
    err = np.abs(out.astype(np.float64) - du.combine(raw.astype(np.float64), H, A, w).numpy())
    assert (err <= du.combine_bound(raw, H, A, w)).all()
    d = rng.normal(size=(7, H * A * w)).astype(np.float32)
    x = d.reshape(7, H, A, w)
    s = np.zeros((7, H, w), np.float32)
    for a in range(A):
        s = (s + x[:, :, a]).astype(np.float32)
    m = (s / np.float32(A)).astype(np.float32)
    got = np.concatenate([(x - m[:, :, None]).astype(np.float32), s[:, :, None]], 2).reshape(7, -1)
    err = np.abs(got.astype(np.float64) - du.backward(d.astype(np.float64), H, A, w))
    assert (err <= du.backward_bound(d, H, A, w)).all()


# ------------------------------------------------------------------ 2. struct layout and header
def test_struct_layout_and_the_header_text(tmp_path):
    from slimdqn import _hip

    text = open(os.path.join(ROOT, "include", "isdqn_hip.h")).read()
    body = " ".join(text[text.index("int32_t dueling;"):text.index("int32_t layer_norm;")].replace("*", " ").split())
    for phrase in ("R = H (A + 1) w", "structural zero", "mean = s / (float)A", "out[(h A + a) w + j] = raw[A][j] + (raw[a][j] - mean)",
                   "draw[A][j] = sum_a d[a][j]", "draw[a][j] = d[a][j] - draw[A][j] / (float)A", "head_raw", "head_raw_target", "dout_raw", "dbh_raw",
                   "spans both halves", "5456"):
        assert phrase in body, phrase
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "isdqn_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(isdqn_net_config), offsetof(isdqn_net_config, n_heads),'
                   ' offsetof(isdqn_net_config, dueling), offsetof(isdqn_net_config, layer_norm)); return 0; }\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses
    exe = tmp_path / "layout"
    subprocess.check_call([hipcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_h, o_d, o_l = (int(x) for x in subprocess.check_output([str(exe)]).split())
    N = _hip.NetConfig
    assert size == ctypes.sizeof(N) and (o_h, o_d, o_l) == (N.n_heads.offset, N.dueling.offset, N.layer_norm.offset)
    assert o_d == o_h + 4 and o_l == o_d + 4 and N.hl_sigma.offset + 8 == size and N.double_q.offset + 4 == size


# ------------------------------------------------------------------ 3. the plan and the refusals of the C ABI
@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


def _cfg(dueling=None, arch="cnn", feats=(32, 64, 64, 512), n_bins=0, n_quantiles=0, double_q=0, n_heads=4, n_actions=9, batch_norm=0, tau=0.0,
         categorical=0, B=32):
    from slimdqn import _hip

    c = _hip.NetConfig()
    c.arch = {"cnn": _hip.ARCH_CNN, "fc": _hip.ARCH_FC, "impala": _hip.ARCH_IMPALA}[arch]
    c.obs_h, c.obs_w, c.obs_c = (84, 84, 4) if arch != "fc" else (1, 1, 8)
    c.n_features = len(feats)
    for i, f in enumerate(feats):
        c.features[i] = f
    c.n_actions, c.n_heads, c.layer_norm, c.batch_size = n_actions, n_heads, 1, B
    c.precision = _hip.PRECISION_BF16X3
    c.gamma_n, c.learning_rate, c.adam_b1, c.adam_b2, c.adam_eps = 0.99, 1e-4, 0.9, 0.999, 1e-8
    c.batch_norm, c.n_bins, c.n_quantiles, c.categorical, c.double_q = batch_norm, n_bins, n_quantiles, categorical, double_q
    if n_bins:
        c.hl_min, c.hl_max, c.hl_sigma = -10.0, 10.0, 0.3
    c.munchausen_tau, c.munchausen_alpha, c.munchausen_clip = tau, 0.9, -1.0
    if dueling is not None:
        c.dueling = dueling
    return c


def _bytes(lib, cfg):
    b = ctypes.c_int64()
    return lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)), b.value


def _region_table(lib, cfg, names):
    out = {}
    for n in names:
        off, size = ctypes.c_int64(), ctypes.c_int64()
        rc = lib.isdqn_net_workspace_region(ctypes.byref(cfg), n.encode(), ctypes.byref(off), ctypes.byref(size))
        out[n] = (off.value, size.value) if rc == 0 else None
    return out


def _infos(lib, cfg):
    from slimdqn import _hip

    n, cnt = ctypes.c_int64(), ctypes.c_int32()
    assert lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), None, 0, ctypes.byref(cnt)) == _hip.OK
    infos = (_hip.TensorInfo * cnt.value)()
    assert lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)) == _hip.OK
    return n.value, {i.name.decode(): i for i in infos}


REGIONS = ["q", "logits", "dout", "da", "slab", "q_values", "targets", "dbh", "adam_consts", "loss_partials", "wsplit", "q_target", "logits_target",
           "act/Conv_0", "z/Conv_1", "dz/Conv_2", "act/Dense_0", "red/Dense_0", "part/Dense_0", "gw/Conv_0", "gw/Dense_0", "gw/Dense_1"]
NEW = ["head_raw", "head_raw_target", "dout_raw", "dbh_raw"]


@pytest.mark.parametrize("kw", [dict(), dict(n_bins=51), dict(n_quantiles=32), dict(double_q=1), dict(n_bins=51, double_q=1), dict(tau=0.03),
                                dict(n_heads=1), dict(arch="fc", feats=(20, 14)), dict(batch_norm=1), dict(arch="impala")])
def test_workspace_plan_with_the_option_off_is_the_plan_without_the_field(lib, kw):
    from slimdqn import _hip

    never, off = _cfg(None, **kw), _cfg(0, **kw)
    (rc0, b0), (rc1, b1) = _bytes(lib, never), _bytes(lib, off)
    assert rc0 == rc1 == _hip.OK and b0 == b1
    assert _region_table(lib, never, REGIONS) == _region_table(lib, off, REGIONS)
    assert all(v is None for v in _region_table(lib, off, NEW).values())
    assert _infos(lib, never)[0] == _infos(lib, off)[0]


@pytest.mark.parametrize("kw,w", [(dict(), 1), (dict(n_bins=51), 51), (dict(n_quantiles=33, double_q=1), 33), (dict(tau=0.03), 1), (dict(n_heads=1, double_q=1), 1)])
def test_workspace_plan_with_dueling_appends_four_regions_and_widens_the_head(lib, kw, w):
    from slimdqn import _hip

    off, on = _cfg(0, **kw), _cfg(1, **kw)
    (rc0, b0), (rc1, b1) = _bytes(lib, off), _bytes(lib, on)
    assert rc0 == rc1 == _hip.OK
    H, A, B = on.n_heads, on.n_actions, on.batch_size
    R = H * (A + 1) * w
    R_p = (R + 7) // 8 * 8
    new = _region_table(lib, on, NEW)
    qt = _region_table(lib, on, ["q_target"])["q_target"]
    assert new["head_raw"][1] >= 2 * B * R_p * 4 and new["dout_raw"][1] >= B * R_p * 4 and new["dbh_raw"][1] >= R_p * 4
    assert (new["head_raw_target"] is None) == (qt is None)
    if qt is not None:
        rows = 2 * B if kw.get("tau") else B
        assert new["head_raw_target"][1] >= rows * R_p * 4
    # behind every region the option shares with the off plan, in the order of the header, and the last one ends the workspace
    old = {n: v for n, v in _region_table(lib, on, REGIONS).items() if v is not None}
    order = [new[n] for n in NEW if new[n] is not None]
    assert min(o for o, _ in order) >= max(o + s for o, s in old.values())
    assert [o for o, _ in order] == sorted(o for o, _ in order) and order[-1][0] + order[-1][1] == b1
    # the combined rows keep the pitch and size they have without the option
    for name in ("q", "logits", "dout", "dbh", "q_target", "logits_target", "loss_partials"):
        a, b = _region_table(lib, off, [name])[name], _region_table(lib, on, [name])[name]
        assert (a is None) == (b is None) and (a is None or a[1] == b[1]), name
    head = _infos(lib, on)[1]["Dense_1/kernel"]
    assert tuple(head.flax_shape[:2]) == (512, R) and tuple(head.dims[:2]) == (R_p, 512)
    assert tuple(_infos(lib, on)[1]["Dense_1/bias"].flax_shape[:1]) == (R,)


def test_every_refusal_returns_its_code(lib):
    from slimdqn import _hip

    table = [
        (dict(dueling=2), _hip.ERR_ARG),
        (dict(dueling=-1), _hip.ERR_ARG),
        (dict(dueling=1, feats=(32, 64, 64, 511)), _hip.ERR_ARG),  # F odd
        (dict(dueling=1, feats=(32, 64, 64)), _hip.ERR_ARG),  # no hidden Dense in front of the head
        (dict(dueling=1, arch="fc", feats=()), _hip.ERR_ARG),
        (dict(dueling=1, arch="fc", feats=(20, 15)), _hip.ERR_ARG),
        (dict(dueling=1, batch_norm=1), _hip.ERR_UNSUPPORTED),
        (dict(dueling=1, arch="impala"), _hip.ERR_UNSUPPORTED),
        (dict(dueling=1, n_bins=51, n_heads=10, n_actions=10), _hip.ERR_UNSUPPORTED),  # R = 5610 > 5456 although 5100 logits fit
        (dict(dueling=1, n_quantiles=31, n_heads=4, n_actions=44), _hip.ERR_UNSUPPORTED),  # 5456 combined values, R = 5580
        (dict(dueling=1, n_heads=66, n_actions=2), _hip.ERR_UNSUPPORTED),  # K = 65 regressed heads
        (dict(dueling=1, n_quantiles=2, n_heads=66, n_actions=2), _hip.ERR_UNSUPPORTED),
    ]
    for kw, code in table:
        rc, _ = _bytes(lib, _cfg(**kw))
        assert rc == code, (kw, rc, lib.isdqn_last_error())
    ok = [dict(dueling=1), dict(dueling=1, n_heads=1), dict(dueling=1, n_actions=1), dict(dueling=1, arch="fc", feats=(20, 14)),
          dict(dueling=1, n_heads=65, n_actions=2), dict(dueling=1, n_bins=51, n_heads=4, n_actions=18, categorical=1),
          dict(dueling=1, n_quantiles=31, n_heads=4, n_actions=43),  # R = 5456
          dict(dueling=1, n_heads=4, n_actions=18, double_q=1), dict(dueling=1, tau=0.03), dict(dueling=1, feats=(32, 64, 64, 64, 2))]
    for kw in ok:
        assert _bytes(lib, _cfg(**kw))[0] == _hip.OK, (kw, lib.isdqn_last_error())


# ------------------------------------------------------------------ 4. the flag, check_dueling, the agents and the entry points
def _parse(argv, algo="isdqn"):
    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    getattr(pa, f"add_{algo}_arguments")(parser)
    names = pa.add_engine_arguments(parser)
    return vars(parser.parse_args(["-en", "x_Game", "-s", "1"] + argv)), names, parser


def test_the_flag_its_default_and_dueling_kwargs():
    from experiments.base import parser_argument as pa

    p, names, parser = _parse([])
    assert "dueling" in names and p["dueling"] is False
    assert pa.dueling_kwargs(p) == {}  # without -duel: the keywords of before the flag
    for algo in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn"):
        assert pa.dueling_kwargs(_parse(["-duel"], algo=algo)[0]) == dict(dueling=True)
    assert pa.dueling_kwargs(_parse(["--dueling"])[0]) == dict(dueling=True)
    assert "Wang et al. 2016" in " ".join(parser.format_help().split())


def test_check_dueling_says_every_refusal_and_nothing_else():
    from slimdqn import _engine

    check = _engine.check_dueling
    check(False, "impala", [1, 2, 3], True)  # off: nothing to refuse
    check(True, "cnn", [32, 64, 64, 512])
    check(True, "fc", [100, 100])
    for args, msg in (((True, "impala", [8, 8, 8, 16]), _engine.DUELING_IMPALA_REFUSED), ((True, "cnn", [8, 8, 8, 16], True), _engine.DUELING_BATCH_NORM_REFUSED),
                      ((True, "cnn", [8, 8, 8]), _engine.DUELING_NEEDS_HIDDEN_DENSE), ((True, "fc", []), _engine.DUELING_NEEDS_HIDDEN_DENSE),
                      ((True, "cnn", [8, 8, 8, 15]), _engine.DUELING_ODD_WIDTH_REFUSED), ((True, "fc", [20, 7]), _engine.DUELING_ODD_WIDTH_REFUSED)):
        with pytest.raises(ValueError) as e:
            check(*args)
        assert str(e.value) == msg


@pytest.mark.parametrize("env,algo,extra", [("atari", "isdqn", ["-bn"]), ("atari", "tfdqn", ["-bn"]), ("atari", "dqn", ["-at", "impala", "-f", "8", "8", "8", "16"]),
                                            ("atari", "analysisdqn", ["-at", "cnn", "-f", "8", "8", "8"]), ("lunar_lander", "dqn", ["-f", "20", "7"]),
                                            ("lunar_lander", "isdqn", ["-f"])])
def test_duel_on_a_network_it_is_not_built_for_is_refused_before_anything_is_written(tmp_path, env, algo, extra):
    from experiments.base.utils import prepare_logs

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, ["-en", "d_Game", "-dw", "-s", "1", "-duel"] + extra, root=str(tmp_path))
    assert "dueling" in str(e.value)
    assert not (tmp_path / env).exists()  # before the output directory is created
    prepare_logs(env, algo, ["-en", "d_Game", "-dw", "-s", "1"] + extra, root=str(tmp_path))  # without -duel the same flags pass


def test_parameters_json_keeps_the_reference_groups(tmp_path):
    """Like the other engine flags (-hl, -qr, -prec), -duel stays out of parameters.json."""
    from experiments.base.utils import prepare_logs

    for env, algo in (("atari", "isdqn"), ("lunar_lander", "dqn")):
        p = prepare_logs(env, algo, ["-en", f"b{algo}_Game", "-dw", "-s", "1", "-duel"], root=str(tmp_path))
        assert p["dueling"] is True
        on = json.load(open(tmp_path / env / "exp_output" / f"b{algo}_Game" / "parameters.json"))
        prepare_logs(env, algo, ["-en", f"a{algo}_Game", "-dw", "-s", "1"], root=str(tmp_path))
        plain = json.load(open(tmp_path / env / "exp_output" / f"a{algo}_Game" / "parameters.json"))
        assert not any("dueling" in k for k in list(on[algo]) + list(on["shared_parameters"]))
        assert set(on[algo]) == set(plain[algo]) and set(on["shared_parameters"]) == set(plain["shared_parameters"])


def test_entry_points_pass_the_keyword_to_their_agents():
    base = os.path.join(ROOT, "is-dqn_amd", "experiments")
    for rel in ("atari/isdqn.py", "atari/dqn.py", "atari/analysisdqn.py", "lunar_lander/isdqn.py", "lunar_lander/dqn.py",
                "atari/tfdqn.py", "atari/analysistfdqn.py", "lunar_lander/tfdqn.py"):
        assert "**dueling_kwargs(p)" in open(os.path.join(base, rel)).read(), rel


def test_agents_take_the_keyword_and_refuse_before_an_engine_is_built():
    from slimdqn import _engine
    from slimdqn._engine import QNetEngine
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    for f in (QNetEngine.__init__, DQN.__init__, iSDQN.__init__, TFDQN.__init__):
        assert inspect.signature(f).parameters["dueling"].default is False
    feats = [8, 8, 8, 15]
    isd = lambda **kw: iSDQN(0, (84, 84, 4), 4, 2, kw.pop("features", feats), True, kw.pop("batch_norm", False), "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    ana = lambda **kw: AnalysisDQN(0, (84, 84, 4), 4, 2, kw.pop("features", feats), True, kw.pop("batch_norm", False), "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    dqn = lambda **kw: DQN(0, (84, 84, 4), 4, kw.pop("features", feats), True, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    tf = lambda **kw: TFDQN(0, (84, 84, 4), 4, kw.pop("features", feats), True, kw.pop("batch_norm", False), "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    atf = lambda **kw: AnalysisTFDQN(0, (84, 84, 4), 4, kw.pop("features", feats), True, kw.pop("batch_norm", False), "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    eng = lambda **kw: QNetEngine((84, 84, 4), 4, 3, kw.pop("features", feats), "cnn", True, 4, **kw)
    # raised before an engine is built (no GPU here: building one would raise something else)
    for make in (isd, ana, dqn, tf, atf, eng):
        with pytest.raises(ValueError) as e:
            make(dueling=True)
        assert str(e.value) == _engine.DUELING_ODD_WIDTH_REFUSED
        with pytest.raises(ValueError) as e:
            make(dueling=True, features=[8, 8, 8])
        assert str(e.value) == _engine.DUELING_NEEDS_HIDDEN_DENSE
    for make in (isd, ana, tf, atf, eng):
        with pytest.raises(ValueError) as e:
            make(dueling=True, features=[8, 8, 8, 16], batch_norm=True)
        assert str(e.value) == _engine.DUELING_BATCH_NORM_REFUSED
