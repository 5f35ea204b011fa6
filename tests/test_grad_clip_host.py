"""Global-norm gradient clipping, the part that needs no GPU (include/isdqn_hip.h, isdqn_net_config::max_grad_norm):

1. the float64 reference of tests/helpers/grad_clip.py against torch.nn.utils.clip_grad_norm_ and against optax's behaviour at the
   edges (n < c, n == c, n == 0, c = inf), and the named wrong readings against the tolerance the GPU tests hold the device to;
2. the struct layout, the plan with the option off and on, and the C ABI's refusals (the plan is host code);
3. the flag, check_grad_clip, grad_clip_kwargs, the entry points and the agents' refusals before an engine is built."""
import argparse
import ctypes
import inspect
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import grad_clip as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 2.0**-23  # the GPU tests' tolerance on norm and scale (tests/test_gpu_grad_clip.py: one fp32 rounding of a float64 value, doubled)
# the leaves of the GPU tests' fc case in the internal layout (obs 8 -> 100 -> 100 -> 8 outputs, LayerNorm): kernels, biases, scales
FC_LEAVES = [(104, 8), (104,), (104,), (104,), (104, 104), (104,), (104,), (104,), (8, 104), (8,)]


def _leaves(seed=0, spread=True):
    rng = np.random.default_rng(seed)
    # (leaf scales two orders of magnitude apart, as the device's are: biases and LayerNorm leaves far above the first kernel)
    return [(rng.normal(size=s) * (10.0 ** rng.uniform(-3, -1) if spread else 1.0)).astype(np.float32) for s in FC_LEAVES]


# ------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("factor", [0.1, 0.5, 0.9, 1.1, 2.0, 50.0])
def test_reference_equals_torch_clip_grad_norm_away_from_the_threshold(factor):
    leaves = _leaves(1)
    n = gc.global_norm(leaves)
    c = factor * n
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in leaves]
    for p, g in zip(ps, leaves):
        p.grad = torch.from_numpy(g.astype(np.float64))
    total = float(torch.nn.utils.clip_grad_norm_(ps, c))
    assert abs(total - n) <= 1e-12 * n
    for p, want in zip(ps, gc.clipped(leaves, c)):
        got = p.grad.numpy()
        assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want) + 1e-300)  # (torch divides by n + 1e-6)


def test_reference_has_optax_behaviour_at_the_edges():
    leaves = _leaves(2)
    n = gc.global_norm(leaves)
    assert n == float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in leaves)))
    assert gc.clip_scale(n, 2 * n) == 1.0 and gc.clip_scale(n, np.nextafter(n, np.inf)) == 1.0  # n < c: untouched
    assert gc.clip_scale(n, n) == 1.0  # n == c: optax's select takes the c / n branch, which is 1
    assert gc.clip_scale(n, np.nextafter(n, 0.0)) < 1.0
    assert gc.clip_scale(n, 0.5 * n) == 0.5
    assert gc.clip_scale(0.0, 1.0) == 1.0 and gc.clip_scale(0.0, np.inf) == 1.0  # n == 0: no 0 / 0
    assert gc.clip_scale(n, np.inf) == 1.0 and gc.clip_scale(1e30, np.inf) == 1.0
    for g, h in zip(leaves, gc.clipped(leaves, np.inf)):
        assert np.array_equal(h, g.astype(np.float64))
    zero = [np.zeros(s, np.float32) for s in FC_LEAVES]
    assert gc.global_norm(zero) == 0.0 and all(np.all(h == 0) and np.isfinite(h).all() for h in gc.clipped(zero, 1.0))
    # a mask takes its elements out of the norm and out of the result
    mask = [None] * len(leaves)
    mask[4] = np.arange(104 * 104).reshape(104, 104) % 2 == 0
    nm = gc.global_norm(leaves, mask)
    assert nm < n and abs(nm**2 + float((leaves[4].astype(np.float64)[~mask[4]] ** 2).sum()) - n**2) <= 1e-12 * n**2
    assert np.all(gc.clipped(leaves, 0.5 * nm, mask)[4][~mask[4]] == 0)


def _max_rel_diff(a, b):
    """largest |a - b| over a leaf, relative to the leaf's largest |b| (0 where both are zero)"""
    worst = 0.0
    for x, y in zip(a, b):
        top = float(np.abs(y).max())
        if top > 0:
            worst = max(worst, float(np.abs(x - y).max()) / top)
        elif float(np.abs(x).max()) > 0:
            worst = np.inf
    return worst


def test_every_wrong_reading_leaves_the_gpu_tolerance_at_one_of_the_gpu_thresholds():
    """The GPU tests run at c in {0.5 n, 2 n, inf} and hold scale and norm to 2^-23 relative; a reading that stayed inside that at all
    three thresholds could not be told from the definition.  (norm_with_structural needs a mask: it is exercised with one.)"""
    leaves = _leaves(3)
    mask = [None] * len(leaves)
    mask[8] = np.arange(8 * 104).reshape(8, 104) % 104 < 52
    n = gc.global_norm(leaves, mask)
    for name, wrong in gc.WRONG.items():
        worst = max(_max_rel_diff(wrong(leaves, c, mask), gc.clipped(leaves, c, mask)) for c in (0.5 * n, 2 * n))
        assert worst > 1000 * REL, (name, worst)
    # at c = inf every reading but clip-by-value's is the identity: that threshold proves "exactly 1.0f", not the readings
    assert _max_rel_diff(gc.per_leaf_norms(leaves, np.inf, mask), gc.clipped(leaves, np.inf, mask)) == 0.0


# ------------------------------------------------------------------ 2. struct layout, plan, refusals of the C ABI
def test_struct_layout_and_the_header_text(tmp_path):
    from slimdqn import _hip

    text = open(os.path.join(ROOT, "include", "isdqn_hip.h")).read()
    body = " ".join(text[text.index("float max_grad_norm;"):text.index("float huber_delta;")].replace("*", " ").split())
    for phrase in ("optax.clip_by_global_norm", "scale = 1 if n < c or n == 0, else c / n", "Adam consumes fl32(g scale)", "float64", "without atomics",
                   "grad_clip_partials", '"grad_clip"', "structural zeros", "unclipped", "ISDQN_ERR_UNSUPPORTED: batch_norm, arch impala"):
        assert phrase in body, phrase
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "isdqn_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(isdqn_net_config), offsetof(isdqn_net_config, adam_eps),'
                   ' offsetof(isdqn_net_config, max_grad_norm), offsetof(isdqn_net_config, huber_delta)); return 0; }\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses
    exe = tmp_path / "layout"
    subprocess.check_call([hipcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_e, o_g, o_h = (int(x) for x in subprocess.check_output([str(exe)]).split())
    N = _hip.NetConfig
    assert size == ctypes.sizeof(N) and (o_e, o_g, o_h) == (N.adam_eps.offset, N.max_grad_norm.offset, N.huber_delta.offset)
    assert o_g == o_e + 4 and o_h == o_g + 4 and N.hl_sigma.offset + 8 == size and N.double_q.offset + 4 == size
    # the fields the header keeps contiguous still are
    names = [f[0] for f in N._fields_]
    i = names.index("huber_delta")
    assert names[i:i + 11] == ["huber_delta", "munchausen_tau", "munchausen_alpha", "munchausen_clip", "batch_norm", "categorical", "n_bins", "n_quantiles",
                               "hl_min", "hl_max", "hl_sigma"]


@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


def _cfg(c=None, arch="cnn", feats=(32, 64, 64, 512), n_bins=0, n_quantiles=0, double_q=0, n_heads=4, n_actions=9, batch_norm=0, dueling=0, B=32):
    from slimdqn import _hip

    cfg = _hip.NetConfig()
    cfg.arch = {"cnn": _hip.ARCH_CNN, "fc": _hip.ARCH_FC, "impala": _hip.ARCH_IMPALA}[arch]
    cfg.obs_h, cfg.obs_w, cfg.obs_c = (84, 84, 4) if arch != "fc" else (1, 1, 8)
    cfg.n_features = len(feats)
    for i, f in enumerate(feats):
        cfg.features[i] = f
    cfg.n_actions, cfg.n_heads, cfg.layer_norm, cfg.batch_size = n_actions, n_heads, 1, B
    cfg.precision = _hip.PRECISION_BF16X3
    cfg.gamma_n, cfg.learning_rate, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps = 0.99, 1e-4, 0.9, 0.999, 1e-8
    cfg.batch_norm, cfg.n_bins, cfg.n_quantiles, cfg.double_q, cfg.dueling = batch_norm, n_bins, n_quantiles, double_q, dueling
    if n_bins:
        cfg.hl_min, cfg.hl_max, cfg.hl_sigma = -10.0, 10.0, 0.3
    cfg.munchausen_alpha, cfg.munchausen_clip = 0.9, -1.0
    if c is not None:
        cfg.max_grad_norm = c
    return cfg


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


REGIONS = ["q", "logits", "dout", "da", "slab", "q_values", "targets", "dbh", "adam_consts", "loss_partials", "wsplit", "q_target", "logits_target",
           "head_raw", "dout_raw", "dbh_raw", "act/Conv_0", "z/Conv_1", "dz/Conv_2", "act/Dense_0", "red/Dense_0", "part/Dense_0", "gw/Conv_0",
           "gw/Dense_0", "gw/Dense_1"]
NEW = ["grad_clip_partials", "grad_clip"]
PLANS = [dict(), dict(n_bins=51), dict(n_quantiles=32, double_q=1), dict(n_heads=1), dict(arch="fc", feats=(100, 100)), dict(dueling=1),
         dict(B=64)]


@pytest.mark.parametrize("kw", PLANS + [dict(batch_norm=1), dict(arch="impala")])
def test_workspace_plan_with_the_option_off_is_the_plan_without_the_field(lib, kw):
    from slimdqn import _hip

    never, off, minus = _cfg(None, **kw), _cfg(0.0, **kw), _cfg(-0.0, **kw)
    (rc0, b0), (rc1, b1), (rc2, b2) = _bytes(lib, never), _bytes(lib, off), _bytes(lib, minus)
    assert rc0 == rc1 == rc2 == _hip.OK and b0 == b1 == b2
    assert _region_table(lib, never, REGIONS) == _region_table(lib, off, REGIONS)
    assert all(v is None for v in _region_table(lib, off, NEW).values())


@pytest.mark.parametrize("kw", PLANS)
@pytest.mark.parametrize("c", [10.0, float("inf"), 1e-30])
def test_workspace_plan_with_clipping_appends_two_regions_behind_everything(lib, kw, c):
    from slimdqn import _hip

    off, on = _cfg(0.0, **kw), _cfg(c, **kw)
    (rc0, b0), (rc1, b1) = _bytes(lib, off), _bytes(lib, on)
    assert rc0 == rc1 == _hip.OK and b1 > b0
    assert _region_table(lib, off, REGIONS) == _region_table(lib, on, REGIONS)  # nothing the off plan has moves or grows
    new = _region_table(lib, on, NEW)
    assert new["grad_clip_partials"][0] == b0 and new["grad_clip"][0] == b0 + new["grad_clip_partials"][1]
    assert new["grad_clip"][0] + new["grad_clip"][1] == b1 and new["grad_clip"][1] >= 16
    # one float64 per workgroup of 64 elements: every tensor rounded up to whole workgroups fits
    n, cnt = ctypes.c_int64(), ctypes.c_int32()
    assert lib.isdqn_net_param_layout(ctypes.byref(on), ctypes.byref(n), None, 0, ctypes.byref(cnt)) == _hip.OK
    infos = (_hip.TensorInfo * cnt.value)()
    assert lib.isdqn_net_param_layout(ctypes.byref(on), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)) == _hip.OK
    assert new["grad_clip_partials"][1] >= 8 * sum((i.size + 63) // 64 for i in infos)
    assert new["grad_clip_partials"][0] % 8 == 0


def test_every_refusal_returns_its_code(lib):
    from slimdqn import _hip

    table = [(dict(c=-1.0), _hip.ERR_ARG), (dict(c=-1e-30), _hip.ERR_ARG), (dict(c=float("nan")), _hip.ERR_ARG), (dict(c=float("-inf")), _hip.ERR_ARG),
             (dict(c=10.0, batch_norm=1), _hip.ERR_UNSUPPORTED), (dict(c=10.0, arch="impala"), _hip.ERR_UNSUPPORTED),
             (dict(c=float("inf"), batch_norm=1), _hip.ERR_UNSUPPORTED), (dict(c=-1.0, batch_norm=1), _hip.ERR_ARG)]
    for kw, code in table:
        rc, _ = _bytes(lib, _cfg(**kw))
        assert rc == code, (kw, rc, lib.isdqn_last_error())
    assert b"gradient clipping" in lib.isdqn_last_error() or b"max_grad_norm" in lib.isdqn_last_error()
    for kw in (dict(c=0.0, batch_norm=1), dict(c=0.0, arch="impala"), dict(c=10.0), dict(c=float("inf"), dueling=1), dict(c=10.0, n_quantiles=51)):
        assert _bytes(lib, _cfg(**kw))[0] == _hip.OK, (kw, lib.isdqn_last_error())


# ------------------------------------------------------------------ 3. the flag, check_grad_clip, the agents and the entry points
def _parse(argv, algo="isdqn"):
    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    getattr(pa, f"add_{algo}_arguments")(parser)
    names = pa.add_engine_arguments(parser)
    return vars(parser.parse_args(["-en", "x_Game", "-s", "1"] + argv)), names, parser


def test_the_flag_its_default_and_grad_clip_kwargs():
    from experiments.base import parser_argument as pa

    p, names, parser = _parse([])
    assert "max_grad_norm" in names and p["max_grad_norm"] == 0.0
    assert pa.grad_clip_kwargs(p) == {}  # without -gc: the keywords of before the flag
    for algo in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn"):
        assert pa.grad_clip_kwargs(_parse(["-gc", "10"], algo=algo)[0]) == dict(max_grad_norm=10.0)
    assert pa.grad_clip_kwargs(_parse(["--max_grad_norm", "inf"])[0]) == dict(max_grad_norm=float("inf"))
    assert pa.grad_clip_kwargs(_parse(["-gc", "0"])[0]) == {}
    assert "optax.clip_by_global_norm" in " ".join(parser.format_help().split())


def test_check_grad_clip_says_every_refusal_and_nothing_else():
    from slimdqn import _engine

    check = _engine.check_grad_clip
    check(0.0, "impala", True)  # off: nothing to refuse
    check(10.0, "cnn")
    check(float("inf"), "fc", False)
    for args, msg in (((10.0, "impala"), _engine.GRAD_CLIP_IMPALA_REFUSED), ((10.0, "cnn", True), _engine.GRAD_CLIP_BATCH_NORM_REFUSED),
                      ((float("inf"), "fc", True), _engine.GRAD_CLIP_BATCH_NORM_REFUSED), ((-1.0, "cnn"), _engine.GRAD_CLIP_NEGATIVE_REFUSED),
                      ((float("nan"), "cnn"), _engine.GRAD_CLIP_NEGATIVE_REFUSED), ((-1.0, "impala", True), _engine.GRAD_CLIP_NEGATIVE_REFUSED)):
        with pytest.raises(ValueError) as e:
            check(*args)
        assert str(e.value) == msg


@pytest.mark.parametrize("env,algo,extra", [("atari", "isdqn", ["-gc", "10", "-bn"]), ("atari", "tfdqn", ["-gc", "inf", "-bn"]),
                                            ("atari", "dqn", ["-gc", "10", "-at", "impala", "-f", "8", "8", "8", "16"]),
                                            ("atari", "analysisdqn", ["-gc", "-1"]), ("lunar_lander", "dqn", ["-gc", "nan"]),
                                            ("lunar_lander", "isdqn", ["-gc", "10", "-bn"])])
def test_gc_on_a_network_it_is_not_built_for_is_refused_before_anything_is_written(tmp_path, env, algo, extra):
    from experiments.base.utils import prepare_logs

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, ["-en", "g_Game", "-dw", "-s", "1"] + extra, root=str(tmp_path))
    assert "gradient clipping" in str(e.value) or "max_grad_norm" in str(e.value)
    assert not (tmp_path / env).exists()  # before the output directory is created
    rest = [a for i, a in enumerate(extra) if a != "-gc" and (i == 0 or extra[i - 1] != "-gc")]
    prepare_logs(env, algo, ["-en", "g_Game", "-dw", "-s", "1"] + rest, root=str(tmp_path))  # without -gc the same flags pass


def test_parameters_json_keeps_the_reference_groups(tmp_path):
    """Like the other engine flags (-hl, -qr, -duel), -gc stays out of parameters.json."""
    from experiments.base.utils import prepare_logs

    for env, algo in (("atari", "isdqn"), ("lunar_lander", "dqn")):
        p = prepare_logs(env, algo, ["-en", f"b{algo}_Game", "-dw", "-s", "1", "-gc", "10"], root=str(tmp_path))
        assert p["max_grad_norm"] == 10.0
        on = json.load(open(tmp_path / env / "exp_output" / f"b{algo}_Game" / "parameters.json"))
        prepare_logs(env, algo, ["-en", f"a{algo}_Game", "-dw", "-s", "1"], root=str(tmp_path))
        plain = json.load(open(tmp_path / env / "exp_output" / f"a{algo}_Game" / "parameters.json"))
        assert not any("grad" in k for k in list(on[algo]) + list(on["shared_parameters"]))
        assert set(on[algo]) == set(plain[algo]) and set(on["shared_parameters"]) == set(plain["shared_parameters"])


def test_entry_points_pass_the_keyword_to_their_agents():
    base = os.path.join(ROOT, "is-dqn_amd", "experiments")
    for rel in ("atari/isdqn.py", "atari/dqn.py", "atari/analysisdqn.py", "lunar_lander/isdqn.py", "lunar_lander/dqn.py",
                "atari/tfdqn.py", "atari/analysistfdqn.py", "lunar_lander/tfdqn.py"):
        assert "**grad_clip_kwargs(p)" in open(os.path.join(base, rel)).read(), rel


def test_agents_take_the_keyword_and_refuse_before_an_engine_is_built():
    from slimdqn import _engine
    from slimdqn._engine import QNetEngine
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    for f in (QNetEngine.__init__, DQN.__init__, iSDQN.__init__, TFDQN.__init__):
        assert inspect.signature(f).parameters["max_grad_norm"].default == 0.0
    feats = [8, 8, 8, 16]
    isd = lambda **kw: iSDQN(0, (84, 84, 4), 4, 2, feats, True, kw.pop("batch_norm", False), kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    ana = lambda **kw: AnalysisDQN(0, (84, 84, 4), 4, 2, feats, True, kw.pop("batch_norm", False), kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    dqn = lambda **kw: DQN(0, (84, 84, 4), 4, feats, True, kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    tf = lambda **kw: TFDQN(0, (84, 84, 4), 4, feats, True, kw.pop("batch_norm", False), kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    atf = lambda **kw: AnalysisTFDQN(0, (84, 84, 4), 4, feats, True, kw.pop("batch_norm", False), kw.pop("arch", "cnn"), 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    eng = lambda **kw: QNetEngine((84, 84, 4), 4, 3, feats, kw.pop("arch", "cnn"), True, 4, **kw)
    # raised before an engine is built (no GPU here: building one would raise something else)
    for make in (isd, ana, dqn, tf, atf, eng):
        for bad in (-1.0, float("nan")):
            with pytest.raises(ValueError) as e:
                make(max_grad_norm=bad)
            assert str(e.value) == _engine.GRAD_CLIP_NEGATIVE_REFUSED
        with pytest.raises(ValueError) as e:
            make(max_grad_norm=10.0, arch="impala")
        assert str(e.value) == _engine.GRAD_CLIP_IMPALA_REFUSED
    for make in (isd, ana, tf, atf, eng):
        with pytest.raises(ValueError) as e:
            make(max_grad_norm=float("inf"), batch_norm=True)
        assert str(e.value) == _engine.GRAD_CLIP_BATCH_NORM_REFUSED
