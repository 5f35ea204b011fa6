"""CPU side of Normalize-and-Project (include/isdqn_hip.h, isdqn_net_project_*): the numpy oracle of tests/helpers/nap.py against the wrong
variants the device tests must be able to tell from it (on THEIR inputs), the layout call, the argument checks and refusals that need no
GPU, the flag and its refusals, the agents' rule, and the build: the kernels' own translation unit and its lint."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from tests.helpers import nap
from tests.helpers import prune as hp

ENTRY_POINTS = [("atari", a) for a in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn")] + [("lunar_lander", a) for a in ("isdqn", "dqn", "tfdqn")]
CONFIGS = ("FC_SMALL", "FC_WIDE", "CNN")
MIN_ULPS = 16


# ------------------------------------------------------------------------------------------------ the oracle and its wrong variants
@pytest.mark.parametrize("config", CONFIGS)
def test_oracle_differs_from_the_wrong_variants_on_the_device_tests_inputs(config):
    """On the "normal" case of the device tests with their target norms, every wrong variant moves the scale of at least one tensor by
    at least 16 float32 ulps in every configuration that can show it: a device result that equals the definition's scales bit for bit
    equals none of them.  Which configuration can show what is asserted too."""
    lay = hp.host_layout(getattr(hp, config))
    p, rho = nap.case_params(lay, "normal"), nap.case_targets(lay)
    out, n, s = nap.project(lay, p, rho)
    assert len(n) == len(s) == len(rho) == len(hp.prunable(lay))
    assert all(x != np.float32(1.0) for x in s)
    # the definition itself: real elements scaled by one float32 multiply, every other float -- the sentinels -- untouched
    keep = nap.not_projected(lay)
    assert (p[keep] == nap.SENTINEL).all() and np.array_equal(hp.bits(out)[keep], hp.bits(p)[keep]) and keep.sum() > 0
    assert np.array_equal(hp.bits(out), hp.bits(nap.scaled(lay, p, s)))
    for info, si in zip(nap.projected(lay), s):
        idx = hp.real_index(lay, info)
        assert np.array_equal(hp.bits(out[idx]), hp.bits(p[idx] * si)) and not (p[idx] == nap.SENTINEL).any()

    def worst(variant, r=rho):
        _, _, s2 = nap.project(lay, p, r, variant)
        return s2

    # padding counted: fc [20, 14] is the configuration with padded rows and lanes in its projected kernels
    padded = any(int(i.size) != r for i, r in zip(hp.prunable(lay), hp.real_counts(lay)))
    assert padded == (config == "FC_SMALL")
    d = [nap.ulps(a, b) for a, b in zip(s, worst("padding"))]
    assert (max(d) >= MIN_ULPS) if padded else (max(d) == 0), d
    # the last Dense projected: the definition leaves it alone (scale 1)
    last = worst("last_dense", rho + [2.0])
    assert [nap.ulps(a, b) for a, b in zip(s, last)] == [0] * len(s) and nap.ulps(last[-1], 1.0) >= MIN_ULPS
    # biases taken into the tensor
    d = [nap.ulps(a, b) for a, b in zip(s, worst("biases"))]
    assert max(d) >= MIN_ULPS, d
    # the norm per output row instead of per tensor
    d = [max(nap.ulps(x, a) for x in rows) for rows, a in zip(worst("per_row"), s)]
    assert max(d) >= MIN_ULPS, d
    # S accumulated in float32: shows in the scale where a tensor has 2^14 terms or more (Dense_1 of fc [256, 256]: 65536; the cnn's
    # Dense_0: 15488 -- just short, but its running sum drifts far enough); tier 1 of the device test sees it on every tensor
    d = [nap.ulps(a, b) for a, b in zip(s, worst("fp32"))]
    assert (max(d) >= MIN_ULPS) == (config != "FC_SMALL"), d
    _, n32, _ = nap.project(lay, p, rho, "fp32")
    counts = hp.real_counts(lay)
    assert any(abs(a / b - 1.0) > c * 2.0 ** -53 for a, b, c in zip(n32, n, counts))


def test_special_tensors_are_left_alone():
    """S = 0, inf or NaN and rho that is not finite or <= 0: scale 1.0f, no element written (a -0.0 keeps its sign)."""
    lay = hp.host_layout(hp.FC_SMALL)
    rho = nap.case_targets(lay)
    p = nap.case_params(lay, "zero")
    out, n, s = nap.project(lay, p, rho)
    assert n[0] == 0.0 and s[0] == np.float32(1.0) and s[1] != np.float32(1.0)
    idx = hp.real_index(lay, nap.projected(lay)[0])
    assert np.array_equal(hp.bits(out[idx]), hp.bits(p[idx])) and np.signbit(out[idx]).any()
    p = nap.case_params(lay, "nonfinite")
    out, n, s = nap.project(lay, p, rho)
    assert n[0] == math.inf and math.isnan(n[1]) and list(s) == [np.float32(1.0)] * 2 and np.array_equal(hp.bits(out), hp.bits(p))
    p = nap.case_params(lay, "normal")
    for bad in (0.0, -1.0, math.inf, math.nan):
        out, n, s = nap.project(lay, p, [bad, rho[1]])
        assert s[0] == np.float32(1.0) and s[1] != np.float32(1.0)
        assert np.array_equal(hp.bits(out[idx]), hp.bits(p[idx])) and not np.array_equal(hp.bits(out), hp.bits(p))
    # denormals are neither flushed on the way in nor on the way out
    p = nap.case_params(lay, "denormal")
    out, n, s = nap.project(lay, p, rho)
    tiny = idx[np.abs(p[idx]) < np.float32(1e-38)]
    assert tiny.size > 0 and (out[tiny] != 0).all() and np.array_equal(hp.bits(out[tiny]), hp.bits(p[tiny] * s[0]))


# ------------------------------------------------------------------------------------------------ the layout call and the argument checks
def _layout_call(lay):
    from slimdqn import _hip

    n, scratch = ctypes.c_int32(), ctypes.c_int64()
    assert lay.lib.isdqn_net_project_layout(ctypes.byref(lay.cfg), ctypes.byref(n), None, 0, ctypes.byref(scratch)) == _hip.OK
    infos = (ctypes.c_int64 * (4 * n.value))()
    assert lay.lib.isdqn_net_project_layout(ctypes.byref(lay.cfg), ctypes.byref(n), infos, n.value, None) == _hip.OK
    return np.array(infos, dtype=np.int64).reshape(n.value, 4), int(scratch.value)


@pytest.mark.parametrize("config", [dict(hp.CNN, features=(32, 64, 64, 512), n_actions=9, n_heads=10), hp.FC_SMALL, hp.FC_WIDE, hp.CNN])
def test_layout_equals_the_prune_layouts_tensors(config):
    lay = hp.host_layout(config)
    infos, scratch = _layout_call(lay)
    n, words, prune_scratch = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
    assert lay.lib.isdqn_net_prune_layout(ctypes.byref(lay.cfg), ctypes.byref(n), None, 0, ctypes.byref(words), ctypes.byref(prune_scratch)) == 0
    pruned = (ctypes.c_int64 * (4 * n.value))()
    assert lay.lib.isdqn_net_prune_layout(ctypes.byref(lay.cfg), ctypes.byref(n), pruned, n.value, None, None) == 0
    assert np.array_equal(infos, np.array(pruned, dtype=np.int64).reshape(n.value, 4))
    tensors = hp.prunable(lay)
    assert [lay.infos[r[0]].name for r in infos] == [t.name for t in tensors]
    assert [int(r[3]) for r in infos] == hp.real_counts(lay)
    chunks = [-(-(int(t.offset) + int(t.size) - (int(t.offset) & ~31)) // 4096) for t in tensors]
    assert scratch == 8 * sum(chunks)  # one double per chunk


def test_null_misaligned_and_unsupported_arguments_without_a_gpu():
    from slimdqn import _hip
    from tests.helpers.redo import HostLayout

    lay = hp.host_layout(hp.FC_SMALL)
    lib, cfg = lay.lib, ctypes.byref(lay.cfg)
    one = 1 << 20  # a stand-in, 16-byte aligned pointer: every call below is refused in front of its first launch
    assert lib.isdqn_net_project_layout(None, None, None, 0, None) == _hip.ERR_ARG
    good = [one, one, one, one, one]  # params, target_norms, norms, scales, scratch
    for i in range(5):
        args = list(good)
        args[i] = None
        assert lib.isdqn_net_project_apply(cfg, *args, None, None) == _hip.ERR_ARG, i
    assert lib.isdqn_net_project_apply(None, *good, None, None) == _hip.ERR_ARG
    for i, off in ((0, 8), (1, 4), (2, 4), (3, 2), (4, 4)):
        args = list(good)
        args[i] += off
        assert lib.isdqn_net_project_apply(cfg, *args, None, None) == _hip.ERR_ARG and "aligned" in _hip.last_error(), i
    assert lib.isdqn_net_project_apply(cfg, *good, one + 16, None) == _hip.ERR_ARG and "aligned" in _hip.last_error()
    for args in ((None, one, one), (one, None, one), (one, one, None), (one + 4, one, one), (one, one + 4, one), (one, one, one + 4)):
        assert lib.isdqn_net_project_norms(cfg, *args, None) == _hip.ERR_ARG, args
    assert lib.isdqn_net_project_norms(None, one, one, one, None) == _hip.ERR_ARG
    impala = HostLayout((84, 84, 4), 4, 3, (8, 8, 8, 16), "impala", True, 4)
    icfg = ctypes.byref(impala.cfg)
    assert lib.isdqn_net_project_layout(icfg, None, None, 0, None) == _hip.ERR_UNSUPPORTED and "impala" in _hip.last_error()
    assert lib.isdqn_net_project_apply(icfg, *good, None, None) == _hip.ERR_UNSUPPORTED
    assert lib.isdqn_net_project_norms(icfg, one, one, one, None) == _hip.ERR_UNSUPPORTED
    bn = hp.host_layout(hp.FC_SMALL)
    bn.cfg.batch_norm = 1
    assert lib.isdqn_net_project_layout(ctypes.byref(bn.cfg), None, None, 0, None) == _hip.ERR_UNSUPPORTED and "batch_norm" in _hip.last_error()
    assert lib.isdqn_net_project_apply(ctypes.byref(bn.cfg), *good, None, None) == _hip.ERR_UNSUPPORTED
    assert {"isdqn_net_project_layout", "isdqn_net_project_norms", "isdqn_net_project_apply"} <= set(_hip.PUBLIC_SYMBOLS)


def test_engine_and_rule_refusals():
    from slimdqn import _projection
    from slimdqn._engine import QNetEngine

    class Bare(QNetEngine):  # what the two calls look at in front of anything else
        def __init__(self):
            pass

    for call in (lambda: QNetEngine.project_weights(Bare()), lambda: QNetEngine.project_norms(Bare())):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == _projection.NAP_NOT_SET_REFUSED
    ok = dict(layer_norm=True)
    _projection.check_network(**ok)
    for kw, message in ((dict(ok, noisy=True), "NAP_NOISY_REFUSED"), (dict(ok, batch_norm=True), "NAP_BATCH_NORM_REFUSED"),
                        (dict(ok, architecture_type="impala"), "NAP_IMPALA_REFUSED"), (dict(layer_norm=False), "NAP_LAYER_NORM_REFUSED")):
        with pytest.raises(ValueError) as e:
            _projection.check_network(**kw)
        assert str(e.value) == getattr(_projection, message)
    with pytest.raises(ValueError) as e:
        _projection.check_targets([1.0], 2)
    assert str(e.value) == _projection.NAP_TARGETS_REFUSED
    assert _projection.scale_logs(np.array([0.5, 1.0, 0.25], np.float32)) == {"weight_scale_min": 0.25, "weight_scale_max": 1.0}


def test_agents_refuse_the_option_before_anything_is_built():
    """No GPU is touched: the rule stands in front of the first engine."""
    from slimdqn import _projection
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    for build in (lambda **kw: iSDQN(0, (8,), 3, 3, [20, 14], kw.pop("ln", True), kw.pop("bn", False), "fc", 1e-2, 0.99, 1, 1, 1000, **kw),
                  lambda **kw: TFDQN(0, (8,), 3, [20, 14], kw.pop("ln", True), kw.pop("bn", False), "fc", 1e-2, 0.99, 1, 1, 1000, **kw)):
        for kw, message in ((dict(ln=False), "NAP_LAYER_NORM_REFUSED"), (dict(bn=True), "NAP_BATCH_NORM_REFUSED")):
            with pytest.raises(ValueError) as e:
                build(weight_projection=True, **kw)
            assert str(e.value) == getattr(_projection, message)
    with pytest.raises(ValueError) as e:
        DQN(0, (8,), 3, [20, 14], False, "fc", 1e-2, 0.99, 1, 1, 1000, weight_projection=True)
    assert str(e.value) == _projection.NAP_LAYER_NORM_REFUSED


# ------------------------------------------------------------------------------------------------ the flag
def _base(env):
    return ["-en", "nap_Synthetic", "-s", "1", "-dw", "-tuf", "16"] + (["-f", "8", "8", "8", "16", "-at", "cnn"] if env == "atari" else [])


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_flag_parses_and_stays_out_of_parameters_json(tmp_path, env, algo):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    p = prepare_logs(env, algo, _base(env) + ["-ln"], root=str(tmp_path))
    assert p["normalize_and_project"] is False and pa.projection_kwargs(p) == {}  # absent: the keywords of today
    p = prepare_logs(env, algo, _base(env) + ["-s", "2", "-ln", "-nap"], root=str(tmp_path))
    assert pa.projection_kwargs(p) == dict(weight_projection=True)
    others = ["-prune", "0.5", "-wd", "0.1", "-redo", "16", "-reset", "32"]
    p = prepare_logs(env, algo, _base(env) + ["-s", "3", "-ln", "--normalize_and_project"] + others, root=str(tmp_path))
    assert pa.projection_kwargs(p) == dict(weight_projection=True) and pa.prune_kwargs(p)["prune_sparsity"] == 0.5
    stored = json.load(open(tmp_path / env / "exp_output" / "nap_Synthetic" / "parameters.json"))
    assert not any("project" in k or "nap" in k for section in stored.values() for k in section)
    base = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "is-dqn_amd", "experiments", env, algo + ".py")
    assert open(base).read().count("**projection_kwargs(p),") == 1


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
@pytest.mark.parametrize("extra,message", [
    (["-nap"], "NAP_LAYER_NORM_REFUSED"),
    (["-nap", "-ln", "-noisy"], "NAP_NOISY_REFUSED"),
])
def test_refusals_come_before_anything_is_written(tmp_path, env, algo, extra, message):
    from experiments.base.utils import prepare_logs
    from slimdqn import _projection

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, _base(env) + extra, root=str(tmp_path))
    assert str(e.value) == getattr(_projection, message)
    assert not os.path.exists(tmp_path / env)


@pytest.mark.parametrize("algo", ["isdqn", "tfdqn", "analysisdqn", "analysistfdqn"])  # (the agents with -bn; -at impala: every atari agent)
def test_batch_norm_and_impala_are_refused(tmp_path, algo):
    from experiments.base.utils import prepare_logs
    from slimdqn import _projection

    for extra, message in ((["-bn"], _projection.NAP_BATCH_NORM_REFUSED), (["-at", "impala"], _projection.NAP_IMPALA_REFUSED)):
        with pytest.raises(ValueError) as e:
            prepare_logs("atari", algo, _base("atari") + ["-ln", "-nap"] + extra, root=str(tmp_path))
        assert str(e.value) == message
        assert not os.path.exists(tmp_path / "atari")


# ------------------------------------------------------------------------------------------------ the build
def test_the_kernels_live_in_a_source_of_their_own_and_pass_the_lint():
    """The pinned sources keep their kernels: the projection kernels are built from build.PROJECT_SOURCES into every variant, they are
    the only kernels of that object, no other object has them, project.h holds no kernel, and scripts/isa_lint.py is clean on the
    assembly."""
    import importlib.util
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(root, "is-dqn_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.PROJECT_SOURCES == ["project_kernels.hip"]
    others = build.SOURCES + build.EXTRA_SOURCES + build.SIDE_SOURCES + build.PRUNE_SOURCES + build.MIXTURE_SOURCES
    assert not set(build.PROJECT_SOURCES) & set(others)
    assert "__global__" not in open(os.path.join(build.CSRC, "project.h")).read()
    for other in others:
        text = open(os.path.join(build.CSRC, other)).read()
        assert "project_sumsq_kernel" not in text and "project_scale_kernel" not in text, other
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    own = build.emit_project_asm()
    assert [os.path.basename(a) for a in own] == ["project_kernels.s"]
    text = open(own[0]).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    assert len(kernels) == 4 and sum("project_scale_kernel" in k for k in kernels) == 2, kernels
    assert sum("project_sumsq_kernel" in k for k in kernels) == 1 and sum("project_norms_kernel" in k for k in kernels) == 1
    assert "atomic" not in text, "the projection has no atomic of any kind"
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "isa_lint.py")] + own, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert re.search(r"project_kernels\.s: 4 functions", r.stdout), r.stdout[:500]
