"""CPU side of gradual magnitude pruning (include/isdqn_hip.h, isdqn_net_prune_*): the schedule against its closed form, the numpy oracle
of tests/helpers/prune.py against the wrong variants the device tests must be able to tell from it (on THEIR inputs), the flags and
their refusals, the layout call, the argument checks that need no GPU, and the build: the kernels' own translation unit and its lint."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.helpers import prune as hp

ENTRY_POINTS = [("atari", a) for a in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn")] + [("lunar_lander", a) for a in ("isdqn", "dqn", "tfdqn")]


# ------------------------------------------------------------------------------------------------ the schedule
def test_schedule_against_the_closed_form():
    from slimdqn import _sparsity as sp

    S, t0, t1 = 0.95, 1000, 9000
    assert sp.sparsity_at(0, S, t0, t1) == 0.0 and sp.sparsity_at(t0 - 1, S, t0, t1) == 0.0
    assert sp.sparsity_at(t0, S, t0, t1) == 0.0  # (the cubic starts at 0: continuous at t0)
    assert sp.sparsity_at(t1, S, t0, t1) == S and sp.sparsity_at(t1 + 12345, S, t0, t1) == S
    assert sp.sparsity_at((t0 + t1) // 2, S, t0, t1) == S * (1.0 - 0.5 ** 3) == S * 0.875
    for t in (t0 + 1, 2500, 5000, 8999):
        x = (t - t0) / (t1 - t0)
        assert sp.sparsity_at(t, S, t0, t1) == S * (1.0 - (1.0 - x) ** 3) == hp.sparsity(t, S, t0, t1)
    ts = np.arange(0, 10000, 37)
    s = np.array([sp.sparsity_at(int(t), S, t0, t1) for t in ts])
    assert (np.diff(s) >= 0).all() and s.max() <= S


def test_counts_round_down_and_never_decrease():
    from slimdqn import _sparsity as sp

    n = [160, 280, 7, 1]
    assert sp.pruned_counts(0.5, n) == [80, 140, 3, 0]
    assert sp.pruned_counts(0.999, n) == [159, 279, 6, 0]  # floor: never all of a tensor below sparsity 1
    assert sp.pruned_counts(0.3, n, previous=[80, 10, 3, 0]) == [80, 84, 3, 0]  # clamped from below
    sched = sp.Schedule(0.9, 10, 110, n)
    assert sched.counts == [0, 0, 0, 0] and not sched.active and sched.sparsity == 0.0
    last = sched.step(5)
    assert last == [0, 0, 0, 0] and not sched.active
    for t in range(10, 200, 10):
        k = sched.step(t)
        assert all(a >= b for a, b in zip(k, last)) and k == hp.counts_at(t, 0.9, 10, 110, n, last)
        last = k
    assert last == [144, 252, 6, 0] and sched.active and sched.sparsity == (144 + 252 + 6) / sum(n)
    assert sched.step(20) == last  # (a clock that went back -- a reset does not move it, but the clamp holds anyway)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            sp.check_sparsity(bad)
    for bad in ((5, 5), (-1, 4), (7, 3), (0.5, 4)):
        with pytest.raises(ValueError):
            sp.check_schedule(*bad)
    for bad in (0, -16, 24):
        with pytest.raises(ValueError):
            sp.check_period(bad, 16)
    assert sp.check_period(32, 16) == 32


# ------------------------------------------------------------------------------------------------ the oracle and its wrong variants
@pytest.mark.parametrize("config", ["FC_SMALL", "FC_WIDE", "CNN"])
def test_oracle_differs_from_the_wrong_variants_on_the_device_tests_inputs(config):
    lay = hp.host_layout(getattr(hp, config))
    n = hp.real_counts(lay)
    full = hp.full_mask(lay)
    k1, k2 = [int(0.3 * x) for x in n], [int(0.7 * x) for x in n]
    # ties to the higher index: all weights equal, and the three magnitudes
    for case in ("equal", "levels"):
        p = hp.case_params(lay, case)
        good = hp.select(lay, p, full, k1)
        assert hp.popcount_pruned(lay, good) == k1
        assert not np.array_equal(good, hp.select(lay, p, full, k1, ties_high=True)), case
    # already pruned elements not ranked first: after a learn step moved them they carry magnitudes again
    p = hp.case_params(lay, "normal")
    m1 = hp.select(lay, p, full, k1)
    moved = np.abs(p) + np.float32(10.0)  # every element larger than before, the pruned ones too: order by magnitude ignores the mask
    moved[hp.pruned_index(lay, m1)] += np.float32(100.0)
    good = hp.select(lay, moved, m1, k2)
    assert not (good & ~m1).any() and hp.popcount_pruned(lay, good) == k2
    assert not np.array_equal(good, hp.select(lay, moved, m1, k2, pruned_first=False))
    # padding lanes counted: the sentinels of the padded lanes are smaller than most weights and would be taken first (fc [20, 14] is
    # the configuration with padded rows and lanes in its prunable kernels: there, and only there, the variant is not the oracle)
    padded = any(int(i.size) != r for i, r in zip(hp.prunable(lay), n))
    assert padded == (config == "FC_SMALL")
    for case in ("normal", "equal", "levels"):
        q = hp.case_params(lay, case)
        assert padded == (not np.array_equal(hp.select(lay, q, full, k1), hp.select(lay, q, full, k1, padding_counts=True))), case
    # the apply pass: +0.0 at pruned positions (a -0.0 there becomes +0.0), every other bit kept -- the sentinels too
    lv = hp.case_params(lay, "levels")
    m, out = hp.update(lay, lv, full, k2)
    idx = hp.pruned_index(lay, m)
    assert (hp.bits(out)[idx] == 0).all()
    keep = np.ones(lv.size, bool)
    keep[idx] = False
    assert np.array_equal(hp.bits(out)[keep], hp.bits(lv)[keep])


def test_key_order_negative_zero_denormals_inf_and_nan():
    lay = hp.host_layout(hp.FC_SMALL)
    info = hp.prunable(lay)[0]
    idx = hp.real_index(lay, info)
    p = np.full(lay.n_param_floats, 1.0, np.float32)
    vals = np.array([np.nan, np.inf, -2.0, 1e-40, -0.0, 0.0, -3e-41, 0.5], np.float32)
    p[idx[: vals.size]] = vals
    k = hp.keys(p, hp.full_mask(lay), idx[: vals.size])
    order = np.lexsort((idx[: vals.size], k))
    assert [int(o) for o in order] == [4, 5, 6, 3, 7, 2, 1, 0]  # -0.0 and 0.0 tie (lower index first), denormals are not zero, NaN above inf
    assert k[4] == k[5] == 1


# ------------------------------------------------------------------------------------------------ flags
def _base(env):
    return ["-en", "prune_Synthetic", "-s", "1", "-dw", "-tuf", "16"] + (["-f", "8", "8", "8", "16", "-at", "cnn"] if env == "atari" else [])


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_flags_parse_and_stay_out_of_parameters_json(tmp_path, env, algo):
    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs

    p = prepare_logs(env, algo, _base(env), root=str(tmp_path))
    assert p["prune_sparsity"] == 0.0 and pa.prune_kwargs(p) == {}
    # -prune 0 and the three other flags alone: the keywords of a run without any of them
    p = prepare_logs(env, algo, _base(env) + ["-s", "2", "-prune", "0", "-prunes", "9", "-prunee", "3", "-prunef", "5"], root=str(tmp_path))
    assert pa.prune_kwargs(p) == {}
    p = prepare_logs(env, algo, _base(env) + ["-s", "3", "-prune", "0.95", "-prunes", "100", "-prunee", "900", "-prunef", "32"], root=str(tmp_path))
    assert pa.prune_kwargs(p) == dict(prune_sparsity=0.95, prune_start=100, prune_end=900, prune_period=32)
    p = prepare_logs(env, algo, _base(env) + ["-s", "4", "--prune_sparsity", "0.5"], root=str(tmp_path))
    assert pa.prune_kwargs(p) == dict(prune_sparsity=0.5, prune_start=0, prune_end=100000, prune_period=16)  # -prunef: -tuf by default
    stored = json.load(open(tmp_path / env / "exp_output" / "prune_Synthetic" / "parameters.json"))
    assert not any("prune" in k for section in stored.values() for k in section)
    base = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "is-dqn_amd", "experiments", env, algo + ".py")
    assert open(base).read().count("**prune_kwargs(p),") == 1


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
@pytest.mark.parametrize("extra,message", [
    (["-prune", "1"], "PRUNE_SPARSITY_REFUSED"),
    (["-prune", "-0.2"], "PRUNE_SPARSITY_REFUSED"),
    (["-prune", "nan"], "PRUNE_SPARSITY_REFUSED"),
    (["-prune", "0.9", "-prunes", "50", "-prunee", "50"], "PRUNE_SCHEDULE_REFUSED"),
    (["-prune", "0.9", "-prunes", "-1"], "PRUNE_SCHEDULE_REFUSED"),
    (["-prune", "0.9", "-prunef", "24"], "PRUNE_PERIOD_REFUSED"),  # -tuf 16
    (["-prune", "0.9", "-prunef", "-16"], "PRUNE_PERIOD_REFUSED"),
    (["-prune", "0.9", "-noisy"], "PRUNE_NOISY_REFUSED"),
])
def test_refusals_come_before_anything_is_written(tmp_path, env, algo, extra, message):
    from experiments.base.utils import prepare_logs
    from slimdqn import _sparsity

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, _base(env) + extra, root=str(tmp_path))
    assert str(e.value) == getattr(_sparsity, message)
    assert not os.path.exists(tmp_path / env)


@pytest.mark.parametrize("algo", ["isdqn", "tfdqn", "analysisdqn", "analysistfdqn"])  # (the agents with -bn; -at impala: every atari agent)
def test_batch_norm_and_impala_are_refused(tmp_path, algo):
    from experiments.base.utils import prepare_logs
    from slimdqn import _sparsity

    for extra, message in ((["-bn"], _sparsity.PRUNE_BATCH_NORM_REFUSED), (["-at", "impala"], _sparsity.PRUNE_IMPALA_REFUSED)):
        with pytest.raises(ValueError) as e:
            prepare_logs("atari", algo, _base("atari") + ["-prune", "0.9"] + extra, root=str(tmp_path))
        assert str(e.value) == message
        assert not os.path.exists(tmp_path / "atari")


def test_engine_refusals_without_a_mask():
    from slimdqn import _sparsity
    from slimdqn._engine import QNetEngine

    class Bare(QNetEngine):  # what the two calls look at in front of anything else
        def __init__(self):
            pass

    for call in (lambda: QNetEngine.prune_apply(Bare()), lambda: QNetEngine.prune_update(Bare(), [0])):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == _sparsity.PRUNE_NOT_SET_REFUSED
    for kw, message in ((dict(noisy=True), "PRUNE_NOISY_REFUSED"), (dict(batch_norm=True), "PRUNE_BATCH_NORM_REFUSED"),
                        (dict(architecture_type="impala"), "PRUNE_IMPALA_REFUSED")):
        with pytest.raises(ValueError) as e:
            _sparsity.check_network(**kw)
        assert str(e.value) == getattr(_sparsity, message)


# ------------------------------------------------------------------------------------------------ the layout call and the argument checks
def _layout_call(lay):
    from slimdqn import _hip

    n, words, scratch = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
    assert lay.lib.isdqn_net_prune_layout(ctypes.byref(lay.cfg), ctypes.byref(n), None, 0, ctypes.byref(words), ctypes.byref(scratch)) == _hip.OK
    infos = (ctypes.c_int64 * (4 * n.value))()
    assert lay.lib.isdqn_net_prune_layout(ctypes.byref(lay.cfg), ctypes.byref(n), infos, n.value, None, None) == _hip.OK
    return np.array(infos, dtype=np.int64).reshape(n.value, 4), int(words.value), int(scratch.value)


@pytest.mark.parametrize("config,flax", [
    (dict(hp.CNN, features=(32, 64, 64, 512), n_actions=9, n_heads=10),
     [(8, 8, 4, 32), (4, 4, 32, 64), (3, 3, 64, 64), (11 * 11 * 64, 512)]),
    (dict(hp.FC_SMALL, features=(200, 100), observation_dim=(8,)), [(8, 200), (200, 100)]),
    (hp.FC_SMALL, [(8, 20), (20, 14)]),
    (hp.CNN, [(8, 8, 4, 8), (4, 4, 8, 8), (3, 3, 8, 8), (11 * 11 * 8, 16)]),
])
def test_layout_counts_are_the_flax_shapes_products(config, flax):
    lay = hp.host_layout(config)
    infos, words, scratch = _layout_call(lay)
    tensors = hp.prunable(lay)
    assert len(infos) == len(tensors) == len(flax)
    for row, t, shape in zip(infos, tensors, flax):
        assert lay.infos[row[0]].name == t.name and int(t.kind) in (0, 1)
        assert (row[1], row[2]) == (int(t.offset), int(t.size))
        assert tuple(int(x) for x in t.flax_shape[: t.ndim]) == shape
        assert row[3] == int(np.prod(shape)) == hp.real_index(lay, t).size
    last = [i for i in lay.infos if int(i.kind) == 1][-1]
    assert last.name not in [lay.infos[r[0]].name for r in infos]  # the last Dense is left dense
    assert words == (lay.n_param_floats + 31) // 32 == hp.mask_words(lay)
    chunks = [-(-(int(t.offset) + int(t.size) - (int(t.offset) & ~31)) // 4096) for t in tensors]
    assert scratch == 4 * sum(4 * 256 + c for c in chunks)


def test_null_misaligned_and_unsupported_arguments_without_a_gpu():
    from slimdqn import _hip

    lay = hp.host_layout(hp.FC_SMALL)
    lib, cfg = lay.lib, ctypes.byref(lay.cfg)
    one = 1 << 20  # a stand-in, 16-byte aligned pointer: every call below is refused in front of its first launch
    k = (ctypes.c_int32 * 2)(0, 0)
    assert lib.isdqn_net_prune_layout(None, None, None, 0, None, None) == _hip.ERR_ARG
    assert lib.isdqn_net_prune_apply(None, one, one, None, None) == _hip.ERR_ARG
    assert lib.isdqn_net_prune_apply(cfg, None, one, None, None) == _hip.ERR_ARG
    assert lib.isdqn_net_prune_apply(cfg, one, None, None, None) == _hip.ERR_ARG
    assert lib.isdqn_net_prune_apply(cfg, one + 4, one, None, None) == _hip.ERR_ARG and "aligned" in _hip.last_error()
    assert lib.isdqn_net_prune_apply(cfg, one, one + 2, None, None) == _hip.ERR_ARG and "aligned" in _hip.last_error()
    assert lib.isdqn_net_prune_apply(cfg, one, one, one + 16, None) == _hip.ERR_ARG and "aligned" in _hip.last_error()
    for args in ((None, k, one, one), (one, None, one, one), (one, k, None, one), (one, k, one, None), (one + 8, k, one, one), (one, k, one + 1, one),
                 (one, k, one, one + 2)):
        assert lib.isdqn_net_prune_update(cfg, *args, None, None) == _hip.ERR_ARG, args
    for bad in ((-1, 0), (161, 0), (0, 281)):  # n = [160, 280]
        assert lib.isdqn_net_prune_update(cfg, one, (ctypes.c_int32 * 2)(*bad), one, one, None, None) == _hip.ERR_ARG
        assert "count" in _hip.last_error()
    from tests.helpers.redo import HostLayout

    impala = HostLayout((84, 84, 4), 4, 3, (8, 8, 8, 16), "impala", True, 4)
    assert lib.isdqn_net_prune_layout(ctypes.byref(impala.cfg), None, None, 0, None, None) == _hip.ERR_UNSUPPORTED and "impala" in _hip.last_error()
    assert lib.isdqn_net_prune_apply(ctypes.byref(impala.cfg), one, one, None, None) == _hip.ERR_UNSUPPORTED
    bn = hp.host_layout(hp.FC_SMALL)
    bn.cfg.batch_norm = 1
    assert lib.isdqn_net_prune_layout(ctypes.byref(bn.cfg), None, None, 0, None, None) == _hip.ERR_UNSUPPORTED and "batch_norm" in _hip.last_error()
    assert lib.isdqn_net_prune_update(ctypes.byref(bn.cfg), one, k, one, one, None, None) == _hip.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the build
def test_the_kernels_live_in_a_source_of_their_own_and_pass_the_lint():
    """The pinned sources keep their kernels: the pruning kernels are built from build.PRUNE_SOURCES into every variant, they are the
    only kernels of that object, no other object has them, prune.h holds no kernel, and scripts/isa_lint.py is clean on the assembly."""
    import importlib.util
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(root, "is-dqn_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.PRUNE_SOURCES == ["prune_kernels.hip"]
    assert not set(build.PRUNE_SOURCES) & set(build.SOURCES + build.EXTRA_SOURCES + build.SIDE_SOURCES)
    assert "__global__" not in open(os.path.join(build.CSRC, "prune.h")).read()
    for other in ("net_kernels.hip", "conservative_kernels.hip", "soft_shift_kernels.hip"):
        assert "prune_select_kernel" not in open(os.path.join(build.CSRC, other)).read()
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    own = build.emit_prune_asm()
    assert [os.path.basename(a) for a in own] == ["prune_kernels.s"]
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(own[0]).read(), re.M)
    assert len(kernels) == 8 and all("prune_select_kernel" in k or "prune_apply_kernel" in k for k in kernels), kernels
    assert sum("prune_apply_kernel" in k for k in kernels) == 2
    for other in build.emit_asm() + build.emit_side_asm():
        text = open(other).read()
        assert "prune_select_kernel" not in text and "prune_apply_kernel" not in text, other
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "isa_lint.py")] + own, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert re.search(r"prune_kernels\.s: 8 functions", r.stdout), r.stdout[:500]
