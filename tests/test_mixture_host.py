"""Host side of REM, the random ensemble mixture: the float64 restatement of tests/helpers/mixture.py against torch autograd and
against the three wrong readings it must be able to tell apart -- on the GPU tests' own inputs, through the oracle forward --, the
exact draw, the ctypes layout of the struct that carries the weights against the C compiler's, flag parsing, every refusal from agents
and entry points, and the argument errors of isdqn_mixture_draw.  The device side is tests/test_gpu_mixture.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import test_gpu_mixture as T
from tests.helpers import mixture as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = [("atari", a) for a in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn")] + [("lunar_lander", a) for a in ("isdqn", "dqn", "tfdqn")]
REM_ENTRY_POINTS = [("atari", "dqn"), ("lunar_lander", "dqn")]


# ---------------------------------------------------------------------------------------------------------------- (a) the restatement
def test_draw_is_a_convex_combination_that_depends_on_seed_count_and_head_count():
    for H in (1, 2, 65, 200, 1024):
        a = hm.draw(H, T.SEED, 0)
        assert a.dtype == np.float32 and a.shape == (H,) and (a > 0).all() and abs(float(a.astype(np.float64).sum()) - 1.0) < H * 2.0**-23
    assert hm.draw(1, T.SEED, 7)[0] == np.float32(1.0)
    a = hm.draw(8, T.SEED, 0)
    assert not np.array_equal(a, hm.draw(8, T.SEED, 1)) and not np.array_equal(a, hm.draw(8, T.SEED + 1, 0))
    assert not np.array_equal(a, hm.draw(8, T.SEED, 2**32))  # (the high word of the count is part of the counter)
    # (u_h does not depend on H: the ratios of a draw of fewer heads are those of its first heads)
    np.testing.assert_allclose(a[:4] / a[0], hm.draw(4, T.SEED, 0) / hm.draw(4, T.SEED, 0)[0], rtol=1e-6)


def test_restatement_is_the_autograd_gradient():
    rng = np.random.default_rng(0)
    B, H, A = 6, 5, 4
    rows, vrows = rng.normal(size=(2 * B, H * A)), rng.normal(size=(B, H * A))
    alpha = hm.draw(H, 3, 0)
    action, reward, terminal = rng.integers(0, A, B), rng.normal(size=B), rng.random(B) < 0.3
    w, g = rng.uniform(0.0, 2.0, B), rng.uniform(0.5, 1.0, B)
    for dq in (False, True):
        for delta in (0.0, 0.6):
            ref = hm.mixture(rows, vrows, alpha, action, reward, terminal, 0.99, A, double_q=dq, weights=w, discount=g, huber_delta=delta)
            t = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
            al = torch.tensor(alpha.astype(np.float64))
            q = (t[:B].reshape(B, H, A)[torch.arange(B), :, torch.tensor(action)] * al).sum(1)
            d = q - torch.tensor(ref["targets"])
            l = d * d if delta == 0.0 else torch.where(d.abs() <= delta, 0.5 * d * d, delta * (d.abs() - 0.5 * delta))
            loss = (torch.tensor(w) * l).mean()
            loss.backward()
            assert abs(float(loss.detach()) - ref["losses"]) < 1e-12
            np.testing.assert_allclose(t.grad.numpy()[:B], ref["dout"], rtol=1e-12, atol=1e-15)
            assert not t.grad.numpy()[B:].any()  # nothing flows through the target
            sel = (rows[B:] if dq else vrows).reshape(B, H, A)
            assert np.array_equal(ref["a_star"], np.einsum("h,bha->ba", alpha.astype(np.float64), sel).argmax(1))


@pytest.mark.parametrize("form", ["target", "same"])
@pytest.mark.parametrize("option", T.OPTIONS)
@pytest.mark.parametrize("case", T.CASES)
def test_wrong_variants_differ_on_the_gpu_tests_own_inputs(case, option, form):
    """The batches of tests/test_gpu_mixture.py bite: on their inputs (through the float64 oracle forward) each wrong reading is more
    than 100 x the comparison's tolerance away from the restatement, and no transition is left out by the argmax rule."""
    H, A, B = case
    ref, fl = T.oracle_case(H, A, B, option, form)
    assert (ref["gap"] >= 10 * fl["q_values"]).all()
    kw = T._option_kw(option)
    b = T._Batch(None, "fc", B, A, seed=3 + H, weights=option == "weights", discount=option == "discount")
    dq = option == "double_q" and form == "target"
    rows, vrows = T.oracle_rows(H, A, "fc", T.FC_FEATS, b, form, dq)
    for variant, key in (("online_only", "targets"), ("max_first", "targets"), ("no_alpha", "dout")):
        if variant == "max_first" and A == 1:
            continue  # (one action: max_a commutes with the mixture)
        wrong = hm.mixture(rows, vrows, hm.draw(H, T.SEED, 1), b.action, b.reward, b.terminal, 0.99, A, double_q=dq, weights=b.weights,
                           discount=b.discount, huber_delta=kw.get("huber_delta", 0.0), variant=variant)
        bound = hm.RTOL * np.abs(ref[key]) + fl[key]
        assert (np.abs(wrong[key] - ref[key]) > 100 * bound).any(), variant


def test_mean_heads_helper_sums_in_float32_and_takes_the_first_maximum():
    q = np.zeros((2, 3 * 4), np.float32)
    q[0, [1, 4 + 1, 8 + 2]] = [1.0, 1.0, 2.0]  # actions 1 and 2 tie at 2.0
    q[1, 3] = -1.0
    act, sums = hm.mean_heads_actions(q, 4)
    assert act.tolist() == [1, 0] and sums.dtype == np.float32 and sums[0].tolist() == [0.0, 2.0, 2.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------- (b) the ABI
def test_batch_mixture_layout_is_the_c_compilers(tmp_path):
    from slimdqn import _hip

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses, here as a host C compiler
    exe = str(tmp_path / "batch_mixture_layout")
    subprocess.run([hipcc, "-x", "c", "-std=c11", "-O0", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "helpers", "batch_mixture_layout.c"), "-o", exe], check=True)
    c = {k: int(v) for k, v in (line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())}
    S = _hip.BatchMixture
    assert ctypes.sizeof(S) == c["sizeof"] and ctypes.sizeof(_hip.BatchConservative) == c["sizeof_conservative"]
    for name in ("flags", "discount", "weight_decay", "cql_alpha", "alpha", "n_mix", "reserved2"):
        assert getattr(S, name).offset == c[name], name
    assert S.alpha.offset == c["sizeof_conservative"] and c["sizeof"] == c["sizeof_conservative"] + 16
    assert (_hip.BATCH_MIXTURE, _hip.ACT_MEAN_HEADS) == (c["ISDQN_BATCH_MIXTURE"], c["ISDQN_ACT_MEAN_HEADS"]) == (16, 32)
    assert len({_hip.BATCH_MIRROR_CURRENT, _hip.BATCH_DISCOUNT, _hip.BATCH_WEIGHT_DECAY, _hip.BATCH_CONSERVATIVE, _hip.BATCH_MIXTURE}) == 5
    assert not _hip.ACT_MEAN_HEADS & _hip.BATCH_MIRROR_CURRENT  # (both travel in isdqn_net_best_actions' flags)


def test_draw_argument_errors_need_no_gpu():
    from slimdqn import _hip

    lib = _hip.lib()
    one = (ctypes.c_int64 * 1)()
    buf = (ctypes.c_float * 4)()
    here = ctypes.cast(one, ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p)
    for H in (0, -1, 1025):
        assert lib.isdqn_mixture_draw(H, 1, here[0], here[1], None) == _hip.ERR_ARG and b"1024" in lib.isdqn_last_error()
    assert lib.isdqn_mixture_draw(4, 1, None, here[1], None) == _hip.ERR_ARG
    assert lib.isdqn_mixture_draw(4, 1, here[0], None, None) == _hip.ERR_ARG
    assert "isdqn_mixture_draw" in _hip.PUBLIC_SYMBOLS


# ---------------------------------------------------------------------------------------------------------------- (c) flags and refusals
BASE = ["-s", "1", "-dw", "-f", "8", "8", "8", "16", "-at", "cnn", "-tuf", "16", "-ln"]


def _argv(env, name, extra):
    return ["-en", name] + (BASE if env == "atari" else ["-s", "1", "-dw", "-f", "20", "14", "-at", "fc", "-tuf", "16", "-ln"]) + extra


@pytest.mark.parametrize("env,algo", ENTRY_POINTS)
def test_flag_parses_and_stays_out_of_parameters_json(tmp_path, env, algo):
    import json

    from experiments.base import parser_argument as pa
    from experiments.base.utils import prepare_logs
    from slimdqn import _mixture

    q = prepare_logs(env, algo, _argv(env, "plain_Synthetic", []), root=str(tmp_path))
    assert q["rem_heads"] == 0 and pa.rem_kwargs(q) == {}  # (off: the keywords of before the flag existed)
    assert pa.rem_kwargs(prepare_logs(env, algo, _argv(env, "zero_Synthetic", ["-rem", "0"]), root=str(tmp_path))) == {}
    text = open(os.path.join(ROOT, "is-dqn_amd", "experiments", env, algo + ".py")).read()
    if (env, algo) in REM_ENTRY_POINTS:
        p = prepare_logs(env, algo, _argv(env, "rem_Synthetic", ["--rem_heads", "200", "-dq"]), root=str(tmp_path))
        assert p["rem_heads"] == 200 and pa.rem_kwargs(p) == dict(rem_heads=200)
        stored = json.load(open(tmp_path / env / "exp_output" / "rem_Synthetic" / "parameters.json"))
        assert all("rem_heads" not in section for section in stored.values())
        assert text.count("**rem_kwargs(p),") == 1
    else:
        with pytest.raises(ValueError) as e:
            prepare_logs(env, algo, _argv(env, "rem_Synthetic", ["-rem", "4"]), root=str(tmp_path))
        assert str(e.value) == _mixture.REM_AGENT_REFUSED
        assert not os.path.exists(tmp_path / env / "exp_output" / "rem_Synthetic")  # refused before anything is written
        assert "rem_kwargs" not in text


def _refusals():
    from slimdqn import _mixture as m

    return [(["-rem", "-1"], m.REM_HEADS_REFUSED), (["-rem", "1025"], m.REM_HEADS_REFUSED), (["-rem", "4", "-noisy"], m.REM_NOISY_REFUSED),
            (["-rem", "4", "-hl"], m.REM_HISTOGRAM_REFUSED), (["-rem", "4", "-qr"], m.REM_QUANTILE_REFUSED),
            (["-rem", "4", "-mq"], m.REM_MUNCHAUSEN_REFUSED), (["-rem", "4", "-cql", "0.5"], m.REM_CQL_REFUSED)]


@pytest.mark.parametrize("env,algo", REM_ENTRY_POINTS)
def test_entry_point_refusals_come_before_anything_is_written(tmp_path, env, algo):
    from experiments.base.utils import prepare_logs

    for extra, message in _refusals():
        with pytest.raises(ValueError) as e:
            prepare_logs(env, algo, _argv(env, "bad_Synthetic", extra), root=str(tmp_path))
        assert str(e.value) == message, extra
    assert not os.path.exists(tmp_path / env)


def test_agent_refusals_come_before_anything_is_built():
    from slimdqn import _mixture as m
    from slimdqn.networks.dqn import DQN

    make = lambda **kw: DQN(0, (8,), 4, [16, 16], True, "fc", 1e-3, 0.99, 1, 1, 8, batch_size=8, **kw)
    for kw, message in ((dict(rem_heads=-1), m.REM_HEADS_REFUSED), (dict(rem_heads=1025), m.REM_HEADS_REFUSED), (dict(rem_heads=2.5), m.REM_HEADS_REFUSED),
                        (dict(rem_heads=True), m.REM_HEADS_REFUSED), (dict(rem_heads=4, noisy=True), m.REM_NOISY_REFUSED),
                        (dict(rem_heads=4, n_bins=11), m.REM_HISTOGRAM_REFUSED), (dict(rem_heads=4, n_quantiles=8), m.REM_QUANTILE_REFUSED),
                        (dict(rem_heads=4, munchausen_tau=0.03), m.REM_MUNCHAUSEN_REFUSED), (dict(rem_heads=4, cql_alpha=0.5), m.REM_CQL_REFUSED)):
        with pytest.raises(ValueError) as e:
            make(**kw)
        assert str(e.value) == message, kw
    assert m.check_rem_heads(0, noisy=True, n_bins=5, cql_alpha=1.0) == 0 and m.check_rem_heads(200) == 200  # (off: nothing is refused)


def test_the_kernels_live_in_a_source_of_their_own_and_pass_the_lint():
    """The pinned sources keep their kernels: the mixture's kernels are built from build.MIXTURE_SOURCES into every variant, they are the
    only kernels of that object, no other source has them, mixture.h holds no kernel, and scripts/isa_lint.py is clean on the assembly."""
    import importlib.util
    import re
    import sys

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.MIXTURE_SOURCES == ["mixture_kernels.hip"]
    assert not set(build.MIXTURE_SOURCES) & set(build.SOURCES + build.EXTRA_SOURCES + build.SIDE_SOURCES + build.PRUNE_SOURCES)
    assert "__global__" not in open(os.path.join(build.CSRC, "mixture.h")).read()
    for other in build.SOURCES + build.EXTRA_SOURCES + build.SIDE_SOURCES + build.PRUNE_SOURCES:
        assert "mix_td_kernel" not in open(os.path.join(build.CSRC, other)).read(), other
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    own = build.emit_mixture_asm()
    assert [os.path.basename(a) for a in own] == ["mixture_kernels.s"]
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(own[0]).read(), re.M)
    assert len(kernels) == 4 and all(any(n in k for n in ("mixture_draw_kernel", "mixture_advance_kernel", "mix_td_kernel", "argmax_mean_rows_kernel"))
                                     for k in kernels), kernels
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_lint.py")] + own, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert re.search(r"mixture_kernels\.s: 4 functions", r.stdout), r.stdout[:500]


def test_where_the_rules_and_the_messages_live():
    from slimdqn import _engine, _mixture
    from slimdqn.networks import _agent

    assert _engine._mixture is _mixture and _agent._mixture is _mixture
    assert not [k for k in vars(_engine) if k.startswith("REM_")]  # (tests/test_options_snapshot_host.py counts the engine's constants)
    header = open(os.path.join(ROOT, "include", "isdqn_hip.h")).read()
    for text in ("#define ISDQN_BATCH_MIXTURE 16", "#define ISDQN_ACT_MEAN_HEADS 32", "typedef struct isdqn_batch_mixture", "0x52454D00",
                 "int isdqn_mixture_draw(int32_t n_heads, uint64_t seed, int64_t* draw_count, float* alpha, void* stream);"):
        assert text in header, text
