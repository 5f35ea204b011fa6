"""Munchausen targets on the GPU (include/isdqn_hip.h, isdqn_net_config::munchausen_tau) against the float64 restatement of
tests/helpers/munchausen.py, which is written from the header's definition:

1.  off is off: tau = 0 with arbitrary alpha / clip is bit-identical to a configuration that never sets the fields, workspace included;
2.  the target step on the device's own head rows (regions "q" / "logits"; iS-DQN K = 1 / 3 / 9, TF-DQN, BatchNorm, histogram heads);
3.  the DQN form: both halves of the value rows come from the target parameters (region "q_target" / "logits_target", [2B] rows);
4.  the head chain against the generic path: in this process (loss_on_batch) and in a child on the development build with
    ISDQN_NO_HEAD_CHAIN=1;
5.  the whole path against the float64 oracle forward with autograd, bf16x3 and single-pass bf16, no pair excluded;
6.  dL/dq keeps one non-zero per (transition, pair);  7. the small-tau limit;  8. the refused combinations;
9.  grad_on_batch with named pairs;  10. run-to-run identity and captured against eager steps;  11. the bounds-checked build;
12. the entry points with -mq.

The target bound.  tests/test_munchausen_host.py holds a float32 evaluation of the definition within 8e-7 x max(1, max |Q| of the
pair's two value rows) of float64 (observed 4.6e-7).  The device gets 4 x that, 3e-6: its expf / logf round differently from numpy's.
Quantities behind the targets keep the Double Q tolerances (rtol 1e-5, atol 1e-7) plus that bound."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.gpu_helpers import adam64
from tests.helpers import munchausen as mh
from tests.helpers import per_weights as pw
from tests.test_gpu_double_q import (ATOL, HEADLINE, HIST, HIST_POS, RTOL, TARGET_SEED, TINY, TOL, _Batch, _cpu, _engine, _feed, _hd, _obs,
                                     _one_step, _params, _rc_grad, _rows, _same_state, _width)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET_BOUND = 3e-6  # x max(1, max |Q| of the transition's two value rows)
FLOAT32_BOUND = 8e-7  # the same scale: a float32 evaluation of the definition against float64 (tests/test_munchausen_host.py)
MU = dict(munchausen_tau=0.03, munchausen_alpha=0.9, munchausen_clip=-1.0)


def _mu(tau=0.03, alpha=0.9, clip=-1.0):
    return dict(munchausen_tau=tau, munchausen_alpha=alpha, munchausen_clip=clip)


def _trows(eng, B, hist=False):
    """the target network's rows [2B][...] of the last *_target call, states first (region "q_target", histogram heads "logits_target")"""
    n, n_p = _width(eng, hist)
    return eng.region("logits_target" if hist else "q_target")[: 2 * B * n_p].reshape(2 * B, n_p)[:, :n].double().cpu()


def _ref(eng, rows, b, value_rows=None, K=None, on0=None, tg0=0, hist=False, huber_delta=0.0):
    K = eng.n_regressed if K is None else K
    on0 = (1 if eng.n_heads >= 2 else 0) if on0 is None else on0
    c = eng.cfg
    return mh.munchausen(rows, b.action, b.reward, b.terminal, float(c.gamma_n), K, on0, tg0, eng.n_actions, float(c.munchausen_tau),
                         float(c.munchausen_alpha), float(c.munchausen_clip), value_rows=value_rows, weights=b.weights,
                         huber_delta=huber_delta, hist=_hd(hist))


def _check_targets(dev, ref, what=""):
    """|dev - f64| <= 3e-6 x max(1, max |Q| of the pair's two value rows), every pair; prints the worst ratio to the bound first"""
    err = np.abs(np.asarray(dev, np.float64) - ref["targets"]) / ref["scale"]
    print(f"{what}targets: worst |dev - f64| / scale {err.max():.3g} = {err.max() / TARGET_BOUND:.2f} of the bound {TARGET_BOUND:g}")
    assert err.shape == ref["targets"].shape and (err <= TARGET_BOUND).all(), err.max()
    # (the helper's two forms; the paper's divides Q by tau inside its softmax, which costs it digits at small tau)
    np.testing.assert_allclose(ref["targets"], ref["paper_targets"], rtol=0, atol=1e-9 * float(ref["scale"].max()))


def _behind(a, b, ref, rtol=RTOL, atol=ATOL):
    """quantities derived from the targets: the Double Q tolerances plus the target bound"""
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol + TARGET_BOUND * float(ref["scale"].max()))


def _close(a, b, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _dout(eng, B, hist=False):
    n, n_p = _width(eng, hist)
    d = eng.region("dout")[: B * n_p].reshape(B, n_p).double().cpu().numpy()
    assert (d[:, n:] == 0).all()
    return d[:, :n]


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("form", ["isdqn", "dqn", "isdqn-hist", "dqn-hist"])
def test_off_keeps_every_bit_and_the_workspace(form):
    hist, single = form.endswith("hist"), form.startswith("dqn")
    feats, K, A, B = (TINY, 3, 5, 6) if hist else (HEADLINE, 9, 9, 12)
    n_heads = 1 if single else 1 + K
    outs, sizes = [], []
    for kw in ({}, _mu(0.0, 0.3, -7.0), _mu(0.0, 5.0, 2.0)):  # never set; tau = 0 with arbitrary (even invalid) alpha / clip
        eng, _ = _engine(feats, A, n_heads, B, seed=3, hist=hist, **kw)
        b = _Batch(eng, "cnn", B, A, seed=5)
        target = None
        if single:
            target = torch.zeros_like(eng.params)
            eng.import_flax(_params(31, feats, A, 1, "cnn", hist=hist), target=target)
        first = _one_step(eng, b, target)
        outs.append(first + _one_step(eng, b, target))  # the learn outputs of two steps, the parameters after each
        sizes.append(eng.workspace_bytes)
        assert float(eng.cfg.munchausen_tau) == 0.0 and int(eng.adam_count.item()) == 2
        with pytest.raises(RuntimeError):  # the target rows exist only with an option that needs them
            eng.region("q_target")
    assert sizes[0] == sizes[1] == sizes[2]
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert np.array_equal(x, y)
    on, _ = _engine(feats, A, n_heads, B, seed=3, hist=hist, **MU)
    assert on.workspace_bytes > sizes[0] and on.region("q_target").numel() >= 2 * B * ((n_heads * A + 7) // 8 * 8)
    for name in ("q", "dout", "wsplit", "loss_partials"):  # appended: nothing else moved
        assert on.region(name).data_ptr() - on.workspace.data_ptr() == eng.region(name).data_ptr() - eng.workspace.data_ptr()


# ------------------------------------------------------------------ 2. the target step on the device's own head rows
# (feats, K, A, B, arch, precision, hist, tau, clip, huber, weights, both sides of the clip asserted); K = 0: one head (TF-DQN)
OWN_ROWS = [
    pytest.param((HEADLINE, 9, 9, 12, "cnn", "bf16x3", False, 0.03, -1.0, 0.0, False, False), id="headline-K9-tau0.03"),
    pytest.param((HEADLINE, 9, 9, 12, "cnn", "bf16x3", False, 0.03, -0.1, 0.5, True, True), id="headline-K9-clip0.1-huber-weights"),
    pytest.param((HEADLINE, 9, 9, 12, "cnn", "bf16x3", False, 1.0, -1.0, 0.0, False, False), id="headline-K9-tau1"),
    pytest.param((TINY, 3, 5, 6, "cnn", "bf16x3", False, 1.0, -1.7, 0.0, True, True), id="tiny-K3-tau1-clip1.7-weights"),
    pytest.param((TINY, 1, 5, 6, "cnn", "bf16x3", False, 0.03, -1.0, 0.0, False, False), id="tiny-K1"),
    pytest.param((TINY, 0, 5, 6, "cnn", "bf16x3", False, 0.03, -0.1, 0.0, False, True), id="tfdqn-tiny"),
    pytest.param(((16, 16), 2, 3, 11, "fc", "bf16x3", False, 0.03, -1.0, 0.5, False, False), id="fc-B11-ragged-huber"),
    pytest.param(((8, 16, 16, 24), 2, 5, 4, "impala", "bf16x3", False, 1.0, -1.0, 0.0, False, False), id="impala-B4"),
    pytest.param((TINY, 3, 5, 6, "cnn", "bf16", False, 0.03, -1.0, 0.0, False, False), id="tiny-bf16"),
    pytest.param((TINY, 3, 5, 6, "cnn", "bf16x3", HIST_POS, 0.03, -0.1, 0.0, True, True), id="tiny-hist-tau0.03"),
    pytest.param((TINY, 3, 5, 6, "cnn", "bf16x3", HIST_POS, 1.0, -1.0, 0.0, False, False), id="tiny-hist-tau1"),
    pytest.param((TINY, 0, 5, 6, "cnn", "bf16x3", HIST_POS, 1.0, -1.0, 0.0, False, False), id="tfdqn-hist"),
]


def _clip_sides(ref, clip, both):
    on, inside = ref["tlp"] < clip, ref["tlp"] > clip
    print(f"bonus on the clip for {on.mean():.2f} of the pairs, inside it for {inside.mean():.2f}; max |target - max form| "
          f"{np.abs(ref['targets'] - ref['max_targets']).max():.3g}")
    if both:
        assert on.any() and inside.any()
    assert (np.abs(ref["targets"] - ref["max_targets"]) > 100 * TARGET_BOUND * ref["scale"]).any()  # the option changes these targets


@pytest.mark.parametrize("shape", OWN_ROWS)
def test_targets_match_float64_on_the_device_rows(shape):
    feats, K, A, B, arch, prec, hist, tau, clip, huber, weights, both = shape
    eng, _ = _engine(feats, A, 1 + K, B, arch=arch, precision=prec, seed=2, hist=hist, huber_delta=huber, **_mu(tau, 0.9, clip))
    b = _Batch(eng, arch, B, A, seed=5, reward_scale=4.0 if hist else 1.0, weights=weights)
    assert b.terminal.any() and not b.terminal.all()
    # histogram heads: also the learn form, which takes the same loss kernel (no head chain) and leaves the priorities and dL/dlogits
    for learn in ((False, True) if hist else (False,)):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        ref = _ref(eng, _rows(eng, B, hist), b, hist=hist, huber_delta=huber)
        _clip_sides(ref, clip, both)
        _check_targets(eng.targets.cpu(), ref)
        _close(eng.q_values.cpu(), ref["q"])
        _behind(losses, ref["losses"], ref)
        if learn:
            _behind(eng.priorities.cpu(), ref["priorities"], ref)
            # dL/dlogit = (softmax - p(y)) / B: the projection turns an error dy of the float32 target y into dp <= dy / (sigma sqrt(2 pi))
            # (tests/test_gpu_double_q.py); dy is 4 ulps of the support's end plus the target bound
            dy = 4 * 2.0 ** -23 * hist["vmax"] + TARGET_BOUND * float(ref["scale"].max())
            _close(_dout(eng, B, hist), ref["dq"], atol=ATOL + dy / (hist["sigma"] * np.sqrt(2 * np.pi)) / B)
    if not hist:  # the terminal rows carry the bonus and no bootstrap
        term = b.terminal.astype(bool)
        _behind(eng.targets.cpu()[term], (b.reward[:, None] + ref["bonus"])[term], ref, rtol=0)


def test_bn_isdqn_targets_and_priorities_match_float64_on_the_device_rows():
    """BatchNorm iS-DQN: both halves are rows of the one training-mode forward; its learn step takes the generic loss kernel, which
    also leaves the priorities and dL/dq."""
    feats, K, A, B = TINY, 2, 3, 4
    eng, _ = _engine(feats, A, 1 + K, B, seed=1, batch_norm=True, **_mu(1.0, 0.9, -1.0))
    b = _Batch(eng, "cnn", B, A, seed=5)
    losses = _cpu(eng.learn_on_batch(b.cb))
    torch.cuda.synchronize()
    ref = _ref(eng, _rows(eng, B), b)
    _clip_sides(ref, -1.0, False)
    _check_targets(eng.targets.cpu(), ref)
    _close(eng.q_values.cpu(), ref["q"])
    _behind(losses, ref["losses"], ref)
    _behind(eng.priorities.cpu(), ref["priorities"], ref)
    _behind(_dout(eng, B), ref["dq"], ref)


# ------------------------------------------------------------------ 3. the DQN form
@pytest.mark.parametrize("shape", [
    pytest.param((HEADLINE, 9, 12, "cnn", False, 0.03, -0.1), id="headline-A9-B12"),
    pytest.param((TINY, 5, 6, "cnn", False, 1.0, -1.7), id="tiny-B6-tau1"),
    pytest.param(((16, 16), 3, 11, "fc", False, 0.03, -0.1), id="fc-B11-ragged"),
    pytest.param((TINY, 5, 6, "cnn", HIST_POS, 0.03, -0.5), id="tiny-hist"),
])
def test_dqn_form_takes_both_halves_of_the_value_rows_from_the_target_parameters(shape):
    """Region "q" holds the ONLINE parameters' rows of the B states, region "q_target" the target parameters' rows over
    concat(state, next_state); loss and learn forms, priorities and dL/dq from the learn form.  Then one network at a time is
    perturbed: the targets follow the target parameters alone, q_values the online parameters alone."""
    feats, A, B, arch, hist, tau, clip = shape
    eng, _ = _engine(feats, A, 1, B, arch=arch, seed=2, hist=hist, **_mu(tau, 0.9, clip))
    tgt = torch.zeros_like(eng.params)
    eng.import_flax(_params(31, feats, A, 1, arch, hist=hist), target=tgt)
    b = _Batch(eng, arch, B, A, seed=5, reward_scale=4.0 if hist else 1.0)
    p0 = eng.params.clone()
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch_target(b.cb, tgt) if learn else eng.loss_on_batch_target(b.cb, tgt))
        torch.cuda.synchronize()
        rows, vrows = _rows(eng, B, hist), _trows(eng, B, hist)
        ref = _ref(eng, rows, b, value_rows=vrows, K=1, on0=0, hist=hist)
        _clip_sides(ref, clip, True)
        assert not np.array_equal(rows[:B].numpy(), vrows[:B].numpy())  # two networks on the same states
        if hist:
            qt = eng.region("q_target")[: 2 * B * 8 * ((A + 7) // 8)].reshape(2 * B, -1)[:, :A].double().cpu()
            _close(qt, mh.hl.expectations(vrows, hist["nb"], hist["vmin"], hist["vmax"]))
        _check_targets(eng.targets.cpu(), ref)
        _close(eng.q_values.cpu(), ref["q"])
        _behind(losses, ref["losses"], ref)
        if learn:
            _behind(eng.priorities.cpu(), ref["priorities"], ref)
            if hist:
                dy = 4 * 2.0 ** -23 * hist["vmax"] + TARGET_BOUND * float(ref["scale"].max())
                _close(_dout(eng, B, hist), ref["dq"], atol=ATOL + dy / (hist["sigma"] * np.sqrt(2 * np.pi)) / B)
            else:
                _behind(_dout(eng, B), ref["dq"], ref)
    eng.params.copy_(p0)
    eng.loss_on_batch_target(b.cb, tgt)
    torch.cuda.synchronize()
    base_q, base_t = _cpu(eng.q_values), _cpu(eng.targets)
    head = [i for i in eng.infos if i.name.decode().endswith("/bias")][-1]  # the head layer's bias: every Q-value moves
    sl = slice(head.offset, head.offset + head.size)
    bump = torch.linspace(0.05, 0.5, head.size, device=tgt.device)
    tgt2 = tgt.clone()
    tgt2[sl] += bump
    eng.loss_on_batch_target(b.cb, tgt2)  # the target parameters only: targets move, q_values keep their bits
    torch.cuda.synchronize()
    moved = np.abs(_cpu(eng.targets) - base_t)
    assert np.array_equal(_cpu(eng.q_values), base_q) and moved.max() > 1e-2 and (moved > 0).mean() > 0.5
    eng.params[sl] += bump
    eng.loss_on_batch_target(b.cb, tgt)  # the online parameters only: targets keep their bits, q_values move
    torch.cuda.synchronize()
    moved = np.abs(_cpu(eng.q_values) - base_q)
    assert np.array_equal(_cpu(eng.targets), base_t) and moved.max() > 1e-2 and (moved > 0).all()


# ------------------------------------------------------------------ 4. head chain vs generic path
HC_SHAPES = {
    "headline-K9-A9-B12": (HEADLINE, 9, 9, 12, "cnn", "bf16x3", 0.0, False, 0.03, -0.1),
    "headline-huber-weights-tau1": (HEADLINE, 9, 9, 12, "cnn", "bf16x3", 0.5, True, 1.0, -1.7),
    "tiny-weights": (TINY, 3, 5, 6, "cnn", "bf16x3", 0.0, True, 0.03, -1.0),
    "fc-ragged-huber": ((32, 32), 2, 4, 11, "fc", "bf16x3", 0.5, False, 0.03, -0.1),
    "tfdqn-tiny": (TINY, 0, 5, 6, "cnn", "bf16x3", 0.0, False, 0.03, -0.1),
    "headline-bf16": (HEADLINE, 9, 9, 12, "cnn", "bf16", 0.0, False, 0.03, -1.0),
}


def _hc_engine(name):
    feats, K, A, B, arch, prec, huber, weights, tau, clip = HC_SHAPES[name]
    eng, _ = _engine(feats, A, 1 + K, B, arch=arch, precision=prec, seed=2, huber_delta=huber, **_mu(tau, 0.9, clip))
    return eng, _Batch(eng, arch, B, A, seed=5, weights=weights)


@pytest.mark.parametrize("name", list(HC_SHAPES))
def test_head_chain_agrees_with_the_generic_path(name):
    feats, K, A, B, arch, prec, huber, weights, tau, clip = HC_SHAPES[name]
    eng, b = _hc_engine(name)
    on0 = 1 if K else 0
    pre = _cpu(eng.loss_on_batch(b.cb))  # generic path: leaves region "q"
    torch.cuda.synchronize()
    gen_q, gen_t = _cpu(eng.q_values), _cpu(eng.targets)
    ref = _ref(eng, _rows(eng, B), b, huber_delta=huber)
    _check_targets(gen_t, ref, "generic ")
    _behind(pre, ref["losses"], ref)
    eng.region("q").zero_()
    losses = _cpu(eng.learn_on_batch(b.cb))  # head chain
    torch.cuda.synchronize()
    assert not eng.region("q").any()  # the head chain keeps its Q rows in LDS: this step did not take the generic kernels
    # the bar of tests/test_gpu_double_q.py between the fused learn path and the forward path: 1e-3
    assert np.abs(_cpu(eng.q_values) - gen_q).max() < 1e-3
    assert np.abs(_cpu(eng.targets) - gen_t).max() < 1e-3
    assert np.abs(losses - pre).max() < 1e-3 * max(1.0, float(np.abs(pre).max()))
    print(f"head chain - generic: q {np.abs(_cpu(eng.q_values) - gen_q).max():.3g} targets {np.abs(_cpu(eng.targets) - gen_t).max():.3g}")
    dout = _dout(eng, B)
    assert np.abs(dout - ref["dq"]).max() < 1e-3 * max(1.0, float(np.abs(ref["dq"]).max()))
    assert ((dout != 0) == (ref["dq"] != 0)).all()
    # the existing loss on the step's OWN q / targets
    w = np.ones(B) if b.weights is None else b.weights
    own = pw.weighted_td(_cpu(eng.q_values), _cpu(eng.targets), w, huber)
    dense = np.zeros((B, max(1 + K, 1), A))
    for k in range(max(K, 1)):
        dense[np.arange(B), on0 + k, b.action] = own["dq"][:, k]
    _close(dout, dense.reshape(B, -1))
    _close(losses, own["losses"])
    _close(eng.priorities.cpu(), np.sqrt(own["l"].mean(1) + 1e-10), rtol=2e-6, atol=1e-9)
    if huber > 0:
        d = np.abs(ref["q"] - ref["targets"])
        assert (d > huber).any() and (d < huber).any()


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/is-dqn_amd")
import numpy as np, torch
from tests.test_gpu_munchausen import _hc_engine
eng, b = _hc_engine(sys.argv[2])
eng.region("q").zero_()
g = torch.zeros_like(eng.params)
losses = eng.learn_on_batch(b.cb, grad_out=g)
torch.cuda.synchronize()
assert eng.region("q").any(), "ISDQN_NO_HEAD_CHAIN=1 did not switch the head chain off"
np.savez(sys.argv[3], losses=losses.cpu().numpy(), q=eng.q_values.cpu().numpy(), t=eng.targets.cpu().numpy(), pr=eng.priorities.cpu().numpy(),
         g=g.cpu().numpy(), p=eng.params.cpu().numpy())
"""


@pytest.mark.parametrize("name", ["headline-K9-A9-B12", "headline-huber-weights-tau1", "tfdqn-tiny"])
def test_learn_step_agrees_with_the_development_build_without_the_head_chain(name, tmp_path):
    """The same learn step in a child process on the development build with ISDQN_NO_HEAD_CHAIN=1 (separate head GEMM, td_kernel, data
    gradient and LayerNorm backward): outputs, the gradient of every parameter and the parameters after the step."""
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="dev", defines=("ISDQN_DEV",))  # (no-op when the build is current)
    out = tmp_path / "generic.npz"
    env = dict(os.environ, ISDQN_HIP_LIB=lib, ISDQN_NO_HEAD_CHAIN="1")
    run = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, str(out)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-3000:]
    gen = np.load(out)
    eng, b = _hc_engine(name)
    g = torch.zeros_like(eng.params)
    eng.region("q").zero_()
    losses = _cpu(eng.learn_on_batch(b.cb, grad_out=g))
    torch.cuda.synchronize()
    assert not eng.region("q").any()  # this process took the head chain
    rel = lambda x, y: float(np.abs(np.asarray(x, np.float64) - y).max() / max(1.0, float(np.abs(y).max())))
    figs = dict(q=rel(_cpu(eng.q_values), gen["q"]), targets=rel(_cpu(eng.targets), gen["t"]), losses=rel(losses, gen["losses"]),
                priorities=rel(_cpu(eng.priorities), gen["pr"]), grad=rel(_cpu(g), gen["g"]), params=rel(_cpu(eng.params), gen["p"]))
    print(name, {k: f"{v:.2e}" for k, v in figs.items()})
    t = TOL["bf16x3"]
    assert figs["q"] < 1e-3 and figs["targets"] < 1e-3 and figs["losses"] < 1e-3 and figs["priorities"] < 1e-3
    assert figs["grad"] < t["grad"] and figs["params"] < 1e-3


# ------------------------------------------------------------------ 5. the whole path against the float64 oracle forward
# (feats, K, A, B, arch, ln, form, params seed, batch seed, tau); form: isdqn | dqn | bn | hist | tfdqn
E2E = {
    "headline-B4": (HEADLINE, 9, 9, 4, "cnn", True, "isdqn", 2, 8, 0.03),
    "tiny-tau1": (TINY, 3, 5, 6, "cnn", True, "isdqn", 2, 1, 1.0),
    "tiny-K1": (TINY, 1, 5, 6, "cnn", True, "isdqn", 2, 1, 0.03),
    "fc-ragged": ((32, 32), 2, 4, 11, "fc", True, "isdqn", 2, 0, 0.03),
    "bn": (TINY, 2, 3, 4, "cnn", True, "bn", 2, 0, 1.0),
    "dqn-tiny": (TINY, 1, 5, 6, "cnn", True, "dqn", 2, 5, 0.03),
    "dqn-fc-tau1": ((32, 32), 1, 4, 11, "fc", True, "dqn", 2, 3, 1.0),
    "tfdqn-tiny": (TINY, 1, 5, 6, "cnn", True, "tfdqn", 2, 1, 0.03),
    "hist-tiny": (TINY, 3, 5, 6, "cnn", True, "hist", 2, 1, 0.03),
    "tiny-bf16": (TINY, 3, 5, 6, "cnn", True, "isdqn", 2, 1, 0.03),
    "tiny-bf16-tau1": (TINY, 3, 5, 6, "cnn", True, "isdqn", 2, 1, 1.0),
    "dqn-tiny-bf16": (TINY, 1, 5, 6, "cnn", True, "dqn", 2, 5, 0.03),
}
E2E_PRECISION = {"tiny-bf16": "bf16", "tiny-bf16-tau1": "bf16", "dqn-tiny-bf16": "bf16"}  # (every other case: bf16x3)
ALPHA, CLIP, GAMMA_N = 0.9, -1.0, 0.99


def oracle_case(name):
    """Everything of a section-5 case that needs no GPU: parameters, batch, the float64 rows (with a graph through the online
    parameters) and the helper's result on them (targets detached)."""
    feats, K, A, B, arch, ln, form, pseed, bseed, tau = E2E[name]
    hist, separate, bn = form == "hist", form == "dqn", form == "bn"
    n_heads = 1 if form in ("dqn", "tfdqn") else 1 + K
    params = _params(pseed, feats, A, n_heads, arch, ln, hist, bn)
    tparams = _params(TARGET_SEED, feats, A, 1, arch, ln, hist) if separate else None
    b = _Batch(None, arch, B, A, seed=bseed, reward_scale=4.0 if hist else 1.0)
    pt = onet.to_torch(params, torch.float64, requires_grad=True)
    stats = None
    if bn:  # training mode on the batch statistics of concat(state, next_state) (isdqn.py:95)
        rng = np.random.default_rng(pseed + 2)
        stats = {m: {"mean": rng.normal(0, 0.3, l["mean"].shape).astype(np.float32), "var": rng.uniform(0.5, 2.0, l["var"].shape).astype(np.float32)}
                 for m, l in onet.init_batch_stats(params).items()}
        rows = onet.forward(pt, torch.cat([b.x_state, b.x_next]), feats, arch, ln, batch_norm=True, batch_stats=onet.to_torch(stats, torch.float64),
                            use_running_average=False, new_stats={})
    else:
        rows = torch.cat([onet.forward(pt, b.x_state, feats, arch, ln), onet.forward(pt, b.x_next, feats, arch, ln)])
    vrows = None
    if separate:
        tt = onet.to_torch(tparams, torch.float64)
        vrows = torch.cat([onet.forward(tt, b.x_state, feats, arch, ln), onet.forward(tt, b.x_next, feats, arch, ln)]).detach()
    on0 = 0 if n_heads == 1 else 1
    ref = mh.munchausen(rows, b.action, b.reward, b.terminal, GAMMA_N, K, on0, 0, A, tau, ALPHA, CLIP, value_rows=vrows,
                        hist=HIST if hist else None)
    return dict(params=params, tparams=tparams, stats=stats, batch=b, pt=pt, rows=rows, ref=ref, n_heads=n_heads, on0=on0)


@pytest.mark.parametrize("name", list(E2E))
def test_whole_path_matches_the_float64_oracle(name):
    from slimdqn._engine import QNetEngine

    feats, K, A, B, arch, ln, form, pseed, bseed, tau = E2E[name]
    prec, lr = E2E_PRECISION.get(name, "bf16x3"), 1e-3
    t = TOL[prec]
    lip = GAMMA_N + 2 * ALPHA  # the target's Lipschitz constant in the head outputs: the Double Q bounds times it
    c = oracle_case(name)
    ref, hist, separate, bn = c["ref"], form == "hist", form == "dqn", form == "bn"
    hkw = dict(n_bins=HIST["nb"], min_value=HIST["vmin"], max_value=HIST["vmax"], sigma=HIST["sigma"]) if hist else {}
    eng = QNetEngine(_obs(arch), A, c["n_heads"], feats, arch, ln, B, gamma_n=GAMMA_N, learning_rate=lr, adam_eps=1.5e-4, precision=prec,
                     batch_norm=bn, **_mu(tau, ALPHA, CLIP), **hkw)
    eng.import_flax(c["params"], batch_stats=c["stats"])
    b = _Batch(eng, arch, B, A, seed=bseed, reward_scale=4.0 if hist else 1.0)
    tgt = None
    if separate:
        tgt = torch.zeros_like(eng.params)
        eng.import_flax(c["tparams"], target=tgt)
    rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - want).max() / max(1.0, float(np.abs(want).max())))
    losses = _cpu(eng.loss_on_batch_target(b.cb, tgt) if separate else eng.loss_on_batch(b.cb))
    dev_t = _cpu(eng.targets)
    assert dev_t.shape == ref["targets"].shape and dev_t.size == B * K  # every pair is compared: a continuous target excludes none
    print(f"{name}: q {rel(_cpu(eng.q_values), ref['q']):.2e} (bound {t['q']:g}) targets {rel(dev_t, ref['targets']):.2e} "
          f"(bound {lip * t['q']:.3g}) loss {rel(losses, ref['losses']):.2e} (bound {lip * t['loss']:.3g}) over {dev_t.size} pairs")
    assert rel(_cpu(eng.q_values), ref["q"]) < t["q"]
    assert rel(dev_t, ref["targets"]) < lip * t["q"]
    assert rel(losses, ref["losses"]) < lip * t["loss"]
    # gradients of every leaf against float64 autograd of the same helper loss; one Adam step from zero moments
    ref["loss_t"].sum().backward()
    p0 = eng.params.clone()
    g = torch.zeros_like(eng.params)
    if separate:  # (the target form has no debug gradient: the gradient-only pass on the same loss)
        eng.grad_on_batch(b.cb, g, target_params=tgt)
        eng.learn_on_batch_target(b.cb, tgt)
    else:
        eng.learn_on_batch(b.cb, grad_out=g)
    torch.cuda.synchronize()
    hip_g = eng.internal_to_flax_grads(g)
    worst = 0.0
    for mod in c["pt"]:
        for leaf, tt in c["pt"][mod].items():
            e = rel(hip_g[mod][leaf], tt.grad.numpy())
            worst = max(worst, e)
            assert e < lip * t["grad"], (mod, leaf, e)
    print(f"  gradients: worst max-rel {worst:.2e} (bound {lip * t['grad']:.3g})")
    if not bn and not separate:
        head = f"Dense_{len(feats) - (0 if arch == 'fc' else 3)}"
        for info in eng.infos:
            if info.name.decode().startswith(head + "/"):
                sl = slice(info.offset, info.offset + info.size)
                pn, m, v, _, _ = adam64(p0[sl].cpu().numpy(), 0.0, 0.0, g[sl].cpu().numpy(), 1, lr, 1.5e-4)
                _close(eng.params[sl].cpu(), pn, rtol=1e-6, atol=1e-9)
                _close(eng.adam_m[sl].cpu(), m, rtol=1e-6, atol=1e-12)
                _close(eng.adam_v[sl].cpu(), v, rtol=1e-5, atol=1e-15)
    assert int(eng.adam_count.item()) == 1


# ------------------------------------------------------------------ 6. gradient sparsity
@pytest.mark.parametrize("path", ["head-chain", "generic"])
@pytest.mark.parametrize("form", ["isdqn", "tfdqn", "isdqn-hist"])
def test_dl_dq_has_one_nonzero_per_transition_and_pair(form, path):
    """No gradient through any Q^val term: head k of the state rows supplies pair k's bonus and is itself learned in pair k - 1, yet
    its columns receive exactly that pair's one entry."""
    hist = HIST_POS if form.endswith("hist") else False
    feats, K, A, B = TINY, (0 if form == "tfdqn" else 3), 5, 6
    eng, _ = _engine(feats, A, 1 + K, B, seed=2, hist=hist, **MU)
    b = _Batch(eng, "cnn", B, A, seed=5, reward_scale=4.0 if hist else 1.0)
    g = torch.zeros_like(eng.params)
    if path == "generic":
        eng.grad_on_batch(b.cb, g)
    else:
        eng.learn_on_batch(b.cb, grad_out=g)
    torch.cuda.synchronize()
    nb = hist["nb"] if hist else 1
    d = _dout(eng, B, hist).reshape(B, 1 + K, A, nb)
    nz = (d != 0).any(-1)  # [B, heads, A]
    Kp, on0 = max(K, 1), (1 if K else 0)
    assert nz.sum() == B * Kp
    for k in range(Kp):
        assert nz[np.arange(B), on0 + k, b.action].all()
    if K:
        assert not nz[:, 0].any()  # head 0 is a value head only
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0


# ------------------------------------------------------------------ 7. the small-tau limit
@pytest.mark.parametrize("form", ["isdqn", "dqn", "tfdqn", "isdqn-hist"])
def test_small_tau_without_bonus_approaches_the_max_form_on_the_same_rows(form):
    """alpha = 0, tau = 1e-3: the device targets lie within gamma^n tau ln A (plus the float32 bound) above the tau = 0 targets on the
    same value rows -- the float64 max form on the device's own rows, and where one forward supplies the rows with the option on and
    off (every form but the DQN one, whose target forward grows from B to 2B rows) the device's own tau = 0 targets too."""
    hist = HIST_POS if form.endswith("hist") else False
    feats, K, A, B, tau = (TINY if hist else HEADLINE), (3 if form.startswith("isdqn") else 0), 9, 12, 1e-3
    got = []
    for kw in ({}, _mu(tau, 0.0, -1.0)):
        eng, _ = _engine(feats, A, 1 + K, B, seed=2, hist=hist, **kw)
        b = _Batch(eng, "cnn", B, A, seed=5)
        vrows = None
        if form == "dqn":
            tgt = torch.zeros_like(eng.params)
            eng.import_flax(_params(31, feats, A, 1, "cnn"), target=tgt)
            eng.loss_on_batch_target(b.cb, tgt)
            vrows = _trows(eng, B) if kw else None
        else:
            eng.loss_on_batch(b.cb)
        torch.cuda.synchronize()
        got.append((_cpu(eng.targets).astype(np.float64), _rows(eng, B, hist).numpy()))
    (t_off, r_off), (t_on, r_on) = got
    ref = _ref(eng, torch.from_numpy(r_on), b, value_rows=vrows, hist=hist)
    lim = 0.99 * tau * np.log(A)
    for name, t0 in (("float64 max form", ref["max_targets"]),) + ((("device, option off", t_off),) if form != "dqn" else ()):
        gap = t_on - t0
        print(f"{form} against the {name}: targets - max form in [{gap.min():.3g}, {gap.max():.3g}], gamma^n tau ln A = {lim:.3g}")
        assert (gap >= -FLOAT32_BOUND * ref["scale"]).all() and (gap <= lim + FLOAT32_BOUND * ref["scale"]).all()
    if form != "dqn":
        assert np.array_equal(r_off, r_on)  # the same forward: the same rows, bit for bit
    assert (ref["bonus"] == 0).all()


# ------------------------------------------------------------------ 8. the refused combinations
def _rc_loss(eng, b):
    from slimdqn import _hip

    return eng.lib.isdqn_net_loss_on_batch(ctypes.byref(eng.cfg), _hip.ptr(eng.params), ctypes.byref(b.cb), _hip.ptr(eng.losses),
                                           _hip.ptr(eng.q_values), _hip.ptr(eng.targets), _hip.ptr(eng.workspace), _hip.stream_ptr(eng.device))


def test_refused_combinations_return_their_codes():
    from slimdqn import _hip

    feats, K, A, B = TINY, 2, 3, 4
    eng, _ = _engine(feats, A, 1 + K, B, seed=1, **MU)
    b = _Batch(eng, "cnn", B, A, seed=5)
    assert _rc_loss(eng, b) == _hip.OK
    good = (0.03, 0.9, -1.0, 0)
    for tau, alpha, clip, dq in ((-0.03, 0.9, -1.0, 0), (0.03, 1.5, -1.0, 0), (0.03, -0.5, -1.0, 0), (0.03, 0.9, 0.5, 0), (0.03, 0.9, -1.0, 1),
                                 (float("nan"), 0.9, -1.0, 0), (0.03, 0.9, float("-inf"), 0)):
        c = eng.cfg
        c.munchausen_tau, c.munchausen_alpha, c.munchausen_clip, c.double_q = tau, alpha, clip, dq
        assert _rc_loss(eng, b) == _hip.ERR_ARG, (tau, alpha, clip, dq)
        assert b"munchausen" in eng.lib.isdqn_last_error()
    c.munchausen_tau, c.munchausen_alpha, c.munchausen_clip, c.double_q = good
    assert _rc_loss(eng, b) == _hip.OK
    torch.cuda.synchronize()
    bn, _ = _engine(feats, A, 1 + K, B, seed=1, batch_norm=True, **MU)
    bb = _Batch(bn, "cnn", B, A, seed=5)
    g = torch.zeros_like(bn.params)
    assert _rc_grad(bn, bb, g, None) == _hip.OK  # BatchNorm without target parameters: supported
    assert _rc_grad(bn, bb, g, bn.params.clone()) == _hip.ERR_UNSUPPORTED
    off, _ = _engine(feats, A, 1 + K, B, seed=1, batch_norm=True)
    b_off = _Batch(off, "cnn", B, A, seed=5)
    assert _rc_grad(off, b_off, g, off.params.clone()) == _hip.OK  # (what the option refuses exists without it)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        _engine(feats, A, 1 + K, B, seed=1, double_q=True, **MU)


# ------------------------------------------------------------------ 9. grad_on_batch with named pairs
@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("pairs", [(2, 1, 1), (1, 0, 2), (1, 1, 1)])
def test_grad_on_batch_with_named_pairs(pairs, with_target):
    """(online_head, target_head, n_pairs): value head target_head + k of the same rows or of the target parameters' 2B rows."""
    on0, tg0, n = pairs
    feats, K, A, B = TINY, 3, 5, 6
    eng, _ = _engine(feats, A, 1 + K, B, seed=2, **_mu(0.03, 0.9, -0.1))
    b = _Batch(eng, "cnn", B, A, seed=5)
    tgt = None
    if with_target:
        tgt = torch.zeros_like(eng.params)
        eng.import_flax(_params(TARGET_SEED, feats, A, 1 + K, "cnn"), target=tgt)
    g = torch.zeros_like(eng.params)
    losses = _cpu(eng.grad_on_batch(b.cb, g, target_params=tgt, online_head=on0, target_head=tg0, n_pairs=n))[:n]
    torch.cuda.synchronize()
    ref = _ref(eng, _rows(eng, B), b, value_rows=_trows(eng, B) if with_target else None, K=n, on0=on0, tg0=tg0)
    _clip_sides(ref, -0.1, True)
    first = lambda t: t.reshape(-1)[: B * n].reshape(B, n).cpu()  # (the call writes [B][n_pairs] rows into the engine's [B][K] buffers)
    _check_targets(first(eng.targets), ref)
    _close(first(eng.q_values), ref["q"])
    _behind(losses, ref["losses"], ref)
    _behind(_dout(eng, B), ref["dq"], ref)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0


# ------------------------------------------------------------------ 10. determinism and graphs
@pytest.mark.parametrize("form", ["isdqn", "dqn", "tfdqn"])
def test_two_learn_steps_are_bit_identical_from_identical_state(form):
    feats, K, A, B = HEADLINE, 9, 9, 32
    runs = []
    for _ in range(2):
        eng, _ = _engine(feats, A, 1 + K if form == "isdqn" else 1, B, seed=1, **MU)
        b = _Batch(eng, "cnn", B, A, seed=3)
        if form == "dqn":
            tgt = torch.zeros_like(eng.params)
            eng.import_flax(_params(TARGET_SEED, feats, A, 1, "cnn"), target=tgt)
            ls = [eng.learn_on_batch_target(b.cb, tgt).clone() for _ in range(2)]
        else:
            ls = [eng.learn_on_batch(b.cb).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.stack(ls), eng.priorities.clone(), eng.targets.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("prioritized", [False, True])
def test_isdqn_captured_learn_steps_equal_eager_steps(prioritized):
    """learn_steps(n) as one replay of a captured n-step graph against n eager update steps, rounds of n = 4 on a replay that grows
    between the rounds; prioritized: with the TD-error write-back inside the graph."""
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

    K, A, B, C, n = 3, 5, 8, 64, 4

    def make(use_graph):
        agent = iSDQN(0, (84, 84, 4), A, K, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 3, 1, 8, adam_eps=1.5e-4, batch_size=B,
                      use_graph=use_graph, **MU)
        assert abs(float(agent._engine.cfg.munchausen_tau) - 0.03) < 1e-8 and not agent._engine.double_q
        sampler = PrioritizedSamplingDistribution(5, C) if prioritized else UniformSamplingDistribution(5)
        agent.priority_writeback = prioritized
        return agent, ReplayBuffer(sampler, B, C, update_horizon=3, gamma=0.99)

    (eager, rb_e), (graphed, rb_g) = make(False), make(True)
    assert torch.equal(eager._engine.params, graphed._engine.params)
    rng = np.random.default_rng(0)
    for _ in range(20):
        _feed((rb_e, rb_g), rng, A, prioritized)
    for rnd in range(6):
        for _ in range(4):
            _feed((rb_e, rb_g), rng, A, prioritized)
        eager.learn_steps(n, rb_e)
        graphed.learn_steps(n, rb_g)
        if rnd % 2 == 1:
            for agent in (eager, graphed):
                agent.update_target_params(0)  # the head shift between two replays
        _same_state(eager, graphed, f"round {rnd}")
        if prioritized:
            ta, tb = rb_e._sampling_distribution._sum_tree, rb_g._sampling_distribution._sum_tree
            assert torch.equal(ta._nodes_dev, tb._nodes_dev)
    assert eager._graphed is None and graphed._graphed is not None and graphed._graphed.S == n
    assert int(eager._engine.adam_count.item()) == 6 * n
    # the option reached the captured engine, and survives an engine rebuilt for another batch size
    other = graphed._engine_for(2 * B)
    assert other.batch_size == 2 * B and (other.munchausen_tau, other.munchausen_alpha, other.munchausen_clip) == (0.03, 0.9, -1.0)
    assert abs(float(other.cfg.munchausen_alpha) - 0.9) < 1e-7 and float(other.cfg.munchausen_clip) == -1.0


@pytest.mark.parametrize("algo", ["dqn", "tfdqn"])
def test_single_head_captured_step_equals_eager_across_target_updates(algo):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.tfdqn import TFDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    A, B, C = 5, 8, 48

    def make(use_graph):
        if algo == "dqn":
            agent = DQN(0, (84, 84, 4), A, [8, 12, 16, 24], True, "cnn", 2e-4, 0.99, 3, 2, 6, adam_eps=1.5e-4, batch_size=B, use_graph=use_graph, **MU)
        else:
            agent = TFDQN(0, (84, 84, 4), A, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 3, 2, 6, adam_eps=1.5e-4, batch_size=B,
                          use_graph=use_graph, **MU)
        assert abs(float(agent._engine.cfg.munchausen_tau) - 0.03) < 1e-8
        return agent, ReplayBuffer(UniformSamplingDistribution(5), B, C, update_horizon=3, gamma=0.99)

    (eager, rb_e), (graphed, rb_g) = make(False), make(True)
    rng = np.random.default_rng(0)
    n_updates = n_targets = 0
    for step in range(1, 61):
        _feed((rb_e, rb_g), rng, A, False)
        if step > 14:
            for agent, rb in ((eager, rb_e), (graphed, rb_g)):
                agent.update_online_params(step, rb)
            le, lg = eager.update_target_params(step), graphed.update_target_params(step)
            assert le[0] == lg[0] and (not le[0] or le[1] == lg[1])
            n_targets += bool(le[0])
            if step % 2 == 0:
                n_updates += 1
                _same_state(eager, graphed, f"step {step}")
                if algo == "dqn":
                    assert torch.equal(eager.target_params.tensor, graphed.target_params.tensor)
    assert n_updates >= 20 and n_targets >= 5 and graphed._graphed is not None and eager._graphed is None


# ------------------------------------------------------------------ 11. the bounds-checked build
def test_no_load_of_the_option_leaves_the_tensors_it_was_given():
    """scripts/bounds_check.py, the cases named mq-*: site 31 (the value head's state / next-state rows in td_kernel and
    hl_loss_kernel; the DQN form reads them from the [2B] regions "q_target" / "logits_target") and every other site on the way."""
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bounds_check.py"), "mq-"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) >= 6 and all(r["case"].startswith("mq-") for r in rows), out.stdout
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent load in {r['case']}: site {r['site']} at {r['addr']}"


# ------------------------------------------------------------------ 12. the entry points
@pytest.mark.parametrize("algo", ["isdqn", "dqn"])
def test_entry_points_with_the_flag(algo, tmp_path, monkeypatch):
    import importlib
    import pickle

    from experiments.base import utils

    logged = []  # what the training loop hands its logger at every target update: {"loss": ..., "networks/k_loss": ...}
    monkeypatch.setattr(utils._NullLogger, "log", lambda self, logs: logged.append(dict(logs)))
    run = importlib.import_module(f"experiments.atari.{algo}").run
    argv = ["-en", "mq_Synthetic", "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "400", "-bs", "8", "-n", "1", "-horizon", "50",
            "-at", "cnn", "-ne", "2", "-ntspe", "200", "-utd", "1", "-nis", "20", "-ed", "100", "-ln", "-tuf", "16", "-env", "synthetic", "-mq"]
    if algo == "isdqn":
        argv += ["-nbi", "2"]
    gathered = run(argv, root=str(tmp_path))  # 2 x 200 environment steps, 380 gradient steps
    assert len(gathered) == 2 and all(np.isfinite(np.asarray(g, np.float64)).all() for g in gathered)
    losses = {k: [float(l[k]) for l in logged if k in l] for k in ("loss",) + (("networks/0_loss", "networks/1_loss") if algo == "isdqn" else ())}
    for k, v in losses.items():
        print(f"{algo} {k}: {len(v)} logged, in [{min(v):.3g}, {max(v):.3g}]")
        assert len(v) >= 20 and np.isfinite(v).all() and max(v) > 0, k  # (a target update every 16 of 380 gradient steps)
    out = tmp_path / "atari" / "exp_output" / "mq_Synthetic"
    stored = json.load(open(out / "parameters.json"))
    assert {k: v for k, v in stored[algo].items() if k.startswith("munchausen")} == dict(
        munchausen=True, munchausen_tau=0.03, munchausen_alpha=0.9, munchausen_clip=-1.0)
    assert not any(k.startswith("munchausen") for k in stored["shared_parameters"])
    model = pickle.load(open(out / algo / "models" / "1", "rb"))["params"]
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())
