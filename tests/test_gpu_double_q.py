"""Double Q-learning targets on the GPU (include/isdqn_hip.h, isdqn_net_config::double_q) against the float64 restatement of
tests/helpers/double_q.py, which is written from the header's definition:

1. off is off: an engine built with double_q=False is bit-identical to one built without the keyword, and a single head without
   target parameters (TF-DQN) gives the same bits with double_q = 1 through the C ABI;
2. the target step on the device's own Q rows (regions "q" / "q_target", "logits" / "logits_target"), exact ties included;
3. the batches bite: a* differs from the value head's own argmax on at least a quarter of the (b, k) pairs, and the targets differ
   from the max form's by more than 100 x the tolerance (asserted inside 2 and 5 on every batch);
4. the head chain (learn_on_batch) against the generic path (loss_on_batch), dL/dq with loss weights and the Huber loss;
5. the whole path against the float64 oracle forward: targets, losses, gradients of every leaf, one Adam step;
6. grad_on_batch with named head pairs, with and without target parameters; the refused combinations;
7. agents: run-to-run bit identity, the captured replay against eager steps, the entry points with -dq.

Section 5 and the argmax.  An argmax is discontinuous, so a (b, k) pair is left out of the comparison only when, IN THE FLOAT64
REFERENCE ALONE, the gap between the selector head's two largest values is below 10 x the q bound x max(1, |q|max); at most 10 % of a
case's pairs may be left out, and the seeds below leave out none (checked on the CPU with the oracle forward:
scripts/double_q_seeds.py).  Under that rule the single-pass bf16 bound (q 8e-2) leaves out every pair whose gap is below 0.8 x the
scale, which is nearly every pair of a freshly initialised network; the bf16 case therefore runs on a network whose head biases give
every head one dominant action (another one per head, so that selector and value head disagree): gaps of about 0.9 x the scale."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.gpu_helpers import adam64, make_frame_batch, perturbed_params
from tests.helpers import double_q as dq
from tests.helpers import per_weights as pw

pytestmark = pytest.mark.gpu

TOL = {"bf16x3": dict(q=1e-3, loss=1e-3, grad=3e-3), "bf16": dict(q=8e-2, loss=5e-2, grad=2.5e-1)}
RTOL, ATOL = 1e-5, 1e-7  # test_gpu_hl_gauss.py::_close: a float32 kernel against float64 on the same inputs
HIST = dict(nb=51, vmin=-10.0, vmax=10.0, sigma=0.75 * 20.0 / 51)
# The checks on the device's own logits (section 2) use a support that does not straddle zero.  A Q-value is the float32 sum of nb
# terms softmax_j * c_j; over [-10, 10] the terms cancel, and a Q-value near zero carries the rounding of terms of size 10 (a few
# 6e-7), which no relative bound covers.  Over [1, 21] every term is positive, so the error is a few ulps of the sum itself and
# rtol 1e-5 holds it for every row, not for lucky ones.  Same bin count and sigma / eta.
HIST_POS = dict(nb=51, vmin=1.0, vmax=21.0, sigma=0.75 * 20.0 / 51)


def _hd(hist):
    """the histogram settings of a case: False / None, True (HIST) or a dict of its own"""
    return None if not hist else (hist if isinstance(hist, dict) else HIST)
FC_OBS = (8,)
HEADLINE, TINY = (32, 64, 64, 512), (7, 9, 11, 13)
BIAS_SCALE = 0.3  # perturbation of biases / LayerNorm parameters: the heads' Q rows spread over a few tenths


def _obs(arch):
    return FC_OBS if arch == "fc" else (84, 84, 4)


def _params(seed, feats, A, n_heads, arch, ln=True, hist=False, batch_norm=False):
    return perturbed_params(seed, _obs(arch), feats, arch, n_heads * A * (HIST["nb"] if hist else 1), ln, scale=BIAS_SCALE, batch_norm=batch_norm)


def _engine(feats, A, n_heads, B, arch="cnn", ln=True, precision="bf16x3", seed=0, lr=1e-3, gamma_n=0.99, hist=False, huber_delta=0.0,
            batch_norm=False, **kw):
    """``kw``: double_q=... (absent: an engine built without the keyword)"""
    from slimdqn._engine import QNetEngine

    params = _params(seed, feats, A, n_heads, arch, ln, hist, batch_norm)
    h = _hd(hist)
    hkw = dict(n_bins=h["nb"], min_value=h["vmin"], max_value=h["vmax"], sigma=h["sigma"]) if hist else {}
    eng = QNetEngine(_obs(arch), A, n_heads, feats, arch, ln, B, gamma_n=gamma_n, learning_rate=lr, adam_eps=1.5e-4, precision=precision,
                     huber_delta=huber_delta, batch_norm=batch_norm, **hkw, **kw)
    stats = None
    if batch_norm:
        rng = np.random.default_rng(seed + 2)
        stats = {m: {"mean": rng.normal(0, 0.3, l["mean"].shape).astype(np.float32), "var": rng.uniform(0.5, 2.0, l["var"].shape).astype(np.float32)}
                 for m, l in onet.init_batch_stats(params).items()}
    eng.import_flax(params, batch_stats=stats)
    return eng, params


class _Batch:
    """One batch in both forms: the engine's C batch (``eng`` given) and the float64 network input [states; next states]."""

    def __init__(self, eng, arch, B, A, seed, reward_scale=1.0, weights=False):
        rng = np.random.default_rng(seed + 100)
        obs = _obs(arch)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.weights = rng.uniform(0.2, 1.0, B).astype(np.float32) if weights else None
        if arch == "fc":
            s = rng.normal(size=(B, obs[0])).astype(np.float32)
            ns = rng.normal(size=(B, obs[0])).astype(np.float32)
            self.action = rng.integers(0, A, B).astype(np.int32)
            self.terminal = (rng.random(B) < 0.3).astype(np.uint8)
            self.x_state, self.x_next = torch.from_numpy(s), torch.from_numpy(ns)
            self.reward = (rng.normal(size=B) * reward_scale).astype(np.float32)
            if eng is not None:
                self.cb = eng.make_batch(state=d(s), next_state=d(ns), action=d(self.action), reward=d(self.reward), terminal=d(self.terminal),
                                         loss_weights=None if self.weights is None else d(self.weights))
        else:
            frames, ids, action, _, terminal, ref = make_frame_batch(B, A, seed=seed, h=obs[0], w=obs[1], stack=obs[2])
            self.action, self.terminal = action, terminal
            self.reward = (rng.normal(size=B) * reward_scale).astype(np.float32)
            self.x_state, self.x_next = torch.from_numpy(ref.state), torch.from_numpy(ref.next_state)
            if eng is not None:
                self.cb = eng.make_batch(frames=d(frames), frame_stride=frames.shape[1], frame_ids=d(ids), action=d(action), reward=d(self.reward),
                                         terminal=d(terminal), loss_weights=None if self.weights is None else d(self.weights))


def _width(eng, hist):
    n = eng.n_heads * eng.n_actions * (HIST["nb"] if hist else 1)
    return n, (n + 7) // 8 * 8


def _rows(eng, B, hist=False):
    """the device's own head-output rows [2B][heads * A (* nb)] of the last forward (region "q", histogram heads "logits")"""
    n, n_p = _width(eng, hist)
    return eng.region("logits" if hist else "q")[: 2 * B * n_p].reshape(2 * B, n_p)[:, :n].double().cpu()


def _target_rows(eng, B, hist=False):
    """the target network's rows [B][...] of the last *_target call (region "q_target", histogram heads "logits_target")"""
    n, n_p = _width(eng, hist)
    return eng.region("logits_target" if hist else "q_target")[: B * n_p].reshape(B, n_p)[:, :n].double().cpu()


def _ref(eng, rows, b, value_rows=None, K=None, on0=None, tg0=0, hist=False, huber_delta=0.0):
    K = eng.n_regressed if K is None else K
    on0 = (1 if eng.n_heads >= 2 else 0) if on0 is None else on0
    return dq.double_q(rows, b.action, b.reward, b.terminal, float(eng.cfg.gamma_n), K, on0, tg0, eng.n_actions, value_rows=value_rows,
                       weights=b.weights, huber_delta=huber_delta, hist=_hd(hist))


def _close(a, b, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _bites(ref):
    """Section 3: the option changes these targets -- a* leaves the value head's own argmax on at least a quarter of the pairs, and
    some target moves by more than 100 x the tolerance of the comparison."""
    share = float((ref["a_star"] != ref["greedy"]).mean())
    assert share >= 0.25, share
    moved = np.abs(ref["targets"] - ref["max_targets"])
    assert (moved > 100 * (RTOL * np.abs(ref["targets"]) + ATOL)).any()
    return share


def _cpu(t):
    return t.detach().cpu().numpy().copy()


# ------------------------------------------------------------------ 1. off is off
def _one_step(eng, b, target=None):
    g = torch.zeros_like(eng.params)
    if target is None:
        losses = eng.learn_on_batch(b.cb, grad_out=g)
    else:
        losses = eng.learn_on_batch_target(b.cb, target)
    torch.cuda.synchronize()
    return [_cpu(x) for x in (losses, eng.q_values, eng.targets, eng.priorities, g, eng.params, eng.adam_m, eng.adam_v)]


@pytest.mark.parametrize("form", ["isdqn", "dqn", "isdqn-hist", "dqn-hist"])
def test_off_keeps_every_bit_and_the_workspace(form):
    hist, single = form.endswith("hist"), form.startswith("dqn")
    feats, K, A, B = (TINY, 3, 5, 6) if hist else (HEADLINE, 9, 9, 12)
    n_heads = 1 if single else 1 + K
    outs, sizes = [], []
    for kw in ({}, dict(double_q=False)):
        eng, _ = _engine(feats, A, n_heads, B, seed=3, hist=hist, **kw)
        b = _Batch(eng, "cnn", B, A, seed=5)
        target = None
        if single:
            target = torch.zeros_like(eng.params)
            eng.import_flax(_params(31, feats, A, 1, "cnn", hist=hist), target=target)
        outs.append(_one_step(eng, b, target))
        sizes.append(eng.workspace_bytes)
        assert int(eng.cfg.double_q) == 0
        with pytest.raises(RuntimeError):  # the target rows exist only with the option
            eng.region("q_target")
    assert sizes[0] == sizes[1]
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    on, _ = _engine(feats, A, n_heads, B, seed=3, hist=hist, double_q=True)
    assert on.workspace_bytes > sizes[0] and on.region("q_target").numel() >= B * ((n_heads * A + 7) // 8 * 8)
    for name in ("q", "dout", "wsplit", "loss_partials"):  # appended: nothing else moved
        assert on.region(name).data_ptr() - on.workspace.data_ptr() == eng.region(name).data_ptr() - eng.workspace.data_ptr()


@pytest.mark.parametrize("hist", [False, True])
def test_single_head_without_target_parameters_has_the_bits_of_off(hist):
    """TF-DQN through the C ABI: selector and value are the same head of the same rows, Q[argmax Q] == max Q."""
    feats, A, B = TINY, 5, 7
    outs = []
    for flag in (False, True):
        eng, _ = _engine(feats, A, 1, B, seed=8, hist=hist, double_q=flag)
        assert int(eng.cfg.double_q) == int(flag)
        b = _Batch(eng, "cnn", B, A, seed=17)
        pre = _cpu(eng.loss_on_batch(b.cb))
        outs.append([pre, _cpu(eng.targets)] + _one_step(eng, b))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 2. the target step on the device's own Q rows
OWN_ROWS = [
    pytest.param((HEADLINE, 9, 9, 12, "cnn", "bf16x3", False), id="headline-K9-A9-B12"),
    pytest.param((TINY, 3, 5, 6, "cnn", "bf16x3", False), id="tiny-B6"),
    pytest.param(((16, 16), 2, 3, 11, "fc", "bf16x3", False), id="fc-B11-ragged"),
    pytest.param(((8, 16, 16, 24), 2, 5, 4, "impala", "bf16x3", False), id="impala-B4"),
    pytest.param((TINY, 3, 5, 6, "cnn", "bf16", False), id="tiny-bf16"),
    pytest.param((TINY, 3, 5, 6, "cnn", "bf16x3", HIST_POS), id="tiny-hist"),
]


@pytest.mark.parametrize("shape", OWN_ROWS)
def test_isdqn_targets_match_float64_on_the_device_rows(shape):
    feats, K, A, B, arch, prec, hist = shape
    eng, _ = _engine(feats, A, 1 + K, B, arch=arch, precision=prec, seed=2, hist=hist, double_q=True)
    b = _Batch(eng, arch, B, A, seed=5, reward_scale=4.0 if hist else 1.0)
    # histogram heads: also the learn form, which takes the same loss kernel (no head chain) and leaves the priorities
    for learn in ((False, True) if hist else (False,)):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        ref = _ref(eng, _rows(eng, B, hist), b, hist=hist)
        share = _bites(ref)
        print(f"a* != greedy on {share:.2f} of the pairs; max |target - max form| {np.abs(ref['targets'] - ref['max_targets']).max():.3g}")
        assert b.terminal.any() and not b.terminal.all()
        if hist:  # selection on float32 expectations of float32 logits against float64 ones: only pairs the rounding cannot flip
            ex = dq.hl.expectations(_rows(eng, B, hist)[B:], hist["nb"], hist["vmin"], hist["vmax"]).reshape(B, 1 + K, A)[:, 1:].numpy()
            top = np.sort(ex, -1)
            assert (top[..., -1] - top[..., -2]).min() > 1e-4
        _close(eng.targets.cpu(), ref["targets"])
        _close(eng.q_values.cpu(), ref["q"])
        _close(losses, ref["losses"])
        if learn:
            _close(eng.priorities.cpu(), ref["priorities"])
            # dL/dlogit = (softmax - p(y)) / B, a check of this file's own.  The device holds the target y in float32: a few ulps of
            # |y| (r + nt * gamma * Q is three roundings on top of Q's own; 4 ulps taken), and the projection turns dy into
            # dp <= dy * max pdf = dy / (sigma sqrt(2 pi)) (a bin's mass is a difference of two values of the Gaussian's integral).
            # With targets up to the support's 21 that floor is 4 * 2^-23 * 21 / (sigma sqrt(2 pi)) / B, on top of the usual bound.
            n, n_p = _width(eng, hist)
            dout = eng.region("dout")[: B * n_p].reshape(B, n_p).double().cpu()
            floor = 4 * 2.0 ** -23 * hist["vmax"] / (hist["sigma"] * np.sqrt(2 * np.pi)) / B
            print(f"max |dout - helper| {np.abs(dout[:, :n].numpy() - ref['dq']).max():.3g} (floor {floor:.3g})")
            _close(dout[:, :n], ref["dq"], atol=ATOL + floor)


def test_bn_isdqn_targets_and_priorities_match_float64_on_the_device_rows():
    """BatchNorm iS-DQN: both heads lie in the rows of the one training-mode forward; its learn step takes the generic loss kernel,
    which also leaves the priorities."""
    feats, K, A, B = TINY, 2, 3, 4
    eng, _ = _engine(feats, A, 1 + K, B, seed=1, batch_norm=True, double_q=True)
    b = _Batch(eng, "cnn", B, A, seed=5)
    losses = _cpu(eng.learn_on_batch(b.cb))
    torch.cuda.synchronize()
    ref = _ref(eng, _rows(eng, B), b)
    _bites(ref)
    _close(eng.targets.cpu(), ref["targets"])
    _close(eng.q_values.cpu(), ref["q"])
    _close(losses, ref["losses"])
    _close(eng.priorities.cpu(), ref["priorities"])


@pytest.mark.parametrize("shape", [
    pytest.param((HEADLINE, 9, 12, "cnn", False), id="headline-A9-B12"),
    pytest.param((TINY, 5, 6, "cnn", False), id="tiny-B6"),
    pytest.param(((16, 16), 3, 11, "fc", False), id="fc-B11-ragged"),
    pytest.param((TINY, 5, 6, "cnn", HIST_POS), id="tiny-hist"),
])
def test_dqn_form_selects_online_and_values_with_the_target_rows(shape):
    """Double DQN: region "q" holds the ONLINE parameters' rows over concat(state, next_state), region "q_target" the target
    parameters' rows over the B next states; loss and learn forms, priorities from the learn form."""
    feats, A, B, arch, hist = shape
    eng, _ = _engine(feats, A, 1, B, arch=arch, seed=2, hist=hist, double_q=True)
    tgt = torch.zeros_like(eng.params)
    eng.import_flax(_params(31, feats, A, 1, arch, hist=hist), target=tgt)
    b = _Batch(eng, arch, B, A, seed=5, reward_scale=4.0 if hist else 1.0)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch_target(b.cb, tgt) if learn else eng.loss_on_batch_target(b.cb, tgt))
        torch.cuda.synchronize()
        rows, vrows = _rows(eng, B, hist), _target_rows(eng, B, hist)
        ref = _ref(eng, rows, b, value_rows=vrows, K=1, on0=0, hist=hist)
        _bites(ref)
        assert not np.array_equal(rows[B:].numpy(), vrows.numpy())  # two networks
        if hist:
            qt = eng.region("q_target")[: B * 8 * ((A + 7) // 8)].reshape(B, -1)[:, :A].double().cpu()
            _close(qt, dq.hl.expectations(vrows, hist["nb"], hist["vmin"], hist["vmax"]))
        _close(eng.targets.cpu(), ref["targets"])
        _close(eng.q_values.cpu(), ref["q"])
        _close(losses, ref["losses"])
        if learn:
            _close(eng.priorities.cpu(), ref["priorities"])
            n, n_p = _width(eng, hist)
            dout = eng.region("dout")[: B * n_p].reshape(B, n_p).double().cpu()
            _close(dout[:, :n], ref["dq"])


@pytest.mark.parametrize("form", ["isdqn", "dqn"])
def test_an_exact_tie_selects_the_first_index_on_the_device(form):
    """fc heads with zeroed weights: every row of a head is its bias vector, and the selector's biases tie two actions exactly."""
    feats, A, B = (16, 16), 4, 9
    K = 2 if form == "isdqn" else 1
    n_heads = 1 + K if form == "isdqn" else 1
    eng, params = _engine(feats, A, n_heads, B, arch="fc", seed=4, double_q=True)
    head = "Dense_2"
    tie = np.array([0.25, 1.5, -0.5, 1.5], np.float32)  # entries 1 and 3 tie; the value head tells them apart
    val = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in params.items()}
    p[head]["kernel"][:] = 0.0
    p[head]["bias"][:] = np.concatenate([val] + [tie] * K) if form == "isdqn" else tie
    eng.import_flax(p)
    b = _Batch(eng, "fc", B, A, seed=6)
    if form == "isdqn":
        eng.loss_on_batch(b.cb)
        rows, vrows, on0 = _rows(eng, B), None, 1
    else:
        tp = {m: {k: v.copy() for k, v in l.items()} for m, l in p.items()}
        tp[head]["bias"][:] = val
        tgt = torch.zeros_like(eng.params)
        eng.import_flax(tp, target=tgt)
        eng.loss_on_batch_target(b.cb, tgt)
        rows, vrows, on0 = _rows(eng, B), _target_rows(eng, B), 0
    torch.cuda.synchronize()
    sel = rows[B:].reshape(B, n_heads, A)[:, on0].numpy()
    assert (sel[:, 1] == sel[:, 3]).all() and (sel[:, 1] > sel[:, 0]).all()  # the tie is exact on the device too
    ref = _ref(eng, rows, b, value_rows=vrows, K=K, on0=on0)
    assert (ref["a_star"] == 1).all()
    _close(eng.targets.cpu(), ref["targets"])
    nt = 1.0 - b.terminal.astype(np.float64)
    _close(eng.targets.cpu()[:, 0], b.reward + nt * float(eng.cfg.gamma_n) * 2.0)  # value 2.0 at index 1, not 4.0 at index 3


# ------------------------------------------------------------------ 4. head chain vs generic path
@pytest.mark.parametrize("shape", [
    pytest.param((HEADLINE, 9, 9, 12, "cnn", "bf16x3", 0.0, False), id="headline-K9-A9-B12"),
    pytest.param((HEADLINE, 9, 9, 12, "cnn", "bf16x3", 0.5, True), id="headline-huber-weights"),
    pytest.param((TINY, 3, 5, 6, "cnn", "bf16x3", 0.0, True), id="tiny-weights"),
    pytest.param(((32, 32), 2, 4, 11, "fc", "bf16x3", 0.5, False), id="fc-ragged-huber"),
    pytest.param((HEADLINE, 9, 9, 12, "cnn", "bf16", 0.0, False), id="headline-bf16"),
])
def test_head_chain_agrees_with_the_generic_path(shape):
    feats, K, A, B, arch, prec, huber, weights = shape
    eng, _ = _engine(feats, A, 1 + K, B, arch=arch, precision=prec, seed=2, huber_delta=huber, double_q=True)
    b = _Batch(eng, arch, B, A, seed=5, weights=weights)
    pre = _cpu(eng.loss_on_batch(b.cb))  # generic path: leaves region "q"
    torch.cuda.synchronize()
    gen_q, gen_t = _cpu(eng.q_values), _cpu(eng.targets)
    ref = _ref(eng, _rows(eng, B), b, huber_delta=huber)
    _bites(ref)
    _close(gen_t, ref["targets"])
    _close(pre, ref["losses"])
    losses = _cpu(eng.learn_on_batch(b.cb))  # head chain
    torch.cuda.synchronize()
    # the bar of tests/test_gpu_fullsize_properties.py between the fused learn path and the forward path: 1e-3.  (Single-pass bf16:
    # both paths round the same operands to bf16 and differ only in the order of the fp32 sums.)
    assert np.abs(_cpu(eng.q_values) - gen_q).max() < 1e-3
    assert np.abs(_cpu(eng.targets) - gen_t).max() < 1e-3
    assert np.abs(losses - pre).max() < 1e-3 * max(1.0, float(np.abs(pre).max()))
    # dL/dq of the head chain: the helper's on the generic rows (same bar), and the existing loss on the step's OWN q / targets
    n, n_p = _width(eng, False)
    dout = _cpu(eng.region("dout")[: B * n_p].reshape(B, n_p).double())
    assert np.abs(dout[:, :n] - ref["dq"]).max() < 1e-3 * max(1.0, float(np.abs(ref["dq"]).max()))
    assert (dout[:, n:] == 0).all() and ((dout[:, :n] != 0) == (ref["dq"] != 0)).all()
    w = np.ones(B) if b.weights is None else b.weights
    own = pw.weighted_td(_cpu(eng.q_values), _cpu(eng.targets), w, huber)
    dense = np.zeros((B, 1 + K, A))
    for k in range(K):
        dense[np.arange(B), 1 + k, b.action] = own["dq"][:, k]
    _close(dout[:, :n], dense.reshape(B, -1))
    _close(losses, own["losses"])
    _close(eng.priorities.cpu(), np.sqrt(own["l"].mean(1) + 1e-10), rtol=2e-6, atol=1e-9)
    if huber > 0:
        d = np.abs(ref["q"] - ref["targets"])
        assert (d > huber).any() and (d < huber).any()


# ------------------------------------------------------------------ 5. the whole path against the float64 oracle forward
# (feats, K, A, B, arch, ln, form, params seed, batch seed); form: isdqn | dqn | bn | hist.  Seeds: see the module docstring.
E2E = {
    "headline-B4": (HEADLINE, 9, 9, 4, "cnn", True, "isdqn", 2, 8),
    "tiny": (TINY, 3, 5, 6, "cnn", True, "isdqn", 2, 1),
    "tiny-noln": ((16, 20, 5, 24), 2, 3, 5, "cnn", False, "isdqn", 2, 0),
    "fc-ragged": ((32, 32), 2, 4, 11, "fc", True, "isdqn", 2, 0),
    "impala": ((8, 16, 16, 24), 2, 5, 4, "impala", True, "isdqn", 2, 0),
    "bn": (TINY, 2, 3, 4, "cnn", True, "bn", 2, 0),
    "dqn-tiny": (TINY, 1, 5, 6, "cnn", True, "dqn", 2, 5),
    "dqn-fc": ((32, 32), 1, 4, 11, "fc", True, "dqn", 2, 3),
    "hist-tiny": (TINY, 3, 5, 6, "cnn", True, "hist", 2, 1),
    "tiny-bf16-dominant": (TINY, 3, 5, 6, "cnn", True, "isdqn", 2, 1),
}
E2E_PRECISION = {"tiny-bf16-dominant": "bf16"}  # (every other case: bf16x3)
# the bf16 case: head h gets the bias DOMINANT at action (2 h + 1) mod A -- consecutive heads prefer different actions -- on top of
# its perturbed bias, so that the selector's largest value leads the second by about 0.9 x the scale (the rule asks for 0.8)
DOMINANT = 20.0
TARGET_SEED = 31


def _with_dominant_actions(params, feats, arch, n_heads, A):
    head = f"Dense_{len(feats) - (0 if arch == 'fc' else 3)}"
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in params.items()}
    for h in range(n_heads):
        p[head]["bias"][h * A + (2 * h + 1) % A] += np.float32(DOMINANT)
    return p


def oracle_case(name):
    """Everything of a section-5 case that needs no GPU: parameters, batch, the float64 rows (with a graph through the online
    parameters), the helper's result on them and the pairs the argmax rule leaves out."""
    feats, K, A, B, arch, ln, form, pseed, bseed = E2E[name]
    hist, single, bn = form == "hist", form == "dqn", form == "bn"
    n_heads = 1 if single else 1 + K
    params = _params(pseed, feats, A, n_heads, arch, ln, hist, bn)
    if name.endswith("dominant"):
        params = _with_dominant_actions(params, feats, arch, n_heads, A)
    tparams = _params(TARGET_SEED, feats, A, 1, arch, ln, hist) if single else None
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
    vrows = onet.forward(onet.to_torch(tparams, torch.float64), b.x_next, feats, arch, ln).detach() if single else None
    on0 = 0 if single else 1
    ref = dq.double_q(rows, b.action, b.reward, b.terminal, 0.99, K, on0, 0, A, value_rows=vrows, hist=HIST if hist else None)
    # the pairs an argmax may flip: decided from the float64 selector rows alone
    sel = rows[B:].detach()
    if hist:
        sel = dq.hl.expectations(sel, HIST["nb"], HIST["vmin"], HIST["vmax"])
    sel = sel.reshape(B, n_heads, A)[:, on0 : on0 + K].numpy()
    top = np.sort(sel, -1)
    gap = top[..., -1] - top[..., -2]
    scale = max(1.0, float(np.abs(sel).max()))
    return dict(params=params, tparams=tparams, stats=stats, batch=b, pt=pt, rows=rows, ref=ref, gap=gap, scale=scale, n_heads=n_heads, on0=on0)


@pytest.mark.parametrize("name", list(E2E))
def test_whole_path_matches_the_float64_oracle(name):
    from slimdqn._engine import QNetEngine

    feats, K, A, B, arch, ln, form, pseed, bseed = E2E[name]
    prec, lr = E2E_PRECISION.get(name, "bf16x3"), 1e-3
    t = TOL[prec]
    c = oracle_case(name)
    ref, hist, single, bn = c["ref"], form == "hist", form == "dqn", form == "bn"
    _bites(ref)
    keep = c["gap"] >= 10 * t["q"] * c["scale"]  # [B, K]: decided from the float64 reference alone
    assert (~keep).mean() <= 0.10, f"{(~keep).sum()} of {keep.size} pairs left out"
    # (losses and gradients sum over every pair, so the committed seeds -- and the bf16 case's biases -- leave out none)
    assert keep.all(), f"{(~keep).sum()} of {keep.size} pairs left out: the committed cases leave out none"
    hkw = dict(n_bins=HIST["nb"], min_value=HIST["vmin"], max_value=HIST["vmax"], sigma=HIST["sigma"]) if hist else {}
    eng = QNetEngine(_obs(arch), A, c["n_heads"], feats, arch, ln, B, gamma_n=0.99, learning_rate=lr, adam_eps=1.5e-4, precision=prec,
                     batch_norm=bn, double_q=True, **hkw)
    eng.import_flax(c["params"], batch_stats=c["stats"])
    b = _Batch(eng, arch, B, A, seed=bseed, reward_scale=4.0 if hist else 1.0)
    tgt = None
    if single:
        tgt = torch.zeros_like(eng.params)
        eng.import_flax(c["tparams"], target=tgt)
    rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - want).max() / max(1.0, float(np.abs(want).max())))
    losses = _cpu(eng.loss_on_batch_target(b.cb, tgt) if single else eng.loss_on_batch(b.cb))
    print(f"{name}: q {rel(_cpu(eng.q_values), ref['q']):.2e} targets {rel(_cpu(eng.targets), ref['targets']):.2e} "
          f"loss {rel(losses, ref['losses']):.2e}; min selector gap {c['gap'].min():.3g} (bound {10 * t['q'] * c['scale']:.3g})")
    assert rel(_cpu(eng.q_values), ref["q"]) < t["q"]
    assert rel(_cpu(eng.targets)[keep], ref["targets"][keep]) < t["q"]
    assert rel(losses, ref["losses"]) < t["loss"]
    # gradients of every leaf against float64 autograd of the same helper loss; one Adam step from zero moments
    ref["loss_t"].sum().backward()
    p0 = eng.params.clone()
    g = torch.zeros_like(eng.params)
    if single:  # (the target form has no debug gradient: the gradient-only pass on the same loss)
        eng.grad_on_batch(b.cb, g, target_params=tgt)
        eng.learn_on_batch_target(b.cb, tgt)
    else:
        eng.learn_on_batch(b.cb, grad_out=g)
    torch.cuda.synchronize()
    hip_g = eng.internal_to_flax_grads(g)
    for mod in c["pt"]:
        for leaf, tt in c["pt"][mod].items():
            e = rel(hip_g[mod][leaf], tt.grad.numpy())
            rn = float(np.linalg.norm(np.asarray(hip_g[mod][leaf], np.float64) - tt.grad.numpy()) / max(np.linalg.norm(tt.grad.numpy()), 1e-30))
            print(f"  grad {mod}/{leaf}: max-rel {e:.2e} norm-rel {rn:.2e}")
            assert e < t["grad"], (mod, leaf, e)
    if not bn:  # (test_gpu_hl_gauss.py section 3c: the head leaves; BatchNorm steps are held to the oracle in test_gpu_batchnorm.py)
        head = f"Dense_{len(feats) - (0 if arch == 'fc' else 3)}"
        # (the target form's learn step exports no gradient -- `g` is the gradient-only pass's -- so the DQN form's parameter update is
        # covered by adam_count here and by the eager-against-captured and run-to-run tests of section 7 only)
        for info in eng.infos:
            if info.name.decode().startswith(head + "/") and not single:
                sl = slice(info.offset, info.offset + info.size)
                pn, m, v, _, _ = adam64(p0[sl].cpu().numpy(), 0.0, 0.0, g[sl].cpu().numpy(), 1, lr, 1.5e-4)
                _close(eng.params[sl].cpu(), pn, rtol=1e-6, atol=1e-9)
                _close(eng.adam_m[sl].cpu(), m, rtol=1e-6, atol=1e-12)
                _close(eng.adam_v[sl].cpu(), v, rtol=1e-5, atol=1e-15)
    assert int(eng.adam_count.item()) == 1


# ------------------------------------------------------------------ 6. grad_on_batch and the refused combinations
@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("pairs", [(2, 1, 1), (1, 0, 2), (1, 1, 1)])
def test_grad_on_batch_with_named_pairs(pairs, with_target):
    """(online_head, target_head, n_pairs): selector head online_head + k of the online parameters, value head target_head + k of
    the same rows or of the target parameters' rows.  (1, 1, 1) without target parameters is one head selecting and valuing."""
    on0, tg0, n = pairs
    feats, K, A, B = TINY, 3, 5, 6
    eng, _ = _engine(feats, A, 1 + K, B, seed=2, double_q=True)
    b = _Batch(eng, "cnn", B, A, seed=5)
    tgt = None
    if with_target:
        tgt = torch.zeros_like(eng.params)
        eng.import_flax(_params(TARGET_SEED, feats, A, 1 + K, "cnn"), target=tgt)
    g = torch.zeros_like(eng.params)
    losses = _cpu(eng.grad_on_batch(b.cb, g, target_params=tgt, online_head=on0, target_head=tg0, n_pairs=n))[:n]
    torch.cuda.synchronize()
    ref = _ref(eng, _rows(eng, B), b, value_rows=_target_rows(eng, B) if with_target else None, K=n, on0=on0, tg0=tg0)
    if with_target or on0 != tg0:
        _bites(ref)
    else:
        assert np.array_equal(ref["targets"], ref["max_targets"])
    first = lambda t: t.reshape(-1)[: B * n].reshape(B, n).cpu()  # (the call writes [B][n_pairs] rows into the engine's [B][K] buffers)
    _close(first(eng.targets), ref["targets"])
    _close(first(eng.q_values), ref["q"])
    _close(losses, ref["losses"])
    n_w, n_p = _width(eng, False)
    dout = eng.region("dout")[: B * n_p].reshape(B, n_p).double().cpu()
    _close(dout[:, :n_w], ref["dq"])
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0


def _rc_grad(eng, b, g, tgt):
    from slimdqn import _hip

    return eng.lib.isdqn_net_grad_on_batch(ctypes.byref(eng.cfg), _hip.ptr(eng.params), _hip.ptr(tgt), ctypes.byref(b.cb), 1, 1, 1, _hip.ptr(g),
                                           _hip.ptr(eng.losses), _hip.ptr(eng.q_values), _hip.ptr(eng.targets), _hip.ptr(eng.workspace),
                                           _hip.stream_ptr(eng.device))


def test_refused_combinations_return_their_codes():
    from slimdqn import _hip

    feats, K, A, B = TINY, 2, 3, 4
    eng, _ = _engine(feats, A, 1 + K, B, seed=1, batch_norm=True, double_q=True)
    b = _Batch(eng, "cnn", B, A, seed=5)
    g = torch.zeros_like(eng.params)
    assert _rc_grad(eng, b, g, None) == _hip.OK  # BatchNorm without target parameters: supported
    assert _rc_grad(eng, b, g, eng.params.clone()) == _hip.ERR_UNSUPPORTED
    off, _ = _engine(feats, A, 1 + K, B, seed=1, batch_norm=True)
    b_off = _Batch(off, "cnn", B, A, seed=5)
    assert _rc_grad(off, b_off, g, off.params.clone()) == _hip.OK  # (what the option refuses exists without it)
    torch.cuda.synchronize()
    plain, _ = _engine(feats, A, 1 + K, B, seed=1, double_q=True)
    bp = _Batch(plain, "cnn", B, A, seed=5)
    plain.cfg.double_q = 2
    assert _rc_grad(plain, bp, g, None) == _hip.ERR_ARG
    rc = plain.lib.isdqn_net_loss_on_batch(ctypes.byref(plain.cfg), _hip.ptr(plain.params), ctypes.byref(bp.cb), _hip.ptr(plain.losses),
                                           _hip.ptr(plain.q_values), _hip.ptr(plain.targets), _hip.ptr(plain.workspace), _hip.stream_ptr(plain.device))
    assert rc == _hip.ERR_ARG and b"double_q" in plain.lib.isdqn_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 7. agents
def test_target_free_agent_refuses_the_option():
    from slimdqn.networks.tfdqn import DOUBLE_Q_REFUSED, TFDQN

    with pytest.raises(ValueError) as e:
        TFDQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, double_q=True)
    assert str(e.value) == DOUBLE_Q_REFUSED


@pytest.mark.parametrize("form", ["isdqn", "dqn"])
def test_two_learn_steps_are_bit_identical_from_identical_state(form):
    feats, K, A, B = HEADLINE, 9, 9, 32
    runs = []
    for _ in range(2):
        eng, _ = _engine(feats, A, 1 + K if form == "isdqn" else 1, B, seed=1, double_q=True)
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


def _feed(rbs, rng, A, prioritized):
    from slimdqn.sample_collection.replay_buffer import TransitionElement

    obs = rng.integers(0, 256, (84, 84), dtype=np.uint8)
    a, r, term = int(rng.integers(0, A)), float(rng.choice([-1.0, 0.0, 1.0])), bool(rng.random() < 0.08)
    for rb in rbs:
        kw = dict(priority=rb._sampling_distribution.MAX_PRIORITY) if prioritized else {}
        rb.add(TransitionElement(obs, a, r, term, term), **kw)


def _same_state(eager, graphed, where):
    for name in ("params", "adam_m", "adam_v", "adam_count", "losses_accum"):
        x, y = getattr(eager._engine, name), getattr(graphed._engine, name)
        assert torch.equal(x, y), f"{where}: {name} differs between the eager and the captured steps"


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
                      use_graph=use_graph, double_q=True)
        assert agent._engine.double_q and int(agent._engine.cfg.double_q) == 1
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
    # the option reached the captured engine, and survives an engine rebuilt for another batch size and a model round trip
    other = graphed._engine_for(2 * B)
    assert other.double_q and other.batch_size == 2 * B and int(other.cfg.double_q) == 1
    model = graphed.get_model()
    assert graphed._engine.double_q and "params" in model


def test_dqn_captured_step_equals_eager_across_target_updates():
    from slimdqn.networks.dqn import DQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    A, B, C = 5, 8, 48

    def make(use_graph):
        agent = DQN(0, (84, 84, 4), A, [8, 12, 16, 24], True, "cnn", 2e-4, 0.99, 3, 2, 6, adam_eps=1.5e-4, batch_size=B, use_graph=use_graph,
                    double_q=True)
        assert int(agent._engine.cfg.double_q) == 1
        return agent, ReplayBuffer(UniformSamplingDistribution(5), B, C, update_horizon=3, gamma=0.99)

    (eager, rb_e), (graphed, rb_g) = make(False), make(True)
    rng = np.random.default_rng(0)
    n_updates = n_targets = n_apart = 0
    for step in range(1, 61):
        _feed((rb_e, rb_g), rng, A, False)
        if step > 14:
            for agent, rb in ((eager, rb_e), (graphed, rb_g)):
                agent.update_online_params(step, rb)
            le, lg = eager.update_target_params(step), graphed.update_target_params(step)
            assert le[0] == lg[0] and (not le[0] or le[1] == lg[1])
            n_targets += bool(le[0])
            n_apart += (not le[0]) and not torch.equal(graphed.params.tensor, graphed.target_params.tensor)
            if step % 2 == 0:
                n_updates += 1
                _same_state(eager, graphed, f"step {step}")
                assert torch.equal(eager.target_params.tensor, graphed.target_params.tensor)
    assert n_updates >= 20 and n_targets >= 5 and graphed._graphed is not None and eager._graphed is None
    assert n_apart >= 30  # between two target updates the selector (online parameters) is not the value network


@pytest.mark.parametrize("algo", ["isdqn", "dqn"])
def test_entry_points_with_the_flag(algo, tmp_path):
    import importlib

    run = importlib.import_module(f"experiments.atari.{algo}").run
    argv = ["-en", "dq_Synthetic", "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "400", "-bs", "8", "-n", "1", "-horizon", "50",
            "-at", "cnn", "-ne", "2", "-ntspe", "200", "-utd", "1", "-nis", "20", "-ed", "100", "-ln", "-tuf", "16", "-env", "synthetic", "-dq"]
    if algo == "isdqn":
        argv += ["-nbi", "2"]
    gathered = run(argv, root=str(tmp_path))  # 2 x 200 environment steps, 380 gradient steps
    assert len(gathered) == 2
    out = tmp_path / "atari" / "exp_output" / "dq_Synthetic"
    stored = json.load(open(out / "parameters.json"))
    assert stored[algo]["double_q"] is True and "double_q" not in stored["shared_parameters"]
    import pickle

    model = pickle.load(open(out / algo / "models" / "1", "rb"))["params"]
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())
