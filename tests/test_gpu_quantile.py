"""QR-DQN quantile-regression heads on the GPU (include/isdqn_hip.h, isdqn_net_config::n_quantiles; csrc/quantile.h) against the
float64 restatement of tests/helpers/quantile.py, which is written from the header's definition:

1. off is off: n_quantiles=0 is bit-identical to an engine built without the keyword, scalar and histogram heads;
2. the loss kernel on the device's own rows (region "logits"), with bounds derived from the summation lengths;
3. the whole path against the float64 oracle forward (loss_on_batch; the *_target form for the single head);
4. gradients of every leaf and one Adam step;
5. Double Q-learning, both forms, exact ties included;
6. acting on the means, shift_params on whole blocks;
7. run-to-run bit identity and the captured multi-step replay;
8. the entry points with -qr.

Every network here gets separated action means.  The means of N near-iid outputs of a freshly perturbed network differ by ~1e-2, which
an argmax cannot hold against the forward's 1e-3; so the head bias of block (h, a) gets SPREAD x pi_h(a), SPREAD = 0.5, pi_h a seeded permutation of
0..A-1 (another one per head: selector and value heads prefer different actions), and every block linspace(-0.5, 0.5, N) across its N
outputs (distinct quantile values).  scripts/quantile_seeds.py checks on the CPU that the committed cases of section 3 then leave out
no pair.

Bounds of section 2 (u = 2^-24; any summation order of n float32 terms errs by at most (n - 1) u sum |terms|): the kernel forms
c_ij = |tau_i - 1{u_ij < 0}| clip(u_ij) with tau_i, 1 - tau_i, u_ij and the product each rounded (4 u), sums N of them, divides by kappa
and scales by w_b / (B N) (a division and a product): (N + 8) u covers it.  The indicators agree exactly (tests/helpers/quantile.py)."""
import json

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.gpu_helpers import adam64, make_frame_batch, perturbed_params
from tests.helpers import quantile as qr

pytestmark = pytest.mark.gpu

U = 2.0**-24
TOL = {"bf16x3": dict(q=1e-3, loss=1e-3, grad=3e-3), "bf16": dict(q=8e-2, loss=5e-2, grad=2.5e-1)}
RTOL, ATOL = 1e-5, 1e-7  # the project's bound of a float32 kernel against float64 on the same inputs (priorities)
FC_OBS = (8,)
HEADLINE, TINY = (32, 64, 64, 512), (7, 9, 11, 13)
SPREAD = 0.5
# single-pass bf16 (q bound 8e-2): the rule of section 3 leaves out every pair whose gap is below 0.8 x max(1, |Q|max), which no
# permutation x spread can meet (its gap is 1 / (A - 1) of its largest mean).  There every head's preferred action -- pi_h(a) = A - 1 --
# gets DOMINANT on top, as the dominant biases of tests/test_gpu_double_q.py: gaps of about 0.9 x the scale.
DOMINANT = {"bf16x3": 0.0, "bf16": 20.0}


def _obs(arch):
    return FC_OBS if arch == "fc" else (84, 84, 4)


def _head(feats, arch):
    return f"Dense_{len(feats) - (0 if arch == 'fc' else 3)}"


def spread_bias(params, feats, arch, n_heads, A, N, seed, dominant=0.0):
    """Block (h, a) of the head bias += SPREAD x pi_h(a) (+ dominant where pi_h(a) = A - 1), every block += linspace(-0.5, 0.5, N)."""
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in params.items()}
    rng = np.random.default_rng(seed + 7)
    bias = p[_head(feats, arch)]["bias"].reshape(n_heads, A, N)
    for h in range(n_heads):
        pi = rng.permutation(A)
        bias[h] += (SPREAD * pi + dominant * (pi == A - 1)).astype(np.float32)[:, None]
    bias += np.linspace(-0.5, 0.5, N, dtype=np.float32)
    return p


def _params(seed, feats, A, n_heads, arch, N, ln=True, dominant=0.0):
    p = perturbed_params(seed, _obs(arch), feats, arch, n_heads * A * N, ln)
    return spread_bias(p, feats, arch, n_heads, A, N, seed, dominant)


def _reward_shift(A, dominant=0.0):
    """centre of the rewards: minus half of what the best action's atoms lead a random action's quantiles by"""
    return -0.5 * (SPREAD * (A - 1) + dominant)


def _engine(feats, A, n_heads, B, N, kappa=1.0, arch="cnn", ln=True, precision="bf16x3", seed=0, lr=1e-3, **kw):
    from slimdqn._engine import QNetEngine

    params = _params(seed, feats, A, n_heads, arch, N, ln, DOMINANT[precision])
    eng = QNetEngine(_obs(arch), A, n_heads, feats, arch, ln, B, gamma_n=0.99, learning_rate=lr, adam_eps=1.5e-4, precision=precision,
                     huber_delta=kappa, n_quantiles=N, **kw)
    eng.import_flax(params)
    return eng, params


class _Batch:
    """One batch in both forms: the engine's C batch (``eng`` given) and the float64 network input [states; next states].  The rewards are
    centred at _reward_shift(A): the atoms come from the value head's best action, the online quantiles from a random one."""

    def __init__(self, eng, arch, B, A, seed, weights=False, reward_shift=None):
        rng = np.random.default_rng(seed + 100)
        obs = _obs(arch)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.weights = rng.uniform(0.2, 1.0, B).astype(np.float32) if weights else None
        shift = _reward_shift(A) if reward_shift is None else reward_shift
        if arch == "fc":
            s = rng.normal(size=(B, obs[0])).astype(np.float32)
            ns = rng.normal(size=(B, obs[0])).astype(np.float32)
            self.action = rng.integers(0, A, B).astype(np.int32)
            self.terminal = (rng.random(B) < 0.3).astype(np.uint8)
            self.x_state, self.x_next = torch.from_numpy(s), torch.from_numpy(ns)
            self.reward = (rng.normal(size=B) + shift).astype(np.float32)
            if eng is not None:
                self.cb = eng.make_batch(state=d(s), next_state=d(ns), action=d(self.action), reward=d(self.reward), terminal=d(self.terminal),
                                         loss_weights=None if self.weights is None else d(self.weights))
        else:
            frames, ids, action, _, terminal, ref = make_frame_batch(B, A, seed=seed, h=obs[0], w=obs[1], stack=obs[2])
            self.action, self.terminal = action, terminal
            self.reward = (rng.normal(size=B) + shift).astype(np.float32)
            self.x_state, self.x_next = torch.from_numpy(ref.state), torch.from_numpy(ref.next_state)
            if eng is not None:
                self.fr, self.ids, self.stride = d(frames), d(ids), frames.shape[1]
                self.cb = eng.make_batch(frames=self.fr, frame_stride=self.stride, frame_ids=self.ids, action=d(action), reward=d(self.reward),
                                         terminal=d(terminal), loss_weights=None if self.weights is None else d(self.weights))

    def obs_kw(self, rows):
        """forward / best_actions keywords for the first `rows` states"""
        if hasattr(self, "fr"):
            stack = self.ids.shape[1] // 2
            return dict(frames=self.fr, frame_stride=self.stride, frame_ids=self.ids[:rows, :stack].contiguous())
        return dict(obs=self.x_state[:rows].cuda())


def _width(eng):
    n = eng.n_heads * eng.n_actions * eng.n_quantiles
    return n, (n + 7) // 8 * 8


def _rows(eng, B, region="logits", n_rows=None):
    """the device's own quantile rows [2B][heads * A * N] of the last forward (region "logits": [2B][padded to 8])"""
    n, n_p = _width(eng)
    n_rows = 2 * B if n_rows is None else n_rows
    return eng.region(region)[: n_rows * n_p].reshape(n_rows, n_p)[:, :n].double().cpu()


def _ref(eng, rows, b, K=None, on0=None, tg0=0, **kw):
    K = eng.n_regressed if K is None else K
    on0 = (1 if eng.n_heads >= 2 else 0) if on0 is None else on0
    return qr.qr_loss(rows, b.action, b.reward, b.terminal, float(eng.cfg.gamma_n), K, on0, tg0, eng.n_actions, eng.n_quantiles,
                      float(eng.cfg.huber_delta), weights=b.weights, **kw)


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _close(a, b, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def check_device_step_against_rows(eng, b, ref, losses, B, K, on0, learn, tag=""):
    """Section 2's derived bounds: the outputs of one loss / learn call against the helper on the device's own rows."""
    A, N = eng.n_actions, eng.n_quantiles
    g = float(eng.cfg.gamma_n)
    # a*: the helper's top-two gap is far above anything rounding moves, for every pair -- the targets below then pin the device's a*
    assert float(ref["gap"].min()) > 1e-5 * max(1.0, ref["qmax"]), (float(ref["gap"].min()), ref["qmax"])
    rows_on = ref["rows_on"]  # [B, K, N] online quantiles at the taken action
    atoms = ref["atoms"]  # [B, K, N] value quantiles at a*
    q_bound = 16 * U * np.abs(rows_on).mean(-1)
    nt = 1.0 - b.terminal.astype(np.float64)
    qv = ref["targets"].numpy() - b.reward[:, None].astype(np.float64)  # = nt gamma^n Q^val(s', a*)
    t_bound = 16 * U * g * nt[:, None] * np.abs(atoms).mean(-1) + 4 * U * (np.abs(b.reward.astype(np.float64))[:, None] + np.abs(qv))
    eq = np.abs(_cpu(eng.q_values).astype(np.float64) - ref["q"].detach().numpy())
    et = np.abs(_cpu(eng.targets).astype(np.float64) - ref["targets"].numpy())
    want_l = ref["losses"].detach().numpy()
    el = np.abs(losses.astype(np.float64) - want_l) / want_l
    l_bound = (N + B + 32) * U
    print(f"{tag}: q err/bound {float((eq / q_bound).max()):.3f}, targets err/bound {float((et / t_bound).max()):.3f}, "
          f"loss rel err {float(el.max()):.3e} (bound {l_bound:.3e}), share u<0 {ref['neg_share']:.2f}, min gap {float(ref['gap'].min()):.3g}")
    assert (eq <= q_bound).all(), float((eq / q_bound).max())
    assert (et <= t_bound).all(), float((et / t_bound).max())
    assert (want_l > 0).all() and (el <= l_bound).all(), el
    if not learn:
        return
    _close(_cpu(eng.priorities), ref["priorities"].numpy())
    n, n_p = _width(eng)
    dout = eng.region("dout")[: B * n_p].reshape(B, n_p).double().cpu().numpy()
    w = np.ones(B) if b.weights is None else b.weights.astype(np.float64)
    bound = np.zeros((B, eng.n_heads, A, N))
    bi, ki = np.arange(B)[:, None], np.arange(K)[None, :]
    bound[bi, on0 + ki, b.action[:, None].astype(np.int64)] = (N + 8) * U * (w[:, None, None] / (B * N)) * ref["cabs"].numpy()
    ed = np.abs(dout[:, :n] - ref["dtheta"].numpy())
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound.reshape(B, -1) > 0, ed / bound.reshape(B, -1), 0.0)
    print(f"{tag}: dout err/bound {float(ratio.max()):.3f} (largest |dout| {float(np.abs(dout).max()):.3g})")
    assert (ed <= bound.reshape(B, -1)).all(), float(ratio.max())  # (a zero bound -- every other output -- asks for exactly 0)
    assert (dout[:, n:] == 0).all()


def _ref_with_rows(eng, rows, b, K=None, on0=None, **kw):
    """_ref plus the two row selections the bounds of section 2 are written in"""
    ref = _ref(eng, rows, b, K=K, on0=on0, **kw)
    B, A, N = rows.shape[0] // 2, eng.n_actions, eng.n_quantiles
    K = ref["q"].shape[1]
    on0 = (1 if eng.n_heads >= 2 else 0) if on0 is None else on0
    bi, ki = np.arange(B)[:, None], np.arange(K)[None, :]
    on = rows[:B].reshape(B, -1, A, N).numpy()
    val = (rows[B:] if kw.get("value_rows") is None else kw["value_rows"]).reshape(B, -1, A, N).numpy()
    ref["rows_on"] = on[bi, on0 + ki, b.action[:, None].astype(np.int64)]
    ref["atoms"] = val[bi, ki, ref["a_star"].numpy()]
    return ref


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("n_bins", [0, 51])
def test_n_quantiles_zero_is_bit_identical_to_an_engine_built_without_the_keyword(n_bins):
    from slimdqn._engine import QNetEngine

    feats, K, A, B = TINY, 3, 5, 6
    hkw = dict(n_bins=n_bins, min_value=-10.0, max_value=10.0, sigma=0.3) if n_bins else {}
    outs, sizes = [], []
    for kw in ({}, dict(n_quantiles=0)):
        params = perturbed_params(3, (84, 84, 4), feats, "cnn", (1 + K) * A * max(n_bins, 1), True)
        eng = QNetEngine((84, 84, 4), A, 1 + K, feats, "cnn", True, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, **hkw, **kw)
        eng.import_flax(params)
        b = _Batch(eng, "cnn", B, A, seed=5, reward_shift=0.0)
        losses = eng.learn_on_batch(b.cb)
        torch.cuda.synchronize()
        assert int(eng.cfg.n_quantiles) == 0 and eng.n_quantiles == 0
        outs.append([_cpu(x) for x in (eng.params, eng.adam_m, eng.adam_v, losses, eng.priorities, eng.q_values, eng.targets)])
        sizes.append(eng.workspace_bytes)
    assert sizes[0] == sizes[1]
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 2. the loss kernel on the device's own rows
OWN_ROWS = [
    pytest.param((2, 1.0, 3, 5, 6, "cnn", TINY), id="N2"),
    pytest.param((64, 1.0, 3, 5, 6, "cnn", TINY), id="N64"),
    pytest.param((65, 1.0, 3, 5, 6, "cnn", TINY), id="N65"),
    pytest.param((200, 1.0, 2, 9, 5, "cnn", TINY), id="N200-four-per-lane"),
    pytest.param((200, 0.0, 2, 9, 5, "cnn", TINY), id="N200-pinball"),
    pytest.param((51, 1.0, 9, 9, 12, "cnn", HEADLINE), id="N51-headline"),
    pytest.param((32, 1.0, 2, 3, 11, "fc", (16, 16)), id="N32-fc-B11-ragged-weights"),
]


@pytest.mark.parametrize("shape", OWN_ROWS)
def test_loss_kernel_matches_float64_on_the_device_rows(shape, request):
    N, kappa, K, A, B, arch, feats = shape
    eng, _ = _engine(feats, A, 1 + K, B, N, kappa, arch=arch)
    b = _Batch(eng, arch, B, A, seed=5, weights=arch == "fc")
    losses = _cpu(eng.learn_on_batch(b.cb))
    torch.cuda.synchronize()
    ref = _ref_with_rows(eng, _rows(eng, B), b)
    assert 0.2 <= ref["neg_share"] <= 0.8, ref["neg_share"]  # both sides of every quantile's indicator
    assert b.terminal.any() and not b.terminal.all()
    check_device_step_against_rows(eng, b, ref, losses, B, K, 1, True, tag=request.node.callspec.id)


# ------------------------------------------------------------------ 3. the whole path against the float64 oracle forward
E2E = {
    "cnn-ln": (TINY, 3, 5, 6, "cnn", True, "bf16x3", False),
    "cnn-noln": ((16, 20, 5, 24), 2, 3, 5, "cnn", False, "bf16x3", False),
    "cnn-headline-B8": (HEADLINE, 9, 9, 8, "cnn", True, "bf16x3", False),
    "fc-ln": ((32, 32), 2, 4, 9, "fc", True, "bf16x3", False),
    "impala-ln": ((8, 16, 16, 24), 2, 5, 4, "impala", True, "bf16x3", False),
    "cnn-ln-bf16": (TINY, 3, 5, 6, "cnn", True, "bf16", False),
    "dqn-tiny": (TINY, 1, 5, 6, "cnn", True, "bf16x3", True),
}
E2E_N, E2E_KAPPA, PARAM_SEED, BATCH_SEED, TARGET_SEED = 32, 1.0, 2, 9, 32


def oracle_case(name):
    """Everything of a section-3 case that needs no GPU: parameters, batch, the float64 rows (with a graph through the online
    parameters), the helper's result on them and the top-two gap of the deciding head's means per pair."""
    feats, K, A, B, arch, ln, prec, single = E2E[name]
    n_heads = 1 if single else 1 + K
    params = _params(PARAM_SEED, feats, A, n_heads, arch, E2E_N, ln, DOMINANT[prec])
    tparams = _params(TARGET_SEED, feats, A, 1, arch, E2E_N, ln, DOMINANT[prec]) if single else None
    b = _Batch(None, arch, B, A, seed=BATCH_SEED, reward_shift=_reward_shift(A, DOMINANT[prec]))
    pt = onet.to_torch(params, torch.float64, requires_grad=True)
    rows = torch.cat([onet.forward(pt, b.x_state, feats, arch, ln), onet.forward(pt, b.x_next, feats, arch, ln)])
    vrows = onet.forward(onet.to_torch(tparams, torch.float64), b.x_next, feats, arch, ln).detach() if single else None
    on0 = 0 if single else 1
    ref = qr.qr_loss(rows, b.action, b.reward, b.terminal, float(np.float32(0.99)), K, on0, 0, A, E2E_N, E2E_KAPPA, value_rows=vrows)
    return dict(params=params, tparams=tparams, batch=b, pt=pt, rows=rows, ref=ref, gap=ref["gap"].numpy(), scale=max(1.0, ref["qmax"]),
                n_heads=n_heads, on0=on0)


@pytest.mark.parametrize("name", list(E2E))
def test_whole_path_matches_the_float64_oracle(name):
    from slimdqn._engine import QNetEngine

    feats, K, A, B, arch, ln, prec, single = E2E[name]
    t = TOL[prec]
    c = oracle_case(name)
    ref = c["ref"]
    # the atoms are taken at an argmax: a pair is left out only when, in the float64 reference alone, the deciding head's top-two gap
    # is below 10 x the q bound x max(1, |Q|max); at most 10 % may be, and the committed cases leave out none
    keep = c["gap"] >= 10 * t["q"] * c["scale"]
    assert (~keep).mean() <= 0.10, f"{(~keep).sum()} of {keep.size} pairs left out"
    assert keep.all(), f"{(~keep).sum()} of {keep.size} pairs left out: the committed cases leave out none"
    eng = QNetEngine(_obs(arch), A, c["n_heads"], feats, arch, ln, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, precision=prec,
                     huber_delta=E2E_KAPPA, n_quantiles=E2E_N)
    eng.import_flax(c["params"])
    b = _Batch(eng, arch, B, A, seed=BATCH_SEED, reward_shift=_reward_shift(A, DOMINANT[prec]))
    rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - np.asarray(want)).max() / max(1.0, float(np.abs(np.asarray(want)).max())))
    forms = [("loss_on_batch", lambda: eng.loss_on_batch(b.cb), ref)] if not single else []
    if single:
        tgt = torch.zeros_like(eng.params)
        eng.import_flax(c["tparams"], target=tgt)
        forms.append(("loss_on_batch_target", lambda: eng.loss_on_batch_target(b.cb, tgt), ref))
        forms.append(("learn_on_batch_target", lambda: eng.learn_on_batch_target(b.cb, tgt), ref))
    for form, call, want in forms:
        losses = _cpu(call())
        torch.cuda.synchronize()
        eq, et = rel(_cpu(eng.q_values), want["q"].detach().numpy()), rel(_cpu(eng.targets), want["targets"].numpy())
        el = rel(losses, want["losses"].detach().numpy())
        print(f"{name} {form}: q {eq:.2e} targets {et:.2e} (bound {t['q']:.0e}) loss {el:.2e} (bound {t['loss']:.0e}); "
              f"min gap {c['gap'].min():.3g} (bound {10 * t['q'] * c['scale']:.3g})")
        assert eq < t["q"] and et < t["q"] and el < t["loss"]


# ------------------------------------------------------------------ 4. gradients and Adam
def _s8_values(region: torch.Tensor, rows, pitch):
    """fp32 values of an S8 activation block [rows][pitch] (every 8 floats: 8 bf16 hi halves, then 8 lo halves)."""
    u16 = region.cpu().numpy()[: rows * pitch].view(np.uint16).reshape(rows, pitch // 8, 2, 8)
    f = lambda h: (h.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return (f(u16[:, :, 0]) + f(u16[:, :, 1])).reshape(rows, pitch)


@pytest.mark.parametrize("shape", [
    pytest.param((TINY, 3, 5, 6, "cnn"), id="cnn-tiny"),
    pytest.param(((32, 32), 2, 4, 9, "fc"), id="fc"),
])
def test_learn_gradients_and_adam_of_quantile_heads(shape):
    feats, K, A, B, arch = shape
    N, lr = 32, 1e-3
    eng, params = _engine(feats, A, 1 + K, B, N, 1.0, arch=arch, seed=4, lr=lr)  # kappa = 1: the gradient is continuous
    b = _Batch(eng, arch, B, A, seed=13)
    p0 = eng.params.clone()
    g = torch.zeros_like(eng.params)
    eng.learn_on_batch(b.cb, grad_out=g)
    torch.cuda.synchronize()
    hip_g = eng.internal_to_flax_grads(g)
    head = _head(feats, arch)
    hid = f"Dense_{int(head.split('_')[1]) - 1}"
    # (a) head leaves against float64 dtheta^T . act from the device's own rows and hidden activations
    ref = _ref(eng, _rows(eng, B), b)
    F = feats[-1]
    act = _s8_values(eng.region(f"act/{hid}"), B, (F + 7) // 8 * 8)[:, :F]
    dl = ref["dtheta"].numpy()
    for leaf, want in (("kernel", act.T @ dl), ("bias", dl.sum(0))):
        got = np.asarray(hip_g[head][leaf], np.float64)
        e = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"head {leaf}: norm-rel {e:.2e} (bound 1e-4)")
        assert e <= 1e-4, (leaf, e)
    # (b) every leaf against float64 autograd of the helper's loss on the oracle forward
    pt = onet.to_torch(params, torch.float64, requires_grad=True)
    rows = torch.cat([onet.forward(pt, b.x_state, feats, arch, True), onet.forward(pt, b.x_next, feats, arch, True).detach()])
    oref = _ref(eng, rows, b)
    assert float(oref["gap"].min()) > 10 * TOL["bf16x3"]["q"] * max(1.0, oref["qmax"])  # no argmax of the oracle forward can flip
    oref["losses"].sum().backward()
    for mod in pt:
        for leaf, t in pt[mod].items():
            want = t.grad.numpy()
            got = np.asarray(hip_g[mod][leaf], np.float64)
            e = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
            print(f"grad {mod}/{leaf}: norm-rel {e:.2e} (bound {10 * TOL['bf16x3']['grad']:.0e})")
            assert e <= 10 * TOL["bf16x3"]["grad"], (mod, leaf, e)
    # (c) Adam on the head leaves: one optax step from zero moments with the device's gradient
    for info in eng.infos:
        if info.name.decode().startswith(head + "/"):
            sl = slice(info.offset, info.offset + info.size)
            pn, m, v, _, _ = adam64(p0[sl].cpu().numpy(), 0.0, 0.0, g[sl].cpu().numpy(), 1, lr, 1.5e-4)
            _close(eng.params[sl].cpu(), pn, rtol=1e-6, atol=1e-9)
            _close(eng.adam_m[sl].cpu(), m, rtol=1e-6, atol=1e-12)
            _close(eng.adam_v[sl].cpu(), v, rtol=1e-5, atol=1e-15)
    assert int(eng.adam_count.item()) == 1


# ------------------------------------------------------------------ 5. Double Q-learning
def _bites(ref, vrows_means, K, tg0=0):
    """a* leaves the value head's own argmax on at least a quarter of the pairs"""
    greedy = qr.first_argmax(vrows_means[:, tg0 : tg0 + K])
    share = float((ref["a_star"] != greedy).double().mean())
    assert share >= 0.25, share
    return share


@pytest.mark.parametrize("shape", [
    pytest.param((TINY, 3, 5, 6, "cnn", 33), id="tiny-N33"),
    pytest.param(((16, 16), 2, 3, 11, "fc", 32), id="fc-B11-ragged"),
])
def test_isdqn_double_q_matches_the_helper_with_selector_rows(shape, request):
    feats, K, A, B, arch, N = shape
    eng, _ = _engine(feats, A, 1 + K, B, N, 1.0, arch=arch, seed=2, double_q=True)
    b = _Batch(eng, arch, B, A, seed=5, weights=arch == "fc")
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        rows = _rows(eng, B)
        ref = _ref_with_rows(eng, rows, b, selector_rows=rows[B:])
        _bites(ref, qr.means(rows[B:], N).reshape(B, 1 + K, A), K)
        check_device_step_against_rows(eng, b, ref, losses, B, K, 1, learn, tag=f"{request.node.callspec.id} learn={learn}")


@pytest.mark.parametrize("shape", [
    pytest.param((TINY, 5, 6, "cnn", 33), id="tiny-N33"),
    pytest.param(((16, 16), 3, 11, "fc", 32), id="fc-B11-ragged"),
])
def test_dqn_form_selects_online_and_takes_the_atoms_of_the_target_rows(shape, request):
    """Double DQN: region "logits" holds the ONLINE parameters' rows over concat(state, next_state), region "logits_target" the target
    parameters' rows over the B next states (region "q_target": their means)."""
    feats, A, B, arch, N = shape
    eng, _ = _engine(feats, A, 1, B, N, 1.0, arch=arch, seed=2, double_q=True)
    tgt = torch.zeros_like(eng.params)
    eng.import_flax(_params(TARGET_SEED, feats, A, 1, arch, N), target=tgt)
    b = _Batch(eng, arch, B, A, seed=5)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch_target(b.cb, tgt) if learn else eng.loss_on_batch_target(b.cb, tgt))
        torch.cuda.synchronize()
        rows, vrows = _rows(eng, B), _rows(eng, B, "logits_target", n_rows=B)
        assert not np.array_equal(rows[B:].numpy(), vrows.numpy())  # two networks
        ref = _ref_with_rows(eng, rows, b, K=1, on0=0, value_rows=vrows, selector_rows=rows[B:])
        _bites(ref, qr.means(vrows, N).reshape(B, 1, A), 1)
        qt = eng.region("q_target")[: B * 8 * ((A + 7) // 8)].reshape(B, -1)[:, :A].double().cpu()
        _close(qt, qr.means(vrows, N), rtol=1e-6, atol=1e-6)
        check_device_step_against_rows(eng, b, ref, losses, B, 1, 0, learn, tag=f"{request.node.callspec.id} learn={learn}")


@pytest.mark.parametrize("form", ["isdqn", "dqn"])
def test_an_exact_tie_in_the_selector_rows_selects_the_first_index(form):
    """fc heads with zeroed weights: every row of a head is its bias vector, and the selector's blocks of actions 1 and 3 are the same
    N values -- their means tie exactly; the value head tells the two apart."""
    feats, A, B, N = (16, 16), 4, 9, 8
    K = 2 if form == "isdqn" else 1
    n_heads = 1 + K if form == "isdqn" else 1
    eng, params = _engine(feats, A, n_heads, B, N, 1.0, arch="fc", seed=4, double_q=True)
    head = "Dense_2"
    lin = np.linspace(-0.5, 0.5, N, dtype=np.float32)
    tie = np.stack([0.25 + lin, 1.5 + lin, -0.5 + lin, 1.5 + lin]).reshape(-1)
    val = np.stack([1.0 + lin, 2.0 + lin, 3.0 + lin, 4.0 + lin]).reshape(-1)
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
        rows, vrows, on0 = _rows(eng, B), _rows(eng, B, "logits_target", n_rows=B), 0
    torch.cuda.synchronize()
    sel = rows[B:].reshape(B, n_heads, A, N)[:, on0].numpy()
    assert (sel[:, 1] == sel[:, 3]).all() and (sel[:, 1] > sel[:, 0]).all()  # the tie is exact on the device too
    ref = _ref(eng, rows, b, K=K, on0=on0, value_rows=vrows, selector_rows=rows[B:])
    assert (ref["a_star"] == 1).all()
    _close(_cpu(eng.targets), ref["targets"].numpy())
    nt = 1.0 - b.terminal.astype(np.float64)
    # value mean 2.0 at index 1, not 4.0 at index 3
    _close(_cpu(eng.targets)[:, 0], b.reward + nt * float(eng.cfg.gamma_n) * float(val.reshape(A, N)[1].astype(np.float64).mean()), rtol=1e-6)


# ------------------------------------------------------------------ 6. acting on the means, shift_params on whole blocks
@pytest.mark.parametrize("arch", ["cnn", "fc"])
def test_forward_best_actions_and_shift(arch):
    feats = TINY if arch == "cnn" else (32, 32)
    K, A, B, N = 3, 5, 8, 33
    eng, params = _engine(feats, A, 1 + K, B, N, 1.0, arch=arch, seed=6)
    b = _Batch(eng, arch, B, A, seed=21)
    q = eng.forward(n_rows=B, **b.obs_kw(B)).double().cpu()
    torch.cuda.synchronize()
    rows = _rows(eng, B)[:B]
    ex = qr.means(rows, N)
    assert q.shape == (B, (1 + K) * A)
    bound = 16 * U * rows.reshape(B, -1, N).abs().mean(-1)  # section 2's bound of a mean
    assert ((q - ex).abs() <= bound).all(), float(((q - ex).abs() / bound).max())
    pt = onet.to_torch(params, torch.float64)
    qo = qr.means(onet.forward(pt, b.x_state, feats, arch, True), N)
    assert (q - qo).abs().max() < 1e-3 * max(1.0, float(qo.abs().max()))
    idx = torch.tensor([i % K for i in range(B)], dtype=torch.int32, device="cuda")
    acts = eng.best_actions(idx_networks=idx, **b.obs_kw(B)).cpu().numpy()
    checked = 0
    for i in range(B):
        row = ex[i].reshape(1 + K, A)[1 + i % K]
        top = torch.sort(row, descending=True).values
        if float(top[0] - top[1]) <= 1e-4:
            continue
        checked += 1
        assert acts[i] == int(row.argmax())
        one = dict(obs=b.x_state[i : i + 1].cuda()) if arch == "fc" else dict(frames=b.fr, frame_stride=b.stride,
                                                                            frame_ids=b.ids[i : i + 1, :4].contiguous())
        assert int(eng.best_action(idx_network=i % K, **one).item()) == int(row.argmax())
    assert checked == B
    # shift_params: head k <- head k + 1 on whole A * N blocks, the last head unchanged, every other tensor unchanged
    before = eng.export_flax()
    flat_before = eng.params.clone()
    eng.shift_params()
    after = eng.export_flax()
    head = _head(feats, arch)
    w = A * N
    for leaf in ("kernel", "bias"):
        x0, x1 = before[head][leaf], after[head][leaf]
        assert np.array_equal(x1, np.concatenate([x0[..., w:], x0[..., -w:]], axis=-1))
    for mod in before:
        if mod != head:
            for leaf in before[mod]:
                assert np.array_equal(before[mod][leaf], after[mod][leaf])
    assert not torch.equal(flat_before, eng.params)


def test_agents_carry_the_quantile_settings_across_a_rebuilt_engine():
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    N = 16
    a = iSDQN(0, (84, 84, 4), 4, 2, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, n_quantiles=N, huber_delta=1.0)
    assert a.network.final_feature == 3 * 4 * N
    assert a.get_model()["params"]["params"]["Dense_1"]["kernel"].shape == (16, 3 * 4 * N)
    a._make_engine(6)  # a batch of another size arrived
    assert a._engine.n_quantiles == N and int(a._engine.cfg.n_quantiles) == N and a._engine.batch_size == 6
    assert float(a._engine.cfg.huber_delta) == 1.0
    assert a.get_model()["params"]["params"]["Dense_1"]["kernel"].shape == (16, 3 * 4 * N)
    d = DQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, n_quantiles=N, huber_delta=1.0)
    assert d.network.final_feature == 4 * N and d._engine.n_quantiles == N and float(d._engine.cfg.huber_delta) == 1.0
    t = TFDQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, n_quantiles=N)
    assert t.network.final_feature == 4 * N and int(t._engine.cfg.n_quantiles) == N


# ------------------------------------------------------------------ 7. determinism and the captured replay
def test_two_learn_steps_are_bit_identical_from_identical_state():
    feats, K, A, B, N = HEADLINE, 9, 9, 32, 51
    runs = []
    for _ in range(2):
        eng, _ = _engine(feats, A, 1 + K, B, N, 1.0, seed=1)
        b = _Batch(eng, "cnn", B, A, seed=3)
        ls = [eng.learn_on_batch(b.cb).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.stack(ls), eng.priorities.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert torch.isfinite(runs[0][3]).all() and (runs[0][3] > 0).all()


class _Replica:
    """bench.Replica's training state (synthetic prefilled replay, headline widths) with quantile heads."""

    def __init__(self, seed=3, capacity=4096, B=32, K=3, A=9, prioritized=False):
        from slimdqn._engine import QNetEngine
        from slimdqn.sample_collection.replay_buffer import ReplayBuffer
        from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

        self.prioritized = prioritized
        sampler = PrioritizedSamplingDistribution(seed, capacity, device="cuda:0") if prioritized else UniformSamplingDistribution(seed, device="cuda:0")
        self.rb = ReplayBuffer(sampler, B, capacity, stack_size=4, update_horizon=1, gamma=0.99, device="cuda:0")
        pri = np.random.default_rng(seed).uniform(0.1, 2.0, capacity) if prioritized else None
        self.rb.prefill_synthetic(capacity, (84, 84), A, seed=seed, p_terminal=0.005, priorities=pri)
        self.eng = QNetEngine((84, 84, 4), A, 1 + K, HEADLINE, "cnn", True, B, gamma_n=0.99, learning_rate=6.25e-5, adam_eps=1.5e-4,
                              device="cuda:0", n_quantiles=51, huber_delta=1.0)
        self.eng.init_params(seed)
        torch.cuda.synchronize()

    def step(self):
        batch = self.rb.sample()
        cb = self.eng.make_batch(frames=batch.frames, frame_stride=batch.frame_stride, frame_ids=batch.frame_ids, action=batch.action,
                                 reward=batch.reward, terminal=batch.is_terminal)
        self.eng.learn_on_batch(cb)
        if self.prioritized:
            self.rb.update_device(batch, self.eng.priorities)


@pytest.mark.parametrize("prioritized", [False, True])
def test_graph_replay_equals_eager_steps(prioritized):
    from slimdqn._graph import GraphedUpdate

    S, n_replays = 4, 2
    eager, graphed = _Replica(prioritized=prioritized), _Replica(prioritized=prioritized)
    assert torch.equal(eager.eng.params, graphed.eng.params)
    g = GraphedUpdate(graphed.rb, graphed.eng, prioritized, S)
    for _ in range(S * n_replays):
        eager.step()
    for _ in range(n_replays):
        g.run()
    torch.cuda.synchronize()
    for name in ("params", "adam_m", "adam_v", "adam_count", "losses_accum"):
        a, b = getattr(eager.eng, name), getattr(graphed.eng, name)
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} elements differ between eager and graph replay"
    assert torch.isfinite(eager.eng.losses_accum).all() and (eager.eng.losses_accum > 0).all()


# ------------------------------------------------------------------ 8. the entry points with -qr
ARGV = ["-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "200", "-bs", "8", "-n", "1", "-horizon", "50", "-at", "cnn", "-ne", "2",
        "-ntspe", "60", "-utd", "4", "-nis", "20", "-ed", "100", "-ln", "-tuf", "16", "-env", "synthetic"]


def test_isdqn_entry_point_with_quantile_heads(tmp_path):
    import pickle

    from experiments.atari.isdqn import run

    gathered = run(["-en", "qr_Synthetic"] + ARGV + ["-nbi", "2", "-qr", "-nq", "16", "-hd", "1"], root=str(tmp_path))
    assert len(gathered) == 2
    out = tmp_path / "atari" / "exp_output" / "qr_Synthetic"
    # (the engine group's flags, -qr and -nq among them, stay out of parameters.json like -hl and -hd)
    stored = json.load(open(out / "parameters.json"))
    assert stored["isdqn"]["n_bellman_iterations"] == 2 and not any("quantile" in k for k in list(stored["isdqn"]) + list(stored["shared_parameters"]))
    model = pickle.load(open(out / "isdqn" / "models" / "1", "rb"))["params"]
    assert model["params"]["Dense_1"]["kernel"].shape == (16, 3 * 9 * 16)
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())


def test_dqn_entry_point_with_quantile_heads_and_double_q(tmp_path):
    import pickle

    from experiments.atari.dqn import run

    gathered = run(["-en", "qrdq_Synthetic"] + ARGV + ["-qr", "-dq", "-hd", "1"], root=str(tmp_path))
    assert len(gathered) == 2
    model = pickle.load(open(tmp_path / "atari" / "exp_output" / "qrdq_Synthetic" / "dqn" / "models" / "1", "rb"))["params"]
    assert model["params"]["Dense_1"]["kernel"].shape == (16, 9 * 32)
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())


@pytest.mark.parametrize("extra", [["-mq"], ["-hl"]])
def test_entry_point_refuses_qr_with_mq_or_hl_before_any_output_directory_exists(tmp_path, extra):
    from experiments.atari.isdqn import run

    with pytest.raises(ValueError) as e:
        run(["-en", "bad_Synthetic"] + ARGV + ["-nbi", "2", "-qr"] + extra, root=str(tmp_path))
    assert "n_quantiles" in str(e.value)
    assert not (tmp_path / "atari").exists()
