"""Dueling value / advantage heads on the GPU (include/isdqn_hip.h, isdqn_net_config::dueling; csrc/dueling.h) against the float64
restatement of tests/helpers/dueling.py, which is written from the header's definition:

 1. off is off: dueling=False is bit-identical to an engine built without the keyword (scalar heads with the head chain, histogram and
    quantile heads), workspace bytes and region offsets included;
 2. the combine and the backward kernel on the device's own rows ("head_raw" -> "q" / "logits", "dout" / "dbh" -> "dout_raw" /
    "dbh_raw"), with derived bounds;
 3. the whole path against the float64 model -- oracle.network's forward with R outputs and a masked head kernel, the helper's combine,
    then the float64 loss helpers of tests/helpers/ -- for the scalar, Huber, -hl, -hl -cat and -qr losses in both precisions:
    loss_on_batch, learn_on_batch with one Adam step, grad_on_batch for every leaf;
 4. the structural zeros stay bit-zero, eager and in the captured multi-step graph;
 5. one composition each: double_q in both forms (exact ties included), Munchausen, the *_target forms, a single head without
    target (TF-DQN), loss_weights;
 6. acting on the combined values, shift_params on whole (A + 1) * w blocks;
 7. ReDo with a dormant last-hidden neuron in each stream;
 8. run-to-run bit identity, captured replay equals eager;
 9. every refusal returns its code (the C ABI on the GPU machine's own build; the CPU suite runs the same table);
10. the five entry points with -duel.

Bounds of section 2 (u = 2^-24; any summation order of n float32 terms errs by at most (n - 1) u sum |terms|).  Combine: the A-term
sum s (at most (A - 1) u sum_a |adv_a| <= (A - 1) u A max_a |adv_a|, which the division by A brings to (A - 1) u max_a |adv_a|), the
division (u max |adv|), the subtraction (u 2 max |adv|) and the addition (u (|V| + 2 max |adv|)) stay below
(A + 2) u (|V| + 2 max_a |adv_a|).  Backward: the value row is the A-term sum, (A - 1) u sum_a |d_a|; an advantage row adds the division
and the subtraction: (A + 1) u (|d_a| + sum_a |d_a| / A).  Where dout has one non-zero per (row, head, j) -- every learn step: one taken
action per transition -- the sum adds zeros and the value gradient equals that entry bit for bit.  The backward bound alone carries a
floor of 2^-126 per operation on rows that are not exactly zero: dout of a histogram head is softmax - p, whose tails run through the
denormal range, where an operation errs by an absolute 2^-149 (or 2^-126 where the hardware flushes) that no multiple of u |d| covers;
the head outputs the combine reads are never that small, and its bound is the one above as it stands.

Every network of sections 3 and 5 gets separated action values through the ADVANTAGE biases, as tests/test_gpu_quantile.py's spread_bias
does for plain heads: advantage (h, a) += SPREAD x pi_h(a) (0.5 for quantile heads, whose action values are means of w outputs; 1.5 for
scalar heads, whose single advantage output moves by about 1 between observations; + DOMINANT on the preferred action in single-pass
bf16), pi_h a seeded permutation; histogram heads get the log-Gaussian bump of tests/test_gpu_categorical.py around STEP x (pi_h(a) -
(A - 1) / 2) on the advantage rows and the bump around 0 on the value row (the mean over the actions that the combine subtracts is a
parabola in z; the value row's bump puts it back, so that every action's logits stay a Gaussian around its own centre).
scripts/dueling_seeds.py checks on the CPU that the committed cases of section 3 leave out no pair."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.gpu_helpers import adam64, make_frame_batch, perturbed_params
from tests.helpers import categorical as c51
from tests.helpers import double_q as dq
from tests.helpers import dueling as du
from tests.helpers import hl_gauss as hl
from tests.helpers import munchausen as mq
from tests.helpers import per_weights as pw
from tests.helpers import quantile as qr

pytestmark = pytest.mark.gpu

U = 2.0**-24
TOL = {"bf16x3": dict(q=1e-3, loss=1e-3, grad=3e-3), "bf16": dict(q=8e-2, loss=5e-2, grad=2.5e-1)}  # tests/test_gpu_quantile.py's table
RTOL, ATOL = 1e-5, 1e-7  # the project's bound of a float32 kernel against float64 on the same inputs
FC_OBS = (8,)
HEADLINE, TINY, FC = (32, 64, 64, 512), (7, 9, 11, 14), (20, 14)
SPREAD, STEP, BUMP_SIGMA = {"scalar": 1.5, "huber": 1.5, "qr": 0.5}, 1.5, 1.0
DOMINANT = {"scalar": {"bf16x3": 0.0, "bf16": 40.0}, "hist": {"bf16x3": 0.0, "bf16": 12.0}}
SUPPORT = {"bf16x3": (-10.0, 10.0), "bf16": (-20.0, 20.0)}
G = float(np.float32(0.99))


def _kind(kind, w, prec="bf16x3"):
    """(engine keywords, components per (head, action)) of a loss kind"""
    vmin, vmax = SUPPORT[prec]
    if kind == "scalar":
        return dict(), 1
    if kind == "huber":
        return dict(huber_delta=1.0), 1
    if kind == "hl":
        return dict(n_bins=w, min_value=vmin, max_value=vmax, sigma=0.75 * (vmax - vmin) / w), w
    if kind == "c51":
        return dict(n_bins=w, min_value=vmin, max_value=vmax, sigma=0.0, categorical=True), w
    assert kind == "qr"
    return dict(n_quantiles=w, huber_delta=1.0), w


def _obs(arch):
    return FC_OBS if arch == "fc" else (84, 84, 4)


def _head(feats, arch):
    return f"Dense_{len(feats) - (0 if arch == 'fc' else 3)}"


def _params(seed, feats, A, H, arch, kind, w, ln=True, prec="bf16x3"):
    """Perturbed parameters with R outputs, the structural zeros written and the action values separated through the advantage biases."""
    hist = kind in ("hl", "c51")
    w = w if kind in ("hl", "c51", "qr") else 1
    p = perturbed_params(seed, _obs(arch), feats, arch, du.raw_width(H, A, w), ln)
    head = _head(feats, arch)
    p = du.mask_head(p, head, feats[-1], H, A, w)
    rng = np.random.default_rng(seed + 7)
    bias = p[head]["bias"].reshape(H, A + 1, w)
    dom = DOMINANT["hist" if hist else "scalar"][prec]
    vmin, vmax = SUPPORT[prec]
    for h in range(H):
        pi = rng.permutation(A)
        for a in range(A):
            if hist:
                mu = STEP * (pi[a] - (A - 1) / 2) + dom * (pi[a] == A - 1)
                bias[h, a] += c51.gauss_bump(w, vmin, vmax, mu, BUMP_SIGMA).astype(np.float32)
            else:
                bias[h, a] += np.float32(SPREAD[kind] * pi[a] + dom * (pi[a] == A - 1))
        if hist:
            bias[h, A] += c51.gauss_bump(w, vmin, vmax, 0.0, BUMP_SIGMA).astype(np.float32)
        elif kind == "qr":
            bias[h, A] += np.linspace(-0.5, 0.5, w, dtype=np.float32)  # distinct quantile values for every action
    return p


def _engine(feats, A, H, B, kind="scalar", w=1, arch="cnn", ln=True, prec="bf16x3", seed=0, lr=1e-3, dueling=True, **kw):
    from slimdqn._engine import QNetEngine

    ekw, w = _kind(kind, w, prec)
    params = _params(seed, feats, A, H, arch, kind, w, ln, prec)
    eng = QNetEngine(_obs(arch), A, H, feats, arch, ln, B, gamma_n=0.99, learning_rate=lr, adam_eps=1.5e-4, precision=prec, dueling=dueling,
                     **{**ekw, **kw})
    eng.import_flax(params)
    return eng, params


class _Batch:
    """One batch in both forms: the engine's C batch (``eng`` given) and the float64 network input [states; next states]."""

    def __init__(self, eng, arch, B, A, seed, weights=False, reward_shift=0.0):
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
            self.reward = (rng.normal(size=B) + reward_shift).astype(np.float32)
            if eng is not None:
                self.cb = eng.make_batch(state=d(s), next_state=d(ns), action=d(self.action), reward=d(self.reward), terminal=d(self.terminal),
                                         loss_weights=None if self.weights is None else d(self.weights))
        else:
            frames, ids, action, _, terminal, ref = make_frame_batch(B, A, seed=seed, h=obs[0], w=obs[1], stack=obs[2])
            self.action, self.terminal = action, terminal
            self.reward = (rng.normal(size=B) + reward_shift).astype(np.float32)
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


def _w(eng):
    return max(eng.n_bins, eng.n_quantiles, 1)


def _region_rows(eng, name, n_rows, width):
    """float64 copy of the first `width` columns of the [n_rows][width padded to 8] rows of a workspace region"""
    pitch = (width + 7) // 8 * 8
    return eng.region(name)[: n_rows * pitch].reshape(n_rows, pitch)[:, :width].cpu().double()  # (converted on the host: denormals survive)


def _raw_rows(eng, n_rows, region="head_raw"):
    return _region_rows(eng, region, n_rows, du.raw_width(eng.n_heads, eng.n_actions, _w(eng)))


def _out_rows(eng, n_rows, region=None):
    """the combined rows every consumer reads: "q" (scalar heads) or "logits" """
    w = _w(eng)
    return _region_rows(eng, region or ("q" if w == 1 else "logits"), n_rows, eng.n_heads * eng.n_actions * w)


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _close(a, b, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _structural(eng):
    """flat indices of the structural zeros in the engine's parameter buffer"""
    info = eng.head_kernel_info()
    return torch.from_numpy(int(info.offset) + du.structural_indices(eng.features[-1], int(info.dims[1]), eng.n_heads, eng.n_actions, _w(eng))).cuda()


def _mirror_is_zero(eng, idx):
    """both bf16 halves of the S8 weight mirror (region "wsplit": every 8 values are 8 hi halves, then 8 lo halves) at flat indices idx"""
    u16 = eng.region("wsplit")[: eng.n_param_floats].view(torch.int16)
    base = (idx // 8) * 16 + idx % 8
    return bool((u16[base] == 0).all() and (u16[base + 8] == 0).all())


def assert_structural_zeros(eng, grad=None, tag=""):
    idx = _structural(eng)
    assert idx.numel() == du.raw_width(eng.n_heads, eng.n_actions, _w(eng)) * (eng.features[-1] // 2)
    for name, t in (("params", eng.params), ("adam_m", eng.adam_m), ("adam_v", eng.adam_v)) + ((("grad_out", grad),) if grad is not None else ()):
        bits = t[idx].view(torch.int32)
        assert bool((bits == 0).all()), f"{tag} {name}: {int((bits != 0).sum())} structural entries are not +0.0f"
    assert _mirror_is_zero(eng, idx), f"{tag} wsplit"


# ------------------------------------------------------------------ the float64 losses on combined rows
def scalar_model(rows, b, K, on0, tg0, A, huber=0.0, value_rows=None, weights=None):
    """Scalar heads, max form, on tests/helpers/per_weights.py's weighted TD loss."""
    rows = torch.as_tensor(rows, dtype=torch.float64)
    B = rows.shape[0] // 2
    act = torch.as_tensor(np.asarray(b.action), dtype=torch.long)
    r = torch.as_tensor(np.asarray(b.reward, np.float64))
    nt = 1.0 - torch.as_tensor(np.asarray(b.terminal, np.float64))
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    val = (rows[B:] if value_rows is None else torch.as_tensor(value_rows, dtype=torch.float64)).detach().reshape(B, -1, A)[:, tg0 : tg0 + K]
    top = torch.sort(val, dim=-1, descending=True).values
    gap = top[..., 0] - top[..., 1] if A > 1 else torch.full(top.shape[:-1], float("inf"), dtype=torch.float64)
    tg = r[:, None] + nt[:, None] * G * val.max(-1).values
    bi, ki = torch.arange(B)[:, None], torch.arange(on0, on0 + K)[None, :]
    on = rows[:B].reshape(B, -1, A)
    q = on[bi, ki, act[:, None]]
    d = q - tg
    l_t = torch.where(d.abs() <= huber, 0.5 * d * d, huber * (d.abs() - 0.5 * huber)) if huber > 0 else d * d
    ref = pw.weighted_td(q.detach().numpy(), tg.numpy(), w, huber)
    dense = torch.zeros(B, on.shape[1], A, dtype=torch.float64)
    dense[bi, ki, act[:, None]] = torch.from_numpy(ref["dq"])
    return dict(q=q, targets=tg, losses=(torch.from_numpy(w)[:, None] * l_t).sum(0) / B, priorities=torch.from_numpy(np.sqrt(ref["l"].mean(1) + 1e-10)),
                d=dense.reshape(B, -1), gap=gap, qmax=float(val.abs().max()))


def loss_model(kind, w, prec, rows, b, K, on0, tg0, A, **kw):
    """dict(q, targets [B, K], losses [K] (torch, differentiable through rows), priorities [B], d = dL/d(combined rows of the states),
    gap [B, K] of the deciding head's action values, qmax) of a loss kind on combined rows [2B][H * A * w]."""
    vmin, vmax = SUPPORT[prec]
    if kind in ("scalar", "huber"):
        return scalar_model(rows, b, K, on0, tg0, A, huber=1.0 if kind == "huber" else 0.0, **kw)
    if kind == "qr":
        r = qr.qr_loss(rows, b.action, b.reward, b.terminal, G, K, on0, tg0, A, w, 1.0, **kw)
        return dict(r, d=r["dtheta"])
    if kind == "c51":
        r = c51.c51_loss(rows, b.action, b.reward, b.terminal, G, K, on0, tg0, A, w, vmin, vmax, **kw)
        return dict(r, d=r["dlogits"])
    assert kind == "hl" and not kw
    r = hl.hl_loss(rows, b.action, b.reward, b.terminal, G, K, on0, tg0, A, w, vmin, vmax, 0.75 * (vmax - vmin) / w)
    ex = hl.expectations(torch.as_tensor(rows, dtype=torch.float64)[rows.shape[0] // 2 :].detach(), w, vmin, vmax).reshape(rows.shape[0] // 2, -1, A)[:, tg0 : tg0 + K]
    top = torch.sort(ex, dim=-1, descending=True).values
    return dict(r, d=r["dlogits"], gap=top[..., 0] - top[..., 1], qmax=float(ex.abs().max()))


def model_rows(params, x, feats, arch, ln, H, A, w, requires_grad=False):
    """The float64 network: oracle forward with R outputs and the masked head kernel, then the helper's combine."""
    pt = onet.to_torch(params, torch.float64, requires_grad=requires_grad)
    masked = du.masked_torch(pt, _head(feats, arch), feats[-1], H, A, w)
    return pt, du.combine(onet.forward(masked, x, feats, arch, ln), H, A, w)


# ------------------------------------------------------------------ 1. off is off
REGIONS = ["q", "logits", "dout", "da", "slab", "q_values", "targets", "dbh", "adam_consts", "loss_partials", "wsplit", "act/Conv_0", "z/Conv_1",
           "dz/Conv_2", "act/Dense_0", "red/Dense_0", "part/Dense_0", "gw/Conv_0", "gw/Dense_0", "gw/Dense_1"]


@pytest.mark.parametrize("hkw", [dict(), dict(n_bins=51, min_value=-10.0, max_value=10.0, sigma=0.3), dict(n_quantiles=33, huber_delta=1.0)],
                         ids=["scalar-head-chain", "n_bins", "n_quantiles"])
def test_dueling_false_is_bit_identical_to_an_engine_built_without_the_keyword(hkw):
    from slimdqn._engine import QNetEngine

    feats, K, A, B = TINY, 3, 5, 6
    w = max(hkw.get("n_bins", 0), hkw.get("n_quantiles", 0), 1)
    outs, plans = [], []
    for kw in ({}, dict(dueling=False)):
        params = perturbed_params(3, (84, 84, 4), feats, "cnn", (1 + K) * A * w, True)
        eng = QNetEngine((84, 84, 4), A, 1 + K, feats, "cnn", True, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, **hkw, **kw)
        eng.import_flax(params)
        assert int(eng.cfg.dueling) == 0 and eng.dueling is False
        b = _Batch(eng, "cnn", B, A, seed=5)
        q = eng.forward(n_rows=B, **b.obs_kw(B)).clone()
        got = [q]
        for _ in range(3):
            losses = eng.learn_on_batch(b.cb)
            got += [losses.clone(), eng.priorities.clone()]
        torch.cuda.synchronize()
        outs.append([_cpu(x) for x in got + [eng.params, eng.adam_m, eng.adam_v, eng.q_values, eng.targets]])
        table = {}
        for name in REGIONS + ["head_raw", "dout_raw", "dbh_raw"]:
            off, size = ctypes.c_int64(), ctypes.c_int64()
            rc = eng.lib.isdqn_net_workspace_region(ctypes.byref(eng.cfg), name.encode(), ctypes.byref(off), ctypes.byref(size))
            table[name] = (off.value, size.value) if rc == 0 else None
        plans.append((eng.workspace_bytes, eng.n_param_floats, table))
    assert plans[0] == plans[1] and plans[0][2]["head_raw"] is None and plans[0][2]["q"] is not None
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 2. combine and backward on the device's own rows
OWN_ROWS = [
    pytest.param(("scalar", 1, 3, 3, 3, "cnn", TINY, "bf16x3"), id="scalar-A3-B3"),
    pytest.param(("scalar", 1, 0, 1, 3, "fc", FC, "bf16x3"), id="scalar-one-head-A1-fc"),
    pytest.param(("huber", 1, 3, 18, 32, "fc", FC, "bf16"), id="huber-A18-B32-fc-bf16"),
    pytest.param(("scalar", 1, 3, 18, 64, "cnn", HEADLINE, "bf16x3"), id="scalar-headline-A18-B64"),
    pytest.param(("qr", 2, 3, 3, 3, "cnn", TINY, "bf16x3"), id="qr-w2"),
    pytest.param(("hl", 51, 3, 3, 32, "fc", FC, "bf16x3"), id="hl-w51-B32-fc"),
    pytest.param(("c51", 51, 0, 18, 3, "cnn", TINY, "bf16"), id="c51-w51-one-head-A18-bf16"),
    pytest.param(("qr", 200, 3, 3, 3, "cnn", TINY, "bf16x3"), id="qr-w200"),
]


@pytest.mark.parametrize("shape", OWN_ROWS)
def test_combine_and_backward_match_float64_on_the_device_rows(shape, request):
    kind, w, K, A, B, arch, feats, prec = shape
    H = 1 + K
    eng, _ = _engine(feats, A, H, B, kind, w, arch=arch, prec=prec)
    w = _w(eng)
    b = _Batch(eng, arch, B, A, seed=5, weights=arch == "fc")
    eng.learn_on_batch(b.cb)
    torch.cuda.synchronize()
    tag = request.node.callspec.id
    # forward: "head_raw" -> "q" / "logits", all 2B rows
    raw = _raw_rows(eng, 2 * B).numpy()
    out = _out_rows(eng, 2 * B).numpy()
    want = du.combine(raw, H, A, w).numpy()
    bound = du.combine_bound(raw, H, A, w, U)
    err = np.abs(out - want)
    print(f"{tag}: combine err/bound {float((err / bound).max()):.3f} (largest |out| {float(np.abs(out).max()):.3g})")
    assert np.abs(raw).max() > 0 and (err <= bound).all(), float((err / bound).max())
    if A == 1:  # the mean of one advantage is that advantage: the head is its value row
        assert np.array_equal(out, raw.reshape(2 * B, H, 2, w)[:, :, 1].reshape(2 * B, -1))
    # backward: "dout" -> "dout_raw", "dbh" -> "dbh_raw"
    n = H * A * w
    d = _region_rows(eng, "dout", B, n).numpy()
    draw = _raw_rows(eng, B, "dout_raw").numpy()
    dbh = _region_rows(eng, "dbh", 1, n).numpy()
    dbh_raw = _raw_rows(eng, 1, "dbh_raw").numpy()
    assert np.abs(d).max() > 0 and np.abs(dbh).max() > 0
    for name, got, src in (("dout_raw", draw, d), ("dbh_raw", dbh_raw, dbh)):
        e = np.abs(got - du.backward(src, H, A, w))
        bd = du.backward_bound(src, H, A, w, U)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bd > 0, e / bd, 0.0)
        print(f"{tag}: {name} err/bound {float(ratio.max()):.3f}")
        assert (e <= bd).all(), (name, float(ratio.max()))  # (a zero bound -- heads no pair regresses -- asks for exactly 0)
    # dout has one non-zero per (row, head, j), the taken action's: the value gradient is that entry, bit for bit
    x = d.reshape(B, H, A, w)
    assert ((x != 0).sum(2) <= 1).all()
    taken = x[np.arange(B), :, b.action.astype(np.int64)]  # [B, H, w]
    assert np.array_equal(draw.reshape(B, H, A + 1, w)[:, :, A], taken)
    # the padded columns are written as zeros
    for region, rows_n, width in (("dout_raw", B, du.raw_width(H, A, w)), ("q" if w == 1 else "logits", 2 * B, n)):
        pitch = (width + 7) // 8 * 8
        full = eng.region(region)[: rows_n * pitch].reshape(rows_n, pitch)
        assert bool((full[:, width:] == 0).all())


# ------------------------------------------------------------------ 3. the whole path against the float64 model
E2E = {  # kind, w, feats, K, A, B, arch, ln
    "scalar": ("scalar", 1, TINY, 3, 5, 6, "cnn", True),
    "scalar-headline-B8": ("scalar", 1, HEADLINE, 9, 9, 8, "cnn", True),
    "huber-fc": ("huber", 1, FC, 2, 4, 9, "fc", True),
    "hl": ("hl", 51, TINY, 3, 5, 6, "cnn", True),
    "c51": ("c51", 51, TINY, 3, 5, 6, "cnn", True),
    "qr": ("qr", 32, TINY, 3, 5, 6, "cnn", True),
    "qr-noln-fc": ("qr", 33, FC, 2, 3, 5, "fc", False),
}
PRECISIONS = ["bf16x3", "bf16"]
PARAM_SEED, BATCH_SEED = 2, 9


def _shift(kind, A, prec):
    """centre of the rewards: about minus what the best action's value leads a random action's by"""
    if kind in ("hl", "c51"):
        return 0.0
    return -0.5 * (SPREAD[kind] * (A - 1) + DOMINANT["scalar"][prec])


def oracle_case(name, prec):
    """Everything of a section-3 case that needs no GPU: parameters, batch, the float64 combined rows (with a graph through the online
    parameters) and the loss helper's result on them."""
    kind, w, feats, K, A, B, arch, ln = E2E[name]
    H = 1 + K
    ekw, w = _kind(kind, w, prec)
    params = _params(PARAM_SEED, feats, A, H, arch, kind, w, ln, prec)
    b = _Batch(None, arch, B, A, seed=BATCH_SEED, reward_shift=_shift(kind, A, prec))
    pt, rows = model_rows(params, torch.cat([b.x_state, b.x_next]), feats, arch, ln, H, A, w, requires_grad=True)
    rows = torch.cat([rows[:B], rows[B:].detach()])
    ref = loss_model(kind, w, prec, rows, b, K, 1, 0, A)
    return dict(params=params, batch=b, pt=pt, rows=rows, ref=ref, gap=np.asarray(ref["gap"]), scale=max(1.0, ref["qmax"]), ekw=ekw, w=w)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(E2E))
def test_whole_path_matches_the_float64_model(name, prec):
    from slimdqn._engine import QNetEngine

    kind, _, feats, K, A, B, arch, ln = E2E[name]
    H = 1 + K
    t = TOL[prec]
    c = oracle_case(name, prec)
    ref, w, lr = c["ref"], c["w"], 1e-3
    # the value is taken at an argmax: a pair is left out only when, in the float64 reference alone, the deciding head's top-two gap is
    # below 10 x the q bound x max(1, |Q|max); the committed cases leave out none (scripts/dueling_seeds.py)
    keep = c["gap"] >= 10 * t["q"] * c["scale"]
    assert keep.all(), f"{(~keep).sum()} of {keep.size} pairs left out: the committed cases leave out none"
    eng = QNetEngine(_obs(arch), A, H, feats, arch, ln, B, gamma_n=0.99, learning_rate=lr, adam_eps=1.5e-4, precision=prec, dueling=True, **c["ekw"])
    eng.import_flax(c["params"])
    b = _Batch(eng, arch, B, A, seed=BATCH_SEED, reward_shift=_shift(kind, A, prec))
    rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - np.asarray(want)).max() / max(1.0, float(np.abs(np.asarray(want)).max())))
    want_q, want_t, want_l = ref["q"].detach().numpy(), np.asarray(ref["targets"]), ref["losses"].detach().numpy()
    ref["losses"].sum().backward()
    want_g = {m: {k: v.grad.numpy() for k, v in l.items()} for m, l in c["pt"].items()}
    head = _head(feats, arch)
    assert (want_g[head]["kernel"][~du.live_mask(feats[-1], H, A, w)] == 0).all()

    def check_outputs(form, losses):
        eq, et, el = rel(_cpu(eng.q_values), want_q), rel(_cpu(eng.targets), want_t), rel(losses, want_l)
        print(f"{name} {prec} {form}: q {eq:.2e} targets {et:.2e} (bound {t['q']:.0e}) loss {el:.2e} (bound {t['loss']:.0e}); min gap "
              f"{c['gap'].min():.3g} (bound {10 * t['q'] * c['scale']:.3g})")
        assert eq < t["q"] and et < t["q"] and el < t["loss"]

    def check_grads(form, g):
        hip_g = eng.internal_to_flax_grads(g)
        for mod in want_g:
            for leaf, want in want_g[mod].items():
                e = np.linalg.norm(np.asarray(hip_g[mod][leaf], np.float64) - want) / max(np.linalg.norm(want), 1e-30)
                print(f"{name} {prec} {form} grad {mod}/{leaf}: norm-rel {e:.2e} (bound {10 * t['grad']:.0e})")
                assert e <= 10 * t["grad"], (form, mod, leaf, e)
        assert (np.asarray(hip_g[head]["kernel"])[~du.live_mask(feats[-1], H, A, w)] == 0).all()

    losses = _cpu(eng.loss_on_batch(b.cb))
    torch.cuda.synchronize()
    check_outputs("loss_on_batch", losses)
    g = torch.full_like(eng.params, float("nan"))
    losses = _cpu(eng.grad_on_batch(b.cb, g))
    torch.cuda.synchronize()
    check_outputs("grad_on_batch", losses)
    check_grads("grad_on_batch", g)
    assert_structural_zeros(eng, grad=g, tag="grad_on_batch")
    p0 = eng.params.clone()
    g2 = torch.zeros_like(eng.params)
    losses = _cpu(eng.learn_on_batch(b.cb, grad_out=g2))
    torch.cuda.synchronize()
    check_outputs("learn_on_batch", losses)
    check_grads("learn_on_batch", g2)
    # one Adam step from zero moments with the device's gradient on the raw head's leaves; the structural zeros stay zeros
    for info in eng.infos:
        if not info.name.decode().startswith(head + "/"):
            continue
        sl = slice(info.offset, info.offset + info.size)
        pn, m, v, _, _ = adam64(p0[sl].cpu().numpy(), 0.0, 0.0, g2[sl].cpu().numpy(), 1, lr, 1.5e-4)
        _close(eng.params[sl].cpu(), pn, rtol=1e-6, atol=1e-9)
        _close(eng.adam_m[sl].cpu(), m, rtol=1e-6, atol=1e-12)
        _close(eng.adam_v[sl].cpu(), v, rtol=1e-5, atol=1e-15)
    assert int(eng.adam_count.item()) == 1
    assert_structural_zeros(eng, grad=g2, tag="learn_on_batch")


# ------------------------------------------------------------------ 4. structural zeros
@pytest.mark.parametrize("shape", [
    pytest.param(("scalar", 1, 3, 5, 6, "cnn", TINY), id="scalar-F14"),
    pytest.param(("qr", 33, 2, 3, 5, "fc", FC), id="qr-w33-fc-F14"),
    pytest.param(("c51", 51, 0, 4, 3, "cnn", (7, 9, 11, 20)), id="c51-one-head-F20"),
])
def test_structural_zeros_survive_three_learn_steps_and_the_initialisers_write_them(shape):
    kind, w, K, A, B, arch, feats = shape
    eng, _ = _engine(feats, A, 1 + K, B, kind, w, arch=arch)
    live = torch.ones(eng.n_param_floats, dtype=torch.bool, device="cuda")
    live[_structural(eng)] = False
    info = eng.head_kernel_info()
    head_live = live[info.offset : info.offset + info.size].reshape(int(info.dims[0]), int(info.dims[1]))[: du.raw_width(1 + K, A, _w(eng)), : feats[-1]]
    b = _Batch(eng, arch, B, A, seed=5)
    g = torch.zeros_like(eng.params)
    for step in range(3):
        eng.learn_on_batch(b.cb, grad_out=g if step == 2 else None)
        torch.cuda.synchronize()
        assert_structural_zeros(eng, grad=g if step == 2 else None, tag=f"step {step}")
    # ... while the weights beside them learn: the live entries that receive a gradient at all (the rows of the regressed heads, on the
    # hidden units some row of the batch activates) carry second moments -- more than a fifth of the live entries in every case here
    view = lambda t: t[info.offset : info.offset + info.size].reshape(int(info.dims[0]), int(info.dims[1]))[: head_live.shape[0], : feats[-1]]
    assert bool((view(eng.adam_v)[head_live] > 0).float().mean() > 0.2)
    tgt = torch.zeros_like(eng.params)
    eng.learn_on_batch_target(b.cb, eng.params.clone()) if K == 0 else eng.learn_on_batch(b.cb)
    torch.cuda.synchronize()
    assert_structural_zeros(eng, tag="fourth step")
    # the initialisers write the zeros and draw the live entries at fan-in F / 2
    fresh = eng.fresh_params(11)
    idx = _structural(eng)
    assert bool((fresh[idx].view(torch.int32) == 0).all())
    kernel = eng.export_flax(fresh)[_head(feats, arch)]["kernel"]
    mask = du.live_mask(feats[-1], 1 + K, A, _w(eng))
    assert kernel.shape == mask.shape and (kernel[~mask] == 0).all() and (kernel[mask] != 0).mean() > 0.99
    F2, R = feats[-1] // 2, mask.shape[1]
    if arch == "cnn":  # xavier_uniform at fan-in F / 2: no live entry beyond its limit, some beyond the limit of fan-in F
        lim2, lim = np.sqrt(6.0 / (F2 + R)), np.sqrt(6.0 / (feats[-1] + R))
        assert lim < np.abs(kernel).max() <= lim2
    eng.init_params(11)
    assert torch.equal(eng.params, fresh)
    # import_flax refuses a non-zero structural zero, export_flax returns the (F, R) kernel as it is
    tree = eng.export_flax()
    assert np.array_equal(tree[_head(feats, arch)]["kernel"], kernel)
    bad = {m: {k: v.copy() for k, v in l.items()} for m, l in tree.items()}
    r, c = np.argwhere(~mask)[len(np.argwhere(~mask)) // 2]
    bad[_head(feats, arch)]["kernel"][r, c] = 1e-3
    with pytest.raises(ValueError) as e:
        eng.import_flax(bad, target=tgt)
    assert "structural zero" in str(e.value) and not bool(tgt.any())


class _Replica:
    """bench.Replica's training state (synthetic prefilled replay, headline widths) with dueling heads."""

    def __init__(self, seed=3, capacity=2048, B=32, K=3, A=9, prioritized=False, **kw):
        from slimdqn._engine import QNetEngine
        from slimdqn.sample_collection.replay_buffer import ReplayBuffer
        from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

        self.prioritized = prioritized
        sampler = PrioritizedSamplingDistribution(seed, capacity, device="cuda:0") if prioritized else UniformSamplingDistribution(seed, device="cuda:0")
        self.rb = ReplayBuffer(sampler, B, capacity, stack_size=4, update_horizon=1, gamma=0.99, device="cuda:0")
        pri = np.random.default_rng(seed).uniform(0.1, 2.0, capacity) if prioritized else None
        self.rb.prefill_synthetic(capacity, (84, 84), A, seed=seed, p_terminal=0.005, priorities=pri)
        self.eng = QNetEngine((84, 84, 4), A, 1 + K, HEADLINE, "cnn", True, B, gamma_n=0.99, learning_rate=6.25e-5, adam_eps=1.5e-4,
                              device="cuda:0", dueling=True, **kw)
        self.eng.init_params(seed)
        torch.cuda.synchronize()

    def step(self):
        batch = self.rb.sample()
        cb = self.eng.make_batch(frames=batch.frames, frame_stride=batch.frame_stride, frame_ids=batch.frame_ids, action=batch.action,
                                 reward=batch.reward, terminal=batch.is_terminal)
        self.eng.learn_on_batch(cb)
        if self.prioritized:
            self.rb.update_device(batch, self.eng.priorities)


# ------------------------------------------------------------------ 8 (and 4). captured replay equals eager, structural zeros in the graph
@pytest.mark.parametrize("kw,prioritized", [(dict(), True), (dict(n_quantiles=51, huber_delta=1.0), False)], ids=["scalar-per", "qr"])
def test_graph_replay_equals_eager_steps_and_keeps_the_structural_zeros(kw, prioritized):
    from slimdqn._graph import GraphedUpdate

    S, n_replays = 3, 1
    eager, graphed = _Replica(prioritized=prioritized, **kw), _Replica(prioritized=prioritized, **kw)
    assert torch.equal(eager.eng.params, graphed.eng.params)
    assert_structural_zeros(graphed.eng, tag="init_params")
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
    assert_structural_zeros(graphed.eng, tag="captured multi-step graph")
    assert_structural_zeros(eager.eng, tag="eager")


@pytest.mark.parametrize("kind,w", [("scalar", 1), ("hl", 51)])
def test_two_learn_steps_are_bit_identical_from_identical_state(kind, w):
    feats, K, A, B = HEADLINE, 9, 9, 32
    runs = []
    for _ in range(2):
        eng, _ = _engine(feats, A, 1 + K, B, kind, w, seed=1)
        b = _Batch(eng, "cnn", B, A, seed=3)
        ls = [eng.learn_on_batch(b.cb).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.stack(ls), eng.priorities.clone(),
                     eng.region("dout_raw").clone(), eng.region("head_raw").clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert torch.isfinite(runs[0][3]).all() and (runs[0][3] > 0).all()


# ------------------------------------------------------------------ 5. one composition each (scalar heads, on the device's own rows)
def _np(x):
    return x.detach().numpy() if torch.is_tensor(x) else np.asarray(x)


TARGET_BOUND = 3e-6  # x max(1, max |Q|): tests/test_gpu_munchausen.py's bound of a float32 target against float64 on the same rows


def _check_step(eng, b, ref, losses, learn):
    """The outputs of one loss / learn call against a float64 helper's result on the device's own combined rows: q_values are copies
    of those rows; the targets keep the float32 target bound; what lies behind them keeps the project's tolerances of a float32
    kernel against float64 (rtol 1e-5, atol 1e-7) plus that bound, as in tests/test_gpu_munchausen.py."""
    scale = max(1.0, float(_out_rows(eng, 2 * eng.batch_size).abs().max()), float(np.abs(_np(ref["targets"])).max()))
    behind = ATOL + TARGET_BOUND * scale
    assert np.array_equal(_cpu(eng.q_values).astype(np.float64), _np(ref["q"]))
    assert (np.abs(_cpu(eng.targets) - _np(ref["targets"])) <= TARGET_BOUND * scale).all()
    _close(losses, _np(ref["losses"]), atol=behind)
    if learn:
        _close(_cpu(eng.priorities), _np(ref["priorities"]), atol=behind)
        H, A, B = eng.n_heads, eng.n_actions, eng.batch_size
        dout = _region_rows(eng, "dout", B, H * A).numpy()
        _close(dout, _np(ref["d"] if "d" in ref else ref["dq"]), atol=behind)
        e = np.abs(_raw_rows(eng, B, "dout_raw").numpy() - du.backward(dout, H, A))
        assert (e <= du.backward_bound(dout, H, A, 1, U)).all()


@pytest.mark.parametrize("arch", ["cnn", "fc"])
def test_isdqn_double_q_and_loss_weights_on_the_combined_rows(arch):
    feats, K, A, B = (TINY, 3, 5, 6) if arch == "cnn" else (FC, 2, 3, 11)
    eng, _ = _engine(feats, A, 1 + K, B, arch=arch, seed=2, double_q=True)
    b = _Batch(eng, arch, B, A, seed=5, weights=True)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        rows = _out_rows(eng, 2 * B)
        ref = dq.double_q(rows, b.action, b.reward, b.terminal, G, K, 1, 0, A, weights=b.weights)
        assert float((ref["a_star"] != ref["greedy"]).mean()) >= 0.25  # the selector leaves the value head's own argmax
        _check_step(eng, b, ref, losses, learn)
        # the weights are honoured: the unweighted losses on the same rows are others
        plain = dq.double_q(rows, b.action, b.reward, b.terminal, G, K, 1, 0, A)
        assert (np.abs(plain["losses"] - ref["losses"]) > 100 * (RTOL * np.abs(ref["losses"]) + ATOL)).all()


@pytest.mark.parametrize("form", ["max", "double_q", "munchausen"])
def test_the_target_forms_read_the_combined_rows_of_the_target_parameters(form):
    """DQN: region "q" holds the online parameters' combined rows, the target parameters' go to rows [B, 2B) of it (max form), or to
    region "q_target" through "head_raw_target" (Double DQN: the B next states; Munchausen: all 2B rows)."""
    feats, A, B, arch = TINY, 5, 6, "cnn"
    kw = dict(double_q=True) if form == "double_q" else dict(munchausen_tau=0.03) if form == "munchausen" else {}
    eng, _ = _engine(feats, A, 1, B, arch=arch, seed=2, **kw)
    tgt = torch.zeros_like(eng.params)
    eng.import_flax(_params(32, feats, A, 1, arch, "scalar", 1), target=tgt)
    b = _Batch(eng, arch, B, A, seed=5)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch_target(b.cb, tgt) if learn else eng.loss_on_batch_target(b.cb, tgt))
        torch.cuda.synchronize()
        rows = _out_rows(eng, 2 * B)
        if form == "max":
            ref = scalar_model(rows, b, 1, 0, 0, A)
        else:
            n_t = B if form == "double_q" else 2 * B
            vrows, vraw = _out_rows(eng, n_t, "q_target"), _raw_rows(eng, n_t, "head_raw_target").numpy()
            assert (np.abs(vrows.numpy() - du.combine(vraw, 1, A).numpy()) <= du.combine_bound(vraw, 1, A, 1, U)).all()
            if form == "double_q":
                assert not np.array_equal(rows[B:].numpy(), vrows.numpy())  # two networks
                ref = dq.double_q(rows, b.action, b.reward, b.terminal, G, 1, 0, 0, A, value_rows=vrows)
            else:
                ref = mq.munchausen(rows, b.action, b.reward, b.terminal, G, 1, 0, 0, A, 0.03, 0.9, -1.0, value_rows=vrows)
        _check_step(eng, b, ref, losses, learn)
    assert_structural_zeros(eng, tag=form)


@pytest.mark.parametrize("form", ["isdqn", "dqn"])
def test_an_exact_tie_in_the_selector_rows_selects_the_first_index(form):
    """fc heads with a zeroed kernel: every raw row is the bias vector.  Advantages 1 and 3 of the selector are the same number, so
    their combined values tie exactly; the value head tells the two apart."""
    feats, A, B = FC, 4, 9
    K = 2 if form == "isdqn" else 1
    H = 1 + K if form == "isdqn" else 1
    eng, params = _engine(feats, A, H, B, arch="fc", seed=4, double_q=True)
    head = _head(feats, "fc")
    tie = np.array([0.25, 1.5, -0.5, 1.5, 0.75], np.float32)  # [adv_0 .. adv_3, value]
    val = np.array([1.0, 2.0, 3.0, 4.0, -0.5], np.float32)
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in params.items()}
    p[head]["kernel"][:] = 0.0
    p[head]["bias"][:] = np.concatenate([val] + [tie] * K) if form == "isdqn" else tie
    eng.import_flax(p)
    b = _Batch(eng, "fc", B, A, seed=6)
    if form == "isdqn":
        eng.loss_on_batch(b.cb)
        rows, vrows, on0 = _out_rows(eng, 2 * B), None, 1
    else:
        tp = {m: {k: v.copy() for k, v in l.items()} for m, l in p.items()}
        tp[head]["bias"][:] = val
        tgt = torch.zeros_like(eng.params)
        eng.import_flax(tp, target=tgt)
        eng.loss_on_batch_target(b.cb, tgt)
        rows, vrows, on0 = _out_rows(eng, 2 * B), _out_rows(eng, B, "q_target"), 0
    torch.cuda.synchronize()
    sel = rows[B:].reshape(B, H, A)[:, on0].numpy()
    assert (sel[:, 1] == sel[:, 3]).all() and (sel[:, 1] > sel[:, 0]).all()  # the tie is exact on the device too
    ref = dq.double_q(rows, b.action, b.reward, b.terminal, G, K, on0, 0, A, value_rows=vrows)
    assert (ref["a_star"] == 1).all()
    _close(_cpu(eng.targets), ref["targets"], atol=ATOL + TARGET_BOUND * 4.0)  # (|Q| <= 4 here)
    nt = 1.0 - b.terminal.astype(np.float64)
    combined = float(du.combine(val[None].astype(np.float64), 1, A)[0, 1])  # the value head's action 1, not its best action 3
    _close(_cpu(eng.targets)[:, 0], b.reward + nt * G * combined, atol=ATOL + TARGET_BOUND * 4.0)


def test_munchausen_on_scalar_heads_and_a_single_head_without_target():
    feats, K, A, B = TINY, 3, 5, 6
    eng, _ = _engine(feats, A, 1 + K, B, seed=2, munchausen_tau=0.03)
    b = _Batch(eng, "cnn", B, A, seed=5)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        ref = mq.munchausen(_out_rows(eng, 2 * B), b.action, b.reward, b.terminal, G, K, 1, 0, A, 0.03, 0.9, -1.0)
        assert np.abs(ref["targets"] - ref["max_targets"]).max() > 1e-3  # the option bites
        _check_step(eng, b, ref, losses, learn)
    # TF-DQN: one head regressed on its own stop-gradient target, through the same parameters
    eng, _ = _engine(feats, A, 1, B, seed=3)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        _check_step(eng, b, scalar_model(_out_rows(eng, 2 * B), b, 1, 0, 0, A), losses, learn)
    assert_structural_zeros(eng, tag="tf-dqn")


def test_grad_on_batch_with_n_pairs_and_target_params():
    feats, K, A, B = TINY, 3, 5, 6
    eng, params = _engine(feats, A, 1 + K, B, seed=2)
    tgt = torch.zeros_like(eng.params)
    eng.import_flax(_params(32, feats, A, 1 + K, "cnn", "scalar", 1), target=tgt)
    b = _Batch(eng, "cnn", B, A, seed=5)
    g = torch.full_like(eng.params, float("nan"))
    losses = _cpu(eng.grad_on_batch(b.cb, g, target_params=tgt, online_head=1, target_head=1, n_pairs=1))[:1]
    torch.cuda.synchronize()
    rows = _out_rows(eng, 2 * B)
    ref = scalar_model(rows, b, 1, 1, 1, A)
    scale = max(1.0, float(rows.abs().max()))
    _close(_cpu(eng.targets).reshape(-1)[:B], np.asarray(ref["targets"]).reshape(-1), atol=ATOL + TARGET_BOUND * scale)  # (targets [B][n_pairs])
    _close(losses, ref["losses"].numpy(), atol=ATOL + TARGET_BOUND * scale)
    assert_structural_zeros(eng, grad=g, tag="grad_on_batch n_pairs")
    # the head's bias gradient is the backward map of the reduced combined-row gradient
    bias = eng.internal_to_flax_grads(g)[_head(feats, "cnn")]["bias"]
    _close(bias, du.backward(ref["d"].numpy().sum(0), 1 + K, A), atol=ATOL + TARGET_BOUND * scale)


# ------------------------------------------------------------------ 6. acting and shift_params
@pytest.mark.parametrize("kind,w,arch", [("scalar", 1, "cnn"), ("scalar", 1, "fc"), ("qr", 33, "cnn"), ("c51", 51, "fc")])
def test_forward_best_actions_and_shift(kind, w, arch):
    feats = TINY if arch == "cnn" else FC
    K, A, B = 3, 5, 8
    H = 1 + K
    eng, params = _engine(feats, A, H, B, kind, w, arch=arch, seed=6)
    w = _w(eng)
    vmin, vmax = SUPPORT["bf16x3"]
    b = _Batch(eng, arch, B, A, seed=21)
    q = eng.forward(n_rows=B, **b.obs_kw(B)).double().cpu()
    torch.cuda.synchronize()
    assert q.shape == (B, H * A)
    raw, rows = _raw_rows(eng, B), _out_rows(eng, B)
    assert ((rows - du.combine(raw, H, A, w)).abs().numpy() <= du.combine_bound(raw.numpy(), H, A, w, U)).all()  # isdqn_net_forward's combine
    value_of = (lambda r: r) if w == 1 else (lambda r: qr.means(r, w)) if kind == "qr" else (lambda r: hl.expectations(r, w, vmin, vmax))
    ex = value_of(rows)  # what forward returns: the combined rows themselves, their means or their expectations
    if w == 1:
        assert torch.equal(q, ex)
    else:
        _close(q, ex, rtol=RTOL, atol=16 * U * float(rows.abs().max()))
    _, orows = model_rows(params, b.x_state, feats, arch, True, H, A, w)
    qo = value_of(orows.detach())
    assert (q - qo).abs().max() < 1e-3 * max(1.0, float(qo.abs().max()))
    idx = torch.tensor([i % K for i in range(B)], dtype=torch.int32, device="cuda")
    acts = eng.best_actions(idx_networks=idx, **b.obs_kw(B)).cpu().numpy()
    adv = raw.reshape(B, H, A + 1, w)[:, :, :A]
    for i in range(B):
        row = ex[i].reshape(H, A)[1 + i % K]
        top = torch.sort(row, descending=True).values
        assert float(top[0] - top[1]) > 1e-4  # separated through the advantage biases
        assert acts[i] == int(row.argmax())
        if w == 1:  # scalar heads: V and the mean are common to the actions, the greedy action is the argmax of the advantages
            assert acts[i] == int(adv[i, 1 + i % K, :, 0].argmax())
        one = dict(obs=b.x_state[i : i + 1].cuda()) if arch == "fc" else dict(frames=b.fr, frame_stride=b.stride,
                                                                            frame_ids=b.ids[i : i + 1, :4].contiguous())
        assert int(eng.best_action(idx_network=i % K, **one).item()) == int(row.argmax())
    # shift_params: head k <- head k + 1 on whole (A + 1) * w blocks (the value rows move with them), bitwise; the last head and every
    # other tensor unchanged
    before = eng.export_flax()
    eng.shift_params()
    after = eng.export_flax()
    head = _head(feats, arch)
    blk = (A + 1) * w
    for leaf in ("kernel", "bias"):
        x0, x1 = before[head][leaf], after[head][leaf]
        assert np.array_equal(x1, np.concatenate([x0[..., blk:], x0[..., -blk:]], axis=-1)) and not np.array_equal(x0, x1)
    for mod in before:
        if mod != head:
            for leaf in before[mod]:
                assert np.array_equal(before[mod][leaf], after[mod][leaf])
    assert bool((eng.params[_structural(eng)].view(torch.int32) == 0).all())


# ------------------------------------------------------------------ 7. ReDo with dueling
def test_redo_recycles_a_dormant_neuron_of_each_stream():
    feats, K, A, B = FC, 2, 3, 8
    H, F = 1 + K, FC[-1]
    eng, params = _engine(feats, A, H, B, "qr", 4, arch="fc", ln=False, seed=3)
    w = _w(eng)
    dormant = [2, F // 2 + 2]  # one hidden unit of the value stream, one of the advantage stream
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in params.items()}
    for c in dormant:
        p["Dense_1"]["kernel"][:, c] = 0.0
        p["Dense_1"]["bias"][c] = -1.0  # relu(-1) = 0 on every row
    eng.import_flax(p)
    b = _Batch(eng, "fc", B, A, seed=5)
    eng.learn_on_batch(b.cb)  # moments everywhere
    fresh = eng.fresh_params(17)
    _, mask, n_recycled = eng.redo(obs=b.x_state.cuda(), n_rows=B, tau=0.0, fresh=fresh)
    torch.cuda.synchronize()
    m1 = mask[1].cpu().numpy()
    assert m1[dormant].all() and int(n_recycled[1].item()) == int(m1.sum()) < F
    tree, ftree = eng.export_flax(), eng.export_flax(fresh)
    kernel = tree["Dense_2"]["kernel"]  # (F, R)
    assert kernel.shape == (F, du.raw_width(H, A, w))
    live = du.live_mask(F, H, A, w)
    for c in np.flatnonzero(m1):
        assert (kernel[c] == 0).all()  # the outgoing column is zero in every raw row, value and advantage rows alike
        assert np.array_equal(tree["Dense_1"]["kernel"][:, c], ftree["Dense_1"]["kernel"][:, c])  # incoming: the fresh draw
    keep = np.flatnonzero(m1 == 0)
    assert (kernel[keep][live[keep]] != 0).all() and (kernel[~live] == 0).all()
    assert_structural_zeros(eng, tag="redo")
    mom = eng.export_flax(eng.adam_v)["Dense_2"]["kernel"]
    assert (mom[np.flatnonzero(m1)] == 0).all() and (mom[keep][live[keep]] > 0).any()
    eng.learn_on_batch(b.cb)
    torch.cuda.synchronize()
    assert_structural_zeros(eng, tag="learn behind redo")


# ------------------------------------------------------------------ 9. refusals
def test_every_refusal_returns_its_code_and_the_engine_says_it_first():
    from slimdqn import _engine, _hip
    from slimdqn._engine import QNetEngine

    mk = lambda **kw: QNetEngine(kw.pop("obs", (84, 84, 4)), kw.pop("A", 4), kw.pop("H", 3), kw.pop("feats", [8, 8, 8, 16]), kw.pop("arch", "cnn"), True, 4,
                                 dueling=True, **kw)
    for kw, msg in ((dict(feats=[8, 8, 8, 15]), _engine.DUELING_ODD_WIDTH_REFUSED), (dict(feats=[8, 8, 8]), _engine.DUELING_NEEDS_HIDDEN_DENSE),
                    (dict(batch_norm=True), _engine.DUELING_BATCH_NORM_REFUSED), (dict(arch="impala"), _engine.DUELING_IMPALA_REFUSED)):
        with pytest.raises(ValueError) as e:
            mk(**kw)
        assert str(e.value) == msg
    for kw in (dict(n_bins=51, min_value=-10.0, max_value=10.0, sigma=0.3, H=10, A=10), dict(H=66, A=2)):
        with pytest.raises(Exception) as e:  # the library's own refusal, through _hip.check
            mk(**kw)
        assert "dueling" in str(e.value)
    # the C ABI's codes, for these two and for what the python layer says first
    eng = mk()
    lib = eng.lib
    b = ctypes.c_int64()
    cfg = _hip.NetConfig.from_buffer_copy(eng.cfg)
    cfg.n_heads, cfg.n_actions = 66, 2  # 65 regressed heads
    assert lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)) == _hip.ERR_UNSUPPORTED
    cfg = _hip.NetConfig.from_buffer_copy(eng.cfg)
    cfg.n_heads, cfg.n_actions, cfg.n_bins, cfg.hl_min, cfg.hl_max, cfg.hl_sigma = 10, 10, 51, -10.0, 10.0, 0.3  # R = 5610 > 5456 >= 5100 logits
    assert lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)) == _hip.ERR_UNSUPPORTED
    cfg.dueling = 0
    assert lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)) == _hip.OK  # (the same heads without the option fit)
    for field, value, code in (("dueling", 2, _hip.ERR_ARG), ("batch_norm", 1, _hip.ERR_UNSUPPORTED), ("arch", _hip.ARCH_IMPALA, _hip.ERR_UNSUPPORTED),
                               ("n_features", 3, _hip.ERR_ARG)):
        cfg = _hip.NetConfig.from_buffer_copy(eng.cfg)
        setattr(cfg, field, value)
        assert lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)) == code, field
    cfg = _hip.NetConfig.from_buffer_copy(eng.cfg)
    cfg.features[3] = 15
    assert lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)) == _hip.ERR_ARG


# ------------------------------------------------------------------ 10. the entry points with -duel
ARGV = ["-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "200", "-bs", "8", "-n", "1", "-horizon", "50", "-at", "cnn", "-ne", "1",
        "-ntspe", "48", "-utd", "4", "-nis", "20", "-ed", "100", "-ln", "-tuf", "16", "-env", "synthetic", "-duel"]


@pytest.mark.parametrize("algo,extra,H,w", [("isdqn", ["-nbi", "2", "-dq"], 3, 1), ("dqn", ["-qr", "-nq", "8", "-hd", "1"], 1, 8),
                                            ("tfdqn", ["-hl", "-cat", "-nb", "11", "-minn", "-10", "-maxn", "10"], 1, 11),
                                            ("analysisdqn", ["-nbi", "2"], 3, 1), ("analysistfdqn", [], 1, 1)])
def test_entry_point_with_dueling_heads(tmp_path, algo, extra, H, w):
    import importlib
    import pickle

    run = importlib.import_module(f"experiments.atari.{algo}").run
    run(["-en", "duel_Synthetic"] + ARGV + extra, root=str(tmp_path))
    out = tmp_path / "atari" / "exp_output" / "duel_Synthetic"
    stored = json.load(open(out / "parameters.json"))
    assert not any("dueling" in k for k in list(stored[algo]) + list(stored["shared_parameters"]))
    model = pickle.load(open(out / algo / "models" / "1", "rb"))["params"]
    kernel = model["params"]["Dense_1"]["kernel"]
    assert kernel.shape == (16, H * 10 * w)  # the synthetic environment has 9 actions: A + 1 = 10 rows per head
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())
    mask = du.live_mask(16, H, 9, w)
    assert (kernel[~mask] == 0).all() and (kernel[mask] != 0).any()
