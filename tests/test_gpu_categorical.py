"""The C51 categorical projection loss on the GPU (include/isdqn_hip.h, isdqn_net_config::categorical; csrc/categorical.h) against the
float64 restatement of tests/helpers/categorical.py, which is written from the header's definition:

1. the loss kernel on the device's own logit rows (region "logits"), with derived bounds;
2. the whole path against the float64 oracle forward (loss_on_batch);
3. gradients of every leaf and one Adam step;
4. Double Q-learning: iS-DQN, the DQN *_target form, the single head of TF-DQN, the gradient-only pass of an analysis agent;
5. run-to-run bit identity, the captured multi-step replay, acting and shift_params against an n_bins-only engine, off is off, the
   Atari entry point with -hl -cat.

Argmax rule.  a* is discontinuous, and a constant added to an action's logits does not move its expectation; so every network here gets
robust gaps through the SHAPE of the head bias: block (h, a) += -(z_j - mu_{h,a})^2 / (2 * 1.0^2), mu_{h,a} = 1.5 * (pi_h(a) - (A - 1) / 2)
for a seeded permutation pi_h per head (selector and value heads prefer different actions) -- a discretised Gaussian around mu_{h,a}.
Single-pass bf16 (q bound 8e-2): the rule of section 2 leaves out every pair whose gap is below 0.8 x max(1, |Q|max); there the
preferred action (pi_h(a) = A - 1) gets DOMINANT on top of its mu, on a support wide enough to hold it.

Bounds of section 1 (u = 2^-24), set with the option's definition (docs/NOTEBOOK.md, "C51 categorical projection loss"):
    |delta b_j| <= 6u (|r| + g |z_j| + |hl_min| + eta) / eta
    |delta m_i| <= 2 sum_j p_j |delta b_j| + (nb + 8) u m_i
max(0, 1 - |b - i|) is 1-Lipschitz in b, and p_j is a float32 softmax ((nb + 8) u).  From them:
    dout_i : (w_b / B) (|delta m_i| + RTOL softmax_i + ATOL)       -- the softmax term at the project's RTOL / ATOL
    l_bk   : sum_i |delta m_i| |l_i| + (nb + 8) u sum_i m_i |l_i| + RTOL |logsumexp| + ATOL   -- the second term: the float32 dot product
    losses : the weighted mean of the l_bk bounds + (B + 8) u mean_b w_b |l_bk|
    q      : 2 (nb + 8) u sum_j softmax_j |z_j|     (numerator and denominator of the expectation)
    targets: g x the q bound of the value row + 2u (|r| + g |Q|)
    priorities: sqrt(mean_k (q bound + target bound)^2) + 8u priority     (a norm is 1-Lipschitz)
Every output outside the taken action's blocks has a zero bound: it must be exactly 0.  The test asserts ratio < 1 and prints the
largest."""
import json

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.gpu_helpers import adam64, make_frame_batch, perturbed_params
from tests.helpers import categorical as c51

pytestmark = pytest.mark.gpu

U = 2.0**-24
TOL = {"bf16x3": dict(q=1e-3, loss=1e-3, grad=3e-3), "bf16": dict(q=8e-2, loss=5e-2, grad=2.5e-1)}  # tests/test_gpu_hl_gauss.py's table
RTOL, ATOL = 1e-5, 1e-7  # the project's bound of a float32 kernel against float64 on the same inputs
FC_OBS = (8,)
HEADLINE, TINY = (32, 64, 64, 512), (7, 9, 11, 13)
NB, VMIN, VMAX = 51, -10.0, 10.0
STEP, BUMP_SIGMA = 1.5, 1.0
# single-pass bf16: gap ~ DOMINANT + 1.5 against 0.8 x scale ~ 0.8 x (DOMINANT + 3); 6 clears it only barely (7.18 against 7.04), 12
# gives 13.4 against 12.1 in the float64 reference, on a support that holds mu = 15
DOMINANT = {"bf16x3": 0.0, "bf16": 12.0}
SUPPORT = {"bf16x3": (VMIN, VMAX), "bf16": (-20.0, 20.0)}


def _obs(arch):
    return FC_OBS if arch == "fc" else (84, 84, 4)


def _head(feats, arch):
    return f"Dense_{len(feats) - (0 if arch == 'fc' else 3)}"


def bump_bias(params, feats, arch, n_heads, A, nb, vmin, vmax, seed, dominant=0.0):
    """Block (h, a) of the head bias += the log-Gaussian bump around mu_{h,a} = STEP (pi_h(a) - (A - 1) / 2) (+ dominant where
    pi_h(a) = A - 1)."""
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in params.items()}
    rng = np.random.default_rng(seed + 7)
    bias = p[_head(feats, arch)]["bias"].reshape(n_heads, A, nb)
    for h in range(n_heads):
        pi = rng.permutation(A)
        for a in range(A):
            mu = STEP * (pi[a] - (A - 1) / 2) + dominant * (pi[a] == A - 1)
            bias[h, a] += c51.gauss_bump(nb, vmin, vmax, mu, BUMP_SIGMA).astype(np.float32)
    return p


def _params(seed, feats, A, n_heads, arch, nb, vmin, vmax, ln=True, dominant=0.0):
    p = perturbed_params(seed, _obs(arch), feats, arch, n_heads * A * nb, ln)
    return bump_bias(p, feats, arch, n_heads, A, nb, vmin, vmax, seed, dominant)


def _engine(feats, A, n_heads, B, nb=NB, vmin=VMIN, vmax=VMAX, arch="cnn", ln=True, precision="bf16x3", seed=0, lr=1e-3, categorical=True, **kw):
    from slimdqn._engine import QNetEngine

    params = _params(seed, feats, A, n_heads, arch, nb, vmin, vmax, ln, DOMINANT[precision])
    ckw = dict(categorical=True, sigma=0.0) if categorical else dict(sigma=0.75 * (vmax - vmin) / nb)  # (sigma is ignored with the option)
    eng = QNetEngine(_obs(arch), A, n_heads, feats, arch, ln, B, gamma_n=0.99, learning_rate=lr, adam_eps=1.5e-4, precision=precision,
                     n_bins=nb, min_value=vmin, max_value=vmax, **ckw, **kw)
    eng.import_flax(params)
    eng.support = (vmin, vmax)
    return eng, params


class _Batch:
    """One batch in both forms: the engine's C batch (``eng`` given) and the float64 network input [states; next states].  Rewards are
    normal x 0.3 x the support's width; with B >= 4 the first four rows are set by hand: a terminal row far below the support, a terminal
    row far above it, a terminal row at ``inside`` and a non-terminal row."""

    def __init__(self, eng, arch, B, A, seed, vmin=VMIN, vmax=VMAX, weights=False, inside=None):
        rng = np.random.default_rng(seed + 100)
        obs = _obs(arch)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.weights = rng.uniform(0.2, 1.0, B).astype(np.float32) if weights else None
        width = vmax - vmin
        if arch == "fc":
            s = rng.normal(size=(B, obs[0])).astype(np.float32)
            ns = rng.normal(size=(B, obs[0])).astype(np.float32)
            self.action = rng.integers(0, A, B).astype(np.int32)
            self.terminal = (rng.random(B) < 0.3).astype(np.uint8)
            self.x_state, self.x_next = torch.from_numpy(s), torch.from_numpy(ns)
        else:
            frames, ids, action, _, terminal, ref = make_frame_batch(B, A, seed=seed, h=obs[0], w=obs[1], stack=obs[2])
            self.action, self.terminal = action, terminal.copy()
            self.x_state, self.x_next = torch.from_numpy(ref.state), torch.from_numpy(ref.next_state)
        self.reward = (rng.normal(size=B) * 0.3 * width).astype(np.float32)
        if B >= 4:
            self.terminal[:4] = (1, 1, 1, 0)
            self.reward[:4] = (vmin - 2 * width, vmax + 2 * width, 0.37 * vmax if inside is None else inside, 0.1 * width)
        if eng is not None:
            lw = None if self.weights is None else d(self.weights)
            if arch == "fc":
                self.cb = eng.make_batch(state=d(s), next_state=d(ns), action=d(self.action), reward=d(self.reward), terminal=d(self.terminal),
                                         loss_weights=lw)
            else:
                self.fr, self.ids, self.stride = d(frames), d(ids), frames.shape[1]
                self.cb = eng.make_batch(frames=self.fr, frame_stride=self.stride, frame_ids=self.ids, action=d(self.action), reward=d(self.reward),
                                         terminal=d(self.terminal), loss_weights=lw)

    def obs_kw(self, rows):
        """forward / best_actions keywords for the first `rows` states"""
        if hasattr(self, "fr"):
            stack = self.ids.shape[1] // 2
            return dict(frames=self.fr, frame_stride=self.stride, frame_ids=self.ids[:rows, :stack].contiguous())
        return dict(obs=self.x_state[:rows].cuda())

    def assert_terminal_and_clamped_rows(self, nb, vmin, vmax, gamma_n):
        """the batch has terminal rows, other rows, and rows whose pushed atoms clamp at either end of the support"""
        z = c51.atoms(nb, vmin, vmax).numpy()
        tz = self.reward.astype(np.float64)[:, None] + ((1.0 - self.terminal) * gamma_n)[:, None] * z[None, :]
        assert self.terminal.any() and not self.terminal.all()
        assert (tz < z[0]).all(1).any() and (tz > z[-1]).all(1).any()  # whole rows beyond either end
        assert ((tz < z[0]).any(1) & ~(tz < z[0]).all(1)).any() or ((tz > z[-1]).any(1) & ~(tz > z[-1]).all(1)).any()  # and partly clamped ones


def _width(eng):
    n = eng.n_heads * eng.n_actions * eng.n_bins
    return n, (n + 7) // 8 * 8


def _rows(eng, B, region="logits", n_rows=None):
    """the device's own logit rows [2B][heads * A * nb] of the last forward (region "logits": [2B][padded to 8])"""
    n, n_p = _width(eng)
    n_rows = 2 * B if n_rows is None else n_rows
    return eng.region(region)[: n_rows * n_p].reshape(n_rows, n_p)[:, :n].double().cpu()


def _ref(eng, rows, b, K=None, on0=None, tg0=0, **kw):
    K = eng.n_regressed if K is None else K
    on0 = (1 if eng.n_heads >= 2 else 0) if on0 is None else on0
    vmin, vmax = eng.support
    return c51.c51_loss(rows, b.action, b.reward, b.terminal, float(eng.cfg.gamma_n), K, on0, tg0, eng.n_actions, eng.n_bins, vmin, vmax,
                        weights=b.weights, **kw)


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _close(a, b, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


LARGEST = {}  # output -> largest err / bound seen in this process (printed by every call)


def _ratio(name, err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    LARGEST[name] = max(LARGEST.get(name, 0.0), float(r.max()))
    return float(r.max())


def check_device_step_against_rows(eng, b, ref, losses, B, K, on0, learn, tag="", priorities=True):
    """Section 1's derived bounds (module docstring): the outputs of one loss / learn / gradient call against the helper on the device's
    own rows.  The call wrote [B][K] rows of q_values / targets."""
    A, nb = eng.n_actions, eng.n_bins
    vmin, vmax = eng.support
    g = float(eng.cfg.gamma_n)
    eta = (vmax - vmin) / nb
    z = np.abs(c51.atoms(nb, vmin, vmax).numpy())
    # a*: the helper's top-two gap is far above anything rounding moves, for every pair -- the targets below then pin the device's a*
    assert float(ref["gap"].min()) > 1e-5 * max(1.0, ref["qmax"]), (float(ref["gap"].min()), ref["qmax"])
    r = np.abs(b.reward.astype(np.float64))
    disc = (1.0 - b.terminal.astype(np.float64)) * g
    w = np.ones(B) if b.weights is None else b.weights.astype(np.float64)
    p, m, la = ref["p"].numpy(), ref["m"].numpy(), ref["la"].numpy()
    s = torch.softmax(ref["la"], -1).numpy()
    db = 6 * U * (r[:, None] + disc[:, None] * z[None, :] + abs(vmin) + eta) / eta  # [B, nb]
    dm = 2 * (p * db[:, None, :]).sum(-1, keepdims=True) + (nb + 8) * U * m  # [B, K, nb]
    q_bound = 2 * (nb + 8) * U * (s * z).sum(-1)
    tq = ref["targets"].numpy() - b.reward.astype(np.float64)[:, None]  # = g Q^val(s', a*)
    t_bound = disc[:, None] * 2 * (nb + 8) * U * (p * z).sum(-1) + 2 * U * (r[:, None] + np.abs(tq))
    lse = torch.logsumexp(ref["la"], -1).numpy()
    l_bound = (dm * np.abs(la)).sum(-1) + (nb + 8) * U * (m * np.abs(la)).sum(-1) + RTOL * np.abs(lse) + ATOL
    l = ref["l"].detach().numpy()
    loss_bound = (w[:, None] * l_bound).mean(0) + (B + 8) * U * (w[:, None] * np.abs(l)).mean(0)
    first = lambda t: _cpu(t).reshape(-1)[: B * K].reshape(B, K).astype(np.float64)
    eq = np.abs(first(eng.q_values) - ref["q"].detach().numpy())
    et = np.abs(first(eng.targets) - ref["targets"].numpy())
    el = np.abs(losses.astype(np.float64)[:K] - ref["losses"].detach().numpy())
    rq, rt, rl = _ratio("q", eq, q_bound), _ratio("targets", et, t_bound), _ratio("losses", el, loss_bound)
    print(f"{tag}: err/bound q {rq:.3f} targets {rt:.3f} losses {rl:.3f} (min gap {float(ref['gap'].min()):.3g})")
    assert rq < 1 and rt < 1 and rl < 1, (rq, rt, rl)
    if not learn:
        return
    if priorities:
        pr = ref["priorities"].numpy()
        p_bound = np.sqrt(((q_bound + t_bound) ** 2).mean(1)) + 8 * U * pr
        rp = _ratio("priorities", np.abs(_cpu(eng.priorities).astype(np.float64) - pr), p_bound)
        print(f"{tag}: err/bound priorities {rp:.3f}")
        assert rp < 1, rp
    n, n_p = _width(eng)
    dout = eng.region("dout")[: B * n_p].reshape(B, n_p).double().cpu().numpy()
    bound = np.zeros((B, eng.n_heads, A, nb))
    bi, ki = np.arange(B)[:, None], np.arange(K)[None, :]
    bound[bi, on0 + ki, b.action[:, None].astype(np.int64)] = (w[:, None, None] / B) * (dm + RTOL * s + ATOL)
    ed = np.abs(dout[:, :n] - ref["dlogits"].numpy())
    rd = _ratio("dout", ed, bound.reshape(B, -1))  # (a zero bound -- every other output -- asks for exactly 0)
    print(f"{tag}: err/bound dout {rd:.3f} (largest |dout| {float(np.abs(dout).max()):.3g}); largest so far {LARGEST}")
    assert rd < 1, rd
    assert (dout[:, n:] == 0).all()
    taken = bound.reshape(B, -1) > 0
    assert (dout[:, :n][~taken] == 0).all() and taken.sum() == B * K * nb


# ------------------------------------------------------------------ 1. the loss kernel on the device's own rows
# (nb, support, K, A, B, arch, trunk, loss_weights) -- each the smallest that reaches one path of c51_loss_kernel
OWN_ROWS = [
    pytest.param((51, (-10.0, 10.0), 3, 5, 6, "cnn", TINY, False), id="nb51-tiny-B6-ragged"),  # R = 4: B ragged against R
    pytest.param((2, (-1.0, 1.0), 2, 3, 11, "fc", (16, 16), False), id="nb2-fc-B11"),  # the minimum
    pytest.param((65, (-10.0, 10.0), 1, 4, 5, "fc", (16, 16), False), id="nb65-fc"),  # one live lane in the second 64-group
    pytest.param((130, (-10.0, 10.0), 1, 4, 5, "fc", (16, 16), False), id="nb130-fc"),  # three groups
    pytest.param((256, (-10.0, 10.0), 1, 5, 5, "fc", (16, 16), False), id="nb256-fc"),  # the maximum: 2 * 5 * 256 <= 5456
    pytest.param((51, (-10.0, 10.0), 9, 9, 8, "cnn", HEADLINE, False), id="nb51-headline"),
    pytest.param((51, (-10.0, 10.0), 3, 5, 6, "cnn", TINY, True), id="nb51-tiny-B6-weights"),
]


@pytest.mark.parametrize("shape", OWN_ROWS)
def test_loss_kernel_matches_float64_on_the_device_rows(shape, request):
    nb, (vmin, vmax), K, A, B, arch, feats, weights = shape
    eng, _ = _engine(feats, A, 1 + K, B, nb, vmin, vmax, arch=arch)
    b = _Batch(eng, arch, B, A, seed=5, vmin=vmin, vmax=vmax, weights=weights)
    b.assert_terminal_and_clamped_rows(nb, vmin, vmax, float(eng.cfg.gamma_n))
    losses = _cpu(eng.learn_on_batch(b.cb))
    torch.cuda.synchronize()
    ref = _ref(eng, _rows(eng, B), b)
    check_device_step_against_rows(eng, b, ref, losses, B, K, 1, True, tag=request.node.callspec.id)
    # the rows set by hand: all mass on the end atom, on the two neighbours of r
    m = ref["m"].numpy()
    assert (np.abs(m[0, :, 0] - 1) < 1e-12).all() and (np.abs(m[1, :, -1] - 1) < 1e-12).all() and ((m[2] > 0).sum(-1) <= 2).all()


def test_dyadic_support_puts_a_terminal_reward_on_an_atom_exactly():
    """[-8, 8] in 64 atoms: eta = 0.25 and the centres are exact in float32.  Row 2 is terminal with r = z_17: b = 17 exactly, and the
    target must be one-hot at atom 17 -- the l == u case in which the textbook scatter form loses the atom's mass."""
    nb, vmin, vmax, K, A, B = 64, -8.0, 8.0, 2, 3, 6
    z = c51.atoms(nb, vmin, vmax).numpy()
    assert z[17] == -3.625 and (z.astype(np.float32).astype(np.float64) == z).all()
    eng, _ = _engine((16, 16), A, 1 + K, B, nb, vmin, vmax, arch="fc")
    b = _Batch(eng, "fc", B, A, seed=5, vmin=vmin, vmax=vmax, inside=z[17])
    b.assert_terminal_and_clamped_rows(nb, vmin, vmax, float(eng.cfg.gamma_n))
    assert tuple(b.terminal[:4]) == (1, 1, 1, 0) and b.reward[2] == np.float32(z[17]) and b.reward[0] < vmin - 16 and b.reward[1] > vmax + 16
    losses = _cpu(eng.learn_on_batch(b.cb))
    torch.cuda.synchronize()
    ref = _ref(eng, _rows(eng, B), b)
    for k in range(K):  # the reference: exactly 0 off the atom, sum_j p_j (1 to a few 1e-16) on it
        for row, atom in ((2, 17), (0, 0), (1, nb - 1)):
            m = ref["m"][row, k].numpy()
            assert abs(m[atom] - 1) < 1e-15 and (np.delete(m, atom) == 0).all()
    check_device_step_against_rows(eng, b, ref, losses, B, K, 1, True, tag="dyadic")
    # the device's rows themselves: dout = (softmax - m) / B is negative at the target's atom and non-negative at every other one
    n, n_p = _width(eng)
    dout = eng.region("dout")[: B * n_p].reshape(B, n_p)[:, :n].double().cpu().numpy().reshape(B, 1 + K, A, nb)
    for row, atom in ((2, 17), (0, 0), (1, nb - 1)):
        blk = dout[row, 1:, int(b.action[row])]  # [K, nb]
        assert (blk[:, atom] < 0).all() and (np.delete(blk, atom, axis=1) >= 0).all()
        s = torch.softmax(ref["la"][row], -1).numpy()
        # nothing leaked off the atom (atol: below float32's smallest normal a softmax tail has no relative precision)
        np.testing.assert_allclose(np.delete(blk, atom, axis=1), np.delete(s, atom, axis=1) / B, rtol=RTOL, atol=1e-37)


# ------------------------------------------------------------------ 2. the whole path against the float64 oracle forward
E2E = {  # the shapes of tests/test_gpu_hl_gauss.py
    "cnn-ln": (TINY, 3, 5, 6, "cnn", True, "bf16x3"),
    "cnn-noln": ((16, 20, 5, 24), 2, 3, 5, "cnn", False, "bf16x3"),
    "cnn-headline-B8": (HEADLINE, 9, 9, 8, "cnn", True, "bf16x3"),
    "fc-ln": ((32, 32), 2, 4, 9, "fc", True, "bf16x3"),
    "impala-ln": ((8, 16, 16, 24), 2, 5, 4, "impala", True, "bf16x3"),
    "cnn-ln-bf16": (TINY, 3, 5, 6, "cnn", True, "bf16"),
}
PARAM_SEED, BATCH_SEED, TARGET_SEED = 2, 9, 32


def oracle_case(name):
    """Everything of a section-2 case that needs no GPU: parameters, batch, the float64 rows, the helper's result on them and the top-two
    gap of the deciding head's expectations per pair."""
    feats, K, A, B, arch, ln, prec = E2E[name]
    vmin, vmax = SUPPORT[prec]
    params = _params(PARAM_SEED, feats, A, 1 + K, arch, NB, vmin, vmax, ln, DOMINANT[prec])
    b = _Batch(None, arch, B, A, seed=BATCH_SEED, vmin=vmin, vmax=vmax)
    pt = onet.to_torch(params, torch.float64)
    rows = torch.cat([onet.forward(pt, b.x_state, feats, arch, ln), onet.forward(pt, b.x_next, feats, arch, ln)])
    ref = c51.c51_loss(rows, b.action, b.reward, b.terminal, float(np.float32(0.99)), K, 1, 0, A, NB, vmin, vmax)
    return dict(params=params, batch=b, rows=rows, ref=ref, gap=ref["gap"].numpy(), scale=max(1.0, ref["qmax"]))


@pytest.mark.parametrize("name", list(E2E))
def test_whole_path_matches_the_float64_oracle(name):
    from slimdqn._engine import QNetEngine

    feats, K, A, B, arch, ln, prec = E2E[name]
    vmin, vmax = SUPPORT[prec]
    t = TOL[prec]
    c = oracle_case(name)
    ref = c["ref"]
    # the distribution is taken at an argmax: a pair is left out only when, in the float64 reference alone, the deciding head's top-two
    # gap is below 10 x the q bound x max(1, |Q|max); at most 10 % may be, and the committed cases leave out none
    keep = c["gap"] >= 10 * t["q"] * c["scale"]
    assert (~keep).mean() <= 0.10, f"{(~keep).sum()} of {keep.size} pairs left out"
    assert keep.all(), f"{(~keep).sum()} of {keep.size} pairs left out: the committed cases leave out none"
    eng = QNetEngine(_obs(arch), A, 1 + K, feats, arch, ln, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, precision=prec,
                     n_bins=NB, min_value=vmin, max_value=vmax, categorical=True)
    eng.import_flax(c["params"])
    b = _Batch(eng, arch, B, A, seed=BATCH_SEED, vmin=vmin, vmax=vmax)
    b.assert_terminal_and_clamped_rows(NB, vmin, vmax, float(eng.cfg.gamma_n))
    rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - np.asarray(want)).max() / max(1.0, float(np.abs(np.asarray(want)).max())))
    losses = _cpu(eng.loss_on_batch(b.cb))
    torch.cuda.synchronize()
    eq, et = rel(_cpu(eng.q_values), ref["q"].numpy()), rel(_cpu(eng.targets), ref["targets"].numpy())
    el = rel(losses, ref["losses"].numpy())
    print(f"{name}: q {eq:.2e} targets {et:.2e} (bound {t['q']:.0e}) loss {el:.2e} (bound {t['loss']:.0e}); "
          f"min gap {c['gap'].min():.3g} (bound {10 * t['q'] * c['scale']:.3g})")
    assert eq < t["q"] and et < t["q"] and el < t["loss"]


# ------------------------------------------------------------------ 3. gradients and Adam
def _s8_values(region: torch.Tensor, rows, pitch):
    """fp32 values of an S8 activation block [rows][pitch] (every 8 floats: 8 bf16 hi halves, then 8 lo halves)."""
    u16 = region.cpu().numpy()[: rows * pitch].view(np.uint16).reshape(rows, pitch // 8, 2, 8)
    f = lambda h: (h.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return (f(u16[:, :, 0]) + f(u16[:, :, 1])).reshape(rows, pitch)


@pytest.mark.parametrize("shape", [
    pytest.param((TINY, 3, 5, 6, "cnn"), id="cnn-tiny"),
    pytest.param(((32, 32), 2, 4, 9, "fc"), id="fc"),
])
def test_learn_gradients_and_adam_of_categorical_heads(shape):
    feats, K, A, B, arch = shape
    lr = 1e-3
    eng, params = _engine(feats, A, 1 + K, B, arch=arch, seed=4, lr=lr)
    b = _Batch(eng, arch, B, A, seed=13)
    p0 = eng.params.clone()
    g = torch.zeros_like(eng.params)
    eng.learn_on_batch(b.cb, grad_out=g)
    torch.cuda.synchronize()
    hip_g = eng.internal_to_flax_grads(g)
    head = _head(feats, arch)
    hid = f"Dense_{int(head.split('_')[1]) - 1}"
    # (a) head leaves against float64 dlogits^T . act from the device's own rows and hidden activations
    ref = _ref(eng, _rows(eng, B), b)
    F = feats[-1]
    act = _s8_values(eng.region(f"act/{hid}"), B, (F + 7) // 8 * 8)[:, :F]
    dl = ref["dlogits"].numpy()
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


# ------------------------------------------------------------------ 4. Double Q-learning
def _bites(eng, ref, vrows, K, tg0=0):
    """a* leaves the value head's own greedy action on at least a quarter of the pairs (asserted on the reference)"""
    vmin, vmax = eng.support
    B = vrows.shape[0]
    greedy = c51.first_argmax(c51.expectations(vrows, eng.n_bins, vmin, vmax).reshape(B, -1, eng.n_actions)[:, tg0 : tg0 + K])
    share = float((ref["a_star"] != greedy).double().mean())
    assert share >= 0.25, share
    return share


@pytest.mark.parametrize("shape", [
    pytest.param((TINY, 3, 5, 6, "cnn", 65), id="tiny-nb65"),
    pytest.param(((16, 16), 2, 3, 11, "fc", 51), id="fc-B11-ragged-weights"),
])
def test_isdqn_double_q_matches_the_helper_with_selector_rows(shape, request):
    feats, K, A, B, arch, nb = shape
    eng, _ = _engine(feats, A, 1 + K, B, nb, arch=arch, seed=2, double_q=True)
    b = _Batch(eng, arch, B, A, seed=5, weights=arch == "fc")
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        rows = _rows(eng, B)
        ref = _ref(eng, rows, b, selector_rows=rows[B:])
        _bites(eng, ref, rows[B:], K)
        check_device_step_against_rows(eng, b, ref, losses, B, K, 1, learn, tag=f"{request.node.callspec.id} learn={learn}")


@pytest.mark.parametrize("shape", [
    pytest.param((TINY, 5, 6, "cnn", 65), id="tiny-nb65"),
    pytest.param(((16, 16), 3, 11, "fc", 51), id="fc-B11-ragged"),
])
def test_dqn_form_selects_online_and_takes_the_distribution_of_the_target_rows(shape, request):
    """Double DQN: region "logits" holds the ONLINE parameters' rows over concat(state, next_state), region "logits_target" the target
    parameters' rows over the B next states (region "q_target": their expectations)."""
    feats, A, B, arch, nb = shape
    eng, _ = _engine(feats, A, 1, B, nb, arch=arch, seed=2, double_q=True)
    tgt = torch.zeros_like(eng.params)
    eng.import_flax(_params(TARGET_SEED, feats, A, 1, arch, nb, VMIN, VMAX), target=tgt)
    assert not torch.equal(tgt, eng.params)
    b = _Batch(eng, arch, B, A, seed=5)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch_target(b.cb, tgt) if learn else eng.loss_on_batch_target(b.cb, tgt))
        torch.cuda.synchronize()
        rows, vrows = _rows(eng, B), _rows(eng, B, "logits_target", n_rows=B)
        assert not np.array_equal(rows[B:].numpy(), vrows.numpy())  # two networks
        ref = _ref(eng, rows, b, K=1, on0=0, value_rows=vrows, selector_rows=rows[B:])
        _bites(eng, ref, vrows, 1)
        qt = eng.region("q_target")[: B * 8 * ((A + 7) // 8)].reshape(B, -1)[:, :A].double().cpu()
        _close(qt, c51.expectations(vrows, nb, VMIN, VMAX), rtol=1e-5, atol=1e-5)
        check_device_step_against_rows(eng, b, ref, losses, B, 1, 0, learn, tag=f"{request.node.callspec.id} learn={learn}")


def test_tfdqn_single_head_is_regressed_on_its_own_distribution():
    """n_heads = 1 without target parameters (TF-DQN): selector and value head are the same rows, so double_q changes no bit."""
    feats, A, B, nb = TINY, 5, 6, 51
    outs = []
    for dq in (False, True):
        eng, _ = _engine(feats, A, 1, B, nb, seed=8, double_q=dq)
        b = _Batch(eng, "cnn", B, A, seed=17)
        for learn in (False, True):
            losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
            torch.cuda.synchronize()
            rows = _rows(eng, B)
            ref = _ref(eng, rows, b, K=1, on0=0, selector_rows=rows[B:] if dq else None)
            check_device_step_against_rows(eng, b, ref, losses, B, 1, 0, learn, tag=f"tfdqn dq={dq} learn={learn}")
        outs.append([_cpu(x) for x in (eng.params, eng.losses, eng.priorities, eng.q_values, eng.targets)])
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_grad_on_batch_through_an_analysis_agent():
    """AnalysisDQN.three_gradients: the target-based and the target-free single-pair gradients and the iS gradient (the last call: all K
    pairs, whose rows and dout the workspace still holds), with double_q and target parameters of another network."""
    from oracle.replay_buffer import ReplayElement
    from slimdqn.networks.analysisdqn import AnalysisDQN

    feats, K, A, B, nb = TINY, 3, 5, 6, 51
    agent = AnalysisDQN(0, (84, 84, 4), A, K, list(feats), True, False, "cnn", 1e-3, 0.99, 1, 1, 4, adam_eps=1.5e-4, batch_size=B,
                        n_bins=nb, min_value=VMIN, max_value=VMAX, categorical=True, double_q=True)
    eng = agent._engine
    assert eng.categorical and int(eng.cfg.categorical) == 1 and eng.cfg.hl_min == VMIN
    eng.support = (VMIN, VMAX)
    eng.import_flax(_params(2, feats, A, 1 + K, "cnn", nb, VMIN, VMAX))
    eng.import_flax(_params(TARGET_SEED, feats, A, 1 + K, "cnn", nb, VMIN, VMAX), target=agent.target_params.tensor)
    b = _Batch(None, "cnn", B, A, seed=5)
    frames, ids, action, _, terminal, refb = make_frame_batch(B, A, seed=5)
    sample = ReplayElement(state=refb.state, action=b.action.astype(np.int64), reward=b.reward.astype(np.float64), next_state=refb.next_state,
                           is_terminal=b.terminal.astype(np.int64))
    g_is, g_tf, g_tb = agent.three_gradients(agent.params, agent.target_params, sample)
    torch.cuda.synchronize()
    for g in (g_is, g_tf, g_tb):
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert not torch.equal(g_tf, g_tb)
    rows = _rows(eng, B)
    ref = _ref(eng, rows, b, selector_rows=rows[B:])
    _bites(eng, ref, rows[B:], K)
    check_device_step_against_rows(eng, b, ref, _cpu(eng.losses), B, K, 1, True, tag="analysis iS gradient", priorities=False)
    head = _head(feats, "cnn")
    got = np.asarray(eng.internal_to_flax_grads(g_is)[head]["bias"], np.float64)
    want = ref["dlogits"].numpy().sum(0)
    assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-4
    # the target-based single pair through the engine directly, against the helper on the two networks' rows
    g = torch.zeros_like(eng.params)
    losses = _cpu(eng.grad_on_batch(agent._c_batch(eng, sample), g, target_params=agent.target_params.tensor, online_head=1, target_head=1, n_pairs=1))
    torch.cuda.synchronize()
    assert torch.equal(g, g_tb)
    rows, vrows = _rows(eng, B), _rows(eng, B, "logits_target", n_rows=B)
    ref = _ref(eng, rows, b, K=1, on0=1, tg0=1, value_rows=vrows, selector_rows=rows[B:])
    check_device_step_against_rows(eng, b, ref, losses, B, 1, 1, True, tag="analysis target-based pair", priorities=False)


# ------------------------------------------------------------------ 5. other checks
def test_two_learn_steps_are_bit_identical_from_identical_state():
    feats, K, A, B = HEADLINE, 9, 9, 32
    runs = []
    for _ in range(2):
        eng, _ = _engine(feats, A, 1 + K, B, seed=1)
        b = _Batch(eng, "cnn", B, A, seed=3)
        ls = [eng.learn_on_batch(b.cb).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.stack(ls), eng.priorities.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert torch.isfinite(runs[0][3]).all() and (runs[0][3] > 0).all()


class _Replica:
    """bench.Replica's training state (synthetic prefilled replay, headline widths) with the categorical loss."""

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
                              device="cuda:0", n_bins=NB, min_value=-10.2, max_value=10.2, categorical=True)
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


@pytest.mark.parametrize("arch", ["cnn", "fc"])
def test_acting_and_shift_params_have_the_bits_of_an_n_bins_only_engine(arch):
    """forward, best_action(s) and shift_params do not change at all: the same parameters give the same bits with and without the option."""
    feats = TINY if arch == "cnn" else (32, 32)
    K, A, B, nb = 3, 5, 8, 65
    cat, params = _engine(feats, A, 1 + K, B, nb, arch=arch, seed=6)
    hist, _ = _engine(feats, A, 1 + K, B, nb, arch=arch, seed=6, categorical=False)
    assert int(cat.cfg.categorical) == 1 and int(hist.cfg.categorical) == 0 and torch.equal(cat.params, hist.params)
    assert cat.workspace_bytes == hist.workspace_bytes
    b = _Batch(cat, arch, B, A, seed=21)
    idx = torch.tensor([i % K for i in range(B)], dtype=torch.int32, device="cuda")
    got = []
    for eng in (cat, hist):
        q = eng.forward(n_rows=B, **b.obs_kw(B)).clone()
        acts = eng.best_actions(idx_networks=idx, **b.obs_kw(B)).clone()
        one = dict(obs=b.x_state[:1].cuda()) if arch == "fc" else dict(frames=b.fr, frame_stride=b.stride, frame_ids=b.ids[:1, :4].contiguous())
        a0 = int(eng.best_action(idx_network=1, **one).item())
        eng.shift_params()
        torch.cuda.synchronize()
        got.append((q, acts, a0, eng.params.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and got[0][2] == got[1][2] and torch.equal(got[0][3], got[1][3])
    q = got[0][0].double().cpu()
    pt = onet.to_torch(params, torch.float64)
    qo = c51.expectations(onet.forward(pt, b.x_state, feats, arch, True), nb, VMIN, VMAX)
    assert q.shape == (B, (1 + K) * A) and (q - qo).abs().max() < 1e-3 * max(1.0, float(qo.abs().max()))
    w = A * nb
    head = _head(feats, arch)
    after = cat.export_flax()[head]["bias"]
    before = params[head]["bias"]
    assert np.array_equal(after, np.concatenate([before[w:], before[-w:]]))


def test_categorical_false_is_bit_identical_to_an_engine_built_without_the_keyword():
    """An n_bins-only engine keeps its bits: categorical=False against the field left untouched, one learn step."""
    from slimdqn._engine import QNetEngine

    feats, K, A, B, nb = TINY, 3, 5, 6, 51
    outs, sizes = [], []
    for kw in ({}, dict(categorical=False)):
        params = perturbed_params(3, (84, 84, 4), feats, "cnn", (1 + K) * A * nb, True)
        eng = QNetEngine((84, 84, 4), A, 1 + K, feats, "cnn", True, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, n_bins=nb, min_value=-10.0,
                         max_value=10.0, sigma=0.3, **kw)
        eng.import_flax(params)
        eng.support = (-10.0, 10.0)
        b = _Batch(eng, "cnn", B, A, seed=5)
        losses = eng.learn_on_batch(b.cb)
        torch.cuda.synchronize()
        assert int(eng.cfg.categorical) == 0 and eng.categorical is False
        outs.append([_cpu(x) for x in (eng.params, eng.adam_m, eng.adam_v, losses, eng.priorities, eng.q_values, eng.targets)])
        sizes.append(eng.workspace_bytes)
    assert sizes[0] == sizes[1]
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    # and the option changes the step: the same engine with it gives other losses
    eng, _ = _engine(feats, A, 1 + K, B, nb, seed=3)
    eng.import_flax(params)
    other = _cpu(eng.learn_on_batch(_Batch(eng, "cnn", B, A, seed=5).cb))
    assert not np.array_equal(other, outs[0][3])


ARGV = ["-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "200", "-bs", "8", "-n", "1", "-horizon", "50", "-at", "cnn", "-ne", "2",
        "-ntspe", "60", "-utd", "4", "-nis", "20", "-ed", "100", "-ln", "-tuf", "16", "-env", "synthetic"]


def test_isdqn_entry_point_with_the_categorical_loss(tmp_path, monkeypatch):
    import pickle

    import slimdqn.networks._agent as agent_mod
    from experiments.atari.isdqn import run

    built = []

    class Recording(agent_mod.QNetEngine):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            built.append((int(self.cfg.categorical), int(self.cfg.n_bins), float(self.cfg.hl_min), float(self.cfg.hl_max)))

    monkeypatch.setattr(agent_mod, "QNetEngine", Recording)
    gathered = run(["-en", "c51_Synthetic"] + ARGV + ["-nbi", "2", "-hl", "-cat", "-nb", "51", "-minn", "-10.2", "-maxn", "10.2"], root=str(tmp_path))
    assert len(gathered) == 2
    assert built and all(x == (1, 51, float(np.float32(-10.2)), float(np.float32(10.2))) for x in built)
    out = tmp_path / "atari" / "exp_output" / "c51_Synthetic"
    # (the engine group's flags, -cat among them, stay out of parameters.json like -hl)
    stored = json.load(open(out / "parameters.json"))
    assert stored["isdqn"]["n_bellman_iterations"] == 2 and not any("categorical" in k for k in list(stored["isdqn"]) + list(stored["shared_parameters"]))
    model = pickle.load(open(out / "isdqn" / "models" / "1", "rb"))["params"]
    assert model["params"]["Dense_1"]["kernel"].shape == (16, 3 * 9 * 51)
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())


@pytest.mark.parametrize("extra", [[], ["-hl", "-mq"], ["-qr"]])
def test_entry_point_refuses_cat_without_hl_or_with_mq_or_qr_before_any_output_directory_exists(tmp_path, extra):
    from experiments.atari.isdqn import run

    with pytest.raises(ValueError) as e:
        run(["-en", "bad_Synthetic"] + ARGV + ["-nbi", "2", "-cat"] + extra, root=str(tmp_path))
    assert "categorical" in str(e.value)
    assert not (tmp_path / "atari").exists()
