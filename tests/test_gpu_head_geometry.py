"""The three distributional loss kernels at the edges of their geometry (csrc/head_loss.h: hl_loss_kernel, c51_loss_kernel,
qr_loss_kernel and the frame they share), against the float64 restatements of tests/helpers on the device's own head-output rows.

The table is tests/helpers/head_geometry.py's (tests/test_head_geometry_host.py holds it to its coverage): R = 3, 2 and 1 transitions per
workgroup, batches ragged against R and shorter than R, K = 64, the widest row the plan takes (5456 outputs), A = 1.  Every network is
the fc torso 8 -> 16 -> 16 with LayerNorm in bf16x3: the head is the object under test.

1. every case of the table for HL-Gauss, C51, and the quantile loss with kappa 1 and 0: everything the contract at the top of
   head_loss.h names, at the tolerances the project already holds these quantities to -- HL-Gauss: rtol 1e-5 / atol 1e-7
   (tests/test_gpu_hl_gauss.py, _close); C51 and quantile: the derived bounds of check_device_step_against_rows in
   tests/test_gpu_categorical.py and tests/test_gpu_quantile.py, called from here.  No number of this file's own.
2. variants on r3-ragged, r2 and r1: per-row discount, Double Q-learning, the conservative term (tests/test_gpu_conservative.py's
   bound), loss-only and gradient-only calls, a call that regresses fewer heads than K (its R is 4 again), run-to-run bit identity.
3. HL-Gauss over bin counts, sigma and support edges; ties; Munchausen at 130 and 256 bins.
4. the widest row through forward, acting and one learn step against the float64 oracle; the three refusals beyond it.

Settings the table leaves open.  Histogram cases use head_geometry.dyadic_support(nb) -- (1, 1 + nb eta), eta a power of two: edges
exact in float32, no expectation near zero -- and sigma = 0.75 * 20 / 51 in value units, the sigma of every existing HL-Gauss test, on a
support of about the same width (16 to 20): a float32 target moves the projection as much as it does in the tests whose tolerance is
used here.  (In bins that is 0.04 at nb = 2 and 4.7 at nb = 256; section 3 varies sigma in bins.)  Every histogram network gets separated
action values through the shape of its head bias, as tests/test_gpu_categorical.py's: block (h, a) += a log-Gaussian bump around
centre + 1.5 (pi_h(a) - (A - 1) / 2), pi_h a seeded permutation, of width / 6 standard deviation -- wide, so that every 64-bin group of
a lane carries softmax mass.  Quantile networks get tests/test_gpu_quantile.py's spread bias.

Every test prints its figures (pytest -s): the lines that start with GEOMETRY are what docs/NOTEBOOK.md's entry quotes."""
import json
import types

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests import test_gpu_categorical as tc
from tests import test_gpu_conservative as tcq
from tests import test_gpu_munchausen as tm
from tests import test_gpu_quantile as tq
from tests.gpu_helpers import perturbed_params
from tests.helpers import head_geometry as hg
from tests.helpers import hl_gauss as hl
from tests.test_gpu_hl_gauss import TOL, _close

pytestmark = pytest.mark.gpu

FC_OBS, FEATS, HEAD = (8,), (16, 16), "Dense_2"
SIGMA = 0.75 * 20.0 / 51  # value units (module docstring)
STEP = 1.5
LOSS_IDS = ("hl", "c51", "qr-huber", "qr-pinball")
VARIANT_LOSSES = ("hl", "c51", "qr-huber")
CASES = [pytest.param(c, id=c.id) for c in hg.CASES]
VARIANTS = [pytest.param(hg.BY_ID[i], id=i) for i in hg.VARIANT_IDS]


def _note(**kw):
    print("GEOMETRY " + json.dumps(kw))


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _is_hist(loss):
    return loss in ("hl", "c51")


def _bump(params, n_heads, A, nb, vmin, vmax, seed, step=STEP):
    """Block (h, a) of the head bias += -(c_j - mu_{h,a})^2 / (2 s^2), mu_{h,a} = centre + step (pi_h(a) - (A - 1) / 2), s = width / 6."""
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in params.items()}
    rng = np.random.default_rng(seed + 7)
    bias = p[HEAD]["bias"].reshape(n_heads, A, nb)
    c = hl.centres(nb, vmin, vmax).numpy()
    s = (vmax - vmin) / 6.0
    for h in range(n_heads):
        pi = rng.permutation(A)
        for a in range(A):
            mu = 0.5 * (vmin + vmax) + step * (pi[a] - (A - 1) / 2)
            bias[h, a] += (-((c - mu) ** 2) / (2.0 * s * s)).astype(np.float32)
    return p


def _params(loss, K, A, nb, support, seed):
    n_heads = K + 1
    if _is_hist(loss):
        return _bump(perturbed_params(seed, FC_OBS, FEATS, "fc", n_heads * A * nb, True), n_heads, A, nb, *support, seed)
    return tq._params(seed, FEATS, A, n_heads, "fc", nb)


def _engine(K, A, nb, B, loss, support=None, sigma=SIGMA, seed=0, params=None, **kw):
    from slimdqn._engine import QNetEngine

    support = hg.dyadic_support(nb) if support is None else support
    if loss == "hl":
        okw = dict(n_bins=nb, min_value=support[0], max_value=support[1], sigma=sigma)
    elif loss == "c51":
        okw = dict(n_bins=nb, min_value=support[0], max_value=support[1], categorical=True, sigma=0.0)
    else:
        okw = dict(n_quantiles=nb, huber_delta=1.0 if loss == "qr-huber" else 0.0)
    params = _params(loss, K, A, nb, support, seed) if params is None else params
    eng = QNetEngine(FC_OBS, A, K + 1, FEATS, "fc", True, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, **okw, **kw)
    eng.import_flax(params)
    eng.support, eng.hl_sigma, eng.loss_name, eng.width = support, sigma, loss, nb
    return eng, params


def _case_engine(case, loss, **kw):
    return _engine(case.K, case.A, case.nb, case.B, loss, **kw)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Batch:
    """One batch in both forms.  Histogram heads: rewards normal x 0.3 x the support's width (the bootstrap value sits near the centre),
    row 0 terminal and far below the support, row 1 not terminal and far above it, row 2 terminal and inside.  Quantile heads:
    tests/test_gpu_quantile.py's rewards, row 0 terminal, row 1 not.  The loss weights are never 1."""

    def __init__(self, eng, B, A, seed=5, discount=None, hand=None):
        rng = np.random.default_rng(seed + 100)
        s, ns = rng.normal(size=(B, FC_OBS[0])).astype(np.float32), rng.normal(size=(B, FC_OBS[0])).astype(np.float32)
        self.x_state, self.x_next = torch.from_numpy(s), torch.from_numpy(ns)
        self.action = rng.integers(0, A, B).astype(np.int32)
        self.terminal = (rng.random(B) < 0.3).astype(np.uint8)
        self.weights = rng.uniform(0.2, 0.9, B).astype(np.float32)
        if _is_hist(eng.loss_name):
            vmin, vmax = eng.support
            width = vmax - vmin
            self.reward = (rng.normal(size=B) * 0.3 * width).astype(np.float32)
            self.terminal[:2] = (1, 0)
            self.reward[:2] = (vmin - 2 * width, vmax + 2 * width)
            if B >= 3:
                self.terminal[2], self.reward[2] = 1, vmin + 0.37 * width
        else:
            self.reward = (rng.normal(size=B) + tq._reward_shift(A)).astype(np.float32)
            self.terminal[:2] = (1, 0)
        if hand is not None:  # (terminal [B], reward [n <= B]): rows set by hand over the draw above
            self.terminal[:] = hand[0]
            self.reward[: len(hand[1])] = hand[1]
        self.discount = None if discount is None else np.asarray(discount, np.float32)
        self.kw = dict(state=_d(s), next_state=_d(ns), action=_d(self.action), reward=_d(self.reward), terminal=_d(self.terminal),
                       loss_weights=_d(self.weights))
        self.cb = eng.make_batch(**self.kw, discount=None if discount is None else _d(self.discount))


def _widths(eng):
    n = eng.n_heads * eng.n_actions * eng.width
    return n, (n + 7) // 8 * 8


def _rows(eng, B):
    """the device's own head-output rows [2B][heads * A * nb] of the last forward (region "logits": [2B][padded to 8])"""
    n, n_p = _widths(eng)
    return eng.region("logits")[: 2 * B * n_p].reshape(2 * B, n_p)[:, :n].double().cpu()


def _dout(eng, B):
    n, n_p = _widths(eng)
    return eng.region("dout")[: B * n_p].reshape(B, n_p).double().cpu().numpy()


class _Sub:
    """The engine as the shared checkers read it after a call that wrote [B][K] rows of q_values / targets into the [B][n_regressed]
    buffers (a call on fewer heads); ``priorities``: what stands in for a call that writes none."""

    def __init__(self, eng, B, K, priorities=None):
        self._eng = eng
        self.q_values = eng.q_values.reshape(-1)[: B * K].reshape(B, K)
        self.targets = eng.targets.reshape(-1)[: B * K].reshape(B, K)
        self.priorities = eng.priorities if priorities is None else priorities

    def __getattr__(self, name):
        return getattr(self._eng, name)


def _ref(eng, b, rows, K, on0, tg0, selector):
    B = rows.shape[0] // 2
    sel = rows[B:] if selector else None
    if eng.loss_name == "hl":
        return hl.hl_loss(rows, b.action, b.reward, b.terminal, float(eng.cfg.gamma_n), K, on0, tg0, eng.n_actions, eng.width, *eng.support,
                          eng.hl_sigma, selector_rows=sel, weights=b.weights, discount=b.discount)
    assert b.discount is None
    if eng.loss_name == "c51":
        return tc._ref(eng, rows, b, K=K, on0=on0, tg0=tg0, selector_rows=sel)
    assert tg0 == 0
    return tq._ref_with_rows(eng, rows, b, K=K, on0=on0, selector_rows=sel)


def _dkey(eng):
    return "dtheta" if eng.loss_name.startswith("qr") else "dlogits"


def _assert_inputs_bite(eng, b, ref):
    """a terminal row and another, loss weights off 1, and (histogram heads) a target clamped at each end of the support"""
    assert b.terminal.any() and not b.terminal.all() and (b.weights != 1).all()
    if _is_hist(eng.loss_name):
        t = np.asarray(ref["targets"])
        assert (t < eng.support[0]).any() and (t > eng.support[1]).any()


def _gap_holds(eng, rows, K, on0, tg0, selector):
    """(histogram heads, the HL-Gauss path: the shared checkers assert their own) no argmax of the deciding head can flip by rounding"""
    B, A = rows.shape[0] // 2, eng.n_actions
    if A == 1:
        return
    ex = hl.expectations(rows[B:], eng.width, *eng.support).reshape(B, -1, A)
    ex = ex[:, on0 : on0 + K] if selector else ex[:, tg0 : tg0 + K]
    top = torch.sort(ex, -1, descending=True).values
    assert float((top[..., 0] - top[..., 1]).min()) > 1e-4  # tests/test_gpu_double_q.py's floor for a float32 selection


def check_call(eng, b, losses, K=None, on0=1, tg0=0, selector=False, priorities=True, dout=True, grad=None, tag="", gap=True):
    """One learn / loss / gradient call against the helper on the device's own rows: losses, q_values, targets, priorities (where the
    call writes them), dout on its true columns, exact zeros everywhere else, and the head-bias gradient from ``grad`` (where given)."""
    B, A, nb = b.action.shape[0], eng.n_actions, eng.width
    K = eng.n_regressed if K is None else K
    rows = _rows(eng, B)
    ref = _ref(eng, b, rows, K, on0, tg0, selector)
    _assert_inputs_bite(eng, b, ref)
    n, n_p = _widths(eng)
    sub = _Sub(eng, B, K, priorities=None if priorities else ref["priorities"])  # (a call without priorities: the reference's own)
    losses = np.asarray(losses)[:K]
    if eng.loss_name == "hl":
        if gap:
            _gap_holds(eng, rows, K, on0, tg0, selector)
        _close(losses, ref["losses"])
        _close(sub.q_values.cpu(), ref["q"])
        _close(sub.targets.cpu(), ref["targets"])
        if priorities:
            _close(eng.priorities.cpu(), ref["priorities"])
        if dout:
            # Double Q-learning: tests/test_gpu_double_q.py's floor for the projection of a float32 target (its derivation is there)
            floor = 4 * 2.0 ** -23 * eng.support[1] / (eng.hl_sigma * np.sqrt(2 * np.pi)) / B if selector else 0.0
            got = _dout(eng, B)[:, :n]
            print(f"{tag}: max |dout - helper| {np.abs(got - ref['dlogits'].numpy()).max():.3g}")
            _close(got, ref["dlogits"], atol=1e-7 + floor)
    elif eng.loss_name == "c51":
        tc.check_device_step_against_rows(sub, b, ref, losses, B, K, on0, dout, tag=tag, priorities=priorities)
    else:
        assert dout or not priorities
        tq.check_device_step_against_rows(sub, b, ref, losses, B, K, on0, dout, tag=tag)
    if not dout:
        return ref
    # exact zeros: the padding columns, head 0 and every head outside the regressed ones, the untaken actions
    got = _dout(eng, B)
    assert (got[:, n:] == 0).all()
    blocks = got[:, :n].reshape(B, eng.n_heads, A, nb)
    taken = np.zeros((B, eng.n_heads, A), bool)
    taken[np.arange(B)[:, None], on0 + np.arange(K)[None, :], b.action[:, None].astype(np.int64)] = True
    assert (blocks[~taken] == 0).all() and not taken[:, 0].any()
    assert (np.abs(blocks[taken]).max(-1) > 0).all()  # and every taken block was written
    if grad is not None:
        # the head-bias gradient: the column sums of the reference's dL/d(output); tests/test_gpu_hl_gauss.py's bound for this leaf
        want = ref[_dkey(eng)].numpy().sum(0)
        bias = np.asarray(eng.internal_to_flax_grads(grad)[HEAD]["bias"], np.float64)
        e = np.linalg.norm(bias - want) / np.linalg.norm(want)
        print(f"{tag}: head bias gradient norm-rel {e:.2e} (bound 1e-4)")
        assert bias.shape == want.shape and e <= 1e-4, e
        assert (bias.reshape(eng.n_heads, A, nb)[~taken.any(0)] == 0).all()  # columns no row of the batch took
    return ref


# ------------------------------------------------------------------ 1. every case of the table, for each loss
@pytest.mark.parametrize("loss", LOSS_IDS)
@pytest.mark.parametrize("case", CASES)
def test_every_output_of_the_contract_at_every_geometry(case, loss):
    assert case.R == hg.rows_per_wg(case.K, case.nb)
    eng, _ = _case_engine(case, loss)
    b = _Batch(eng, case.B, case.A)
    g = torch.zeros_like(eng.params)
    losses = _cpu(eng.learn_on_batch(b.cb, grad_out=g))
    torch.cuda.synchronize()
    check_call(eng, b, losses, grad=g, tag=f"{case.id} {loss}")
    _note(test="contract", case=case.id, loss=loss, R=case.R, workgroups=case.n_wg)


# ------------------------------------------------------------------ 2. variants on r3-ragged, r2 and r1
D1, D2 = np.float32(0.97**3), np.float32(0.5)  # tests/test_gpu_horizon.py's two discounts


@pytest.mark.parametrize("loss", VARIANT_LOSSES)
@pytest.mark.parametrize("case", VARIANTS)
def test_discount_is_taken_row_by_row(case, loss):
    """tests/test_gpu_horizon.py's form: a tensor of D1 and D2 by row against the uniform runs at gamma_n = D1 and D2 -- q_values,
    targets, priorities and the rows of dout equal those of the uniform run at the row's value, bit for bit.  HL-Gauss: the mixed run
    also against the helper with ``discount``."""
    B = case.B
    which = np.arange(B) % 2
    values = np.array([D1, D2], np.float32)

    def run(gamma_n, discount):
        eng, _ = _case_engine(case, loss)
        eng.cfg.gamma_n = float(gamma_n)
        b = _Batch(eng, B, case.A, discount=discount)
        losses = _cpu(eng.learn_on_batch(b.cb))
        torch.cuda.synchronize()
        return eng, b, losses, dict(q_values=_cpu(eng.q_values), targets=_cpu(eng.targets), priorities=_cpu(eng.priorities), dout=_dout(eng, B))

    uniform = [run(v, None)[3] for v in values]
    eng, b, losses, got = run(0.123, values[which])  # (gamma_n is ignored once the tensor is there)
    for v in range(2):
        rows = which == v
        for k in got:
            assert np.array_equal(got[k][rows], uniform[v][k][rows]), f"{k}: rows at discount {values[v]} differ from the uniform run at it"
    assert not np.array_equal(uniform[0]["targets"], uniform[1]["targets"])
    if loss == "hl":
        check_call(eng, b, losses, tag=f"{case.id} discount")


@pytest.mark.parametrize("loss", VARIANT_LOSSES)
@pytest.mark.parametrize("case", VARIANTS)
def test_double_q_selector(case, loss):
    eng, _ = _case_engine(case, loss, double_q=True)
    b = _Batch(eng, case.B, case.A)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        ref = check_call(eng, b, losses, selector=True, priorities=learn, dout=learn, tag=f"{case.id} {loss} double_q learn={learn}")
    if case.A > 1 and loss != "hl":  # the selector bites: a* leaves the value head's own greedy action somewhere
        rows = _rows(eng, case.B)
        greedy = _ref(eng, b, rows, case.K, 1, 0, False)["a_star"]
        assert (ref["a_star"] != greedy).any()


@pytest.mark.parametrize("loss", VARIANT_LOSSES)
@pytest.mark.parametrize("case", VARIANTS)
def test_conservative_term_on_the_row_partition(case, loss):
    """tests/test_gpu_conservative.py's checks 1 to 3 and its bound, on a partition of 3, 2 and 1 rows: the increments of dout, of the
    head-bias gradient and of the losses against conservative.restate on the device's own rows."""
    ALPHA, U = tcq.ALPHA, tcq.U
    B, K, A, nb = case.B, case.K, case.A, case.nb
    eng, _ = _case_engine(case, loss)
    b = _Batch(eng, B, A)
    kw = dict(n_bins=nb, min_value=eng.support[0], max_value=eng.support[1]) if _is_hist(loss) else dict(n_quantiles=nb)
    c = dict(B=B, K=K, A=A, kw=kw)
    host = dict(action=b.action, weights=b.weights)
    plain, on, again = (tcq._grad_call(eng, c, x) for x in (b.cb, tcq._with_cql(b.cb, ALPHA), tcq._with_cql(b.cb, ALPHA)))
    for name in plain:
        assert np.array_equal(tcq._bits(again[name]), tcq._bits(on[name])), f"{name} differs between two calls at alpha = {ALPHA}"
    for name in ("q_values", "targets", "rows"):
        assert np.array_equal(tcq._bits(on[name]), tcq._bits(plain[name])), f"{name} moved with the term"
    l_on = tcq._loss_call(eng, tcq._with_cql(b.cb, ALPHA))
    assert np.array_equal(tcq._bits(l_on["losses"]), tcq._bits(on["losses"]))
    r = tcq._restated(c, host, plain["rows"])
    W = r["dout"].shape[-1]
    lo, hi = A * W, (1 + K) * A * W
    t64, bound = r["dout"].reshape(B, K * A * W), r["bound"].reshape(B, K * A * W)
    want = plain["dout"][:, lo:hi].astype(np.float64) + t64
    tol = bound + U * np.abs(want)
    err = np.abs(on["dout"][:, lo:hi].astype(np.float64) - want)
    print(f"{case.id} {loss}: worst |dout - restated| / bound = {(err / np.maximum(tol, 1e-300)).max():.3f}")
    assert (err <= tol).all(), f"dout off the restatement by {(err / np.maximum(tol, 1e-300)).max():.2f} bounds"
    if A > 1:  # (one action: logsumexp_a Q - Q_a is 0 and so is the increment)
        # the restatement alone is far outside the bound in every (transition, pair): a build that ignores the term cannot pass
        assert (np.abs(r["dout"]) > 100.0 * r["bound"]).reshape(B, K, -1).any(-1).all()
    else:
        assert (r["dout"] == 0).all() and np.abs(r["loss"]).max() < 1e-12
    outside = np.ones(plain["dout"].shape[1], bool)  # (the padding columns of the pitch included)
    outside[lo:hi] = False
    assert np.array_equal(tcq._bits(on["dout"][:, outside]), tcq._bits(plain["dout"][:, outside])), "a column outside the regressed heads moved"
    want_dbh = want.sum(0)
    tol_dbh = tol.sum(0) + (B + 2) * U * np.abs(want).sum(0)
    err_dbh = np.abs(on["dbh"][lo:hi].astype(np.float64) - want_dbh)
    assert (err_dbh <= tol_dbh).all(), f"dbh off by {(err_dbh / np.maximum(tol_dbh, 1e-300)).max():.2f} bounds"
    w = b.weights.astype(np.float64)
    want_l = plain["losses"][:K].astype(np.float64) + r["loss"]
    terms = ALPHA * w[:, None] * np.abs(r["c"]) / B
    tol_l = (ALPHA * w[:, None] / B * r["c_bound"]).sum(0) + (B + 4) * U * (np.abs(plain["losses"][:K]) + terms.sum(0))
    err_l = np.abs(on["losses"][:K].astype(np.float64) - want_l)
    print(f"{case.id} {loss}: losses worst error / bound {(err_l / tol_l).max():.3f}")
    assert (err_l <= tol_l).all(), (err_l, tol_l)


@pytest.mark.parametrize("loss", VARIANT_LOSSES)
@pytest.mark.parametrize("case", VARIANTS)
def test_loss_only_and_gradient_only_calls(case, loss):
    """loss_on_batch (no dout) and grad_on_batch from the same parameters give the losses, q_values and targets of learn_on_batch bit for
    bit; the gradient-only call's dout and head-bias gradient against the helper."""
    eng, _ = _case_engine(case, loss)
    b = _Batch(eng, case.B, case.A)
    outs = []
    g = torch.zeros_like(eng.params)
    for call in ("loss", "grad", "learn"):
        if call == "loss":
            losses = _cpu(eng.loss_on_batch(b.cb))
            torch.cuda.synchronize()
            check_call(eng, b, losses, priorities=False, dout=False, tag=f"{case.id} {loss} loss-only")
        elif call == "grad":
            losses = _cpu(eng.grad_on_batch(b.cb, g))
            torch.cuda.synchronize()
            check_call(eng, b, losses, priorities=False, grad=g, tag=f"{case.id} {loss} gradient-only")
        else:
            losses = _cpu(eng.learn_on_batch(b.cb))
            torch.cuda.synchronize()
        outs.append((losses, _cpu(eng.q_values), _cpu(eng.targets)))
    for other in outs[:2]:
        for x, y in zip(other, outs[2]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))


@pytest.mark.parametrize("loss", VARIANT_LOSSES)
def test_a_call_on_fewer_heads_than_k_takes_four_rows_again(loss):
    """The analysis gradients name their pairs: one pair of r3-ragged's engine has K * nb = 256 and R = 4, B = 5 in workgroups of 4 + 1,
    while the row pitch, the head offsets and the partial rows stay those of the 10-head engine."""
    case = hg.BY_ID["r3-ragged"]
    on0, tg0, n = (1, 0, 1) if loss.startswith("qr") else (2, 1, 1)  # (the quantile checker's atoms are those of value heads 0 ..)
    assert case.R == 3 and hg.rows_per_wg(n, case.nb) == 4
    eng, _ = _case_engine(case, loss)
    b = _Batch(eng, case.B, case.A)
    g = torch.zeros_like(eng.params)
    losses = _cpu(eng.grad_on_batch(b.cb, g, online_head=on0, target_head=tg0, n_pairs=n))
    torch.cuda.synchronize()
    check_call(eng, b, losses, K=n, on0=on0, tg0=tg0, priorities=False, grad=g, tag=f"r3-ragged {loss} pair ({on0}, {tg0})")


@pytest.mark.parametrize("loss", VARIANT_LOSSES)
@pytest.mark.parametrize("case", VARIANTS)
def test_two_learn_steps_are_bit_identical_from_identical_state(case, loss):
    runs = []
    for _ in range(2):
        eng, _ = _case_engine(case, loss, seed=1)
        b = _Batch(eng, case.B, case.A, seed=3)
        ls = [eng.learn_on_batch(b.cb).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.stack(ls), eng.priorities.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert torch.isfinite(runs[0][3]).all() and int(eng.adam_count.item()) == 2


# ------------------------------------------------------------------ 3. HL-Gauss over bin counts, sigma and support edges
GK, GA, GB = hg.GRID_K, hg.GRID_A, hg.GRID_B
GRID = [pytest.param(g, id=g[0]) for g in hg.grid_cases()]


class _GridBatch(_Batch):
    """B = 7 with rewards and terminals set by hand: rows 0 / 1 terminal with the reward exactly v_min / v_max; rows 2 / 3 not terminal and
    30 beyond each end; row 4 terminal with the reward on an interior edge; row 5 terminal on a bin centre (both the float32 nearest:
    exact on grid A); row 6 not terminal with a random reward in (0.2, 0.3) x the support's width -- positive, as the bootstrap values
    max_a Q are here (the bias bumps put the best action above the centre 0): r + g max Q cannot cancel to a target near zero, where a
    float32 sum of two terms of size 4 has no relative precision left for rtol to hold (tests/test_gpu_double_q.py, HIST_POS)."""

    def __init__(self, eng, nb, seed=5):
        vmin, vmax = eng.support
        self.edge = np.float32(hl.edges(nb, vmin, vmax).numpy()[nb // 2 + (1 if nb > 2 else 0)])
        self.centre = np.float32(hl.centres(nb, vmin, vmax).numpy()[nb // 3])
        r6 = np.random.default_rng(seed + 200).uniform(0.2, 0.3) * (vmax - vmin)
        hand = (np.array([1, 1, 0, 0, 1, 1, 0], np.uint8), np.array([vmin, vmax, vmin - 30.0, vmax + 30.0, self.edge, self.centre, r6], np.float32))
        super().__init__(eng, GB, GA, seed, hand=hand)


def _grid_engine(nb, vmin, vmax, ratio, seed=0, **kw):
    eta = (vmax - vmin) / nb
    return _engine(GK, GA, nb, GB, "hl", support=(vmin, vmax), sigma=ratio * eta, seed=seed, **kw)


@pytest.mark.parametrize("grid", GRID)
def test_hl_gauss_per_lane_arithmetic(grid):
    """q_values, targets and priorities at the project's tolerance; losses and dout against the helper given y = the device's own float32
    targets, within 8 x the difference between the helper's float32 and float64 evaluations of the same inputs on the CPU (floor: the
    project's atol 1e-7) -- the bound comes from the CPU alone, never from the device's figures."""
    gid, vmin, vmax, nb, ratio = grid
    eng, _ = _grid_engine(nb, vmin, vmax, ratio)
    b = _GridBatch(eng, nb)
    assert hg.rows_per_wg(GK, nb) == 4
    losses = _cpu(eng.learn_on_batch(b.cb))
    torch.cuda.synchronize()
    rows = _rows(eng, GB)
    args = (b.action, b.reward, b.terminal, float(eng.cfg.gamma_n), GK, 1, 0, GA, nb, vmin, vmax, eng.hl_sigma)
    ref = hl.hl_loss(rows, *args, weights=b.weights)
    t = ref["targets"].numpy()
    # the targets are all of: exactly v_min, exactly v_max, beyond each end, on an interior edge, on a bin centre
    assert (t[0] == vmin).all() and (t[1] == vmax).all() and (t[2] < vmin - 10).all() and (t[3] > vmax + 10).all()
    assert (t[4] == float(b.edge)).all() and (t[5] == float(b.centre)).all() and vmin < float(b.edge) < vmax
    if vmin == -8.0:  # grid A: the edge and the centre are exact
        eta = (vmax - vmin) / nb
        assert ((float(b.edge) - vmin) / eta) % 1 == 0 and ((float(b.centre) - vmin) / eta) % 1 == 0.5
    _gap_holds(eng, rows, GK, 1, 0, False)
    _close(eng.q_values.cpu(), ref["q"])
    _close(eng.targets.cpu(), ref["targets"])
    _close(eng.priorities.cpu(), ref["priorities"])
    dev_t = eng.targets.double().cpu()
    assert torch.equal(dev_t[[0, 1, 4, 5]], ref["targets"][[0, 1, 4, 5]])  # a terminal row's target is its reward, bit for bit
    r64 = hl.hl_loss(rows, *args, weights=b.weights, y=dev_t)
    r32 = hl.hl_loss(rows.float(), *args, weights=b.weights, y=dev_t.float(), dtype=torch.float32)
    n, _ = _widths(eng)
    dout = _dout(eng, GB)[:, :n]
    cpu_l = float((r32["losses"].double() - r64["losses"]).abs().max())
    cpu_d = float((r32["dlogits"].double() - r64["dlogits"]).abs().max())
    dev_l = float(np.abs(losses.astype(np.float64) - r64["losses"].numpy()).max())
    dev_d = float(np.abs(dout - r64["dlogits"].numpy()).max())
    _note(test="grid", case=gid, R=4, workgroups=hg.workgroups(GB, 4), cpu_f32_vs_f64=dict(losses=cpu_l, dout=cpu_d), device=dict(losses=dev_l, dout=dev_d),
          bound=dict(losses=max(8 * cpu_l, 1e-7), dout=max(8 * cpu_d, 1e-7)))
    assert dev_l <= max(8 * cpu_l, 1e-7), (dev_l, cpu_l)
    assert dev_d <= max(8 * cpu_d, 1e-7), (dev_d, cpu_d)


@pytest.mark.parametrize("grid", GRID)
def test_hl_gauss_dout_of_a_pair_sums_to_zero(grid):
    """Softmax and projection both sum to one: each (row, pair)'s nb entries of dout sum to zero within nb x 2^-23 x the largest |entry|
    of that (row, pair).

    At two bins both histograms are near 1/2 and may nearly agree: float32 roundings of softmax_j and of p_j (2^-24 of 1/2 each) would be
    several times this bound, which is relative to their difference.  hl_loss_kernel therefore forms the difference in double, each
    histogram over the double sum of its own float32 terms, and rounds it once (csrc/hl_gauss.h)."""
    gid, vmin, vmax, nb, ratio = grid
    eng, _ = _grid_engine(nb, vmin, vmax, ratio)
    b = _GridBatch(eng, nb)
    eng.learn_on_batch(b.cb)
    torch.cuda.synchronize()
    n, _ = _widths(eng)
    dout = _dout(eng, GB)[:, :n]
    blocks = dout.reshape(GB, GK + 1, GA, nb)[np.arange(GB)[:, None], 1 + np.arange(GK)[None, :], b.action[:, None].astype(np.int64)]  # [B, K, nb]
    sums, largest = np.abs(blocks.sum(-1)), np.abs(blocks).max(-1)
    worst = float((sums / (nb * 2.0 ** -23 * largest)).max())
    _note(test="sum-to-zero", case=gid, worst_sum_over_bound=worst, worst_sum=float(sums.max()))
    assert (largest > 0).all() and (sums <= nb * 2.0 ** -23 * largest).all(), worst


@pytest.mark.parametrize("nb", hg.grid_bin_counts())
def test_hl_expectations_forward_and_acting_at_every_bin_count(nb):
    """hl_expect_kernel: eng.forward's Q rows against the expectations of the device's logits, best_actions / best_action against their
    first argmax (tests/test_gpu_hl_gauss.py's tolerances)."""
    vmin, vmax = ((-8.0, 8.0) if nb in hg.GRID_EXACT[1] else (-10.0, 10.0))
    eng, _ = _grid_engine(nb, vmin, vmax, 0.75, seed=6)
    b = _Batch(eng, GB, GA, seed=21)
    q = eng.forward(n_rows=GB, obs=b.x_state.cuda()).double().cpu()
    torch.cuda.synchronize()
    ex = hl.expectations(_rows(eng, GB)[:GB], nb, vmin, vmax)
    assert q.shape == (GB, (1 + GK) * GA)
    _close(q, ex, rtol=1e-5, atol=1e-6)
    idx = torch.tensor([i % GK for i in range(GB)], dtype=torch.int32, device="cuda")
    acts = eng.best_actions(idx_networks=idx, obs=b.x_state.cuda()).cpu().numpy()
    for i in range(GB):
        row = ex[i].reshape(1 + GK, GA)[1 + i % GK]
        top = torch.sort(row, descending=True).values
        assert float(top[0] - top[1]) >= 1e-4  # (the bias bumps separate the actions: no row is left out)
        assert acts[i] == int(row.argmax())
        assert int(eng.best_action(idx_network=i % GK, obs=b.x_state[i : i + 1].cuda()).item()) == int(row.argmax())


def _tie_params(K, A, nb, vmin, vmax, tied_heads, seed=4):
    """Parameters in which actions 1 and 2 of every head in ``tied_heads`` have identical kernel columns and bias (bit-equal logits) and
    lead action 0, whose bias puts its mass on the lowest bins; in every other head action 2 leads action 1 leads action 0."""
    n_heads = K + 1
    p = perturbed_params(seed, FC_OBS, FEATS, "fc", n_heads * A * nb, True)
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in p.items()}
    c = hl.centres(nb, vmin, vmax).numpy()
    s = (vmax - vmin) / 6.0
    kern = p[HEAD]["kernel"].reshape(FEATS[-1], n_heads, A, nb)
    bias = p[HEAD]["bias"].reshape(n_heads, A, nb)
    mid = 0.5 * (vmin + vmax)
    for h in range(n_heads):
        for a, mu in enumerate((mid - 3.0, mid + 1.0, mid + 3.0)):
            bias[h, a] += (-((c - mu) ** 2) / (2.0 * s * s)).astype(np.float32)
        if h in tied_heads:
            kern[:, h, 2] = kern[:, h, 1]
            bias[h, 2] = bias[h, 1]
    return p


@pytest.mark.parametrize("nb", [65, 256])
def test_the_lower_index_wins_a_tie_everywhere(nb):
    """K = 3, A = 3, heads 1 and 3 tied between actions 1 and 2 (bit-equal logits, asserted on the device's rows).  Head 3 is the
    selector of pair 2, whose value head 2 tells the two actions apart: a* = 1 shows in the target.  Head 1 is the value head of pair 1:
    the plain max and the Munchausen soft value run over the tie.  Acting on heads 1 and 3 returns action 1."""
    K, A, B = 3, 3, GB
    vmin, vmax = hg.dyadic_support(nb)
    params = _tie_params(K, A, nb, vmin, vmax, tied_heads=(1, 3))
    g = 0.99
    for mode in ("max", "double_q", "munchausen"):
        kw = dict(double_q=True) if mode == "double_q" else dict(tm.MU) if mode == "munchausen" else {}
        eng, _ = _engine(K, A, nb, B, "hl", params=params, **kw)
        b = _Batch(eng, B, A)
        if mode == "max":  # acting first: the learn step below moves the tied columns apart (only the taken action has a gradient)
            for i in range(B):
                assert int(eng.best_action(idx_network=0, obs=b.x_state[i : i + 1].cuda()).item()) == 1  # head 1
                assert int(eng.best_action(idx_network=2, obs=b.x_state[i : i + 1].cuda()).item()) == 1  # head 3
                assert int(eng.best_action(idx_network=1, obs=b.x_state[i : i + 1].cuda()).item()) == 2  # head 2: no tie
            idx = torch.tensor([0, 2, 1, 2, 0, 1, 2], dtype=torch.int32, device="cuda")
            acts = eng.best_actions(idx_networks=idx, obs=b.x_state.cuda()).cpu().numpy()
            assert np.array_equal(acts, np.where(idx.cpu().numpy() == 1, 2, 1))
        losses = _cpu(eng.learn_on_batch(b.cb))
        torch.cuda.synchronize()
        rows = _rows(eng, B)
        blocks = rows.reshape(2 * B, K + 1, A, nb)
        for h in (1, 3):
            assert torch.equal(blocks[:, h, 1], blocks[:, h, 2])  # the tie is exact on the device
        ex = hl.expectations(rows, nb, vmin, vmax).reshape(2 * B, K + 1, A)
        assert (ex[:, :, 0] < ex[:, :, 1] - 1e-2).all() and (ex[:, [0, 2], 1] < ex[:, [0, 2], 2] - 1e-2).all()
        nt = 1.0 - b.terminal.astype(np.float64)
        dev_t = eng.targets.double().cpu().numpy()
        if mode == "max":
            check_call(eng, b, losses, tag=f"tie nb={nb} max", gap=False)
        elif mode == "double_q":
            ref = check_call(eng, b, losses, selector=True, tag=f"tie nb={nb} double_q", gap=False)
            # pair 2: value head 2 at a* = 1, not at its own (and the higher tied index's) action 2
            _close(dev_t[:, 2], b.reward + nt * g * ex[B:, 2, 1].numpy())
            assert (np.abs(dev_t[:, 2] - (b.reward + nt * g * ex[B:, 2, 2].numpy()))[nt > 0] > 1e-2).all()
            np.testing.assert_allclose(ref["targets"].numpy()[:, 2], b.reward + nt * float(eng.cfg.gamma_n) * ex[B:, 2, 1].numpy(), rtol=1e-13)
        else:
            ref = tm._ref(eng, rows, b, hist=dict(nb=nb, vmin=vmin, vmax=vmax, sigma=SIGMA))
            tm._check_targets(dev_t, ref, f"tie nb={nb} ")
            _close(eng.q_values.cpu(), ref["q"])


@pytest.mark.parametrize("nb", [130, 256])
def test_munchausen_targets_at_three_and_four_groups_per_lane(nb):
    """tests/test_gpu_munchausen.py's checks of the histogram form (its bounds, imported), once each at nb = 130 and nb = 256."""
    K, A, B = 2, 3, GB
    vmin, vmax = hg.dyadic_support(nb)
    hist = dict(nb=nb, vmin=vmin, vmax=vmax, sigma=SIGMA)
    eng, _ = _engine(K, A, nb, B, "hl", support=(vmin, vmax), seed=2, **tm.MU)
    b = _Batch(eng, B, A)
    for learn in (False, True):
        losses = _cpu(eng.learn_on_batch(b.cb) if learn else eng.loss_on_batch(b.cb))
        torch.cuda.synchronize()
        ref = tm._ref(eng, _rows(eng, B), b, hist=hist)
        assert (np.abs(ref["targets"] - ref["max_targets"]) > 100 * tm.TARGET_BOUND * ref["scale"]).any()  # the option changes these targets
        tm._check_targets(eng.targets.cpu(), ref, f"nb={nb} ")
        _close(eng.q_values.cpu(), ref["q"])
        tm._behind(losses, ref["losses"], ref)
        if learn:
            tm._behind(eng.priorities.cpu(), ref["priorities"], ref)
            dy = 4 * 2.0 ** -23 * vmax + tm.TARGET_BOUND * float(ref["scale"].max())
            n, _ = _widths(eng)
            d = _dout(eng, B)
            assert (d[:, n:] == 0).all()
            tm._close(d[:, :n], ref["dq"], atol=tm.ATOL + dy / (SIGMA * np.sqrt(2 * np.pi)) / B)


# ------------------------------------------------------------------ 4. the widest row
WIDEST = hg.BY_ID["r3-widest"]


def _oracle_rows(params, b, requires_grad=False):
    pt = onet.to_torch(params, torch.float64, requires_grad=requires_grad)
    on, nx = onet.forward(pt, b.x_state, FEATS, "fc", True), onet.forward(pt, b.x_next, FEATS, "fc", True)
    return pt, torch.cat([on, nx.detach() if requires_grad else nx])


def test_widest_row_forward_and_acting_against_the_float64_oracle():
    """5456 outputs: dense_post_kernel stages three rows in 64 KB of LDS."""
    case = WIDEST
    assert case.row == hg.MAX_ROW
    eng, params = _case_engine(case, "hl", seed=6)
    b = _Batch(eng, case.B, case.A, seed=21)
    vmin, vmax = eng.support
    _, rows = _oracle_rows(params, b)
    qo = hl.expectations(rows[: case.B], case.nb, vmin, vmax)
    q = eng.forward(n_rows=case.B, obs=b.x_state.cuda()).double().cpu()
    torch.cuda.synchronize()
    t = TOL["bf16x3"]["q"]
    scale = max(1.0, float(qo.abs().max()))
    print(f"widest row: forward |q - oracle| / scale {float((q - qo).abs().max()) / scale:.2e} (bound {t:.0e})")
    assert q.shape == qo.shape and float((q - qo).abs().max()) < t * scale
    ex = hl.expectations(_rows(eng, case.B)[: case.B], case.nb, vmin, vmax)
    _close(q, ex, rtol=1e-5, atol=1e-6)  # and hl_expect_kernel on the device's own logits
    idx = torch.tensor([i % case.K for i in range(case.B)], dtype=torch.int32, device="cuda")
    acts = eng.best_actions(idx_networks=idx, obs=b.x_state.cuda()).cpu().numpy()
    for i in range(case.B):
        row = qo[i].reshape(case.n_heads, case.A)[1 + i % case.K]
        assert abs(float(row[0] - row[1])) > 10 * t * scale  # no argmax of the oracle can flip within the forward's bound
        assert acts[i] == int(row.argmax())
        assert int(eng.best_action(idx_network=i % case.K, obs=b.x_state[i : i + 1].cuda()).item()) == int(row.argmax())


def test_widest_row_learn_step_gradients_against_the_float64_oracle():
    case = WIDEST
    eng, params = _case_engine(case, "hl", seed=4)
    b = _Batch(eng, case.B, case.A, seed=13)
    g = torch.zeros_like(eng.params)
    eng.learn_on_batch(b.cb, grad_out=g)
    torch.cuda.synchronize()
    hip_g = eng.internal_to_flax_grads(g)
    pt, rows = _oracle_rows(params, b, requires_grad=True)
    vmin, vmax = eng.support
    ref = hl.hl_loss(rows, b.action, b.reward, b.terminal, float(eng.cfg.gamma_n), case.K, 1, 0, case.A, case.nb, vmin, vmax, SIGMA, weights=b.weights)
    ref["losses"].sum().backward()
    for mod in pt:
        for leaf, t in pt[mod].items():
            want = t.grad.numpy()
            got = np.asarray(hip_g[mod][leaf], np.float64)
            e = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
            print(f"widest row: grad {mod}/{leaf}: norm-rel {e:.2e} (bound {TOL['bf16x3']['grad']:.0e})")
            assert e <= TOL["bf16x3"]["grad"], (mod, leaf, e)


@pytest.mark.parametrize("loss, message", [
    pytest.param("hl", r"histogram heads: n_heads \* n_actions \* n_bins must be <= 5456", id="hl"),
    pytest.param("c51", r"histogram heads: n_heads \* n_actions \* n_bins must be <= 5456", id="c51"),
    pytest.param("qr-huber", r"quantile heads: n_heads \* n_actions \* n_quantiles must be <= 5456", id="qr"),
])
def test_one_output_beyond_the_widest_row_is_refused_through_the_engine(loss, message):
    assert 11 * 2 * 249 > hg.MAX_ROW >= 11 * 2 * 248
    params = types.SimpleNamespace()  # (never imported: the engine refuses before it allocates)
    with pytest.raises(NotImplementedError, match=message):
        _engine(10, 2, 249, 4, loss, params=params)
