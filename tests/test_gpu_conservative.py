"""The conservative (CQL) term on the device (include/isdqn_hip.h, isdqn_batch_conservative) against the float64 restatement of
tests/helpers/conservative.py applied to the device's own head-output rows, through every layer up to the agents and the flag.

Sites (the shapes of tests/test_gpu_adamw.py, the smallest at which the term's kernels can go wrong):
  fc-a4     8 -> 100 -> 100, A = 4, K = 1, B = 33: ragged against the 64 transitions of a workgroup
  fc-a5     A = 5, K = 2, B = 32: 15 columns in a pitch of 16
  fc-a18    A = 18, K = 9, B = 5
  fc-qr51 / fc-qr65   quantile heads, N = 51 and 65 (two lane groups), K = 2, B = 5: ragged against the R = 4 transitions of a workgroup
  fc-hl51 / fc-c51    histogram heads, 51 bins on [-10, 10], HL-Gauss and categorical, K = 2, B = 5
  fc-duel   8 -> 20 -> 14 with dueling heads: the rows behind the combine
  cnn-bn / impala     84 x 84 x 4, (8, 8, 8, 16), B = 4
  cnn       (32, 64, 64, 512), K = 9, A = 9, B = 32, once
Every site's loss weights hold one zero and one weight above 1.

THE BOUND of an element of the increment t of dL/d(output) (and so of dout_new = fl32(dout_old + t)), derived, never taken from what
the device returned.  The definition runs conservative.op_count(kind, A, W) float32 operations on the way to t (counted there, one by
one), each within u = 2^-24 relative of a quantity that is at most (1 + S) times the element's own scale alpha w_b / B max|dQ/d(output)|,
S being the largest magnitude an action value of the pair is formed from -- |Q_a| on scalar heads, |theta| on quantile heads, the
support's |z_j| and the logits' spread on histogram heads (the exponent's rounding enters pi multiplied by it).  So

    |t_device - t_64| <= op_count u (1 + S) alpha w_b / B max|dQ/d(output)|,   and   |dout_new - (dout_old + t_64)| <= that + u |dout_new|.

A row of weight 0 has bound 0 + the sum's rounding, and the device adds an exact 0 there.  The head-bias gradient sums B such elements
in float32: the sum of their bounds plus (B + 2) u sum_b |dout_new|.  A loss sums B terms alpha w_b c_bk / B, c within op_count u (1 + S),
plus (B + 4) u of the sum of the (non-negative) terms."""
import ctypes
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import conservative as hc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ALPHA = 0.7
FC = dict(obs=(8,), feats=(100, 100), arch="fc")
HIST = dict(n_bins=51, min_value=-10.0, max_value=10.0, sigma=0.3)
SITES = {
    "fc-a4": dict(FC, K=1, A=4, B=33),
    "fc-a5": dict(FC, K=2, A=5, B=32),
    "fc-a18": dict(FC, K=9, A=18, B=5),
    "fc-qr51": dict(FC, K=2, A=4, B=5, kw=dict(n_quantiles=51, huber_delta=1.0)),
    "fc-qr65": dict(FC, K=2, A=4, B=5, kw=dict(n_quantiles=65, huber_delta=1.0)),
    "fc-hl51": dict(FC, K=2, A=4, B=5, kw=dict(HIST)),
    "fc-c51": dict(FC, K=2, A=4, B=5, kw=dict(HIST, categorical=True)),
    "fc-duel": dict(obs=(8,), feats=(20, 14), arch="fc", K=2, A=4, B=32, kw=dict(dueling=True)),
    "cnn-bn": dict(obs=(84, 84, 4), feats=(8, 8, 8, 16), arch="cnn", K=2, A=5, B=4, kw=dict(batch_norm=True)),
    "impala": dict(obs=(84, 84, 4), feats=(8, 8, 8, 16), arch="impala", K=2, A=5, B=4),
    "cnn": dict(obs=(84, 84, 4), feats=(32, 64, 64, 512), arch="cnn", K=9, A=9, B=32),
}


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).reshape(-1).view(np.int64 if a.dtype.itemsize == 8 else np.int32 if a.dtype.itemsize == 4 else np.uint8)


def _with_cql(batch, alpha):
    """The caller's side of the C ABI, written out: an isdqn_batch_conservative around the fields of ``batch``, the flag set."""
    from slimdqn import _hip

    b = _hip.BatchConservative()
    for name, _ in _hip.Batch._fields_:
        setattr(b, name, getattr(batch, name))
    b.flags = batch.flags | _hip.BATCH_CONSERVATIVE
    b.cql_alpha = alpha
    b._keep = batch
    return b


def _kind(c):
    kw = c.get("kw", {})
    return "quantile" if kw.get("n_quantiles") else "histogram" if kw.get("n_bins") else "scalar"


@functools.lru_cache(maxsize=None)
def _site(name, n_heads=None, noisy=False):
    from slimdqn._engine import QNetEngine

    c = SITES[name]
    A, B = c["A"], c["B"]
    kw = dict(c.get("kw", {}), **({"noisy": True} if noisy else {}))
    eng = QNetEngine(c["obs"], A, n_heads or 1 + c["K"], c["feats"], c["arch"], True, B, gamma_n=0.99, learning_rate=1e-3,
                     adam_eps=1e-8 if c["arch"] == "fc" else 1.5e-4, **kw)
    eng.init_params(3)
    rng = np.random.default_rng(17)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    w = rng.uniform(0.5, 1.5, B).astype(np.float32)
    w[0], w[1] = 0.0, 1.7
    host = dict(action=rng.integers(0, A, B).astype(np.int32), reward=rng.normal(size=B).astype(np.float32),
                terminal=(rng.random(B) < 0.3).astype(np.uint8), weights=w)
    common = dict(action=dev(host["action"]), reward=dev(host["reward"]), terminal=dev(host["terminal"]), loss_weights=dev(w))
    if c["arch"] == "fc":
        d = c["obs"][0]
        host["state"], host["next_state"] = rng.normal(size=(B, d)).astype(np.float32), rng.normal(size=(B, d)).astype(np.float32)
        batch = eng.make_batch(state=dev(host["state"]), next_state=dev(host["next_state"]), **common)
    else:
        h, wd, stack = c["obs"]
        n_frames = 3 * B + 8
        ids = rng.integers(0, n_frames, (B, 2 * stack)).astype(np.int32)
        ids[rng.random(ids.shape) < 0.1] = -1
        batch = eng.make_batch(frames=dev(rng.integers(0, 256, (n_frames, h * wd), dtype=np.uint8)), frame_stride=h * wd, frame_ids=dev(ids), **common)
    assert type(batch).__name__ == "Batch" and eng.cql_alpha == 0.0
    return eng, batch, host


def _pitch(eng, c):
    """Row pitch of the head-output rows and of "dout": the head layer's width rounded up to 8 (net_plan.h: nlog_p)."""
    W = 1 if _kind(c) == "scalar" else c["kw"].get("n_quantiles") or c["kw"]["n_bins"]
    return -(-eng.n_heads * c["A"] * W // 8) * 8


def _rows(eng, c):
    """The head-output rows of the B states the loss of the last call read, [B, H, A, W] (every head), float64."""
    kind = _kind(c)
    W = 1 if kind == "scalar" else c["kw"].get("n_quantiles") or c["kw"]["n_bins"]
    r = eng.region("q" if kind == "scalar" else "logits").cpu().numpy()
    H = eng.n_heads
    pitch = _pitch(eng, c)
    return r[: 2 * c["B"] * pitch].reshape(2 * c["B"], pitch)[:, : H * c["A"] * W].reshape(2 * c["B"], H, c["A"], W).astype(np.float64)


def _grad_call(eng, c, batch):
    grad = torch.zeros_like(eng.params)
    eng.grad_on_batch(batch, grad)
    torch.cuda.synchronize()
    B = c["B"]
    dout = eng.region("dout").cpu().numpy()
    pitch = _pitch(eng, c)
    out = dict(grad=grad.cpu().numpy(), losses=eng.losses.cpu().numpy().copy(), q_values=eng.q_values.cpu().numpy().copy(),
               targets=eng.targets.cpu().numpy().copy(), dout=dout[: B * pitch].reshape(B, pitch).copy(), dbh=eng.region("dbh").cpu().numpy()[:pitch].copy(),
               rows=_rows(eng, c))
    return out


def _loss_call(eng, batch):
    eng.loss_on_batch(batch)
    torch.cuda.synchronize()
    return dict(losses=eng.losses.cpu().numpy().copy(), q_values=eng.q_values.cpu().numpy().copy(), targets=eng.targets.cpu().numpy().copy())


def _restated(c, host, rows, on0=1):
    kind = _kind(c)
    kw = c.get("kw", {})
    z = hc.support(kw["n_bins"], kw["min_value"], kw["max_value"]) if kind == "histogram" else None
    r = hc.restate(rows[: c["B"], on0 : on0 + c["K"]], host["action"], host["weights"], ALPHA, kind, z)
    # S: the largest magnitude an action value of the pair is formed from
    mine = np.abs(rows[: c["B"], on0 : on0 + c["K"]])
    if kind == "histogram":
        lg = rows[: c["B"], on0 : on0 + c["K"]]
        S = np.maximum(np.abs(z).max(), (lg.max(-1) - lg.min(-1)).max((-1,)))[..., None, None] * np.ones_like(mine)
    else:
        S = mine.max((-1, -2), keepdims=True) * np.ones_like(mine)
    W = mine.shape[-1]
    n = hc.op_count(kind, c["A"], W)
    scale = (ALPHA * host["weights"].astype(np.float64) / c["B"])[:, None, None, None] * np.abs(r["dq"]).max((-1, -2), keepdims=True)
    r["bound"] = n * U * (1.0 + S) * scale                                                         # [B, K, A, W]
    r["c_bound"] = n * U * (1.0 + S[..., 0, 0])                                                    # [B, K]
    return r


@pytest.mark.parametrize("name", list(SITES))
def test_the_term_is_the_restatement_on_the_devices_own_rows(name):
    """Checks 1 to 3.  loss_on_batch and grad_on_batch without the flag, with the flag at alpha = 0 and at alpha = 0.7: the flag at 0 is
    the call without it in every output and in the regions "dout" and "dbh", bit for bit; at 0.7, q_values and targets keep their bits;
    "dout", "dbh" and losses are the alpha = 0 values plus the restatement's increments within THE BOUND of the module docstring; the
    restatement's increment is far outside the bound on every regressed head (on the restatement alone: a build that ignores the option
    cannot pass); a second call at 0.7 returns the bits of the first."""
    c = SITES[name]
    eng, batch, host = _site(name)
    B, K, A = c["B"], c["K"], c["A"]
    plain, zero, on, again = (_grad_call(eng, c, b) for b in (batch, _with_cql(batch, 0.0), _with_cql(batch, ALPHA), _with_cql(batch, ALPHA)))
    for n in plain:
        assert np.array_equal(_bits(zero[n]), _bits(plain[n])), f"{name}: {n} with the flag at 0 is not the call without the flag"
        assert np.array_equal(_bits(again[n]), _bits(on[n])), f"{name}: {n} differs between two calls at alpha = {ALPHA}"
    for n in ("q_values", "targets", "rows"):
        assert np.array_equal(_bits(on[n]), _bits(plain[n])), f"{name}: {n} moved with the term"
    l_plain, l_zero, l_on = _loss_call(eng, batch), _loss_call(eng, _with_cql(batch, 0.0)), _loss_call(eng, _with_cql(batch, ALPHA))
    for n in l_plain:
        assert np.array_equal(_bits(l_zero[n]), _bits(l_plain[n])) and np.array_equal(_bits(l_plain[n]), _bits(plain[n])), (name, n)
    assert np.array_equal(_bits(l_on["losses"]), _bits(on["losses"])) and np.array_equal(_bits(l_on["q_values"]), _bits(plain["q_values"]))
    assert np.array_equal(_bits(l_on["targets"]), _bits(plain["targets"]))

    r = _restated(c, host, plain["rows"])
    W = r["dout"].shape[-1]
    lo, hi = A * W, (1 + K) * A * W  # the regressed heads' columns (online heads 1 .. K)
    t64 = r["dout"].reshape(B, K * A * W)
    bound = r["bound"].reshape(B, K * A * W)
    # the restatement alone: far outside the bound on every regressed head -- more than 100 bounds on at least a third of each head's
    # elements (a histogram head's dQ/dlogit vanishes on the bins beside Q_a and wherever the softmax puts no mass)
    per_head = (np.abs(r["dout"]) > 100.0 * r["bound"]).reshape(B, K, -1)[host["weights"] > 0].mean((0, 2))
    assert (per_head > 1.0 / 3.0).all(), f"{name}: the increment is within 100 bounds on most of some head: {per_head}"
    want = plain["dout"][:, lo:hi].astype(np.float64) + t64
    tol = bound + U * np.abs(want)
    err = np.abs(on["dout"][:, lo:hi].astype(np.float64) - want)
    print(f"{name}: worst |dout - restated| / bound = {(err / np.maximum(tol, 1e-300)).max():.3f}, op_count {hc.op_count(_kind(c), A, W)}")
    assert (err <= tol).all(), f"{name}: dout off the restatement by {(err / np.maximum(tol, 1e-300)).max():.2f} bounds"
    # (values, not bits: the loss kernels leave -0 where a negative derivative met the weight 0, and fl32(-0 + +0) is +0)
    assert np.array_equal(on["dout"][host["weights"] == 0], plain["dout"][host["weights"] == 0]), "a row of weight 0 moved"
    outside = np.ones(plain["dout"].shape[1], bool)  # (the padding columns of the pitch included)
    outside[lo:hi] = False
    assert np.array_equal(_bits(on["dout"][:, outside]), _bits(plain["dout"][:, outside])), f"{name}: a column outside the regressed heads moved"
    want_dbh = want.sum(0)
    tol_dbh = tol.sum(0) + (B + 2) * U * np.abs(want).sum(0)
    err_dbh = np.abs(on["dbh"][lo:hi].astype(np.float64) - want_dbh)
    assert (err_dbh <= tol_dbh).all(), f"{name}: dbh off by {(err_dbh / np.maximum(tol_dbh, 1e-300)).max():.2f} bounds"
    assert (np.abs(r["dbh"].reshape(-1)) > 10.0 * tol_dbh).mean() > 0.5
    w = host["weights"].astype(np.float64)
    want_l = plain["losses"][:K].astype(np.float64) + r["loss"]
    terms = ALPHA * w[:, None] * np.abs(r["c"]) / B
    tol_l = (ALPHA * w[:, None] / B * r["c_bound"]).sum(0) + (B + 4) * U * (np.abs(plain["losses"][:K]) + terms.sum(0))
    err_l = np.abs(on["losses"][:K].astype(np.float64) - want_l)
    print(f"{name}: losses {on['losses'][:K]} (alpha = 0: {plain['losses'][:K]}), worst error / bound {(err_l / tol_l).max():.3f}")
    assert (err_l <= tol_l).all() and (np.abs(r["loss"]) > 100.0 * tol_l).all(), (name, err_l, tol_l)


# ---------------------------------------------------------------------------------------------------------------- check 4: float64 autograd
def _torch_model(eng, host, c, rows, targets, alpha, on0=1):
    """The fc network from export_flax in float64 (Dense -> LayerNorm (eps 1e-6, fast variance) -> ReLU, twice, then the head) and
    sum_k (1 / B) sum_b w_b (l_bk + alpha c_bk) with the device's targets / target atoms as constants; returns the leaf gradients."""
    P = {m: {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in leaves.items()} for m, leaves in eng.export_flax().items()}
    x = torch.tensor(host["state"], dtype=torch.float64)
    for i in range(2):
        x = x @ P[f"Dense_{i}"]["kernel"] + P[f"Dense_{i}"]["bias"]
        mean, mean2 = x.mean(-1, keepdim=True), (x * x).mean(-1, keepdim=True)
        x = (x - mean) * (torch.rsqrt(torch.clamp(mean2 - mean * mean, min=0.0) + 1e-6) * P[f"LayerNorm_{i}"]["scale"]) + P[f"LayerNorm_{i}"]["bias"]
        x = torch.relu(x)
    out = x @ P["Dense_2"]["kernel"] + P["Dense_2"]["bias"]
    B, K, A = c["B"], c["K"], c["A"]
    kind = _kind(c)
    W = 1 if kind == "scalar" else c["kw"]["n_quantiles"]
    th = out.reshape(B, eng.n_heads, A, W)[:, on0 : on0 + K]
    q = th.mean(-1)
    act = torch.tensor(host["action"].astype(np.int64))
    w = torch.tensor(host["weights"], dtype=torch.float64)
    idx = act[:, None, None].expand(B, K, 1)
    qa = q.gather(2, idx)[..., 0]
    if kind == "scalar":
        l = (qa - torch.tensor(targets, dtype=torch.float64)) ** 2
    else:  # quantile Huber loss, kappa = 1, against the target atoms built from the device's own next-state rows
        nxt = rows[B:, 0:K]  # value heads 0 .. K - 1 on the next states, [B, K, A, N]
        best = nxt.mean(-1).argmax(-1)
        atoms = np.take_along_axis(nxt, best[..., None, None].repeat(W, -1), 2)[:, :, 0]
        disc = (1.0 - host["terminal"].astype(np.float64)) * 0.99
        t = torch.tensor(host["reward"].astype(np.float64)[:, None, None] + disc[:, None, None] * atoms)  # [B, K, N]
        tha = th.gather(2, act[:, None, None, None].expand(B, K, 1, W))[:, :, 0]  # [B, K, N]
        u = t[:, :, None, :] - tha[:, :, :, None]  # [B, K, i, j]
        tau = ((torch.arange(W, dtype=torch.float64) + 0.5) / W)[None, None, :, None]
        hub = torch.where(u.abs() <= 1.0, 0.5 * u * u, u.abs() - 0.5)
        l = ((tau - (u < 0).double()).abs() * hub).sum((-1, -2)) / W
    cterm = torch.logsumexp(q, -1) - qa
    loss = ((w[:, None] * (l + alpha * cterm)).sum(0) / B).sum()
    loss.backward()
    return {m: {k: v.grad.numpy() for k, v in leaves.items()} for m, leaves in P.items()}, float(loss.detach())


def _hold_to_autograd(eng, c, host, grad, rows, targets, what):
    from tests.test_gpu_network import TOL, _flat_err

    g = eng.internal_to_flax_grads(torch.from_numpy(grad).cuda() if isinstance(grad, np.ndarray) else grad)
    want, _ = _torch_model(eng, host, c, rows, targets, ALPHA)
    without, _ = _torch_model(eng, host, c, rows, targets, 0.0)
    for mod in want:
        for leaf in want[mod]:
            e = _flat_err(g[mod][leaf], want[mod][leaf])
            print(f"{what} {mod}/{leaf}: rel err {e:.2e}, the term moves the leaf by {_flat_err(without[mod][leaf], want[mod][leaf]):.2e}")
            assert e < TOL["bf16x3"]["grad"], f"{what} grad {mod}/{leaf}: rel err {e}"
    # on the float64 model alone: the term moves the head kernel by several bounds (a quantile head's share is 1 / N per output)
    assert _flat_err(without["Dense_2"]["kernel"], want["Dense_2"]["kernel"]) > 3 * TOL["bf16x3"]["grad"], "the term is within the bound on the head kernel"


@pytest.mark.parametrize("name", ["fc-a5", "fc-qr51"])
def test_the_reduced_gradient_against_float64_autograd(name):
    """Check 4: grad_on_batch at alpha = 0.7 through internal_to_flax_grads against torch float64 autograd of the whole loss, held to
    the leaf-gradient bound tests/test_gpu_network.py applies in bf16x3 (3e-3 of the leaf's maximum)."""
    c = SITES[name]
    eng, batch, host = _site(name)
    on = _grad_call(eng, c, _with_cql(batch, ALPHA))
    _hold_to_autograd(eng, c, host, on["grad"], on["rows"], on["targets"], name)


# ---------------------------------------------------------------------------------------------------------------- check 5: learn steps
STATE = ("params", "adam_m", "adam_v", "adam_count", "losses_accum")


def _snapshot(eng, names=STATE):
    return {n: getattr(eng, n).clone() for n in names}


def _restore(eng, snap):
    for n, t in snap.items():
        getattr(eng, n).copy_(t)


def test_learn_step_with_the_term():
    """Check 5, learn_on_batch and its debug form: parameters move, and not as without the term; the returned gradient obeys check 4's
    bound; adam_count advances by 1; q_values and targets are those of the generic loss path on the same rows (a gradient-only call
    without the flag: the plain learn step of this site runs the head chain, whose head GEMM rounds differently) and the priorities are
    their TD error."""
    c = SITES["fc-a5"]
    eng, batch, host = _site("fc-a5")
    snap = _snapshot(eng)
    try:
        generic = _grad_call(eng, c, batch)
        eng.learn_on_batch(batch)
        plain = _snapshot(eng)
        _restore(eng, snap)
        grad = torch.zeros_like(eng.params)
        eng.learn_on_batch(_with_cql(batch, ALPHA), grad_out=grad)
        torch.cuda.synchronize()
        assert eng.adam_count.item() == snap["adam_count"].item() + 1
        assert not torch.equal(eng.params, snap["params"]) and not torch.equal(eng.params, plain["params"])
        for n in ("q_values", "targets"):
            assert np.array_equal(_bits(getattr(eng, n)), _bits(generic[n])), n
        td2 = (generic["q_values"].astype(np.float64) - generic["targets"]) ** 2
        assert np.allclose(eng.priorities.cpu().numpy(), np.sqrt(td2.mean(1) + 1e-10), rtol=1e-6, atol=0)
        with_grad = eng.params.clone()
        rows, targets = _rows(eng, c), eng.targets.cpu().numpy().copy()
        _restore(eng, snap)
        _hold_to_autograd(eng, c, host, grad, rows, targets, "learn_on_batch_debug")
        eng.learn_on_batch(_with_cql(batch, ALPHA))  # the plain entry point: the bits of its debug form
        assert torch.equal(eng.params, with_grad)
    finally:
        _restore(eng, snap)


def test_target_form_and_noisy_learn_step_with_the_term():
    """Check 5, the DQN form (separate target parameters, one head) and the noisy learn step: parameters move, and not as without the
    term; adam_count advances by 1; the DQN form's q_values, targets and priorities keep the bits of the step without the term; a malformed alpha is ISDQN_ERR_ARG and leaves everything untouched."""
    from slimdqn import _hip

    eng, batch, host = _site("fc-a5", 1)
    target = eng.params.clone()
    snap = _snapshot(eng)
    try:
        eng.learn_on_batch_target(batch, target)
        plain = eng.params.clone()
        outputs = {n: getattr(eng, n).clone() for n in ("q_values", "targets", "priorities")}
        _restore(eng, snap)
        eng.learn_on_batch_target(_with_cql(batch, ALPHA), target)
        assert eng.adam_count.item() == snap["adam_count"].item() + 1
        for n, t in outputs.items():  # (neither step runs the head chain: the bits of the step without the term)
            assert np.array_equal(_bits(getattr(eng, n)), _bits(t)), n
        assert not torch.equal(eng.params, snap["params"]) and not torch.equal(eng.params, plain)
        _restore(eng, snap)
        for bad in (-0.5, float("nan"), float("inf")):
            b = _with_cql(batch, bad)
            args = [_hip.ptr(eng.adam_m), _hip.ptr(eng.adam_v), _hip.ptr(eng.adam_count), ctypes.byref(b), _hip.ptr(eng.losses), _hip.ptr(eng.losses_accum),
                    _hip.ptr(eng.q_values), _hip.ptr(eng.targets), _hip.ptr(eng.priorities), _hip.ptr(eng.workspace), _hip.stream_ptr(eng.device)]
            assert eng.lib.isdqn_net_learn_on_batch(ctypes.byref(eng.cfg), _hip.ptr(eng.params), *args) == _hip.ERR_ARG and "cql_alpha" in _hip.last_error()
            assert eng.lib.isdqn_net_learn_on_batch_target(ctypes.byref(eng.cfg), _hip.ptr(eng.params), _hip.ptr(target), *args) == _hip.ERR_ARG
            with pytest.raises(RuntimeError):
                eng.loss_on_batch(b)
            torch.cuda.synchronize()
            for n in STATE:
                assert torch.equal(getattr(eng, n), snap[n]), (bad, n)
    finally:
        _restore(eng, snap)
    neng, nbatch, _ = _site("fc-a5", None, True)
    names = STATE + ("sigma", "sigma_m", "sigma_v", "noise_count")
    neng.resample_noise()
    nsnap = _snapshot(neng, names)
    try:
        neng._noisy_learn(nbatch, None)
        plain = {n: getattr(neng, n).clone() for n in ("params", "sigma")}
        _restore(neng, nsnap)
        neng._noisy_learn(_with_cql(nbatch, 0.0), None)
        assert torch.equal(neng.params, plain["params"]) and torch.equal(neng.sigma, plain["sigma"])
        _restore(neng, nsnap)
        neng._noisy_learn(_with_cql(nbatch, ALPHA), None)
        assert neng.adam_count.item() == nsnap["adam_count"].item() + 1
        for n in ("params", "sigma"):
            assert not torch.equal(getattr(neng, n), nsnap[n]) and not torch.equal(getattr(neng, n), plain[n]), n
        _restore(neng, nsnap)
        with pytest.raises(RuntimeError):
            neng._noisy_learn(_with_cql(nbatch, -1.0), None)
        torch.cuda.synchronize()
        for n in names:
            assert torch.equal(getattr(neng, n), nsnap[n]), n
    finally:
        _restore(neng, nsnap)


def test_make_batch_builds_the_struct_only_while_the_term_is_on():
    from slimdqn import _hip

    eng, batch, host = _site("fc-a5")
    B = SITES["fc-a5"]["B"]
    fields = dict(state=torch.zeros(B, 8, device="cuda"), next_state=torch.zeros(B, 8, device="cuda"), action=torch.zeros(B, dtype=torch.int32, device="cuda"),
                  reward=torch.zeros(B, device="cuda"), terminal=torch.zeros(B, dtype=torch.uint8, device="cuda"))
    disc = torch.ones(B, device="cuda")
    try:
        eng.set_conservative(ALPHA)
        b = eng.make_batch(mirror_current=True, **fields)
        assert type(b) is _hip.BatchConservative and b.flags == _hip.BATCH_CONSERVATIVE | _hip.BATCH_MIRROR_CURRENT and b.cql_alpha == np.float32(ALPHA)
        assert b.discount is None and b.weight_decay == 0.0 and b.reserved == 0
        b = eng.make_batch(discount=disc, **fields)
        assert b.flags == _hip.BATCH_CONSERVATIVE | _hip.BATCH_DISCOUNT and b.discount == disc.data_ptr()
        eng.set_weight_decay(0.1)
        b = eng.make_batch(**fields)
        assert b.flags == _hip.BATCH_CONSERVATIVE | _hip.BATCH_WEIGHT_DECAY and (b.weight_decay, b.decay_kinds, b.cql_alpha) == (np.float32(0.1), 3, np.float32(ALPHA))
        eng.set_weight_decay(0.0)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                eng.set_conservative(bad)
        assert eng.cql_alpha == ALPHA
        # the engine's own batch computes what the hand-written struct computes
        st, nx, action, reward, terminal = batch._keep[2:7]
        own = _loss_call(eng, eng.make_batch(state=st, next_state=nx, action=action, reward=reward, terminal=terminal, loss_weights=batch._keep[8]))
        hand = _loss_call(eng, _with_cql(batch, ALPHA))
        for n in own:
            assert np.array_equal(_bits(own[n]), _bits(hand[n])), n
    finally:
        eng.set_conservative(0.0)
        eng.set_weight_decay(0.0)
    assert type(eng.make_batch(**fields)) is _hip.Batch


# ---------------------------------------------------------------------------------------------------------------- checks 6 and 7: agents
def _agents(cls, use_graph, **kw):
    from tests.test_gpu_reset import _agent_and_replay

    return _agent_and_replay(cls, use_graph, **kw)


def test_eight_captured_steps_with_the_term_are_eight_eager_steps():
    """Check 6: an 8-step GraphedUpdate of an agent with the term (uniform sampler) ends on the bits of eight eager steps, and not on those
    of an agent without; set_conservative drops the captured steps, which are captured again with the new weight."""
    from slimdqn.networks.isdqn import iSDQN

    (eager, rb_e), (graphed, rb_g), (plain, rb_p) = _agents(iSDQN, False, cql_alpha=ALPHA), _agents(iSDQN, True, cql_alpha=ALPHA), _agents(iSDQN, False)
    for agent, rb in ((eager, rb_e), (graphed, rb_g), (plain, rb_p)):
        agent.learn_steps(8, rb)
    assert eager._graphed is None and graphed._graphed is not None and graphed._graphed.S == 8
    for n in STATE:
        assert torch.equal(getattr(eager._engine, n), getattr(graphed._engine, n)), f"{n} differs between the eager and the captured steps"
    assert not torch.equal(eager._engine.params, plain._engine.params) and eager._engine.adam_count.item() == 8
    g = graphed._graphed
    for agent in (eager, graphed):
        agent._engine.set_conservative(0.25)
    assert g.graph is None  # dropped by the engine
    for agent, rb in ((eager, rb_e), (graphed, rb_g)):
        agent.learn_steps(8, rb)
    assert graphed._graphed is g and g.graph is not None and g.chained[0].cql_alpha == np.float32(0.25)
    for n in STATE:
        assert torch.equal(getattr(eager._engine, n), getattr(graphed._engine, n)), f"{n} differs after the weight changed"


@pytest.mark.parametrize("agent_name", ["iSDQN", "DQN", "TFDQN", "AnalysisDQN", "AnalysisTFDQN"])
def test_agents_take_cql_alpha(agent_name):
    """Check 7: every agent hands cql_alpha to every engine it builds; one update of the three training agents differs from the same
    agent without the term, and a refused value fails before anything is built."""
    from slimdqn import _conservative, _hip

    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    cls = getattr(importlib.import_module(f"slimdqn.networks.{agent_name.lower()}"), agent_name)
    A = 5
    args = (0, (84, 84, 4), A) + ((2,) if agent_name in ("iSDQN", "AnalysisDQN") else ()) + ([8, 12, 16, 24], False)
    args += () if agent_name == "DQN" else (False,)  # (batch_norm: every agent but DQN takes it in front of the torso)
    make = lambda **kw: cls(*args, "cnn", 2e-4, 0.99, 1, 1, 1000, adam_eps=1.5e-4, batch_size=8, **kw)
    with pytest.raises(ValueError) as e:
        make(cql_alpha=-1.0)
    assert str(e.value) == _conservative.CQL_ALPHA_REFUSED
    agent = make(cql_alpha=ALPHA)
    assert agent.cql_alpha == ALPHA and agent._engine.cql_alpha == ALPHA
    if agent_name in ("iSDQN", "DQN", "TFDQN"):
        plain = make()
        assert torch.equal(plain._engine.params, agent._engine.params)
        for a in (plain, agent):
            rb = ReplayBuffer(UniformSamplingDistribution(5), 8, 128, update_horizon=1, gamma=0.99)
            rng = np.random.default_rng(0)
            for _ in range(80):
                term = bool(rng.random() < 0.08)
                rb.add(TransitionElement(rng.integers(0, 256, (84, 84), dtype=np.uint8), int(rng.integers(0, A)), float(rng.choice([-1.0, 0.0, 1.0])), term, term))
            a.update_online_params(0, rb)
        torch.cuda.synchronize()
        assert type(agent._graphed.chained[0]) is _hip.BatchConservative and type(plain._graphed.chained[0]) is _hip.Batch
        assert not torch.equal(plain._engine.params, agent._engine.params) and agent._engine.adam_count.item() == 1
    agent._engine_for(4)
    assert (agent._engine.cql_alpha, agent._engine.batch_size) == (ALPHA, 4)


def test_entry_point_with_the_flag(tmp_path):
    """Check 7: -cql through the Atari DQN entry point on the synthetic environment, with quantile heads (QR-DQN + CQL): it trains, stays
    finite and keeps the flag out of parameters.json; a refused value fails before anything is written."""
    import pickle

    run = importlib.import_module("experiments.atari.dqn").run
    argv = ["-en", "cql_Synthetic", "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "400", "-bs", "8", "-n", "1", "-horizon", "50",
            "-at", "cnn", "-ne", "1", "-ntspe", "120", "-utd", "1", "-nis", "20", "-ed", "100", "-ln", "-tuf", "16", "-env", "synthetic",
            "-qr", "-nq", "8", "-hd", "1", "-cql", "1.0"]
    gathered = run(argv, root=str(tmp_path))
    assert len(gathered) == 1
    out = tmp_path / "atari" / "exp_output" / "cql_Synthetic"
    stored = json.load(open(out / "parameters.json"))
    assert all("cql_alpha" not in section for section in stored.values())
    model = pickle.load(open(out / "dqn" / "models" / "1", "rb"))["params"]
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())
    with pytest.raises(ValueError):
        run(["-en", "bad_Synthetic"] + argv[2:-1] + ["-1"], root=str(tmp_path))
    assert not (tmp_path / "atari" / "exp_output" / "bad_Synthetic").exists()


def test_offline_training_end_to_end(tmp_path, monkeypatch):
    """Check 8: 600 steps of DQN on the synthetic LunarLander logged with -logrb, then -offline on that log with -cql 1 -evals 100, two
    epochs of 50 gradient steps: the replay holds what the online run's held and takes no add after the fill, the logged losses are
    finite, evaluation returns are written where an epoch's returns go."""
    from experiments.base import offline

    run = importlib.import_module("experiments.lunar_lander.dqn").run
    base = ["-s", "1", "-dw", "-f", "20", "14", "-at", "fc", "-ln", "-tuf", "16", "-env", "synthetic", "-rbc", "1000", "-bs", "8", "-horizon", "50",
            "-utd", "1", "-nis", "20", "-ed", "100"]
    log_dir = str(tmp_path / "log")
    run(["-en", "online"] + base + ["-ne", "1", "-ntspe", "600", "-logrb", log_dir], root=str(tmp_path))
    n_logged = offline.dataset_size(log_dir)
    assert 600 <= n_logged <= 650 and json.load(open(os.path.join(log_dir, offline.META)))["n_actions"] == 4
    seen = {}
    fill, train = offline.fill_replay, offline.train_offline

    def fill_spy(rb, directory):
        n = fill(rb, directory)
        seen.update(rb=rb, elements=rb.add_count, n=n)
        return n

    def train_spy(rng, p, *rest):
        seen["p"] = p
        return train(rng, p, *rest)

    monkeypatch.setattr(offline, "fill_replay", fill_spy)
    monkeypatch.setattr(offline, "train_offline", train_spy)
    gathered = run(["-en", "offline"] + base + ["-ne", "2", "-ntspe", "50", "-cql", "1", "-offline", log_dir, "-evals", "100"], root=str(tmp_path))
    assert len(gathered) == 2 and [int(g[2]) for g in gathered] == [50, 100]
    assert seen["n"] == n_logged and seen["rb"].add_count == seen["elements"] > 500  # no add after the fill
    logs = [d for d in seen["p"]["wandb"].history if "epoch" not in d]
    assert [d["n_training_steps"] for d in logs] == [16, 32, 48, 64, 80, 96]
    assert all(np.isfinite(v) for d in seen["p"]["wandb"].history for v in d.values() if isinstance(v, (int, float)))
    stored = json.load(open(tmp_path / "lunar_lander" / "exp_output" / "offline" / "dqn" / "episode_returns_and_lengths" / "1.json"))
    assert len(stored["episode_returns"]) == 2 and all(len(r) >= 1 and np.isfinite(r).all() for r in stored["episode_returns"])
    assert all(sum(l) >= 100 for l in stored["episode_lengths"])
    assert os.path.exists(tmp_path / "lunar_lander" / "exp_output" / "offline" / "dqn" / "models" / "1")
    # without -evals no environment is built: the agent is sized from the log
    monkeypatch.setattr(importlib.import_module("experiments.lunar_lander.dqn"), "make_environment", lambda p: pytest.fail("an environment was built"))
    gathered = run(["-en", "offline_blind"] + base + ["-ne", "1", "-ntspe", "20", "-cql", "1", "-offline", log_dir], root=str(tmp_path))
    assert len(gathered) == 1 and int(gathered[0][2]) == 20
    with pytest.raises(ValueError, match="more than the replay's capacity"):
        run(["-en", "offline_small"] + [a if a != "1000" else "100" for a in base] + ["-ne", "1", "-ntspe", "20", "-offline", log_dir], root=str(tmp_path))
