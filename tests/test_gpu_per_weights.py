"""Importance-sampling weights of prioritized replay on the GPU (include/isdqn_hip.h: isdqn_tree_query_weighted,
isdqn_batch.loss_weights) against the float64 restatement of tests/helpers/per_weights.py:

  * the weighted query: indices / status / leaves bit for bit with isdqn_tree_query, weights within one float32 ulp;
  * the weighted loss: NULL == all ones bit for bit, power-of-two weights scale everything behind dL/dq exactly, seeded weights
    against float64 from the device's own q_values / targets, linearity of the whole backward;
  * the captured update with weights on against eager steps, run-to-run identity, the entry point with -per -pe -isb -isbe."""
import json

import numpy as np
import pytest
import torch

from tests import sumtree_cases
from tests.gpu_helpers import make_frame_batch, perturbed_params
from tests.helpers import hl_gauss as hl
from tests.helpers import per_weights as pw

pytestmark = pytest.mark.gpu

U32 = 2.0**-24
BETAS = (0.0, 0.4, 0.5, 1.0)
NB, VMIN, VMAX = 51, -10.0, 10.0
SIGMA = 0.75 * (VMAX - VMIN) / NB
FC_OBS = (8,)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ===================================================================================== 5. the weighted query
def _filled_tree(capacity, seed):
    """A tree as PrioritizedSamplingDistribution builds it (one spare leaf when the capacity is a power of two: the extra level
    has a zero right subtree), its ``capacity`` leaves filled from a seeded generator."""
    from slimdqn.sample_collection.sum_tree import SumTree

    tree = SumTree(capacity + 1 if capacity & (capacity - 1) == 0 else capacity)
    rng = np.random.default_rng(seed)
    vals = np.exp(rng.uniform(np.log(1e-2), np.log(1e1), capacity))  # three decades
    tree.set(np.arange(capacity, dtype=np.int32), vals)
    return tree


def _check_weighted_query(tree, units, beta, unit=True):
    """One weighted query against the plain query and the float64 helper; returns the share of weights that differ at all."""
    n = units.numel()
    tree._status.zero_()
    plain = tree.query_device(units, unit=unit)
    status_plain = int(tree._status.item())
    tree._status.zero_()
    leaf = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    w = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    beta_dev = torch.tensor([beta], dtype=torch.float32, device="cuda")
    idx = tree.query_device(units, unit=unit, beta=beta_dev, weights_out=w, leaf_out=leaf)
    status = int(tree._status.item())
    tree._status.zero_()
    assert torch.equal(idx, plain), "indices differ from isdqn_tree_query"
    assert status == status_plain, (status, status_plain)
    leaves = tree._nodes_dev[tree._first_leaf_offset + idx.long()]
    assert torch.equal(leaf, leaves), "out_leaf differs from the gathered leaves"
    want = pw.weights(leaves.cpu().numpy(), float(np.float32(beta)), n_keys=max(tree._capacity, 2), root=float(tree._nodes_dev[0].item())).astype(np.float32)
    got = w.cpu().numpy()
    steps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    share = float((steps != 0).mean())
    assert steps.max() <= 1, f"weights differ from float32(helper) by {steps.max()} float32 ulp ({share:.2%} of the elements differ at all)"
    assert np.isfinite(got).all() and got.max() == 1.0, got.max()
    assert (got > 0).all() and (got <= 1.0).all()
    if beta == 0.0:
        assert (got == 1.0).all()
    return share


@pytest.mark.parametrize("capacity", [5, 1000, 4096, 1_000_000])  # 4096: the spare-leaf case
def test_weighted_query_on_seeded_trees(capacity):
    tree = _filled_tree(capacity, seed=capacity)
    rng = np.random.default_rng(7 + capacity)
    shares = []
    for n in (1, 32, 256, 4096):
        units = _d(rng.random(n))
        for beta in BETAS:
            shares.append(_check_weighted_query(tree, units, beta))
    # absolute targets (targets_are_unit = 0) take the same path
    root = float(tree._nodes_dev[0].item())
    _check_weighted_query(tree, _d(rng.random(256) * root), 0.5, unit=False)
    print(f"capacity {capacity}: largest share of weights one float32 ulp off the helper: {max(shares):.3%}")
    # without beta the call is the plain query, any n; with it n is limited
    big = _d(rng.random(5000))
    assert tree.query_device(big, unit=True).numel() == 5000
    with pytest.raises(AssertionError):
        tree.query_device(big, unit=True, beta=0.5, weights_out=torch.empty(5000, dtype=torch.float32, device="cuda"))  # ISDQN_ERR_SHAPE


def test_weighted_query_on_the_shared_sum_tree_cases():
    from slimdqn.sample_collection.sum_tree import SumTree

    n_queries = 0
    for name, capacity, ops in sumtree_cases.all_cases():
        tree = SumTree(capacity)
        for op in ops:
            if op[0] == "set":
                tree.set(op[1], op[2])
            elif op[0] == "swap_remove":
                a, b = int(op[1][0]), int(op[1][1])
                tree.set(np.asarray([a, b], dtype=np.int32), np.asarray([tree.get(b), 0.0]))
            elif op[0] in ("query", "query_u"):
                if tree.root == 0.0:
                    continue
                t = _d(np.asarray(op[1], np.float64).reshape(-1))
                for beta in BETAS:
                    _check_weighted_query(tree, t, beta, unit=op[0] == "query_u")
                n_queries += 1
    assert n_queries >= 60


def test_zero_leaf_gets_weight_one_and_stays_out_of_the_minimum():
    """A hand-written node array (the buffer is the caller's): depth 3, leaves [2, 0 | 0.5, 8] under inner sums that send the draw
    2.25 to the right of the first pair -- the leaf holding 0.0 (an inconsistent inner sum, as rounding at the tree's right edge
    leaves it) -- and the others to positive leaves."""
    from slimdqn import _hip

    lib = _hip.lib()
    nodes = _d(np.array([11.0, 2.5, 8.5, 2.0, 0.0, 0.5, 8.0], np.float64))
    targets = _d(np.array([1.0, 2.25, 2.75, 5.0], np.float64))  # -> leaves 0, 1 (value 0.0), 2, 3
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    leaf = torch.zeros(4, dtype=torch.float64, device="cuda")
    w = torch.zeros(4, dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    beta = torch.tensor([0.5], dtype=torch.float32, device="cuda")
    rc = lib.isdqn_tree_query_weighted(nodes.data_ptr(), 3, targets.data_ptr(), 4, 0, beta.data_ptr(), idx.data_ptr(), leaf.data_ptr(),
                                       w.data_ptr(), status.data_ptr(), _hip.stream_ptr(nodes.device))
    assert rc == 0
    assert idx.tolist() == [0, 1, 2, 3] and leaf.tolist() == [2.0, 0.0, 0.5, 8.0] and int(status.item()) == 0
    assert w.tolist() == [0.5, 1.0, 1.0, 0.25]  # p_min = 0.5, not 0: (0.5 / 2)^0.5, (0.5 / 8)^0.5
    assert np.array_equal(w.cpu().numpy(), pw.weights([2.0, 0.0, 0.5, 8.0], 0.5, n_keys=4, root=11.0).astype(np.float32))
    # no positive leaf among the draws: all ones (the status word reports the empty tree)
    nodes.zero_()
    rc = lib.isdqn_tree_query_weighted(nodes.data_ptr(), 3, targets.data_ptr(), 4, 1, beta.data_ptr(), idx.data_ptr(), None,
                                       w.data_ptr(), status.data_ptr(), _hip.stream_ptr(nodes.device))
    assert rc == 0 and w.tolist() == [1.0] * 4 and int(status.item()) & _hip.STATUS_EMPTY_TREE


def _minimum_tree(tie=False):
    """64 leaves, every value a multiple of 2^-10 (all partial sums and midpoints are exact, so the absolute target
    cum[j] - value[j] / 2 lands in leaf j on any descent): leaf 37 holds 2^-10, the others 0.5 to 4; ``tie``: leaf 5 holds 2^-10 too."""
    from oracle.sum_tree import SumTree as Oracle
    from slimdqn.sample_collection.sum_tree import SumTree

    vals = np.random.default_rng(64).integers(512, 4097, 64) / 1024.0
    vals[37] = 1.0 / 1024.0
    if tie:
        vals[5] = 1.0 / 1024.0
    o, tree = Oracle(64), SumTree(64)
    o.set(np.arange(64, dtype=np.int32), vals)
    tree.set(np.arange(64, dtype=np.int32), vals)
    return o, tree, vals, np.cumsum(vals) - vals / 2.0


@pytest.mark.parametrize("n", [1, 64, 65, 1024, 1025, 4096])
def test_batch_minimum_found_at_every_draw_position(n):
    """The smallest leaf is drawn at exactly one position p of the batch -- the first or last lane of a wave, the last draw, a
    thread's second entry (p >= 1024) -- or twice, or tied with another leaf: a reduction that loses that lane leaves weights
    above 1 behind, which _check_weighted_query rejects."""
    o, tree, vals, mid = _minimum_tree()
    rng = np.random.default_rng(n)
    others = np.delete(np.arange(64), 37)
    for p in sorted({q for q in (0, 63, 64, n - 1) if q < n}):
        leaves = rng.choice(others, n)
        leaves[p] = 37
        targets = mid[leaves]
        np.testing.assert_array_equal(o.query(targets), leaves)
        for beta in (0.5, 1.0):
            _check_weighted_query(tree, _d(targets), beta, unit=False)
        got = tree.query_device(_d(targets)).cpu().numpy()
        assert got[p] == 37 and (got == 37).sum() == 1
    if n >= 65:  # the minimum twice (two threads, or one thread's two entries at n = 1025); then tied between two leaves
        leaves = rng.choice(others, n)
        leaves[0] = leaves[n - 1] = 37
        _check_weighted_query(tree, _d(mid[leaves]), 0.5, unit=False)
        o2, tree2, vals2, mid2 = _minimum_tree(tie=True)
        leaves = rng.choice(np.delete(np.arange(64), [5, 37]), n)
        leaves[63], leaves[64] = 5, 37
        np.testing.assert_array_equal(o2.query(mid2[leaves]), leaves)
        _check_weighted_query(tree2, _d(mid2[leaves]), 0.5, unit=False)


# ===================================================================================== engines and batches
CONFIGS = {
    # name: (feats, n_heads, A, B, arch, ln, extra engine keywords, target parameters)
    "c2-head-chain": ((32, 64, 64, 512), 10, 9, 256, "cnn", True, {}, False),
    "cnn-noln": ((7, 9, 11, 13), 4, 5, 6, "cnn", False, {}, False),
    "fc": ((32, 32), 3, 4, 9, "fc", True, {}, False),
    "one-head": ((7, 9, 11, 13), 1, 5, 6, "cnn", True, {}, False),
    "one-head-target": ((7, 9, 11, 13), 1, 5, 6, "cnn", True, {}, True),
    "batchnorm": ((7, 9, 11, 13), 4, 5, 6, "cnn", True, dict(batch_norm=True), False),
    "hl-gauss": ((7, 9, 11, 13), 4, 5, 6, "cnn", True, dict(n_bins=NB, min_value=VMIN, max_value=VMAX, sigma=SIGMA), False),
    "huber": ((7, 9, 11, 13), 4, 5, 6, "cnn", True, dict(huber_delta=1.0), False),
    "bf16": ((7, 9, 11, 13), 4, 5, 6, "cnn", True, dict(precision="bf16"), False),
}


class _Setup:
    """An engine with seeded parameters and one seeded batch; ``cb(weights)`` is the C batch with that weights tensor."""

    def __init__(self, name, seed=3, B=None, **more):
        from slimdqn._engine import QNetEngine

        feats, n_heads, A, B0, arch, ln, kw, target = CONFIGS[name]
        B = B or B0
        kw = {**kw, **more}
        obs = FC_OBS if arch == "fc" else (84, 84, 4)
        self.name, self.A, self.B, self.arch, self.n_heads = name, A, B, arch, n_heads
        bn = bool(kw.get("batch_norm", False))
        nb = int(kw.get("n_bins", 0))
        params = perturbed_params(seed, obs, feats, arch, n_heads * A * max(nb, 1), ln, batch_norm=bn)
        self.eng = eng = QNetEngine(obs, A, n_heads, feats, arch, ln, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, **kw)
        eng.import_flax(params)
        self.target = None
        if target:
            self.target = torch.zeros_like(eng.params)
            eng.import_flax(perturbed_params(seed + 30, obs, feats, arch, n_heads * A * max(nb, 1), ln), target=self.target)
        rng = np.random.default_rng(seed + 100)
        scale = 15.0 if nb else 1.0
        if arch == "fc":
            self.kw = dict(state=_d(rng.normal(size=(B, obs[0])).astype(np.float32)), next_state=_d(rng.normal(size=(B, obs[0])).astype(np.float32)),
                           action=_d(rng.integers(0, A, B).astype(np.int32)), reward=_d((rng.normal(size=B) * scale).astype(np.float32)),
                           terminal=_d((rng.random(B) < 0.3).astype(np.uint8)))
        else:
            frames, ids, action, reward, terminal, _ = make_frame_batch(B, A, seed=seed)
            self.kw = dict(frames=_d(frames), frame_stride=frames.shape[1], frame_ids=_d(ids), action=_d(action),
                           reward=_d((reward * scale).astype(np.float32)), terminal=_d(terminal))
        self.action = self.kw["action"].cpu().numpy()
        self.K = eng.n_regressed
        self.oh = 1 if n_heads >= 2 else 0
        torch.cuda.synchronize()
        self.state0 = [t.clone() for t in self._state()]

    def _state(self):
        e = self.eng
        return (e.params, e.adam_m, e.adam_v, e.adam_count, e.losses_accum)

    def reset(self):
        for dst, src in zip(self._state(), self.state0):
            dst.copy_(src)
        self.eng.invalidate_mirror()

    def cb(self, weights=None):
        return self.eng.make_batch(loss_weights=weights, **self.kw)

    def learn(self, weights=None, grad_out=None):
        if self.target is not None:
            return self.eng.learn_on_batch_target(self.cb(weights), self.target)
        return self.eng.learn_on_batch(self.cb(weights), grad_out=grad_out)

    def grad(self, weights=None):
        g = torch.zeros_like(self.eng.params)
        self.eng.grad_on_batch(self.cb(weights), g, target_params=self.target)
        return g

    def outputs(self):
        e = self.eng
        torch.cuda.synchronize()
        return dict(losses=e.losses.clone(), q_values=e.q_values.clone(), targets=e.targets.clone(), priorities=e.priorities.clone())

    def dout(self):
        """dL/dq (dL/dlogits with histogram heads) of the last learn / grad call: [B][width padded to 8]"""
        width = self.n_heads * self.A * max(self.eng.n_bins, 1)
        wp = (width + 7) // 8 * 8
        return self.eng.region("dout")[: self.B * wp].reshape(self.B, wp).clone(), width


def _tree_weights(B, seed=11, beta=0.5):
    """Weights in (0, 1] from a real isdqn_tree_query_weighted call on a tree whose priorities spread over three decades."""
    tree = _filled_tree(4096, seed)
    w = torch.zeros(B, dtype=torch.float32, device="cuda")
    tree.query_device(_d(np.random.default_rng(seed).random(B)), unit=True, beta=beta, weights_out=w)
    tree.check_status()
    assert float(w.max()) == 1.0 and (B < 8 or float(w.min()) < 0.5), w.min()
    return w


# ===================================================================================== 6. NULL == all ones
@pytest.mark.parametrize("name", list(CONFIGS))
def test_null_weights_equal_all_ones_bit_for_bit(name):
    s = _Setup(name)
    ones = torch.ones(s.B, dtype=torch.float32, device="cuda")
    runs = []
    for w in (None, ones):
        s.reset()
        per_step = []
        for _ in range(3):
            s.learn(w)
            per_step.append(s.outputs())
        runs.append((per_step, [t.clone() for t in s._state()]))
    (steps_a, state_a), (steps_b, state_b) = runs
    for i, (a, b) in enumerate(zip(steps_a, steps_b)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"step {i}: {k} differs between NULL and all-ones weights"
    for n, a, b in zip(("params", "adam_m", "adam_v", "adam_count", "losses_accum"), state_a, state_b):
        assert torch.equal(a, b), f"{n} differs between NULL and all-ones weights ({(a != b).sum().item()} elements)"
    assert int(state_a[3].item()) == 3 and not torch.equal(state_a[0], s.state0[0])
    # and the loss-only entry point
    s.reset()
    la = (s.eng.loss_on_batch_target(s.cb(None), s.target) if s.target is not None else s.eng.loss_on_batch(s.cb(None))).clone()
    lb = (s.eng.loss_on_batch_target(s.cb(ones), s.target) if s.target is not None else s.eng.loss_on_batch(s.cb(ones))).clone()
    assert torch.equal(la, lb)


# ===================================================================================== 7. power-of-two scaling
def _assert_half(name, full, half):
    bad = (half != 0.5 * full).nonzero().reshape(-1)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(f"{name}: {bad.numel()} elements are not exactly half; first: index {i}, unweighted {full.reshape(-1)[i].item()!r}, "
                             f"weighted {half.reshape(-1)[i].item()!r}")


@pytest.mark.parametrize("name", ["c2-head-chain", "cnn-noln", "hl-gauss", "one-head-target"])
def test_half_weights_scale_losses_dout_and_gradient_exactly(name):
    s = _Setup(name, B=32 if name == "c2-head-chain" else None)
    half = torch.full((s.B,), 0.5, dtype=torch.float32, device="cuda")
    res = {}
    for key, w in (("full", None), ("half", half)):
        g = s.grad(w)
        out = s.outputs()
        out["grad"], (out["dout"], _) = g, s.dout()
        res[key] = out
    for k in ("q_values", "targets"):
        assert torch.equal(res["full"][k], res["half"][k]), k
    for k in ("losses", "dout", "grad"):
        assert res["full"][k].abs().max() > 0
        _assert_half(f"grad_on_batch {k}", res["full"][k].reshape(-1), res["half"][k].reshape(-1))
    if s.target is None:  # the learn path (head chain where the shape has one): dout and the gradient the optimizer consumed
        res = {}
        for key, w in (("full", None), ("half", half)):
            s.reset()
            g = torch.zeros_like(s.eng.params)
            s.learn(w, grad_out=g)
            out = s.outputs()
            out["grad"], (out["dout"], _) = g, s.dout()
            res[key] = out
        for k in ("q_values", "targets", "priorities"):
            assert torch.equal(res["full"][k], res["half"][k]), k
        for k in ("losses", "dout", "grad"):
            _assert_half(f"learn_on_batch {k}", res["full"][k].reshape(-1), res["half"][k].reshape(-1))


# ===================================================================================== 8. seeded weights against float64
def _check_scalar_against_float64(s, w, out, dout, huber_delta):
    B, K, A = s.B, s.K, s.A
    ref = pw.weighted_td(out["q_values"].cpu().numpy(), out["targets"].cpu().numpy(), w.cpu().numpy(), huber_delta)
    d, width = dout
    d = d.double().cpu().numpy()
    cols = (s.oh + np.arange(K))[None, :] * A + s.action[:, None]  # [B, K]
    got = d[np.arange(B)[:, None], cols]
    err = np.abs(got - ref["dq"])
    bound = 4 * U32 * np.abs(ref["dq"])
    worst = float((err / np.maximum(np.abs(ref["dq"]), 1e-300)).max() / U32)
    print(f"{s.name}: worst dout error {worst:.3f} units of 2^-24 relative (bound 4)")
    assert (err <= bound).all(), f"dout: worst relative error {worst} x 2^-24"
    mask = np.ones_like(d, dtype=bool)
    mask[np.arange(B)[:, None], cols] = False
    assert (d[mask] == 0).all(), "dout has non-zero entries off the taken actions"
    losses = out["losses"].double().cpu().numpy()
    lbound = (B + 4) * U32 * ref["abs_terms"]
    print(f"{s.name}: loss error / bound = {(np.abs(losses - ref['losses']) / lbound).max():.4f}")
    assert (np.abs(losses - ref["losses"]) <= lbound).all(), (losses, ref["losses"], lbound)


@pytest.mark.parametrize("name,path", [("c2-head-chain", "learn"), ("c2-head-chain", "grad"), ("huber", "learn"), ("huber", "grad"),
                                       ("cnn-noln", "learn"), ("fc", "grad"), ("one-head-target", "learn")])
def test_seeded_weights_match_float64_from_the_device_q_values(name, path):
    s = _Setup(name, B=64 if name == "c2-head-chain" else None)
    w = _tree_weights(s.B)
    run = (lambda ww: s.learn(ww)) if path == "learn" else (lambda ww: s.grad(ww))
    s.reset()
    run(None)
    plain = s.outputs()
    s.reset()
    run(w)
    out, dout = s.outputs(), s.dout()
    for k in ("q_values", "targets") + (("priorities",) if path == "learn" else ()):
        assert torch.equal(plain[k], out[k]), f"{k} changed with weights"
    assert not torch.equal(plain["losses"], out["losses"])
    _check_scalar_against_float64(s, w, out, dout, float(s.eng.cfg.huber_delta))


@pytest.mark.parametrize("path", ["learn", "grad"])
def test_seeded_weights_with_histogram_heads(path):
    s = _Setup("hl-gauss")
    w = _tree_weights(s.B)
    run = (lambda ww: s.learn(ww)) if path == "learn" else (lambda ww: s.grad(ww))
    s.reset()
    run(None)
    plain = s.outputs()
    s.reset()
    run(w)
    out, (dout, nlog) = s.outputs(), s.dout()
    for k in ("q_values", "targets") + (("priorities",) if path == "learn" else ()):
        assert torch.equal(plain[k], out[k]), f"{k} changed with weights"
    B = s.B
    nlog_p = (nlog + 7) // 8 * 8
    logits = s.eng.region("logits")[: 2 * B * nlog_p].reshape(2 * B, nlog_p)[:, :nlog].double().cpu()
    ref = hl.hl_loss(logits, s.action, s.kw["reward"].cpu().numpy(), s.kw["terminal"].cpu().numpy(), float(s.eng.cfg.gamma_n), s.K, s.oh, 0,
                     s.A, NB, VMIN, VMAX, SIGMA)
    wd = w.double().cpu()
    # the bound tests/test_gpu_hl_gauss.py holds the unweighted cross-entropy and dL/dlogits to (|w| <= 1 cannot enlarge an absolute error)
    np.testing.assert_allclose(out["losses"].double().cpu().numpy(), (wd[:, None] * ref["ce"]).mean(0).numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(dout[:, :nlog].double().cpu().numpy(), (wd[:, None] * ref["dlogits"]).numpy(), rtol=1e-5, atol=1e-7)
    assert (dout[:, nlog:] == 0).all()


# ===================================================================================== 9. linearity of the whole backward
@pytest.mark.parametrize("name", ["c2-head-chain", "cnn-noln", "fc"])
def test_backward_is_linear_in_the_weights(name):
    s = _Setup(name, B=32 if name == "c2-head-chain" else None)
    B = s.B
    rng = np.random.default_rng(5)
    in_s = np.zeros(B, np.float32)
    in_s[rng.permutation(B)[: B // 2]] = 1.0
    w_s, w_c = _d(in_s), _d(1.0 - in_s)
    layers = [i.name.decode().split("/")[0] for i in s.eng.infos if i.kind in (0, 1)][:-1]  # every layer but the head has a dz region

    def row_width(layer):
        """floats per transition of a layer's dz region (internal layout: [rows][pixels][channels padded to 8])"""
        kind, i = layer.split("_")
        if kind == "Conv":
            hw = s.eng.observation_dim[0]
            for k, st in ((8, 4), (4, 2), (3, 1))[: int(i) + 1]:
                hw = -(-hw // st)
            return hw * hw * ((s.eng.features[int(i)] + 7) // 8 * 8)
        return (s.eng.features[int(i) + (3 if s.arch == "cnn" else 0)] + 7) // 8 * 8

    def run(w):
        g = s.grad(w)
        torch.cuda.synchronize()
        return g, {l: s.eng.region("dz/" + l)[: B * row_width(l)].reshape(B, -1).clone() for l in layers}

    g_all, dz_all = run(None)
    g_s, dz_s = run(w_s)
    g_c, dz_c = run(w_c)
    worst = 0.0
    for info in s.eng.infos:
        sl = slice(info.offset, info.offset + info.size)
        full = g_all[sl].double()
        if float(full.abs().max()) == 0.0:
            continue
        ratio = float(((g_s[sl].double() + g_c[sl].double()) - full).abs().max() / full.abs().max())
        worst = max(worst, ratio)
        # the bound tests/test_gpu_network.py holds a gradient to where only arithmetic differs (its mask-pinned check)
        assert ratio <= 1e-4, f"{info.name.decode()}: max |grad(S) + grad(S^c) - grad| / max |grad| = {ratio}"
    print(f"{name}: worst linearity ratio {worst:.3e}")
    checked = 0
    for l in layers:
        for dz, w in ((dz_s[l], in_s), (dz_c[l], 1.0 - in_s)):
            zero_rows, one_rows = torch.from_numpy(w == 0).cuda(), torch.from_numpy(w == 1).cuda()
            assert (dz[zero_rows] == 0).all(), f"dz/{l}: rows of weight 0 are not exactly zero"
            assert torch.equal(dz[one_rows], dz_all[l][one_rows]), f"dz/{l}: rows of weight 1 differ from the unweighted run"
        checked += int(float(dz_all[l].abs().max()) > 0)
    assert checked >= 1, "no dz region was written"


# ===================================================================================== 10. graph == eager with weights on
def _prioritized_replay(B, capacity=2048, seed=5, alpha=1.0):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution

    sampler = PrioritizedSamplingDistribution(seed, capacity, priority_exponent=alpha, device="cuda:0")
    rb = ReplayBuffer(sampler, B, capacity, stack_size=4, update_horizon=1, gamma=0.99, device="cuda:0")
    pri = np.exp(np.random.default_rng(seed).uniform(np.log(0.05), np.log(5.0), capacity))
    rb.prefill_synthetic(capacity, (84, 84), 5, seed=seed, p_terminal=0.01, priorities=pri)
    return rb


def _compare_agents(eager, rb_e, graphed, rb_g):
    torch.cuda.synchronize()
    for name in ("params", "adam_m", "adam_v", "adam_count", "losses_accum"):
        x, y = getattr(eager._engine, name), getattr(graphed._engine, name)
        assert torch.equal(x, y), f"{name}: {(x != y).sum().item()} elements differ between eager and captured steps"
    ta, tb = rb_e._sampling_distribution._sum_tree, rb_g._sampling_distribution._sum_tree
    assert torch.equal(ta._nodes_dev, tb._nodes_dev), "tree nodes differ"
    assert torch.equal(ta._max_dev, tb._max_dev), "max_recorded_priority differs"
    assert rb_e._sampling_distribution._rng_key.bit_generator.state == rb_g._sampling_distribution._rng_key.bit_generator.state
    assert eager._is_step == graphed._is_step == 8
    ta.check_status()
    tb.check_status()


def test_graph_replay_equals_eager_steps_with_weights_isdqn():
    from slimdqn.networks.isdqn import iSDQN

    K, A, B = 3, 5, 8

    def make(use_graph):
        agent = iSDQN(0, (84, 84, 4), A, K, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 1, 1, 100, adam_eps=1.5e-4, batch_size=B,
                      use_graph=use_graph)
        agent.priority_writeback = True
        agent.set_importance_sampling(0.4, 1.0, n_steps=6)  # anneals across the eight steps, constant on the last two
        return agent, _prioritized_replay(B)

    (eager, rb_e), (graphed, rb_g) = make(False), make(True)
    fresh = eager._engine.params.clone()
    for step in range(8):
        eager.update_online_params(step, rb_e)
    graphed.learn_steps(4, rb_g)
    first = graphed._graphed
    exe = first.graph
    betas_1 = first.betas.clone()
    graphed.learn_steps(4, rb_g)
    assert graphed._graphed is first and first.graph is exe and graphed._captures == 1  # no re-capture for new betas
    assert first.weighted and not torch.equal(betas_1, first.betas)
    assert first.betas.tolist() == [float(np.float32(0.4 + 0.6 * t / 6)) if t < 6 else 1.0 for t in range(4, 8)]
    _compare_agents(eager, rb_e, graphed, rb_g)
    assert eager._graphed is None and not torch.equal(fresh, eager._engine.params)
    w = first.weights.cpu().numpy()
    assert (w > 0).all() and (w <= 1).all() and (w.max(1) == 1.0).all() and w.min() < 0.9
    # weights on / off is part of what a request has to match: an unweighted agent state captures anew
    plain = iSDQN(0, (84, 84, 4), A, K, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 1, 1, 100, adam_eps=1.5e-4, batch_size=B)
    plain.priority_writeback = True
    plain.learn_steps(4, rb_g)
    assert not plain._graphed.weighted and plain._graphed.weights is None


def test_graph_replay_equals_eager_steps_with_weights_dqn():
    from slimdqn.networks.dqn import DQN

    A, B = 5, 8

    def make(use_graph):
        agent = DQN(0, (84, 84, 4), A, [8, 12, 16, 24], True, "cnn", 2e-4, 0.99, 1, 1, 100, adam_eps=1.5e-4, batch_size=B, use_graph=use_graph)
        agent.priority_writeback = True
        agent.set_importance_sampling(0.4, 1.0, n_steps=6)
        agent.target_params.tensor.mul_(0.75)  # a target that is not the online network
        return agent, _prioritized_replay(B)

    (eager, rb_e), (graphed, rb_g) = make(False), make(True)
    for step in range(8):
        eager.update_online_params(step, rb_e)
    target = graphed._target_tensor(graphed.target_params)
    eng = graphed._engine
    g = graphed._graphed_update(rb_g, learn=lambda cb: eng.learn_on_batch_target(cb, target), key=target.data_ptr(), steps=4)
    exe = g.graph
    for _ in range(2):
        g.run(graphed._next_betas(4))
    assert graphed._graphed is g and g.graph is exe and graphed._captures == 1 and g.weighted and g.writeback
    _compare_agents(eager, rb_e, graphed, rb_g)


# ===================================================================================== 11. run to run
def test_weighted_c2_step_is_bit_identical_run_to_run():
    w = _tree_weights(256)
    runs = []
    for _ in range(2):
        s = _Setup("c2-head-chain")
        ls = [s.learn(w).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((s.eng.params.clone(), s.eng.adam_m.clone(), s.eng.adam_v.clone(), torch.stack(ls), s.eng.priorities.clone(),
                     s.eng.losses_accum.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ===================================================================================== 12. the entry point
def test_entry_point_with_importance_sampling(tmp_path):
    from experiments.atari import isdqn as entry

    seen = {}
    wire = entry._wire_prioritized

    def spy(agent, rb, p=None):
        wire(agent, rb, p)
        seen["agent"], seen["rb"] = agent, rb

    entry._wire_prioritized = spy
    try:
        argv = ["-en", "is_Synthetic", "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "200", "-bs", "8", "-n", "3", "-horizon", "50",
                "-at", "cnn", "-ne", "2", "-ntspe", "60", "-utd", "4", "-nis", "20", "-ed", "100", "-nbi", "2", "-ln", "-tuf", "16",
                "-env", "synthetic", "-per", "-pe", "0.6", "-isb", "0.4", "-isbe", "1.0"]
        gathered = entry.run(argv, root=str(tmp_path))
    finally:
        entry._wire_prioritized = wire
    assert len(gathered) == 2
    out = tmp_path / "atari" / "exp_output" / "is_Synthetic"
    params = json.load(open(out / "parameters.json"))
    assert (params["isdqn"]["priority_exponent"], params["isdqn"]["is_beta"], params["isdqn"]["is_beta_end"]) == (0.6, 0.4, 1.0)
    agent, rb = seen["agent"], seen["rb"]
    assert agent.importance_sampling and agent._is_schedule == (0.4, 1.0, 25) and agent._is_step >= 20
    assert rb._sampling_distribution._priority_exponent == 0.6
    rb._sampling_distribution._sum_tree.check_status()  # status word clean
    res = json.load(open(out / "isdqn" / "episode_returns_and_lengths" / "1.json"))
    assert len(res["episode_returns"]) == 2
    import pickle

    model = pickle.load(open(out / "isdqn" / "models" / "1", "rb"))["params"]
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())
    assert torch.isfinite(agent._engine.losses).all() and torch.isfinite(agent._engine.losses_accum).all()
    with pytest.raises(ValueError):
        entry.run(["-en", "bad_Synthetic", "-s", "1", "-dw", "-env", "synthetic", "-isb", "0.4"], root=str(tmp_path))
