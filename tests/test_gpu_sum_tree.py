"""GPU parity: HIP sum tree vs the golden vectors produced by the REFERENCE class, bit for bit,
through the C ABI (slimdqn.sample_collection.sum_tree.SumTree wraps isdqn_tree_*)."""
import hashlib

import numpy as np
import pytest

from tests.helpers import sum_tree_edges as edges
from tests.sumtree_cases import all_cases, replay

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(all_cases()), ids=lambda c: c[0])
def test_hip_tree_matches_reference_golden(case, golden_sum_tree):
    from slimdqn.sample_collection.sum_tree import SumTree

    name, capacity, ops = case
    g = golden_sum_tree
    tree = SumTree(capacity)
    results = replay(tree, ops)
    nodes = tree._nodes
    assert tree._depth == int(g[f"{name}/depth"])
    assert tree._first_leaf_offset == int(g[f"{name}/first_leaf_offset"])
    assert nodes.size == int(g[f"{name}/n_nodes"])
    if f"{name}/nodes" in g:
        np.testing.assert_array_equal(nodes, g[f"{name}/nodes"])
    else:
        np.testing.assert_array_equal(nodes[:1023], g[f"{name}/nodes_top"])
    assert hashlib.sha256(nodes.tobytes()).digest() == g[f"{name}/nodes_sha256"].tobytes()
    assert tree.root == float(g[f"{name}/root"])
    assert tree.max_recorded_priority == float(g[f"{name}/max_recorded_priority"])
    assert len(results) == int(g[f"{name}/n_queries"])
    for i, r in enumerate(results):
        np.testing.assert_array_equal(r, g[f"{name}/query{i}"])


def test_hip_tree_matches_oracle_on_fresh_random_ops():
    from oracle.sum_tree import SumTree as Oracle
    from slimdqn.sample_collection.sum_tree import SumTree

    rng = np.random.default_rng(99)
    for capacity in (37, 5000, 300_000):
        o, h = Oracle(capacity), SumTree(capacity)
        for _ in range(8):
            n = int(rng.integers(1, 700))
            idx = rng.integers(0, capacity, n).astype(np.int32)
            val = rng.uniform(0, 5, n)
            o.set(idx, val)
            h.set(idx, val)
            t = rng.uniform(0, o.root, 333)
            np.testing.assert_array_equal(o.query(t), h.query(t))
        np.testing.assert_array_equal(o._nodes, h._nodes)


def test_hip_tree_reference_error_conventions():
    from slimdqn.sample_collection.sum_tree import SumTree

    with pytest.raises(AssertionError):
        SumTree(capacity=-1)
    t = SumTree(100)
    with pytest.raises(AssertionError):
        t.set(0, -1)
    with pytest.raises(ValueError):
        t.query(1.0)  # empty tree
    t.set(5, 1.0)
    assert t.query(0.99) == 5
    with pytest.raises(ValueError):
        t.query(1.0)  # target == root
    # device-side latch: negative value leaves the tree untouched
    import torch

    before = t._nodes.copy()
    t.set_device(torch.tensor([1, 2], dtype=torch.int32, device="cuda"), torch.tensor([1.0, -2.0], dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        t.check_status()
    np.testing.assert_array_equal(before, t._nodes)
    # a rejected set leaves the recorded maximum alone too, whatever is wrong with it (9.0 would raise it)
    t.set(np.arange(100, dtype=np.int32), np.linspace(0.5, 2.0, 100))
    before, max_before = t._nodes.copy(), t.max_recorded_priority
    assert max_before == 2.0
    n_leaves = 1 << (t._depth - 1)
    for idx, val in [([1, 2, 3], [9.0, float("nan"), 1.0]), ([1, 2, 3], [9.0, 1.0, -0.5]), ([1, -1, 3], [9.0, 1.0, 1.0]),
                     ([1, 2, n_leaves], [9.0, 1.0, 1.0])]:
        t.set_device(torch.tensor(idx, dtype=torch.int32, device="cuda"), torch.tensor(val, dtype=torch.float64, device="cuda"))
        with pytest.raises(AssertionError):
            t.check_status()
        np.testing.assert_array_equal(before.view(np.int64), t._nodes.view(np.int64))
        assert t.max_recorded_priority == max_before, (idx, val)
    t.set_device(torch.tensor([1, 2, 3], dtype=torch.int32, device="cuda"), torch.tensor([9.0, 1.0, 1.0], dtype=torch.float64, device="cuda"))
    t.check_status()
    assert t.max_recorded_priority == 9.0 and t.get(1) == 9.0


def test_tree_set_without_a_maximum_pointer():
    """isdqn_tree_set(max_recorded_priority = NULL): the nodes as the oracle's, n on both sides of the 1024 threads."""
    import torch
    from oracle.sum_tree import SumTree as Oracle
    from slimdqn import _hip
    from slimdqn.sample_collection.sum_tree import SumTree

    rng = np.random.default_rng(31)
    o, h = Oracle(5000), SumTree(5000)
    for n in (1, 700, 1025, 4096):
        idx = rng.integers(0, 5000, n).astype(np.int32)
        idx[rng.permutation(n)[: n // 3]] = idx[0]
        val = rng.uniform(0.0, 5.0, n)
        o.set(idx, val)
        d_idx, d_val = torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda()
        rc = h._lib.isdqn_tree_set(h._nodes_dev.data_ptr(), h._depth, d_idx.data_ptr(), d_val.data_ptr(), n, None, h._status.data_ptr(),
                                   _hip.stream_ptr(h.device))
        assert rc == 0
        h.check_status()
        np.testing.assert_array_equal(h._nodes.view(np.int64), o._nodes.view(np.int64))
        assert h.max_recorded_priority == 1.0
    assert o.max_recorded_priority > 4.0  # what the pointer would have received


def test_unit_target_query_matches_numpy_uniform():
    """query(unit draws) == reference sampling: rng.uniform(0, root, n) -> query (samplers.py:110-111)."""
    import torch
    from oracle.sum_tree import SumTree as Oracle
    from slimdqn.sample_collection.sum_tree import SumTree

    rng = np.random.default_rng(5)
    cap = 100_000
    o, h = Oracle(cap), SumTree(cap)
    for s in range(0, cap, 4096):
        n = min(4096, cap - s)
        idx = np.arange(s, s + n, dtype=np.int32)
        val = rng.uniform(0.1, 2.0, n)
        o.set(idx, val)
        h.set(idx, val)
    ref = o.query(np.random.default_rng(0).uniform(0.0, o.root, size=256))
    u = torch.from_numpy(np.random.default_rng(0).random(256)).cuda()
    got = h.query_device(u, unit=True).cpu().numpy()
    h.check_status()
    np.testing.assert_array_equal(ref, got)


# ------------------------------------------------------------------------------------- edge cases (tests/helpers/sum_tree_edges.py)
def _same_nodes(h, o, what):
    """Node bits equal (0.0 and -0.0 differ); a failure names the first node instead of printing 16 MB."""
    a, b = h._nodes, o._nodes
    assert a.shape == b.shape
    if np.array_equal(a.view(np.int64), b.view(np.int64)):
        return a, b
    bad = np.nonzero(a.view(np.int64) != b.view(np.int64))[0]
    assert bad.size == 0, f"{what}: {bad.size} nodes differ; first: node {bad[0]}, HIP {a[bad[0]]!r}, oracle {b[bad[0]]!r}"


@pytest.mark.parametrize("case", list(edges.set_limit_cases()), ids=lambda c: c[0])
def test_set_at_the_batch_limits_matches_the_oracle(case):
    from oracle.sum_tree import SumTree as Oracle
    from slimdqn.sample_collection.sum_tree import SumTree

    name, capacity, ops = case
    o, h = Oracle(capacity), SumTree(capacity)
    for k, op in enumerate(ops):
        edges.replay_edges(o, [op])
        edges.replay_edges(h, [op])  # SumTree.set checks the status word itself
        what = f"{name} op {k} (n = {len(op[1])})"
        a, b = _same_nodes(h, o, what)
        assert h.max_recorded_priority == float(o.max_recorded_priority), what
    assert hashlib.sha256(a.tobytes()).digest() == hashlib.sha256(b.tobytes()).digest()  # as the golden test compares them
    assert int(h._status.item()) == 0


@pytest.mark.parametrize("case", list(edges.swap_remove_cases()), ids=lambda c: c[0])
def test_swap_remove_kernel_matches_the_oracle(case):
    from oracle.sum_tree import SumTree as Oracle
    from slimdqn.sample_collection.sum_tree import SumTree

    name, capacity, ops = case
    o, h = Oracle(capacity), SumTree(capacity)
    for k, op in enumerate(ops):
        edges.replay_edges(o, [op])
        edges.replay_edges(h, [op])
        _same_nodes(h, o, f"{name} op {k} {op[0]} {op[1:] if op[0] != 'set' else ''}")
    h.check_status()
    assert int(h._status.item()) == 0


@pytest.mark.parametrize("case", list(edges.query_boundary_cases()), ids=lambda c: c[0])
def test_query_boundaries_match_the_oracle(case):
    import torch
    from oracle.sum_tree import SumTree as Oracle
    from slimdqn.sample_collection.sum_tree import SumTree

    name, capacity, ops = case
    o, h = Oracle(capacity), SumTree(capacity)
    sets = [op for op in ops if op[0] == "set"]
    edges.replay_edges(o, sets)
    edges.replay_edges(h, sets)
    _same_nodes(h, o, name)
    n_targets = 0
    for op in ops:
        if op[0] != "query":
            continue
        want = o.query(op[1])
        t = torch.from_numpy(op[1]).cuda()
        plain = h.query_device(t).cpu().numpy()
        weights = torch.empty(len(op[1]), dtype=torch.float32, device="cuda")
        weighted = h.query_device(t, beta=0.5, weights_out=weights).cpu().numpy()
        h.check_status()  # no target out of range
        np.testing.assert_array_equal(plain, want)
        np.testing.assert_array_equal(weighted, want)
        n_targets += len(want)
    assert n_targets >= 64 * (o._depth - 1)
