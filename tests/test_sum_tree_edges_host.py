"""CPU checks of the case lists in tests/helpers/sum_tree_edges.py: the GPU tests that replay them (test_gpu_sum_tree.py,
test_gpu_replay_buffer.py) compare the HIP tree with the oracle bit for bit, which proves something only where a wrong
implementation would give other bits.  So here the oracle is held against deliberately wrong numpy variants on the same
cases, and the sampler scripts against the conditions the differential run relies on.

The wrong variants of ``set`` (sum_tree.py:20-47):
  descending   the deltas reach every ancestor in descending leaf order (an identity with fewer than two distinct leaves)
  last         the LAST occurrence of a leaf is kept (an identity for a batch without duplicates)
  recompute    parents are recomputed from their children instead of receiving the deltas
"""
import numpy as np
import pytest

from oracle.sum_tree import SumTree as Oracle
from tests.helpers import sum_tree_edges as edges

SET_CASES = list(edges.set_limit_cases())
SWAP_CASES = list(edges.swap_remove_cases())
QUERY_CASES = list(edges.query_boundary_cases())


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _set_variant(nodes, first_leaf, depth, idx, val, mode):
    """One ``set`` in place, vectorised: np.add.at adds in index order, as the reference's own np.add.at does."""
    node = first_leaf + np.asarray(idx, np.int64)
    delta = np.asarray(val).astype(np.float64) - nodes[node]
    if mode == "last":
        uniq, pos = np.unique(node[::-1], return_index=True)
        delta_u = delta[::-1][pos]
    else:
        uniq, pos = np.unique(node, return_index=True)
        delta_u = delta[pos]
    if mode == "descending":
        uniq, delta_u = uniq[::-1], delta_u[::-1]
    if mode == "recompute":
        nodes[uniq] = nodes[uniq] + delta_u
        parents = uniq
        for _ in range(depth - 1):
            parents = np.unique((parents - 1) // 2)
            nodes[parents] = nodes[2 * parents + 1] + nodes[2 * parents + 2]
        return
    cur = uniq
    for _ in range(depth):
        np.add.at(nodes, cur, delta_u)
        cur = (cur - 1) // 2


def _touched(first_leaf, depth, idx):
    cur = np.unique(first_leaf + np.asarray(idx, np.int64))
    out = [cur]
    for _ in range(depth - 1):
        cur = np.unique((cur - 1) // 2)
        out.append(cur)
    return np.concatenate(out)


@pytest.mark.parametrize("case", SET_CASES, ids=lambda c: c[0])
def test_set_limit_cases_separate_the_oracle_from_wrong_variants(case):
    name, capacity, ops = case
    pattern = name.rsplit("_", 1)[1]
    tree = Oracle(capacity)
    first, depth = tree._first_leaf_offset, tree._depth
    mine = tree._nodes.copy()  # the vectorised restatement, op by op; anchored to the oracle class at the end
    n_fill = len(edges.fill_ops(capacity, np.random.default_rng(0)))
    sizes = []
    for k, (kind, idx, val) in enumerate(ops):
        assert kind == "set"
        n = len(idx)
        assert n >= 1 and idx.min() >= 0 and idx.max() < capacity
        if k >= n_fill and n >= 2:
            sizes.append(n)
            distinct = len(np.unique(idx))
            if pattern in "cde":
                assert distinct == n, "patterns (c), (d), (e) hold no duplicates"
            if pattern == "b":
                assert distinct == 1 and len(np.unique(np.asarray(val, np.float64))) == n
            touched = _touched(first, depth, idx)
            old = mine[touched].copy()
            got = {}
            for mode in ("oracle", "descending", "last", "recompute"):
                _set_variant(mine, first, depth, idx, val, mode)
                got[mode] = _bits(mine[touched])
                mine[touched] = old
            if distinct >= 2:
                assert (got["descending"] != got["oracle"]).any(), f"n = {n}: descending leaf order gives the same nodes"
            if distinct < n:
                assert (got["last"] != got["oracle"]).any(), f"n = {n}: keeping the last occurrence gives the same nodes"
            assert (got["recompute"] != got["oracle"]).any(), f"n = {n}: recomputing parents gives the same nodes"
        _set_variant(mine, first, depth, idx, val, "oracle")
        before = float(tree.max_recorded_priority)
        tree.set(idx, val)
        if k >= n_fill and len(np.unique(idx)) < n:  # the maximum sits on an occurrence that np.unique drops
            assert float(tree.max_recorded_priority) > max(before, float(tree._nodes[first:].max()))
    np.testing.assert_array_equal(_bits(mine), _bits(tree._nodes))
    if pattern == "chunked":
        assert sizes == [4097, 10000, 4097]
    elif pattern in "ab":
        assert sizes == [n for n in edges.SET_SIZES if n >= 2]
    else:
        assert sizes == [n for n in edges.SET_SIZES if 2 <= n <= min(capacity, 20000)]


def test_set_limit_cases_cover_the_issue_grid():
    names = [c[0] for c in SET_CASES]
    assert names == [f"set_c{c}_{p}" for c in edges.SET_CAPACITIES for p in edges.SET_PATTERNS] + ["set_c65536_chunked"]
    # pattern (d): below the ancestor of an aligned block of 8 the runs take every length mod 4
    for name, capacity, ops in SET_CASES:
        if name.endswith("_d") and capacity >= 5000:
            idx = ops[-1][1]
            assert len(idx) == 4096
            runs = np.unique(idx // 8, return_counts=True)[1]
            assert set(runs % 4) == {0, 1, 2, 3}
    # pattern (a): duplicates and unsorted indices among the entries i >= 1024, 2048, 3072 (a thread's 2nd to 4th entry)
    for name, capacity, ops in SET_CASES:
        if name.endswith("_a") and capacity >= 5000:
            idx = ops[-1][1]
            assert len(idx) == 4096
            firsts = np.zeros(4096, bool)
            firsts[np.unique(idx, return_index=True)[1]] = True
            for lo in (1024, 2048, 3072):
                assert (~firsts[lo : lo + 1024]).any() and firsts[lo : lo + 1024].any()
                assert (np.diff(idx[lo : lo + 1024]) < 0).any()


def _swap_wrong_order(nodes, first, depth, a, b):
    """{node: value} after a swap-remove that adds the two deltas to a shared ancestor in descending node order."""
    na, nb = first + a, first + b
    da, db = nodes[nb] - nodes[na], 0.0 - nodes[nb]
    (n0, d0), (n1, d1) = sorted([(na, da), (nb, db)])
    out = {}
    for _ in range(depth):
        if n0 == n1:
            out[n0] = (nodes[n0] + d1) + d0
        else:
            out[n0], out[n1] = nodes[n0] + d0, nodes[n1] + d1
        n0, n1 = (n0 - 1) // 2, (n1 - 1) // 2
    return out


@pytest.mark.parametrize("case", SWAP_CASES, ids=lambda c: c[0])
def test_swap_remove_cases_separate_the_add_orders(case):
    name, capacity, ops = case
    tree = Oracle(capacity)
    first, depth = tree._first_leaf_offset, tree._depth
    pairs, detected, kinds = 0, 0, set()
    leaves = 1 << (depth - 1)
    for op in ops:
        wrong = None
        if op[0] == "swap_remove_kernel":
            a, b = op[1], op[2]
            assert 0 <= a < capacity and 0 <= b < capacity
            kinds.add("equal" if a == b else "reversed" if a > b else "forward")
            if a != b:
                kinds.add(f"apart{abs(a - b)}")
                if a // 2 == b // 2:
                    kinds.add("siblings")
                if (a < leaves // 2) != (b < leaves // 2):
                    kinds.add("root_only")
                if tree.get(b) == 0.0:
                    kinds.add("zero_b")
                wrong = _swap_wrong_order(tree._nodes, first, depth, a, b)
        edges.replay_edges(tree, [op])
        if wrong is not None:
            pairs += 1
            detected += any(np.float64(tree._nodes[k]).view(np.int64) != np.float64(v).view(np.int64) for k, v in wrong.items())
    assert "equal" in kinds
    if capacity >= 2:
        assert {"forward", "reversed", "siblings", "root_only", "zero_b", "apart1"} <= kinds, kinds
        print(f"{name}: the wrong add order is detected in {detected} of {pairs} pairs")
        assert detected >= 0.25 * pairs, f"{name}: the wrong add order shows in only {detected} of {pairs} pairs"
    if capacity >= 1000:
        assert {"apart2", "apart3", "apart5", "apart17"} <= kinds, kinds


@pytest.mark.parametrize("case", QUERY_CASES, ids=lambda c: c[0])
def test_query_boundary_cases_hit_the_boundaries(case):
    name, capacity, ops = case
    tree = Oracle(capacity)
    results = edges.replay_edges(tree, ops)
    targets = np.concatenate([op[1] for op in ops if op[0] == "query"])
    got = np.concatenate(results)
    assert len(targets) == len(got) >= 64 * (tree._depth - 1)
    assert targets[0] == 0.0 and np.nextafter(targets[1], np.inf) == tree.root
    assert (tree._nodes[tree._first_leaf_offset :] == 0.0).sum() >= 50
    # the probes of one boundary land on both sides of it, for most boundaries met (a left sum of 0.0 has nothing to its left)
    groups = edges.QUERY_GROUPS[name]
    assert len(groups) == len(targets)
    split = sum(len(set(got[groups == node].tolist())) > 1 for node in np.unique(groups[groups >= 0]))
    positive = int((tree._nodes[np.unique(groups[groups >= 0])] > 0.0).sum())
    print(f"{name}: {split} of {positive} boundaries with a positive left sum have probes on both sides")
    assert positive >= 8 * (tree._depth - 1) and split >= 0.9 * positive


@pytest.mark.parametrize("capacity,seed,exponent", edges.SAMPLER_RUNS)
def test_sampler_scripts_run_on_the_oracle_alone(capacity, seed, exponent):
    ops = edges.sampler_script(capacity, seed)
    stats = edges.run_sampler_script(ops, edges.SamplerMirror(seed, capacity, exponent), exact_update_device=exponent == 1.0)
    print(dict(stats))
    kinds = ["add", "remove", "update", "sample"] + (["update_device"] if exponent == 1.0 else [])
    for kind in kinds + ["via_" + e for e in edges.SAMPLE_ENTRIES]:
        assert stats[kind] >= 100, (kind, stats[kind])
    assert stats["add_max"] >= 100
    assert stats["key_comparison_lost"] == 0
    assert stats["mid_block_size_change"] >= 1 and stats["block_used_up"] >= 1
    assert stats["sample_skipped"] <= stats["sample"] // 10
    if capacity == 4096:
        assert stats["auto_flush"] >= 1
        burst = 0
        for op in ops:
            if op[0] != "add":
                break
            burst += 1
        assert burst >= 1100
