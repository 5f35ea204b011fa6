"""Seeded edge cases for the float64 sum tree and the prioritized sampler (pure numpy, no GPU).

The generators yield ``(name, capacity, ops)`` in the op vocabulary of tests/sumtree_cases.py plus
``("swap_remove_kernel", a, b)``: the sampler's removal as ONE call.  ``replay_edges`` applies the ops to
the oracle (where that op is ``set([a, b], [get(b), 0.0])``, or ``set(a, 0.0)`` when a == b: oracle/samplers.py
``remove``) or to the HIP tree (``swap_remove_device(a, b)``).

  set_limit_cases       one ``set`` per batch size around the kernel's limits (1024 threads, 4 entries per thread,
                        ISDQN_TREE_MAX_BATCH = 4096 pairs), five index patterns each, and one case above 4096 pairs
  swap_remove_cases     near / sibling / far / equal / reversed pairs on an evolving tree
  query_boundary_cases  targets on, and one ulp either side of, the left-subtree sums met on root-to-leaf paths
  sampler_script        a seeded op sequence for PrioritizedSamplingDistribution, with ``SamplerMirror`` (the oracle
                        plus the staging the device sampler documents) and ``run_sampler_script`` (the differential run)

None of these cases belongs to sumtree_cases.all_cases(): that list is tied to tests/golden/sum_tree.npz.
"""
import numpy as np

from tests.sumtree_cases import replay

TREE_MAX_BATCH = 4096
SET_CAPACITIES = (5, 5000, 65536, 1_000_000)
SET_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 2049, 4093, 4095, 4096)
SET_PATTERNS = "abcde"
# One seed per (capacity, pattern): the first from 1 up with which EVERY batch of the case separates the oracle from the wrong
# variants of tests/test_sum_tree_edges_host.py.  A batch of three pairs on an eight-leaf tree shows a wrong order only by luck.
SET_SEEDS = {
    5: dict(a=140, b=11, c=4, d=9, e=3),
    5000: dict(a=1, b=1, c=4, d=1, e=6),
    65536: dict(a=2, b=1, c=1, d=1, e=3),
    1_000_000: dict(a=2, b=1, c=1, d=1, e=3),
}
SWAP_CAPACITIES = (1, 2, 3, 8, 1000, 1_000_000)
# capacity 2: the first seed of 400 tried that clears the host test's 25 % floor with room (18 of 30 pairs; most seeds show the
# wrong add order in 2 to 6 of 30, whatever the priority range: the root is the only shared ancestor there)
SWAP_SEEDS = {1: 4322, 2: 183, 3: 4324, 8: 4329, 1000: 5321, 1_000_000: 1004321}
QUERY_CAPACITIES = (1000, 1_000_000)
MAX_PRIORITY = "max"  # PrioritizedSamplingDistribution.MAX_PRIORITY
MAX_PENDING = 1024    # PrioritizedSamplingDistribution.MAX_PENDING
PREFETCH = 64         # UniformSamplingDistribution.PREFETCH
SAMPLE_SIZES = (1, 5, 32, 33, 256)
SAMPLE_ENTRIES = ("sample", "sample_device", "sample_weighted_device", "draw_rows")
SAMPLER_RUNS = [  # (capacity, seed, priority_exponent)
    (8, 11, 1.0),
    (60, 12, 1.0),
    (1000, 13, 1.0),
    (4096, 14, 1.0),
    (60, 15, 0.6),
]


def _i(a):
    return np.asarray(a, dtype=np.int32).reshape(-1)


# ------------------------------------------------------------------------------------------------ set at the batch limits
def fill_ops(capacity, rng):
    """Dense ascending fill of the first min(capacity, 20000) leaves, 4096 at a time (as sumtree_cases.seeded_cases)."""
    fill = min(capacity, 20000)
    ops = []
    for start in range(0, fill, TREE_MAX_BATCH):
        n = min(TREE_MAX_BATCH, fill - start)
        ops.append(("set", np.arange(start, start + n, dtype=np.int32), rng.uniform(0.1, 2.0, n)))
    return ops


def _blocks_of_eight(rng, fill, n):
    """n distinct leaves in aligned blocks of 8; the blocks hold 1, 2, ..., 8, 1, ... of them, so the run of deltas below a
    block's ancestor has every length mod 4 (the set kernel adds a run four at a time, then the tail)."""
    n_blocks = fill // 8
    if n_blocks == 0 or n <= 8:
        base = 8 * int(rng.integers(0, max(n_blocks, 1)))
        return base + rng.permutation(min(8, fill))[:n]
    leaves = []
    for k, b in enumerate(rng.permutation(n_blocks)):
        take = min(n - len(leaves), 1 + k % 8)
        if take == 0:
            break
        leaves.extend((8 * b + rng.permutation(8)[:take]).tolist())
    if len(leaves) < n:  # the tree is too small for that mix: top up with leaves not used yet
        rest = np.setdiff1d(np.arange(8 * n_blocks), np.asarray(leaves))
        leaves.extend(rng.permutation(rest)[: n - len(leaves)].tolist())
    return rng.permutation(np.asarray(leaves))


def _window(rng, fill):
    """First leaf of a random aligned block of 8.  The batches of up to 8 pairs stay inside one block: leaves that far apart
    as random ones share only ancestors near the root, and two or three deltas there seldom round differently in another
    order -- a wrong order would pass (tests/test_sum_tree_edges_host.py holds every batch to showing it)."""
    return 8 * int(rng.integers(0, max(fill // 8, 1)))


def set_pattern_indices(pattern, rng, capacity, fill, n):
    """int32 [n] leaf indices of one pattern, or None where the capacity has no n distinct leaves for it."""
    if pattern == "a":  # random, about half the entries forced onto one leaf at random positions
        idx = _window(rng, fill) + rng.integers(0, min(8, fill), n) if n <= 8 else rng.integers(0, fill, n)
        idx[rng.permutation(n)[: n // 2]] = idx[0]
        return _i(idx)
    if pattern == "b":  # every entry on the same leaf
        return _i(np.full(n, rng.integers(0, fill)))
    if n > fill:
        return None
    if pattern == "c":  # descending distinct leaves, about every second leaf of a range: long runs with gaps
        if n <= 8:
            return _i(_window(rng, fill) + np.sort(rng.permutation(min(8, fill))[:n])[::-1])
        return _i(np.sort(rng.permutation(min(fill, 2 * n))[:n])[::-1])
    if pattern == "d":
        return _i(_blocks_of_eight(rng, fill, n))
    if pattern == "e":  # leaf 0 and the last leaf of the tree together with random others
        if n == 1:
            return _i([capacity - 1])
        others = 1 + rng.permutation(min(7, fill - 1) if n <= 8 else fill - 1)[: n - 2]
        others = others[others != capacity - 1]
        while len(others) < n - 2:  # only when capacity - 1 was drawn (capacity == fill)
            extra = 1 + int(rng.integers(0, fill - 1))
            if extra != capacity - 1 and extra not in others:
                others = np.append(others, extra)
        return _i(rng.permutation(np.concatenate([[0, capacity - 1], others])))
    raise ValueError(pattern)


def _set_values(rng, k, idx, pattern):
    """uniform(0, 3) values, exact zeros in every fourth op, float32-typed in every second (as seeded_cases).  With
    duplicates in the batch one LATER occurrence carries a value above everything set before: max_recorded_priority takes
    it although the leaf does not (sum_tree.py:31 is evaluated before np.unique)."""
    n = len(idx)
    vals = rng.uniform(0.0, 3.0, n)
    if k % 4 == 2 and pattern != "b":
        vals[rng.integers(0, n, size=max(1, n // 8))] = 0.0
    later = np.ones(n, bool)
    later[np.unique(idx, return_index=True)[1]] = False
    if later.any():
        vals[rng.choice(np.nonzero(later)[0])] = 3.0 + (k + 1) / 64.0
    if k % 2 == 0 and (pattern != "b" or len(np.unique(vals.astype(np.float32))) == n):  # (b) wants n different values
        return vals.astype(np.float32)
    return vals


def set_case(capacity, pattern, seed):
    fill = min(capacity, 20000)
    rng = np.random.default_rng(seed)
    ops = fill_ops(capacity, rng)
    k = 0
    for n in SET_SIZES:
        idx = set_pattern_indices(pattern, rng, capacity, fill, n)
        if idx is None:
            continue
        ops.append(("set", idx, _set_values(rng, k, idx, pattern)))
        k += 1
    return f"set_c{capacity}_{pattern}", capacity, ops


def set_limit_cases():
    for capacity in SET_CAPACITIES:
        for pattern in SET_PATTERNS:
            yield set_case(capacity, pattern, SET_SEEDS[capacity][pattern])
    # above the kernel limit: SumTree.set de-duplicates on the host and feeds ascending chunks
    capacity, fill = 65536, 20000
    rng = np.random.default_rng(7999)
    ops = fill_ops(capacity, rng)
    for k, n in enumerate((4097, 10000)):  # 4097 with duplicates: one chunk after the host's unique; 10000: two chunks
        idx = set_pattern_indices("a", rng, capacity, fill, n)
        ops.append(("set", idx, _set_values(rng, k, idx, "a")))
    idx = _i(np.arange(30000, 30000 - 4097, -1))  # 4097 distinct, descending: a second chunk of one pair
    ops.append(("set", idx, _set_values(rng, 3, idx, "c")))
    yield "set_c65536_chunked", capacity, ops


# ------------------------------------------------------------------------------------------------ swap-remove
def _swap_pairs(rng, capacity, fill):
    """(a, b, keep) triples; keep: leave the zeroed leaves as they are, the next pair wants leaf[b] == 0."""
    if capacity == 1:
        return [(0, 0, False)] * 3
    if capacity == 2:
        return [(0, 1, False), (1, 0, False)] * 14 + [(0, 0, False), (1, 1, False), (0, 1, True), (0, 1, False), (1, 1, False)]
    if capacity == 3:  # 0 and 1 are siblings; 2 meets them at the root only
        cycle = [(0, 1, False), (1, 0, False), (0, 1, False), (1, 2, False), (1, 0, False), (0, 2, False), (2, 0, False), (2, 1, False)]
        return cycle * 5 + [(2, 2, False), (0, 0, False), (0, 2, True), (1, 2, False), (1, 1, False)]
    leaves = 1 << int(np.ceil(np.log2(capacity)))
    last = fill - 1
    pairs = []
    for d in (1, 2, 3, 5, 17):
        if d >= fill:
            continue
        for _ in range(6):
            a = int(rng.integers(0, fill - d))
            pairs.append((a, a + d) if rng.random() < 0.5 else (a + d, a))  # a > b: the C ABI allows it
    for _ in range(8):  # siblings
        a = 2 * int(rng.integers(0, fill // 2))
        pairs.append((a, a + 1) if rng.random() < 0.5 else (a + 1, a))
    for a in (last - 1, last - 2, int(rng.integers(0, fill // 2))):  # b the last filled leaf: a buffer's eviction
        pairs.append((max(a, 0), last))
    # the root is the only common ancestor
    right = capacity - 1 if capacity > leaves // 2 else None
    if right is not None:
        pairs.append((int(rng.integers(0, min(fill, leaves // 2))), right))
        pairs.append((right, 0))
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    out = [(a, b, False) for a, b in pairs]
    a = int(rng.integers(1, fill - 1))
    out += [(a, a, False), (0, 0, False), (last, last, False)]
    out += [(a, a + 1, True), (a - 1, a + 1, False)]  # the second pair finds leaf[b] == 0
    return out


def swap_remove_cases():
    for capacity in SWAP_CAPACITIES:
        rng = np.random.default_rng(SWAP_SEEDS[capacity])
        fill = min(capacity, TREE_MAX_BATCH)

        def draw(n):
            if capacity == 2:  # the only shared ancestor is the root: uniform(0.1, 2) never separates the add orders there
                return np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
            return rng.uniform(0.1, 2.0, n)

        ops = [("set", np.arange(fill, dtype=np.int32), draw(fill))]
        if capacity > fill:
            ops.append(("set", _i([capacity - 1]), draw(1)))
        zero = set()
        for a, b, keep in _swap_pairs(rng, capacity, fill):
            ops.append(("swap_remove_kernel", int(a), int(b)))
            if b in zero or a == b:
                zero.add(a)
            else:
                zero.discard(a)
            zero.add(b)
            if not keep:  # what the next adds would do: the emptied leaves get fresh priorities
                z = sorted(zero)
                ops.append(("set", _i(z), draw(len(z))))
                zero.clear()
        yield f"swap_c{capacity}", capacity, ops


# ------------------------------------------------------------------------------------------------ query boundaries
QUERY_GROUPS = {}  # case name -> per target, the node whose sum it probes (filled by query_boundary_cases)


def query_boundary_cases():
    from oracle.sum_tree import SumTree as Oracle

    for capacity in QUERY_CAPACITIES:
        rng = np.random.default_rng(8800 + capacity)
        ops = []
        fill = min(capacity, 20000)
        for op in fill_ops(capacity, rng):
            op[2][rng.random(len(op[2])) < 0.1] = 0.0  # some zero leaves
            ops.append(op)
        if capacity > fill:  # a few leaves in the right half, so that paths turn right at the root too
            far = _i(np.sort(rng.permutation(capacity - 600_000)[:300] + 600_000))
            vals = rng.uniform(0.1, 2.0, len(far))
            vals[::7] = 0.0
            ops.append(("set", far, vals))
        tree = Oracle(capacity)
        replay(tree, ops)
        nodes, depth, first = tree._nodes, tree._depth, tree._first_leaf_offset
        root = float(tree.root)
        targets, groups = [0.0, float(np.nextafter(root, 0.0))], [-1, -2]
        positive = np.nonzero(nodes[first:] > 0.0)[0]
        for leaf in rng.choice(positive, 64, replace=False):
            path = [first + int(leaf)]
            while path[-1] != 0:
                path.append((path[-1] - 1) // 2)
            path = path[::-1]
            subtracted = []  # the left sums the descent has subtracted so far, in its own order
            for level in range(depth - 1):
                left = 2 * path[level] + 1
                ls = nodes[left]
                probes = []
                for r in (ls, np.nextafter(ls, np.inf), np.nextafter(ls, -np.inf)):
                    t = r
                    for s in reversed(subtracted):
                        t = t + s
                    probes.append(float(t))
                # one ulp of what the descent subtracts from is coarser than one ulp of ls: the neighbours of the absolute target too
                probes += [float(np.nextafter(probes[0], np.inf)), float(np.nextafter(probes[0], -np.inf))]
                targets += probes
                groups += [left] * len(probes)
                if path[level + 1] != left:
                    subtracted.append(ls)
        t, g = np.asarray(targets, np.float64), np.asarray(groups)
        keep = (t >= 0.0) & (t < root)  # what the oracle rejects is dropped
        t = t[keep]
        QUERY_GROUPS[f"query_c{capacity}"] = g[keep]
        for s in range(0, len(t), TREE_MAX_BATCH):
            ops.append(("query", t[s : s + TREE_MAX_BATCH]))
        yield f"query_c{capacity}", capacity, ops


# ------------------------------------------------------------------------------------------------ replay
def replay_edges(tree, ops, after_op=None):
    """sumtree_cases.replay plus the swap-remove kernel op; ``after_op(op)`` is called after every op."""
    results = []
    for op in ops:
        if op[0] == "swap_remove_kernel":
            a, b = int(op[1]), int(op[2])
            if hasattr(tree, "swap_remove_device"):
                tree.swap_remove_device(a, b)
            elif a == b:
                tree.set(a, 0.0)
            else:
                tree.set(np.asarray([a, b], dtype=np.int32), np.asarray([tree.get(b), 0.0]))
        else:
            results.extend(replay(tree, [op]))
        if after_op is not None:
            after_op(op)
    return results


# ------------------------------------------------------------------------------------------------ the sampler
def sampler_script(capacity, seed, n_ops=3000):
    """Ops for PrioritizedSamplingDistribution(max_capacity=capacity):
         ("add", key, p)                       p a float in [0.05, 5] (log-uniform), 0.0, or MAX_PRIORITY
         ("remove", key)                       an eviction (oldest or random key, once more than `capacity` are live) or a random removal
         ("update" | "update_device", keys, priorities)   with duplicate keys and some zeros
         ("sample", entry, size, rows)         entry one of SAMPLE_ENTRIES; rows > 1 only for "draw_rows"
    Keys are fresh integers; every update / remove names live keys.  At capacity 4096 the script opens with 1150 adds and
    nothing between them: the 1024th is flushed by add() itself."""
    rng = np.random.default_rng(seed)
    ops, live = [], []
    state = dict(key=0, size=32, rotation=0)

    def priority():
        u = rng.random()
        if u < 0.30:
            return MAX_PRIORITY
        if u < 0.36:
            return 0.0
        return float(np.exp(rng.uniform(np.log(0.05), np.log(5.0))))

    def add(evict=True):
        ops.append(("add", state["key"], priority()))
        live.append(state["key"])
        state["key"] += 1
        if evict and len(live) > capacity:
            victim = live[0] if rng.random() < 0.7 else live[int(rng.integers(0, len(live)))]
            live.remove(victim)
            ops.append(("remove", victim))

    def update(kind):
        m = int(rng.choice([1, 5, 32, 33]))
        keys = rng.choice(np.asarray(live), m)
        if m > 1:
            keys[-1] = keys[0]
        pr = np.exp(rng.uniform(np.log(0.05), np.log(5.0), m))
        pr[rng.random(m) < 0.1] = 0.0
        ops.append((kind, keys.astype(np.int32), pr))

    def sample(rows=None):
        entry = SAMPLE_ENTRIES[state["rotation"] % 4]
        state["rotation"] += 1
        if rows is None:
            rows = int(rng.integers(1, 4)) if entry == "draw_rows" else 1
        ops.append(("sample", entry, state["size"], rows if entry == "draw_rows" else 1))

    for _ in range(1150 if capacity >= 4096 else min(capacity, 1000)):
        add(evict=False)
    long_run_done = False
    while len(ops) < n_ops:
        if not long_run_done and len(ops) >= n_ops // 2:
            # one block of PREFETCH batches used up without a size change, with a draw_rows call across its end
            long_run_done = True
            state["size"] = 5 if state["size"] != 5 else 33
            state["rotation"] = 0
            for _ in range(60):
                sample()
            ops.append(("sample", "draw_rows", state["size"], 3))  # batches 60-62
            ops.append(("sample", "draw_rows", state["size"], 4))  # batches 63 | 0-2 of the next block
            for _ in range(8):
                sample()
            continue
        u = rng.random()
        if not live or u < 0.33:
            add()
        elif u < 0.45:
            update("update")
        elif u < 0.57:
            update("update_device")
        elif u < 0.66:
            victim = live[int(rng.integers(0, len(live)))]
            live.remove(victim)
            ops.append(("remove", victim))
        else:
            if rng.random() < 0.35:
                state["size"] = int(rng.choice(SAMPLE_SIZES))
            sample()
    return ops


class SamplerMirror:
    """oracle.samplers.PrioritizedSamplingDistribution plus the staging the device sampler documents: adds wait in a list;
    whatever flushes on the device (a sample, an update, a remove, the MAX_PENDING-th staged add) applies them as ONE set
    over the block, every MAX_PRIORITY entry resolved to the tree's max_recorded_priority BEFORE that block.  A power-of-two
    capacity gets the spare leaf the device sampler adds."""

    def __init__(self, seed, capacity, priority_exponent=1.0):
        from oracle.samplers import PrioritizedSamplingDistribution

        leaves = capacity + 1 if capacity & (capacity - 1) == 0 else capacity
        self.o = PrioritizedSamplingDistribution(seed, leaves, priority_exponent)
        self.pending = []

    @property
    def tree(self):
        return self.o._sum_tree

    def flush(self):
        if not self.pending:
            return False
        top = float(self.tree.max_recorded_priority)
        idx = np.asarray([i for i, _ in self.pending], np.int32)
        val = np.asarray([top if v is None else v for _, v in self.pending], np.float64)
        self.pending = []
        self.tree.set(idx, val)
        return True

    def add(self, key, p):
        """True when this add flushed the staged block."""
        from oracle.samplers import UniformSamplingDistribution

        UniformSamplingDistribution.add(self.o, key)
        self.pending.append((self.o._key_to_index[key], None if isinstance(p, str) else float(self.o._transform(p))))
        return len(self.pending) >= MAX_PENDING and self.flush()

    def update(self, keys, priorities):
        self.flush()
        self.o.update(keys, priorities)

    def remove(self, key):
        self.flush()
        self.o.remove(key)

    def draw(self, size):
        """The dense indices of one reference batch: uniform(0, root, size) -> SumTree.query."""
        return self.tree.query(self.o._rng_key.uniform(0.0, self.tree.root, size))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run_sampler_script(ops, mirror, dev=None, exact_update_device=True):
    """Runs the script on the mirror and, when given, on the device sampler ``dev``, asserting after every flushing op that
    the node bits and max_recorded_priority are equal, after every sampling op that the dense indices are equal (and the keys,
    whenever every index is below the live count), at the end that the key tables are equal and the status word is clean.
    Sampling ops are skipped while the oracle's root is not positive (the reference raises there).  Returns the statistics
    tests/test_sum_tree_edges_host.py holds the committed scripts to."""
    import collections

    stats = collections.Counter()
    block_size, block_used = None, 0
    o = mirror.o

    def same_tree(what):
        if dev is None:
            return
        a, b = dev._tree._nodes, mirror.tree._nodes
        assert not dev._pend_idx, f"{what}: adds still staged"
        bad = np.nonzero(_bits(a) != _bits(b))[0]
        assert bad.size == 0, f"{what}: {bad.size} nodes differ; first: node {bad[0]}, device {a[bad[0]]!r}, oracle {b[bad[0]]!r}"
        assert dev._tree.max_recorded_priority == float(mirror.tree.max_recorded_priority), what

    for n_op, op in enumerate(ops):
        kind = op[0]
        what = f"op {n_op} {kind}"
        if kind == "add":
            _, key, p = op
            flushed = mirror.add(key, p)
            if dev is not None:
                dev.add(key, p)
            stats["add"] += 1
            stats["add_max"] += isinstance(p, str)
            if flushed:
                stats["auto_flush"] += 1
                same_tree(what)
        elif kind in ("update", "update_device"):
            _, keys, pr = op
            if kind == "update_device" and not exact_update_device:
                kind = "update"  # update_device's pow is outside the bit-exact contract
            mirror.update(keys, pr)
            if dev is not None:
                if kind == "update":
                    dev.update(keys, pr)
                else:
                    import torch

                    idx = np.asarray([dev._key_to_index[k] for k in keys.tolist()], np.int32)
                    dev.update_device(torch.from_numpy(idx).to(dev.device), torch.from_numpy(pr).to(dev.device))
            stats[kind] += 1
            same_tree(what)
        elif kind == "remove":
            mirror.remove(op[1])
            if dev is not None:
                dev.remove(op[1])
            stats["remove"] += 1
            same_tree(what)
        elif kind == "sample":
            _, entry, size, rows = op
            mirror.flush()
            if not mirror.tree.root > 0.0:
                stats["sample_skipped"] += 1
                continue
            live = len(o._index_to_key)
            if dev is not None:
                if entry == "draw_rows":
                    units = dev.draw_rows_device(rows, size)
                    got = [dev._sum_tree.query_device(units[r], unit=True).cpu().numpy() for r in range(rows)]
                elif entry == "sample":
                    got = [np.asarray([dev._key_to_index[k] for k in dev.sample(size).tolist()], np.int32)]
                elif entry == "sample_device":
                    got = [dev.sample_device(size).cpu().numpy()]
                else:
                    idx, weights = dev.sample_weighted_device(size, 0.5)
                    w = weights.cpu().numpy()
                    assert w.shape == (size,) and np.isfinite(w).all() and (w > 0).all() and (w <= 1).all(), what
                    got = [idx.cpu().numpy()]
            for r in range(rows):
                if size != block_size or block_used >= PREFETCH:
                    stats["mid_block_size_change"] += block_size is not None and size != block_size and 0 < block_used < PREFETCH
                    stats["block_used_up"] += block_size == size and block_used >= PREFETCH
                    block_size, block_used = size, 0
                block_used += 1
                want = mirror.draw(size)
                valid = bool((want < live).all())
                stats["batches"] += 1
                stats["key_comparison_lost"] += not valid
                if dev is not None:
                    np.testing.assert_array_equal(got[r], want, err_msg=f"{what} ({entry}, size {size}, row {r})")
                    if valid:
                        assert dev.keys_of(got[r]).tolist() == [o._index_to_key[i] for i in want], what
            stats["sample"] += 1
            stats["via_" + entry] += 1
            same_tree(what)
        else:
            raise ValueError(kind)
    mirror.flush()
    if dev is not None:
        dev.flush()
        same_tree("end")
        assert dev._index_to_key == o._index_to_key and dev._key_to_index == o._key_to_index
        assert int(dev._tree._status.item()) == 0, "status word not clean"
    return stats
