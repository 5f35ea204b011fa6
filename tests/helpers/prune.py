"""numpy restatement of the definition of include/isdqn_hip.h, isdqn_net_prune_* -- gradual magnitude pruning -- on the flat parameter
vector of the internal layout, the wrong variants the tests must be able to tell from it (the pattern of tests/helpers/soft_shift.py: each
wrong variant is first shown to differ from the definition on the test's own inputs), and the schedule restated from the issue's formula.

Which elements are REAL is derived here from the engine's own import path, not from the library: a Flax-shaped array of ones through
``_to_internal`` is 1 at real positions and 0 at every padded lane and row.  A QNetEngine or a tests.helpers.redo.HostLayout can be passed
as ``lay``.  The selection is a stable sort on (key, index): key 0 for an element the old mask says pruned, else 1 + the bits of |w|."""
import math

import numpy as np

U32 = np.uint32


def prunable(lay):
    """The prunable tensor infos in layout order: kinds 0 and 1 but the last Dense."""
    kernels = [i for i in lay.infos if int(i.kind) in (0, 1)]
    assert int(kernels[-1].kind) == 1
    return kernels[:-1]


def real_index(lay, info, padding_counts=False):
    """Flat buffer indices of the real elements of ``info`` in ascending order (``padding_counts``: the WRONG variant, every internal
    element)."""
    if padding_counts:
        return np.arange(int(info.offset), int(info.offset + info.size), dtype=np.int64)
    shape = tuple(int(x) for x in info.flax_shape[: info.ndim])
    ones = lay._to_internal(info, np.ones(shape, np.float32))
    assert ones.size == int(info.size)
    return int(info.offset) + np.flatnonzero(ones).astype(np.int64)


def real_counts(lay):
    return [int(np.prod([int(x) for x in i.flax_shape[: i.ndim]])) for i in prunable(lay)]


def mask_words(lay):
    return (int(lay.n_param_floats) + 31) // 32


def full_mask(lay):
    return np.full(mask_words(lay), 0xFFFFFFFF, U32)


def get_bits(mask, idx):
    return ((mask[idx >> 5] >> (idx & 31).astype(U32)) & U32(1)).astype(bool)


def keys(params, mask, idx, pruned_first=True):
    """The 33-bit order as int64; ``pruned_first`` False: the WRONG variant that ranks an already pruned element by its magnitude."""
    w = np.ascontiguousarray(params, dtype=np.float32).view(U32)[idx].astype(np.int64) & 0x7FFFFFFF
    k = 1 + w
    if pruned_first:
        k[~get_bits(mask, idx)] = 0
    return k


def select(lay, params, mask, counts, *, ties_high=False, pruned_first=True, padding_counts=False):
    """The new mask words (uint32) of isdqn_net_prune_update: per tensor the counts[i] smallest (key, index) cleared, every other real
    bit set, no other bit touched.  Keyword arguments select the WRONG variants."""
    new = np.array(mask, dtype=U32, copy=True)
    for info, k in zip(prunable(lay), counts):
        idx = real_index(lay, info, padding_counts)
        assert 0 <= k <= idx.size
        key = keys(params, mask, idx, pruned_first)
        order = np.lexsort((-idx if ties_high else idx, key))  # (last key is the primary one)
        pruned = np.zeros(idx.size, bool)
        pruned[order[:k]] = True
        np.bitwise_or.at(new, idx[~pruned] >> 5, (U32(1) << (idx[~pruned] & 31).astype(U32)))
        np.bitwise_and.at(new, idx[pruned] >> 5, ~(U32(1) << (idx[pruned] & 31).astype(U32)))
    return new


def span(lay):
    t = prunable(lay)
    return int(t[0].offset), int(t[-1].offset + t[-1].size)


def apply(lay, params, mask):
    """isdqn_net_prune_apply on a host copy: +0.0 wherever a bit is clear inside the prunable span."""
    p = np.array(params, dtype=np.float32, copy=True)
    lo, hi = span(lay)
    idx = np.arange(lo, hi, dtype=np.int64)
    p[idx[~get_bits(mask, idx)]] = np.float32(0.0)
    return p


def update(lay, params, mask, counts):
    new = select(lay, params, mask, counts)
    return new, apply(lay, params, new)


def pruned_index(lay, mask):
    """Flat indices of all real prunable elements the mask says pruned."""
    out = [idx[~get_bits(mask, idx)] for idx in (real_index(lay, i) for i in prunable(lay))]
    return np.concatenate(out)


def popcount_pruned(lay, mask):
    return [int((~get_bits(mask, real_index(lay, i))).sum()) for i in prunable(lay)]


def bits(a):
    return np.ascontiguousarray(a).view(U32)


# ---- the schedule, from the formula (float64) ----
def sparsity(t, S, t0, t1):
    if t < t0:
        return 0.0
    if t >= t1:
        return float(S)
    return float(S) * (1.0 - (1.0 - (t - t0) / (t1 - t0)) ** 3)


def counts_at(t, S, t0, t1, n_real, previous=None):
    k = [int(math.floor(sparsity(t, S, t0, t1) * n)) for n in n_real]
    return k if previous is None else [max(a, b) for a, b in zip(k, previous)]


# ---- the networks of the device tests (tests/test_gpu_prune.py, tests/test_gpu_prune_bounds.py) ----
FC_SMALL = dict(observation_dim=(8,), n_actions=4, n_heads=3, features=(20, 14), architecture_type="fc", layer_norm=False, batch_size=4)
FC_WIDE = dict(observation_dim=(8,), n_actions=4, n_heads=3, features=(256, 256), architecture_type="fc", layer_norm=False, batch_size=4)
CNN = dict(observation_dim=(84, 84, 4), n_actions=4, n_heads=3, features=(8, 8, 8, 16), architecture_type="cnn", layer_norm=True, batch_size=4)


def make_engine(c, **extra):
    """The QNetEngine of one of the configurations above (a GPU is needed)."""
    from slimdqn._engine import QNetEngine

    return QNetEngine(c["observation_dim"], c["n_actions"], c["n_heads"], c["features"], c["architecture_type"], c["layer_norm"],
                      c["batch_size"], **extra)


def host_layout(c):
    from tests.helpers.redo import HostLayout

    return HostLayout(c["observation_dim"], c["n_actions"], c["n_heads"], c["features"], c["architecture_type"], c["layer_norm"], c["batch_size"])


SENTINEL = np.float32(-1e-3)  # smaller in magnitude than most real values: a selection that counted padding lanes would take them first


def case_params(lay, case, seed=0):
    """A flat parameter buffer for the named case: real prunable elements hold the case's values, every other float of the buffer --
    padding lanes, biases, the last Dense -- SENTINEL, which must survive."""
    rng = np.random.default_rng(seed)
    p = np.full(int(lay.n_param_floats), SENTINEL, np.float32)
    for info in prunable(lay):
        idx = real_index(lay, info)
        n = idx.size
        if case == "normal":
            v = rng.standard_normal(n).astype(np.float32)
        elif case == "equal":
            v = np.full(n, 0.25, np.float32)
        elif case == "levels":  # three magnitudes with mixed signs, -0.0, denormals, one inf
            v = rng.choice(np.array([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], np.float32), n)
            v[rng.integers(0, n, max(n // 16, 1))] = np.float32(-0.0)
            v[rng.integers(0, n, max(n // 16, 1))] = np.float32(1e-40)
            v[rng.integers(0, n, max(n // 16, 1))] = np.float32(-3e-41)
            v[int(rng.integers(0, n))] = np.float32(np.inf)
        else:
            raise KeyError(case)
        p[idx] = v
    return p
