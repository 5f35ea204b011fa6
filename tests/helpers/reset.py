"""numpy float32 restatements of the two definitions of include/isdqn_hip.h -- isdqn_net_reset (shrink-and-perturb resets) and
isdqn_net_ema (EMA targets) -- on flat buffers of the internal layout, driven by the tensor-info table, and the wrong variants the tests
must be able to tell from them (the pattern of tests/helpers/sum_tree_edges.py: each wrong variant is first shown to differ from the
definition on the test's own inputs, so that a device result that equals the definition cannot equal a variant).

Every product and every sum below is ONE float32 numpy operation on float32 operands: fl32(s * p), fl32(q * f), then their fl32 sum --
what __fmul_rn / __fadd_rn compute.  A QNetEngine or a tests.helpers.redo.HostLayout can be passed as ``lay``."""
import numpy as np

F32 = np.float32


def layout_numbers(lay):
    """(n_layers, first_dense_layer) from the tensor table alone: the layer list is indexed 0 .. max(info.layer); the first Dense layer
    is the lowest layer that holds a Dense kernel (kind 1)."""
    return max(int(i.layer) for i in lay.infos) + 1, min(int(i.layer) for i in lay.infos if int(i.kind) == 1)


def _classes(lay, split_layer, by_kind=False):
    """Per tensor: True = upper.  ``by_kind``: the wrong rule 'Dense kernels and everything of a Dense layer found by KIND' -- upper iff the
    tensor is a Dense kernel (kind 1) or a plain bias (kind 2), whatever its layer."""
    if by_kind:
        return [int(i.kind) in (1, 2) for i in lay.infos]
    return [int(i.layer) >= int(split_layer) for i in lay.infos]


def _blend(s, q, p, f, read_p_when_s_is_zero=False, fma=False):
    s, q = F32(s), F32(q)
    with np.errstate(invalid="ignore", over="ignore"):
        if s == 0 and not read_p_when_s_is_zero:
            return (q * f).astype(F32)
        if fma:  # fl32(s * p + fl32(q * f)) with the first product unrounded: what a contracted v_fma_f32 gives (float64 holds s * p exactly)
            return (np.float64(s) * p.astype(np.float64) + (q * f).astype(F32).astype(np.float64)).astype(F32)
        return ((s * p).astype(F32) + (q * f).astype(F32)).astype(F32)


def reset(lay, params, adam_m, adam_v, adam_count, fresh, split_layer, lower, upper, *, by_kind=False, moments="rule",
          read_p_when_s_is_zero=False, fma=False):
    """isdqn_net_reset on host copies; returns new (params, adam_m, adam_v, adam_count).  ``lower`` / ``upper``: the factor pairs (s, q);
    ``adam_m`` / ``adam_v`` may both be None, ``adam_count`` None (left alone).  The keyword arguments select the WRONG variants:
    ``by_kind`` (class by tensor kind instead of by layer), ``moments`` = "everywhere" / "nowhere" (cleared over every tensor / kept
    over every tensor, instead of exactly where parameters are written), ``read_p_when_s_is_zero`` (s * p + q * f with s = 0: a NaN or
    Inf parameter survives as NaN), ``fma`` (the sum contracted with the first product)."""
    p = np.array(params, dtype=F32, copy=True)
    m = None if adam_m is None else np.array(adam_m, dtype=F32, copy=True)
    v = None if adam_v is None else np.array(adam_v, dtype=F32, copy=True)
    f = np.asarray(fresh, F32)
    for info, is_upper in zip(lay.infos, _classes(lay, split_layer, by_kind)):
        s, q = upper if is_upper else lower
        sl = slice(int(info.offset), int(info.offset) + int(info.size))
        touched = not (F32(s) == 1 and F32(q) == 0)
        if touched:
            p[sl] = _blend(s, q, p[sl], f[sl], read_p_when_s_is_zero, fma)
        if m is not None and (moments == "everywhere" or (moments == "rule" and touched)):
            m[sl] = 0
            v[sl] = 0
    count = None if adam_count is None else np.zeros_like(np.asarray(adam_count))
    return p, m, v, count


WRONG_RESETS = {
    "class by kind": dict(by_kind=True),
    "moments cleared everywhere": dict(moments="everywhere"),
    "moments kept everywhere": dict(moments="nowhere"),
    "p read when s == 0": dict(read_p_when_s_is_zero=True),
    "fma-contracted sum": dict(fma=True),
}


def ema(target, online, tau, lerp=False):
    """isdqn_net_ema on host copies: t' = fl32(fl32(omt * t) + fl32(tau * p)), omt = fl32(1 - tau); tau = 0 leaves the target, tau = 1
    copies the bits of ``online``.  ``lerp``: the WRONG variant t + tau * (p - t)."""
    t, p, tau = np.array(target, dtype=F32, copy=True), np.asarray(online, F32), F32(tau)
    if tau == 0:
        return t
    if tau == 1:
        return p.copy()
    if lerp:
        return (t + (tau * (p - t).astype(F32)).astype(F32)).astype(F32)
    omt = F32(1.0) - tau
    return ((omt * t).astype(F32) + (tau * p).astype(F32)).astype(F32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
