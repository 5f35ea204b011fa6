"""float64 numpy restatement of the definition of include/isdqn_hip.h, isdqn_net_project_* -- Normalize-and-Project -- on the flat parameter
vector of the internal layout, and the wrong variants the tests must be able to tell from it (the pattern of tests/helpers/prune.py: each
wrong variant is first shown to differ from the definition on the tests' own inputs, tests/test_nap_host.py).

Which elements are REAL comes from tests/helpers/prune.real_index (the engine's own import path, not the library).  S_i is math.fsum of
the exact float64 squares: the correctly rounded sum, against which ANY order of N float64 additions of non-negative terms is within
N * 2^-53 relative.  A QNetEngine or a tests.helpers.redo.HostLayout can be passed as ``lay``."""
import math

import numpy as np

from tests.helpers import prune as hp

F32, F64 = np.float32, np.float64
VARIANTS = ("padding", "last_dense", "biases", "per_row", "fp32")

# every float of the buffer that is no real projected element -- padding lanes and rows, biases, LayerNorm vectors, the last Dense --
# holds this: large enough that a norm which counted any of them moves the scale by far more than 16 fp32 ulps (tests/test_nap_host.py
# asserts it), and no value a projected element of the cases below takes
SENTINEL = F32(-0.75)


def projected(lay, last_dense=False):
    """The projected tensor infos in layout order: pruning's (``last_dense``: the WRONG variant that takes the last Dense too)."""
    return [i for i in lay.infos if int(i.kind) in (0, 1)] if last_dense else hp.prunable(lay)


def _bias_of(lay, info):
    return next(i for i in lay.infos if int(i.layer) == int(info.layer) and int(i.kind) == 2)


def _rows(lay, info, idx):
    """The output row (Flax's last axis) of every flat index of ``idx``."""
    shape = tuple(int(x) for x in info.flax_shape[: info.ndim])
    ids = np.broadcast_to(np.arange(1, shape[-1] + 1, dtype=F32), shape)
    internal = lay._to_internal(info, np.ascontiguousarray(ids))
    rows = internal[idx - int(info.offset)].astype(np.int64) - 1
    assert (rows >= 0).all()
    return rows


def sumsq(w, fp32=False):
    """S of the float32 values ``w``: fsum of the exact float64 squares (``fp32``: the WRONG variant, a running float32 sum)."""
    w = np.ascontiguousarray(w, dtype=F32)
    if fp32:
        return float(np.cumsum(w * w, dtype=F32)[-1]) if w.size else 0.0
    return math.fsum((w.astype(F64) ** 2).tolist())


def scale_of(rho, norm):
    """s_i of the definition from rho_i and n_i (float64): 1.0f where the tensor is left alone (sqrt(S) is 0, inf or NaN exactly where S
    is)."""
    if not (norm > 0.0 and math.isfinite(norm) and rho > 0.0 and math.isfinite(rho)):
        return F32(1.0)
    with np.errstate(over="ignore"):
        return F32(F64(rho) / F64(norm))


def _fsum_or_special(w):
    """sumsq, with inf / NaN members handled as IEEE addition of non-negative squares would."""
    if np.isnan(w).any():
        return float("nan")
    if np.isinf(w).any():
        return float("inf")
    return sumsq(w)


def _norm(w):
    S = _fsum_or_special(w)
    return math.sqrt(S) if S == S else float("nan")


def norms(lay, params):
    """n_i of every projected tensor of the definition, with the correctly rounded sum."""
    p = np.ascontiguousarray(params, dtype=F32)
    return [_norm(p[hp.real_index(lay, i)]) for i in projected(lay)]


def scaled(lay, params, scales):
    """The buffer after the projection with the given per-tensor float32 scales: every real element of tensor i becomes fl32(w * s_i)
    (one float32 multiply), every other float keeps its bits; a tensor whose scale is 1.0f is not written."""
    out = np.array(params, dtype=F32, copy=True)
    for info, s in zip(projected(lay), scales):
        if F32(s) == F32(1.0):
            continue
        idx = hp.real_index(lay, info)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            out[idx] = out[idx] * F32(s)
    return out


def project(lay, params, rhos, variant=None):
    """(new buffer, norms, scales) of one projection.  ``variant`` None: the definition.  Otherwise one of VARIANTS, each WRONG:
    "padding" counts and scales every internal element; "last_dense" projects the last Dense too (``rhos`` then has one more entry);
    "biases" takes the layer's bias into the tensor, norm and scaling; "per_row" gives every output row the norm rho_i / sqrt(rows) (its
    norms and scales are arrays per row); "fp32" accumulates S in float32."""
    assert variant is None or variant in VARIANTS
    out = np.array(params, dtype=F32, copy=True)
    tensors = projected(lay, last_dense=variant == "last_dense")
    assert len(rhos) == len(tensors)
    all_norms, all_scales = [], []
    for info, rho in zip(tensors, rhos):
        idx = hp.real_index(lay, info, padding_counts=variant == "padding")
        if variant == "biases":
            b = _bias_of(lay, info)
            idx = np.concatenate([idx, hp.real_index(lay, b)])
        if variant == "per_row":
            rows = _rows(lay, info, idx)
            n_rows = int(rows.max()) + 1
            nr = np.array([_norm(out[idx[rows == r]]) for r in range(n_rows)])
            sr = np.array([scale_of(rho / math.sqrt(n_rows), n) for n in nr], dtype=F32)
            out[idx] = out[idx] * sr[rows]
            all_norms.append(nr)
            all_scales.append(sr)
            continue
        n = math.sqrt(sumsq(out[idx], fp32=True)) if variant == "fp32" else _norm(out[idx])
        s = scale_of(rho, n)
        if s != F32(1.0):
            with np.errstate(over="ignore", invalid="ignore", under="ignore"):
                out[idx] = out[idx] * s
        all_norms.append(n)
        all_scales.append(s)
    return out, all_norms, all_scales


def ulps(a, b):
    """Distance of two positive finite float32 in units of the last place."""
    return abs(int(np.array(a, F32).view(np.int32)) - int(np.array(b, F32).view(np.int32)))


# ---- the inputs of the device tests (tests/test_gpu_nap.py) and of the host tests that vet the oracle on them ----
CASES = ("normal", "zero", "nonfinite", "denormal")


def case_params(lay, case, seed=0):
    """A flat parameter buffer for the named case: real projected elements hold the case's values, every other float SENTINEL.
    "normal": standard normal draws.  "zero": tensor 0 is all +0.0 / -0.0.  "nonfinite": tensor 0 holds one inf, tensor 1 one NaN.
    "denormal": normal draws with every eighth element a float32 denormal of either sign."""
    rng = np.random.default_rng(seed)
    p = np.full(int(lay.n_param_floats), SENTINEL, F32)
    for t, info in enumerate(projected(lay)):
        idx = hp.real_index(lay, info)
        v = rng.standard_normal(idx.size).astype(F32)
        if case == "zero" and t == 0:
            v[:] = 0.0
            v[::3] = F32(-0.0)
        elif case == "nonfinite" and t < 2:
            v[int(rng.integers(0, idx.size))] = F32(np.inf) if t == 0 else F32(np.nan)
        elif case == "denormal":
            v[::8] = F32(1e-40)
            v[4::16] = F32(-3e-41)
        elif case not in CASES:
            raise KeyError(case)
        assert not (v == SENTINEL).any()
        p[idx] = v
    return p


def case_targets(lay):
    """Target norms of the device tests: positive, different per tensor, none of them the norm a case's tensor already has."""
    return [1.5 + 0.75 * t for t in range(len(projected(lay)))]


def not_projected(lay):
    """Mask over the flat buffer: True at every float that is no real projected element."""
    keep = np.ones(int(lay.n_param_floats), bool)
    for info in projected(lay):
        keep[hp.real_index(lay, info)] = False
    return keep
