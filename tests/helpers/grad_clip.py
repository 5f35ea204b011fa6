"""float64 restatement of clipping by the global norm, written from the header text alone (include/isdqn_hip.h,
isdqn_net_config::max_grad_norm; optax.clip_by_global_norm):

    n     = sqrt( sum over every element of every leaf of g^2 )        (structural zeros of a dueling head kernel masked out)
    scale = 1 if n < c or n == 0, else c / n
    Adam consumes g * scale

and the wrong readings the GPU tests must be able to tell from it.  numpy only."""
import numpy as np


def _leaves(leaves):
    return [np.asarray(g, np.float64) for g in leaves]


def global_norm(leaves, live_masks=None):
    """One norm over all leaves together.  ``live_masks``: per leaf None or a bool array of the leaf's shape, False on the
    elements that are not part of the norm."""
    total = 0.0
    for k, g in enumerate(_leaves(leaves)):
        if live_masks is not None and live_masks[k] is not None:
            g = np.where(live_masks[k], g, 0.0)
        total += float(np.sum(g * g))
    return float(np.sqrt(total))


def clip_scale(n, c):
    n, c = float(n), float(c)
    return 1.0 if (n < c or n == 0.0) else c / n


def clipped(leaves, c, live_masks=None):
    """The gradient Adam consumes: every leaf times the one scale (masked elements are zero)."""
    s = clip_scale(global_norm(leaves, live_masks), c)
    out = []
    for k, g in enumerate(_leaves(leaves)):
        if live_masks is not None and live_masks[k] is not None:
            g = np.where(live_masks[k], g, 0.0)
        out.append(g * s)
    return out


# ---- wrong readings (each returns what Adam would consume, leaf by leaf)
def per_leaf_norms(leaves, c, live_masks=None):
    """every leaf clipped by its own norm"""
    return [clipped([g], c, None if live_masks is None else [live_masks[k]])[0] for k, g in enumerate(leaves)]


def norm_with_structural(leaves, c, live_masks=None):
    """the norm taken over the raw gradient, the dueling head's structural entries included (the entries themselves still masked)"""
    s = clip_scale(global_norm(leaves, None), c)
    return [np.where(True if live_masks is None or live_masks[k] is None else live_masks[k], g, 0.0) * s for k, g in enumerate(_leaves(leaves))]


def l1_norm(leaves, c, live_masks=None):
    n1 = sum(float(np.abs(g).sum()) for g in clipped(leaves, np.inf, live_masks))
    s = clip_scale(n1, c)
    return [g * s for g in clipped(leaves, np.inf, live_masks)]


def clip_by_value(leaves, c, live_masks=None):
    return [np.clip(g, -c, c) for g in clipped(leaves, np.inf, live_masks)]


def always_scaled(leaves, c, live_masks=None):
    """c / (n + 1e-6) without the n < c test: a gradient below the threshold is scaled UP"""
    n = global_norm(leaves, live_masks)
    s = float(c) / (n + 1e-6)
    return [g * s for g in clipped(leaves, np.inf, live_masks)]


WRONG = {"per_leaf_norms": per_leaf_norms, "norm_with_structural": norm_with_structural, "l1_norm": l1_norm, "clip_by_value": clip_by_value,
         "always_scaled": always_scaled}
