"""AdamW restated in numpy, independent of the kernels (include/isdqn_hip.h, isdqn_batch_decay -- THE definition).

  decay32      the definition itself on top of a given Adam result p1: fl32(p1 - fl32(lr * fl32(wd * p0))), three float32 roundings, no FMA
               (numpy's float32 array arithmetic rounds every operation once);
  adamw64      one AdamW step in float64 in optax's form: p0 - lr * (m_hat / (sqrt(v_hat) + eps) + wd * p0);
  decay_mask   which elements of the flat internal parameter buffer decay under a kind mask (TensorInfo.kind);
  decay_bound  what the definition's two extra roundings may add to tests.gpu_helpers.adam_bounds' bound on p."""
import numpy as np

KINDS_KERNELS, KINDS_ALL = 0x03, 0x7F  # include/isdqn_hip.h: ISDQN_DECAY_KINDS_KERNELS / _ALL (kinds 7, 8: running statistics, never)
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))  # the float32 constants the kernels hold (tests/gpu_helpers.py)


def decay32(p1, p0, lr, wd):
    """p_new of the definition for float32 arrays p1 (Adam's result) and p0 (the element before the step)."""
    p1, p0 = np.asarray(p1, np.float32), np.asarray(p0, np.float32)
    lr, wd = np.float32(lr), np.float32(wd)
    t = (wd * p0).astype(np.float32)
    t = (lr * t).astype(np.float32)
    return (p1 - t).astype(np.float32)


def adamw64(p0, m0, v0, g, t, lr, eps, wd, b1=B1, b2=B2):
    """optax.adamw on float64 copies (scale_by_adam, add_decayed_weights, scale(-lr)): new p, m, v.  ``t``: the count after the increment."""
    p0, m0, v0, g = (np.asarray(a, np.float64) for a in (p0, m0, v0, g))
    m = b1 * m0 + (1 - b1) * g
    v = b2 * v0 + (1 - b2) * (g * g)
    u = (m / (1.0 - b1**t)) / (np.sqrt(v / (1.0 - b2**t)) + eps)
    return p0 - lr * (u + wd * p0), m, v


def decay_mask(infos, n_floats, kinds):
    """bool [n_floats]: True on every element of a tensor whose kind has its bit in ``kinds`` (``infos``: objects with offset, size, kind)."""
    mask = np.zeros(n_floats, bool)
    for info in infos:
        if (int(kinds) >> int(info.kind)) & 1:
            mask[info.offset : info.offset + info.size] = True
    return mask


def decay_bound(p0, p_new, lr, wd):
    """Error the decay adds to a float32 Adam step measured against float64 AdamW, per element, given adam_bounds' bound on p1:
    fl32(wd * p0) and fl32(lr * .) are within (2 u + u^2) of lr * wd * |p0| together (u = 2^-24; + one denormal spacing each, the
    absolute floor of a rounding), and the subtraction rounds p_new once more: half a spacing of p_new.  (adam_bounds already holds
    half a spacing of p1 for the rounding of p1 itself, which the kernel does perform.)"""
    u, tiny = 2.0**-24, 2.0**-149
    p0 = np.abs(np.asarray(p0, np.float64))
    return (2 * u + u * u) * lr * wd * p0 + 2 * tiny + 0.5 * np.spacing(np.abs(np.asarray(p_new)).astype(np.float32)).astype(np.float64)
