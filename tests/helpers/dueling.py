"""float64 restatement of the dueling value / advantage heads, written from the header text alone (include/isdqn_hip.h,
isdqn_net_config::dueling).  Torch, so that the gradient can also come from autograd.

With w = max(n_bins, n_quantiles, 1), A actions, H heads and F the width of the last hidden Dense (F2 = F / 2):

  raw head    R = H * (A + 1) * w outputs; output ((h * (A + 1)) + c) * w + j is head h, stream row c, component j; c < A is
              advantage a = c, c = A is the value;
  streams     the value rows read the hidden units [0, F2), the advantage rows [F2, F); every other weight of the (F, R) kernel is
              a structural zero;
  combine     out[(h * A + a) * w + j] = raw[A][j] + (raw[a][j] - (sum_a raw[a][j]) / A);
  backward    draw[A][j] = sum_a d[a][j], draw[a][j] = d[a][j] - draw[A][j] / A.

The float64 network of the GPU tests is oracle.network.forward with R outputs and the head kernel multiplied by ``live_mask``, then
``combine``; the existing float64 loss helpers of this directory take the combined rows."""
import numpy as np
import torch


def raw_width(H, A, w=1):
    return H * (A + 1) * w


def raw_index(h, c, j, A, w=1):
    """Output index of head h, stream row c (c < A: advantage c; c = A: the value), component j."""
    return (h * (A + 1) + c) * w + j


def live_mask(F, H, A, w=1):
    """bool (F, R) over the head's Flax kernel: True where a weight lives, False on a structural zero."""
    F2 = F // 2
    m = np.zeros((F, raw_width(H, A, w)), bool)
    for h in range(H):
        for c in range(A + 1):
            for j in range(w):
                o = raw_index(h, c, j, A, w)
                if c == A:
                    m[:F2, o] = True
                else:
                    m[F2:F, o] = True
    return m


def structural_indices(F, in_p, H, A, w=1):
    """Offsets of the structural zeros inside the head kernel's INTERNAL form [R padded][in_p] ([out][in], in_p = F padded to 8),
    ascending: row o, columns [F2, F) of a value row and [0, F2) of an advantage row.  The padded columns [F, in_p) and the padded rows
    are not among them (they are padding, zero for every network)."""
    F2 = F // 2
    out = []
    for o in range(raw_width(H, A, w)):
        value = (o // w) % (A + 1) == A
        cols = range(F2, F) if value else range(0, F2)
        out.extend(o * in_p + c for c in cols)
    return np.asarray(out, np.int64)


def combine(raw, H, A, w=1):
    """[n, R] raw rows -> [n, H * A * w] combined rows (torch float64, differentiable)."""
    raw = torch.as_tensor(raw, dtype=torch.float64)
    r = raw.reshape(raw.shape[0], H, A + 1, w)
    adv, val = r[:, :, :A], r[:, :, A:]
    mean = adv.sum(2, keepdim=True) / A
    return (val + (adv - mean)).reshape(raw.shape[0], H * A * w)


def combine_loops(raw, H, A, w=1):
    """The same by plain loops over (row, head, j) on Python floats: an independent reading of the header."""
    raw = np.asarray(raw, np.float64)
    out = np.zeros((raw.shape[0], H * A * w))
    for n in range(raw.shape[0]):
        for h in range(H):
            for j in range(w):
                s = 0.0
                for a in range(A):
                    s += raw[n, raw_index(h, a, j, A, w)]
                mean = s / A
                for a in range(A):
                    out[n, (h * A + a) * w + j] = raw[n, raw_index(h, A, j, A, w)] + (raw[n, raw_index(h, a, j, A, w)] - mean)
    return out


def backward(d, H, A, w=1):
    """[n, H * A * w] gradient w.r.t. the combined rows -> [n, R] gradient w.r.t. the raw rows (numpy float64).  A vector (the reduced
    head-bias gradient) goes through the same map."""
    d = np.asarray(d, np.float64)
    one = d.ndim == 1
    x = d.reshape(-1, H, A, w)
    s = np.zeros((x.shape[0], H, w))
    for a in range(A):  # ascending a
        s = s + x[:, :, a]
    out = np.concatenate([x - (s / A)[:, :, None], s[:, :, None]], axis=2).reshape(x.shape[0], raw_width(H, A, w))
    return out[0] if one else out


def combine_bound(raw, H, A, w=1, u=2.0**-24):
    """Bound of |fp32 combine - exact| per combined output, [n, H * A * w]: the A-term sum, one division, one subtraction and one
    addition give (A + 2) u (|V| + 2 max_a |adv_a|)."""
    r = np.abs(np.asarray(raw, np.float64)).reshape(-1, H, A + 1, w)
    b = (A + 2) * u * (r[:, :, A] + 2.0 * r[:, :, :A].max(2))  # [n, H, w]
    return np.broadcast_to(b[:, :, None, :], (r.shape[0], H, A, w)).reshape(r.shape[0], H * A * w)


FLOOR = 2.0**-126  # the smallest normal float32: an operation whose operand or result is denormal errs by at most this, flushed or not


def backward_bound(d, H, A, w=1, u=2.0**-24):
    """Bound of |fp32 backward - exact| per raw output, [n, R]: the value row is an A-term sum, (A - 1) u sum_a |d_a|; an advantage row
    adds a division and a subtraction, (A + 1) u (|d_a| + sum_a |d_a| / A); plus the denormal floor of every operation whose operand or
    result is below the smallest normal float32 (softmax tails of a histogram head are), none where the row is exactly zero."""
    x = np.abs(np.asarray(d, np.float64)).reshape(-1, H, A, w)
    s = x.sum(2)
    floor = np.where(s > 0, FLOOR, 0.0)
    adv = (A + 1) * (u * (x + (s / A)[:, :, None]) + floor[:, :, None])
    val = (A - 1) * (u * s + floor)
    return np.concatenate([adv, val[:, :, None]], axis=2).reshape(x.shape[0], raw_width(H, A, w))


def mask_head(params, head, F, H, A, w=1):
    """A copy of a Flax-layout numpy pytree whose head kernel (F, R) has its structural zeros written."""
    p = {m: {k: v.copy() for k, v in l.items()} for m, l in params.items()}
    p[head]["kernel"] = np.where(live_mask(F, H, A, w), p[head]["kernel"], 0).astype(p[head]["kernel"].dtype)  # (+0.0, never -0.0)
    return p


def masked_torch(pt, head, F, H, A, w=1):
    """The torch pytree ``pt`` with the head kernel multiplied by the live mask inside the graph: autograd then leaves exactly 0 on the
    structural zeros of the kernel leaf, as the device's masked gradient does."""
    q = {m: dict(l) for m, l in pt.items()}
    q[head]["kernel"] = pt[head]["kernel"] * torch.from_numpy(live_mask(F, H, A, w)).to(pt[head]["kernel"].dtype)
    return q
