"""The conservative (CQL) term of include/isdqn_hip.h (isdqn_batch_conservative), restated in float64 numpy from head-output rows.

``rows``: [B, K, A, W] -- the outputs of the K regressed online heads on the B states; W = 1 for scalar heads, N for quantile heads,
n_bins for histogram heads.  ``kind``: "scalar", "quantile" or "histogram".

    Q_a   = the output | the mean of the N values | sum_j p_j z_j, p = softmax(logits), z_j = vmin + (j + 1/2) eta
    c_bk  = m + log(sum_a exp(Q_a - m)) - Q_{a_b},  m = max_a Q_a
    loss  = (alpha / B) sum_b w_b c_bk                                      the increment of losses[k]
    dout  = alpha w_b / B (softmax_a Q - 1{a = a_b}) dQ_a/d(output)          the increment of dL/d(head output)
    dbh   = sum_b dout                                                       the increment of the head-bias gradient

``wrong``: one of the mistakes the tests must be able to tell from the definition -- "no_inv_n" (dQ/dtheta = 1 on quantile heads),
"no_centre" (dQ/dlogit = p_j z_j on histogram heads), "no_indicator" (pi alone, without the taken action's 1)."""
import numpy as np

KINDS = ("scalar", "quantile", "histogram")


def support(n_bins, vmin, vmax):
    eta = (float(vmax) - float(vmin)) / n_bins
    return float(vmin) + (np.arange(n_bins, dtype=np.float64) + 0.5) * eta


def action_values(rows, kind, z=None, wrong=None):
    """(Q [B, K, A], dQ/d(output) [B, K, A, W]) in float64."""
    rows = np.asarray(rows, np.float64)
    assert rows.ndim == 4 and kind in KINDS
    W = rows.shape[-1]
    if kind == "scalar":
        assert W == 1
        return rows[..., 0], np.ones_like(rows)
    if kind == "quantile":
        return rows.mean(-1), np.full_like(rows, 1.0 if wrong == "no_inv_n" else 1.0 / W)
    z = np.asarray(z, np.float64)
    assert z.shape == (W,)
    e = np.exp(rows - rows.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    q = (p * z).sum(-1)
    return q, p * (z if wrong == "no_centre" else z - q[..., None])


def restate(rows, action, weights, alpha, kind, z=None, wrong=None):
    """dict(q, c [B, K], loss [K], dout [B, K, A, W], dbh [K, A, W]) of the term on ``rows`` (weights None: 1)."""
    q, dq = action_values(rows, kind, z, wrong)
    B, K, A = q.shape
    action = np.asarray(action).astype(np.int64)
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    m = q.max(-1, keepdims=True)
    ex = np.exp(q - m)
    s = ex.sum(-1, keepdims=True)
    taken = np.take_along_axis(q, action[:, None, None].repeat(K, 1), 2)[..., 0]
    c = (m + np.log(s))[..., 0] - taken
    pi = ex / s
    onehot = np.zeros((B, 1, A))
    onehot[np.arange(B), 0, action] = 0.0 if wrong == "no_indicator" else 1.0
    g = (float(alpha) * w / B)[:, None, None] * (pi - onehot)
    dout = g[..., None] * dq
    return dict(q=q, c=c, loss=float(alpha) * (w[:, None] * c).sum(0) / B, dout=dout, dbh=dout.sum(0), pi=pi, dq=dq)


def head_rows(region_rows, B, on0, K, A, W):
    """[B, K, A, W] of the regressed heads from the first B head-output rows of a workspace region ([rows][pitch], any pitch)."""
    r = np.asarray(region_rows)[:B, on0 * A * W : (on0 + K) * A * W]
    return r.reshape(B, K, A, W)


def op_count(kind, A, W):
    """fp32 operations of the definition that one element of the increment goes through, each worth one relative 2^-24 of a quantity no
    larger than (1 + S) times the element's own scale alpha w_b / B max|dQ|, S the largest magnitude Q is formed from:
      scalar     A + 10: Q_a - m (1), expf (2, and the exponent's own rounding enters multiplied by |Q|: the factor 1 + S), the A - 1
                 additions of the sum, the division (1), the indicator's subtraction (1), alpha w and / B (2), the product (1), rounded up;
      quantile   + N + 2: each Q_a is N - 1 additions and a division and moves pi through the exponent; the increment is divided by N;
      histogram  + 5 n_bins + 30: the softmax of a (n_bins + 4), z_j (2), the weighted sum and its division (n_bins + 2) give Q_a
                 (2 n_bins + 8), which moves pi through the exponent and stands in z_j - Q_a; p_j (n_bins + 4), the subtraction and the
                 two products (3): (2 n_bins + 8) + (3 n_bins + 16) + 1, rounded up."""
    return A + 10 + (0 if kind == "scalar" else W + 2 if kind == "quantile" else 5 * W + 30)
