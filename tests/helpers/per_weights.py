"""float64 restatement of the importance-sampling weights of prioritized replay and of the weighted TD loss
(include/isdqn_hip.h: isdqn_tree_query_weighted, isdqn_batch.loss_weights; Schaul et al. 2016, section 3.4).

``weights`` is the paper's form with the number of stored keys N and the tree's root R written out,
    w_i = (N P(i))^(-beta) / max_j (N P(j))^(-beta),   P(i) = p_i / R,
so that the cancellation of N and R the kernel relies on -- w_i = (p_min / p_i)^beta, ``weights_short`` -- is tested rather
than assumed.  Sampled leaves that are not positive stay out of the maximum and get weight 1; with no positive leaf every
weight is 1."""
import numpy as np


def weights(leaves, beta, n_keys=None, root=None):
    """float64 weights [n] of the sampled ``leaves`` [n]; ``n_keys`` (N) defaults to n, ``root`` (R) to the leaves' sum."""
    p = np.asarray(leaves, np.float64).reshape(-1)
    pos = p > 0.0
    w = np.ones_like(p)
    if not pos.any():
        return w
    N = np.float64(len(p) if n_keys is None else n_keys)
    R = np.float64(p[pos].sum() if root is None else root)
    raw = np.power(N * (p[pos] / R), -np.float64(beta))
    w[pos] = raw / raw.max()
    return w


def weights_short(leaves, beta):
    """(p_min / p_i)^beta over the positive leaves: the form the kernel evaluates."""
    p = np.asarray(leaves, np.float64).reshape(-1)
    pos = p > 0.0
    w = np.ones_like(p)
    if pos.any():
        w[pos] = np.power(p[pos].min() / p[pos], np.float64(beta))
    return w


def td_loss(d, huber_delta=0.0):
    """Per-element loss and its derivative for d = q - target: squared error, or Huber with ``huber_delta`` > 0."""
    d = np.asarray(d, np.float64)
    if huber_delta > 0:
        a = np.abs(d)
        return np.where(a <= huber_delta, 0.5 * d * d, huber_delta * (a - 0.5 * huber_delta)), np.clip(d, -huber_delta, huber_delta)
    return d * d, 2.0 * d


def weighted_td(q, targets, w, huber_delta=0.0):
    """q, targets [B, K], w [B] -> dict(losses [K] = (1 / B) sum_b w_b l_bk, dq [B, K] = w_b l'(d_bk) / B, l [B, K] unweighted,
    abs_terms [K] = (1 / B) sum_b |w_b l_bk|)."""
    q, t, w = np.asarray(q, np.float64), np.asarray(targets, np.float64), np.asarray(w, np.float64)
    B = q.shape[0]
    d = q - t
    l, dl = td_loss(d, huber_delta)
    return dict(losses=(w[:, None] * l).sum(0) / B, dq=w[:, None] * dl / B, l=l, abs_terms=np.abs(w[:, None] * l).sum(0) / B)
