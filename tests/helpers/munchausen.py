"""float64 restatement of the Munchausen targets (include/isdqn_hip.h, isdqn_net_config::munchausen_tau), written from that
definition: for every regressed pair k < K with value head v = tg0 + k

    V(x)      = m + tau * log( sum_a exp((Q^val_v(x, a) - m) / tau) ),   m = max_a Q^val_v(x, a)
    bonus_bk  = alpha * clip( Q^val_v(s_b, a_b) - V(s_b), l0, 0 )
    target_bk = r_b + bonus_bk + (1 - terminal_b) * gamma^n * V(s'_b)

``rows`` are the head outputs of the ONLINE parameters on [states; next states] ([2B][heads * A] Q-values, or [2B][heads * A * nb]
logits with ``hist``).  ``value_rows`` ([2B][...], the target parameters on [states; next states]) supply Q^val when given, ``rows``
themselves otherwise.  No gradient flows through any Q^val term.  The same target is also computed in the paper's form
(``paper_targets``), independently: r + alpha clip(tau ln pi(a|s), l0, 0) + (1 - terminal) gamma^n sum_a' pi(a'|s') (Q - tau ln pi)(s', a')
with pi = softmax(Q / tau).  Everything behind the target is the existing loss: tests/helpers/per_weights.py (squared / Huber,
importance weights) and tests/helpers/hl_gauss.py (projection and cross-entropy of the histogram heads)."""
import numpy as np
import torch

from tests.helpers import hl_gauss as hl
from tests.helpers import per_weights as pw


def soft_value(q, tau):
    """tau * logsumexp(q / tau) over the last axis in the max-subtracted form, in the dtype of ``q`` (float64 unless it is float32)."""
    q = np.asarray(q)
    dt = np.float32 if q.dtype == np.float32 else np.float64
    q, tau = q.astype(dt), dt(tau)
    m = q.max(-1)
    s = np.zeros(m.shape, dt)
    for a in range(q.shape[-1]):  # a left-to-right sum: what a float32 evaluation of the definition does
        s = (s + np.exp((q[..., a] - m) / tau)).astype(dt)
    return (m + tau * np.log(s)).astype(dt)


def targets(q_state, q_next, action, reward, terminal, gamma_n, tau, alpha, clip, dtype=np.float64):
    """The definition on the value head's rows q_state / q_next [B, K, A], every operation in ``dtype``.  Returns
    (targets [B, K], bonus [B, K], unclipped tau ln pi(a_b|s_b) [B, K])."""
    dt = dtype
    qs, qn = np.asarray(q_state).astype(dt), np.asarray(q_next).astype(dt)
    B = qs.shape[0]
    r = np.asarray(reward).astype(dt)[:, None]
    nt = (dt(1) - np.asarray(terminal).astype(dt))[:, None]
    qa = qs[np.arange(B), :, np.asarray(action).astype(np.int64)]  # [B, K]
    tlp = (qa - soft_value(qs, tau)).astype(dt)
    bonus = (dt(alpha) * np.minimum(np.maximum(tlp, dt(clip)), dt(0))).astype(dt)
    tg = (r + bonus + nt * dt(gamma_n) * soft_value(qn, tau)).astype(dt)
    return tg, bonus, tlp


def paper_targets(q_state, q_next, action, reward, terminal, gamma_n, tau, alpha, clip):
    """The paper's form in float64, through the policy: pi = softmax(Q / tau) (scipy-free log-softmax)."""
    qs, qn = np.asarray(q_state, np.float64), np.asarray(q_next, np.float64)
    B = qs.shape[0]

    def log_softmax(x):
        z = x - x.max(-1, keepdims=True)
        return z - np.log(np.exp(z).sum(-1, keepdims=True))

    lp_s, lp_n = log_softmax(qs / tau), log_softmax(qn / tau)
    lpa = lp_s[np.arange(B), :, np.asarray(action).astype(np.int64)]
    bonus = alpha * np.clip(tau * lpa, clip, 0.0)
    soft = (np.exp(lp_n) * (qn - tau * lp_n)).sum(-1)
    r = np.asarray(reward, np.float64)[:, None]
    nt = 1.0 - np.asarray(terminal, np.float64)[:, None]
    return r + bonus + nt * gamma_n * soft


def triple_loop(q_state, q_next, action, reward, terminal, gamma_n, tau, alpha, clip):
    """Targets by a plain loop over (b, k, a) in Python floats."""
    import math

    qs, qn = np.asarray(q_state, np.float64), np.asarray(q_next, np.float64)
    B, K, A = qs.shape
    tg = np.zeros((B, K))

    def v(row):
        m = row[0]
        for a in range(1, A):
            if row[a] > m:
                m = row[a]
        s = 0.0
        for a in range(A):
            s += math.exp((row[a] - m) / tau)
        return m + tau * math.log(s)

    for b in range(B):
        for k in range(K):
            x = float(qs[b, k, int(action[b])]) - v(qs[b, k])
            x = clip if x < clip else (0.0 if x > 0.0 else x)
            tg[b, k] = float(reward[b]) + alpha * x + (1.0 - float(terminal[b])) * gamma_n * v(qn[b, k])
    return tg


def munchausen(rows, action, reward, terminal, gamma_n, K, on0, tg0, A, tau, alpha, clip, value_rows=None, weights=None, huber_delta=0.0,
               hist=None):
    """``hist``: None (scalar heads) or dict(nb, vmin, vmax, sigma).  Returns a dict:
    targets / paper_targets / max_targets [B, K] (this definition / the paper's form / the max form on the same value rows), bonus and
    tlp [B, K] (alpha clip(.) and the unclipped tau ln pi(a_b|s_b)), scale [B, K] (max(1, max |Q| of the pair's two value rows)),
    q [B, K], losses [K], priorities [B], dq (dL/d rows of the states: [B, heads * A], histogram heads [B, heads * A * nb]),
    loss_t (torch, [K]: differentiable through ``rows`` when those carry a graph; the targets are detached)."""
    rows = torch.as_tensor(rows, dtype=torch.float64)
    B = rows.shape[0] // 2
    act = torch.as_tensor(np.asarray(action), dtype=torch.long)
    r = np.asarray(reward, np.float64)
    w = torch.ones(B, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights), dtype=torch.float64)
    ex = (lambda t: hl.expectations(t, hist["nb"], hist["vmin"], hist["vmax"])) if hist else (lambda t: t)
    vr = rows.detach() if value_rows is None else torch.as_tensor(value_rows, dtype=torch.float64).detach()
    assert vr.shape[0] == 2 * B
    val = ex(vr).reshape(2 * B, -1, A)[:, tg0 : tg0 + K].numpy()  # [2B, K, A]
    qs, qn = val[:B], val[B:]
    tg_np, bonus, tlp = targets(qs, qn, action, reward, terminal, gamma_n, tau, alpha, clip)
    tg = torch.from_numpy(tg_np)
    nt = 1.0 - np.asarray(terminal, np.float64)
    out = dict(targets=tg_np, bonus=bonus, tlp=tlp, paper_targets=paper_targets(qs, qn, action, reward, terminal, gamma_n, tau, alpha, clip),
               max_targets=r[:, None] + nt[:, None] * gamma_n * qn.max(-1),
               scale=np.maximum(1.0, np.maximum(np.abs(qs).max(-1), np.abs(qn).max(-1))))
    bi, ki = torch.arange(B)[:, None], torch.arange(on0, on0 + K)[None, :]
    if hist:
        nb = hist["nb"]
        on = rows[:B].reshape(B, -1, A, nb)
        la = on[bi, ki, act[:, None]]  # [B, K, nb]
        sm = torch.softmax(la, -1)
        q = (sm * hl.centres(nb, hist["vmin"], hist["vmax"])).sum(-1)
        p = hl.projection(tg, nb, hist["vmin"], hist["vmax"], hist["sigma"])
        ce = torch.logsumexp(la, -1) - (p * la).sum(-1)
        loss_t = (w[:, None] * ce).sum(0) / B
        dq = torch.zeros(B, on.shape[1], A, nb, dtype=torch.float64)
        dq[bi, ki, act[:, None]] = (w[:, None, None] * (sm - p)).detach() / B
        losses = loss_t.detach().numpy()
    else:
        on = rows[:B].reshape(B, -1, A)
        q = on[bi, ki, act[:, None]]  # [B, K]
        d = q - tg
        if huber_delta > 0:
            l_t = torch.where(d.abs() <= huber_delta, 0.5 * d * d, huber_delta * (d.abs() - 0.5 * huber_delta))
        else:
            l_t = d * d
        loss_t = (w[:, None] * l_t).sum(0) / B
        ref = pw.weighted_td(q.detach().numpy(), tg_np, w.numpy(), huber_delta)
        losses = ref["losses"]
        dq = torch.zeros(B, on.shape[1], A, dtype=torch.float64)
        dq[bi, ki, act[:, None]] = torch.from_numpy(ref["dq"])
    td2 = (q.detach() - tg) ** 2
    if not hist and huber_delta > 0:  # the priorities are the configured per-element loss, unweighted (as without the option)
        td2 = torch.from_numpy(pw.td_loss((q.detach() - tg).numpy(), huber_delta)[0])
    out.update(q=q.detach().numpy(), losses=np.asarray(losses), priorities=np.sqrt(td2.mean(1).numpy() + 1e-10),
               dq=dq.reshape(B, -1).numpy(), loss_t=loss_t)
    return out
