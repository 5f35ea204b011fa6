"""float64 restatement of the Double Q-learning targets (include/isdqn_hip.h, isdqn_net_config::double_q), written from that
definition: for every regressed pair k < K with value head v = tg0 + k and selector head s = on0 + k

    a*_bk     = the FIRST index attaining max_a Q^sel_s(s'_b, a)
    target_bk = r_b + (1 - terminal_b) * gamma^n * Q^val_v(s'_b, a*_bk)

``rows`` are the head outputs of the ONLINE parameters on [states; next states] ([2B][heads * A] Q-values, or [2B][heads * A * nb]
logits with ``hist``): their next-state half is the selector.  ``value_rows`` ([B][...], the target parameters on the next states)
supply the value when given, the same next-state half otherwise.  No gradient flows through selector or value.  Everything behind
the target is the existing loss: tests/helpers/per_weights.py (squared / Huber, importance weights) and tests/helpers/hl_gauss.py
(projection and cross-entropy of the histogram heads)."""
import numpy as np
import torch

from tests.helpers import hl_gauss as hl
from tests.helpers import per_weights as pw


def first_argmax(x):
    """Lowest index attaining the maximum along the last axis (strict >, as a left-to-right scan keeps it)."""
    return np.argmax(np.asarray(x, np.float64), axis=-1)  # numpy documents the first occurrence


def double_q(rows, action, reward, terminal, gamma_n, K, on0, tg0, A, value_rows=None, weights=None, huber_delta=0.0, hist=None):
    """``hist``: None (scalar heads) or dict(nb, vmin, vmax, sigma).  Returns a dict:
    a_star [B, K], greedy [B, K] (first argmax of the VALUE head: what the max form picks), targets / max_targets [B, K] (this
    definition / the max form on the same rows), q [B, K], losses [K], priorities [B], dq (dL/d rows of the states: [B, heads * A],
    histogram heads [B, heads * A * nb]), loss_t (torch, [K]: differentiable through ``rows`` when those carry a graph)."""
    rows = torch.as_tensor(rows, dtype=torch.float64)
    B = rows.shape[0] // 2
    act = torch.as_tensor(np.asarray(action), dtype=torch.long)
    r = torch.as_tensor(np.asarray(reward), dtype=torch.float64)
    nt = 1.0 - torch.as_tensor(np.asarray(terminal), dtype=torch.float64)
    w = torch.ones(B, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights), dtype=torch.float64)
    ex = (lambda t: hl.expectations(t, hist["nb"], hist["vmin"], hist["vmax"])) if hist else (lambda t: t)
    sel_q = ex(rows[B:].detach()).reshape(B, -1, A)
    val_q = sel_q if value_rows is None else ex(torch.as_tensor(value_rows, dtype=torch.float64).detach()).reshape(B, -1, A)
    sel = sel_q[:, on0 : on0 + K]  # [B, K, A]
    val = val_q[:, tg0 : tg0 + K]
    a_star = torch.from_numpy(first_argmax(sel.numpy()))
    boot = val.gather(-1, a_star[..., None])[..., 0]
    tg = r[:, None] + nt[:, None] * gamma_n * boot
    tg_max = r[:, None] + nt[:, None] * gamma_n * val.max(-1).values
    bi, ki = torch.arange(B)[:, None], torch.arange(on0, on0 + K)[None, :]
    out = dict(a_star=a_star.numpy(), greedy=first_argmax(val.numpy()), targets=tg.numpy(), max_targets=tg_max.numpy())
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
        ref = pw.weighted_td(q.detach().numpy(), tg.numpy(), w.numpy(), huber_delta)
        losses = ref["losses"]
        dq = torch.zeros(B, on.shape[1], A, dtype=torch.float64)
        dq[bi, ki, act[:, None]] = torch.from_numpy(ref["dq"])
    td2 = (q.detach() - tg) ** 2
    if not hist and huber_delta > 0:  # the priorities are the configured per-element loss, unweighted (as without the option)
        td2 = torch.from_numpy(pw.td_loss((q.detach() - tg).numpy(), huber_delta)[0])
    out.update(q=q.detach().numpy(), losses=np.asarray(losses), priorities=np.sqrt(td2.mean(1).numpy() + 1e-10),
               dq=dq.reshape(B, -1).numpy(), loss_t=loss_t)
    return out


def triple_loop(rows, action, reward, terminal, gamma_n, K, on0, tg0, A, value_rows=None):
    """a* and targets of scalar heads by a plain loop over (b, k, a), strict > (the lowest index wins)."""
    rows = np.asarray(rows, np.float64)
    B = rows.shape[0] // 2
    vr = rows[B:] if value_rows is None else np.asarray(value_rows, np.float64)
    a_star = np.zeros((B, K), np.int64)
    tg = np.zeros((B, K))
    for b in range(B):
        for k in range(K):
            best, bv = 0, rows[B + b, (on0 + k) * A]
            for a in range(1, A):
                x = rows[B + b, (on0 + k) * A + a]
                if x > bv:
                    best, bv = a, x
            a_star[b, k] = best
            tg[b, k] = float(reward[b]) + (1.0 - float(terminal[b])) * gamma_n * vr[b, (tg0 + k) * A + best]
    return a_star, tg
