"""float64 restatement of the QR-DQN quantile-regression loss of the Q-network heads, written from the header text alone
(include/isdqn_hip.h, isdqn_net_config::n_quantiles).  Torch, so that the gradient can also come from autograd.

Head layout: output ((h * A) + a) * N + i is theta_i of action a of head h, the quantile at tau_i = (i + 1/2) / N;
Q_h(s, a) = (1 / N) sum_i theta_i.

The target atoms t_j = r + ((1 - terminal) gamma^n) theta_j are rounded to float32 by the header's expression (two roundings, in that
order) before they are differenced: the difference of two float32 numbers is exact in float64, so on float32 rows every indicator
1{u_ij < 0} agrees with a device that evaluates the same expression, and a pinball gradient cannot flip by rounding."""
import numpy as np
import torch


def means(rows, N):
    """[..., n * N] quantile values -> [..., n] means."""
    r = torch.as_tensor(rows, dtype=torch.float64)
    return r.reshape(*r.shape[:-1], -1, N).mean(-1)


def taus(N):
    return (torch.arange(N, dtype=torch.float64) + 0.5) / N


def first_argmax(q):
    """First index attaining the maximum along the last axis (strict >: the lowest index wins)."""
    return torch.as_tensor(np.argmax(np.asarray(q.detach(), np.float64), axis=-1), dtype=torch.long)


def target_atoms_f32(reward, terminal, gamma_n, theta):
    """t_j = r + ((1 - terminal) * gamma^n) * theta_j in float32, each operation rounded once, as float64 values.  theta: [B, K, N]."""
    r = np.asarray(reward, np.float32)[:, None, None]
    disc = ((np.float32(1.0) - np.asarray(terminal, np.float32)) * np.float32(gamma_n)).astype(np.float32)[:, None, None]
    prod = (disc * np.asarray(theta, np.float32)).astype(np.float32)
    return torch.from_numpy((r + prod).astype(np.float32).astype(np.float64))


def huber_parts(u, kappa):
    """h_kappa(u) and h'_kappa(u)."""
    if kappa > 0:
        h = torch.where(u.abs() <= kappa, 0.5 * u * u, kappa * (u.abs() - 0.5 * kappa)) / kappa
        return h, u.clamp(-kappa, kappa) / kappa
    return u.abs(), torch.sign(u)


def qr_loss(rows, action, reward, terminal, gamma_n, K, on0, tg0, A, N, kappa, value_rows=None, selector_rows=None, weights=None):
    """The loss of the B transitions from the head outputs of their 2B rows ([states; next states], [2B][n_heads * A * N]).  Online head
    on0 + k at the taken action is regressed on the atoms of head tg0 + k of `value_rows` ([B] rows of the next states; default: rows
    [B, 2B)) at a* = the first argmax of that head's means -- or, with `selector_rows` ([B] rows), of the means of head on0 + k of those.
    No gradient flows through value or selector rows.  `weights`: [B] loss weights (default 1).
    Returns dict(q [B, K], targets [B, K], a_star [B, K], losses [K], priorities [B], dtheta [B, n_heads * A * N], l [B, K],
    cabs [B, K, N] = sum_j |c_ij| with c_ij = |tau_i - 1{u_ij < 0}| h'(u_ij), neg_share = share of u_ij < 0,
    gap [B, K] = top-two gap of the deciding head's means, qmax = largest |mean| among them)."""
    rows = torch.as_tensor(rows, dtype=torch.float64)
    B = rows.shape[0] // 2
    act = torch.as_tensor(np.asarray(action), dtype=torch.long)
    r = torch.as_tensor(np.asarray(reward, np.float64))
    nt = 1.0 - torch.as_tensor(np.asarray(terminal, np.float64))
    w = torch.ones(B, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights, np.float64))
    on = rows[:B].reshape(B, -1, A, N)
    val = (rows[B:] if value_rows is None else torch.as_tensor(value_rows, dtype=torch.float64)).detach().reshape(B, -1, A, N)
    vq = val.mean(-1)[:, tg0 : tg0 + K]  # [B, K, A]
    if selector_rows is None:
        dq = vq
    else:
        dq = torch.as_tensor(selector_rows, dtype=torch.float64).detach().reshape(B, -1, A, N).mean(-1)[:, on0 : on0 + K]
    a_star = first_argmax(dq)  # [B, K]
    top = torch.sort(dq, dim=-1, descending=True).values
    gap = top[..., 0] - top[..., 1] if A > 1 else torch.full(top.shape[:-1], float("inf"), dtype=torch.float64)
    bi, ki = torch.arange(B)[:, None], torch.arange(K)[None, :]
    targets = r[:, None] + nt[:, None] * gamma_n * vq[bi, ki, a_star]
    atoms = val[bi, tg0 + ki, a_star]  # [B, K, N]
    t = target_atoms_f32(reward, terminal, gamma_n, atoms.numpy())
    th = on[bi, on0 + ki, act[:, None]]  # [B, K, N]
    q = th.mean(-1)
    u = t[:, :, None, :] - th[:, :, :, None]  # [B, K, i, j]
    neg = (u < 0).to(torch.float64)
    wt = (taus(N)[None, None, :, None] - neg).abs()
    h, hp = huber_parts(u, kappa)
    l = (wt * h).sum(-1).sum(-1) / N  # [B, K]
    c = (wt * hp).detach()
    dth = torch.zeros(B, on.shape[1], A, N, dtype=torch.float64)
    dth[bi, on0 + ki, act[:, None]] = -(w[:, None, None] / (B * N)) * c.sum(-1)
    td2 = (q - targets) ** 2
    return dict(q=q, targets=targets, a_star=a_star, losses=(w[:, None] * l).mean(0), priorities=torch.sqrt(td2.mean(1).detach() + 1e-10),
                dtheta=dth.reshape(B, -1), l=l, cabs=c.abs().sum(-1), neg_share=float(neg.mean()), gap=gap, qmax=float(dq.abs().max()))


def qr_loss_loops(rows, action, reward, terminal, gamma_n, K, on0, tg0, A, N, kappa, value_rows=None, selector_rows=None, weights=None):
    """The same quantities by plain loops over (transition, pair, i, j) on Python floats: an independent reading of the header."""
    rows = np.asarray(rows, np.float64)
    B = rows.shape[0] // 2
    on = rows[:B].reshape(B, -1, A, N)
    val = (rows[B:] if value_rows is None else np.asarray(value_rows, np.float64)).reshape(B, -1, A, N)
    sel = None if selector_rows is None else np.asarray(selector_rows, np.float64).reshape(B, -1, A, N)
    n_heads = on.shape[1]
    q, tg, a_star = np.zeros((B, K)), np.zeros((B, K)), np.zeros((B, K), np.int64)
    l = np.zeros((B, K))
    dth = np.zeros((B, n_heads, A, N))
    for b in range(B):
        wb = 1.0 if weights is None else float(weights[b])
        disc32 = np.float32(np.float32(1.0) - np.float32(terminal[b])) * np.float32(gamma_n)
        for k in range(K):
            decide = val[b, tg0 + k] if sel is None else sel[b, on0 + k]
            best, best_q = 0, sum(decide[0]) / N
            for a in range(1, A):
                m = sum(decide[a]) / N
                if m > best_q:
                    best, best_q = a, m
            a_star[b, k] = best
            atoms = val[b, tg0 + k, best]
            tg[b, k] = float(reward[b]) + (1.0 - float(terminal[b])) * gamma_n * (sum(atoms) / N)
            th = on[b, on0 + k, int(action[b])]
            q[b, k] = sum(th) / N
            for i in range(N):
                tau = (i + 0.5) / N
                acc_l = acc_g = 0.0
                for j in range(N):
                    tj = float(np.float32(np.float32(reward[b]) + np.float32(disc32 * np.float32(atoms[j]))))
                    u = tj - float(th[i])
                    wt = abs(tau - (1.0 if u < 0 else 0.0))
                    if kappa > 0:
                        hub = 0.5 * u * u if abs(u) <= kappa else kappa * (abs(u) - 0.5 * kappa)
                        acc_l += wt * hub / kappa
                        acc_g += wt * min(max(u, -kappa), kappa) / kappa
                    else:
                        acc_l += wt * abs(u)
                        acc_g += wt * ((u > 0) - (u < 0))
                l[b, k] += acc_l / N
                dth[b, on0 + k, int(action[b]), i] = -(wb / (B * N)) * acc_g
    wv = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    return dict(q=q, targets=tg, a_star=a_star, losses=(wv[:, None] * l).mean(0), priorities=np.sqrt(((q - tg) ** 2).mean(1) + 1e-10),
                dtheta=dth.reshape(B, -1), l=l)
