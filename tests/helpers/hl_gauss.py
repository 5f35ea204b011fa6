"""float64 restatement of the HL-Gauss histogram loss of the Q-network heads (include/isdqn_hip.h, isdqn_net_config::n_bins;
csrc/hl_gauss.h).  Torch, so that the gradient can also come from autograd.

Head layout: logit ((h * A) + a) * nb + j is bin j of action a of head h over [v_min, v_max] cut into nb bins of width
eta = (v_max - v_min) / nb; centres c_j = v_min + (j + 1/2) eta, edges e_i = v_min + i eta."""
import math

import torch


def centres(nb, vmin, vmax):
    eta = (vmax - vmin) / nb
    return vmin + (torch.arange(nb, dtype=torch.float64) + 0.5) * eta


def edges(nb, vmin, vmax):
    eta = (vmax - vmin) / nb
    return vmin + torch.arange(nb + 1, dtype=torch.float64) * eta


def expectations(logits, nb, vmin, vmax):
    """[..., n * nb] logits -> [..., n] expectations sum_j softmax(l)_j c_j."""
    l = torch.as_tensor(logits, dtype=torch.float64)
    l = l.reshape(*l.shape[:-1], -1, nb)
    return (torch.softmax(l, -1) * centres(nb, vmin, vmax)).sum(-1)


def projection(y, nb, vmin, vmax, sigma):
    """Target histograms [..., nb] of the scalars y: clamp to the support, then the Gaussian's mass per bin, normalised."""
    y = torch.as_tensor(y, dtype=torch.float64).clamp(vmin, vmax)
    u = torch.special.erf((edges(nb, vmin, vmax) - y[..., None]) / (math.sqrt(2.0) * sigma))
    return (u[..., 1:] - u[..., :-1]) / (u[..., -1:] - u[..., :1])


def hl_loss(logits, action, reward, terminal, gamma_n, K, on0, tg0, A, nb, vmin, vmax, sigma):
    """The loss of the B transitions from the logits of their 2B rows ([states; next states], [2B][n_heads * A * nb]).
    Online head on0 + k at the taken action is regressed on head tg0 + k of the next states (no gradient through those).
    Returns dict(losses [K], q [B, K], targets [B, K], priorities [B], dlogits [B, n_heads * A * nb], ce [B, K])."""
    l = torch.as_tensor(logits, dtype=torch.float64)
    B = l.shape[0] // 2
    act = torch.as_tensor(action, dtype=torch.long)
    r = torch.as_tensor(reward, dtype=torch.float64)
    nt = 1.0 - torch.as_tensor(terminal, dtype=torch.float64)
    on = l[:B].reshape(B, -1, A, nb)
    nx = l[B:].detach().reshape(B, -1, A, nb)
    q_next = (torch.softmax(nx, -1) * centres(nb, vmin, vmax)).sum(-1)  # [B, heads, A]
    tg = r[:, None] + nt[:, None] * gamma_n * q_next[:, tg0 : tg0 + K].max(-1).values  # [B, K]
    la = on[torch.arange(B)[:, None], torch.arange(on0, on0 + K)[None, :], act[:, None]]  # [B, K, nb]
    q = (torch.softmax(la, -1) * centres(nb, vmin, vmax)).sum(-1)
    p = projection(tg, nb, vmin, vmax, sigma)
    ce = torch.logsumexp(la, -1) - (p * la).sum(-1)
    dl = torch.zeros(B, on.shape[1], A, nb, dtype=torch.float64)
    dl[torch.arange(B)[:, None], torch.arange(on0, on0 + K)[None, :], act[:, None]] = (torch.softmax(la, -1) - p).detach() / B
    td2 = (q - tg) ** 2
    return dict(losses=ce.mean(0), q=q, targets=tg, priorities=torch.sqrt(td2.mean(1).detach() + 1e-10), dlogits=dl.reshape(B, -1), ce=ce)
