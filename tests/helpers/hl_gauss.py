"""float64 restatement of the HL-Gauss histogram loss of the Q-network heads (include/isdqn_hip.h, isdqn_net_config::n_bins;
csrc/hl_gauss.h).  Torch, so that the gradient can also come from autograd.

Head layout: logit ((h * A) + a) * nb + j is bin j of action a of head h over [v_min, v_max] cut into nb bins of width
eta = (v_max - v_min) / nb; centres c_j = v_min + (j + 1/2) eta, edges e_i = v_min + i eta."""
import math

import numpy as np
import torch


def centres(nb, vmin, vmax, dtype=torch.float64):
    eta = (vmax - vmin) / nb
    return vmin + (torch.arange(nb, dtype=dtype) + 0.5) * eta


def edges(nb, vmin, vmax, dtype=torch.float64):
    eta = (vmax - vmin) / nb
    return vmin + torch.arange(nb + 1, dtype=dtype) * eta


def expectations(logits, nb, vmin, vmax):
    """[..., n * nb] logits -> [..., n] expectations sum_j softmax(l)_j c_j."""
    l = torch.as_tensor(logits, dtype=torch.float64)
    l = l.reshape(*l.shape[:-1], -1, nb)
    return (torch.softmax(l, -1) * centres(nb, vmin, vmax)).sum(-1)


def projection(y, nb, vmin, vmax, sigma, dtype=torch.float64):
    """Target histograms [..., nb] of the scalars y: clamp to the support, then the Gaussian's mass per bin, normalised."""
    y = torch.as_tensor(y, dtype=dtype).clamp(vmin, vmax)
    u = torch.special.erf((edges(nb, vmin, vmax, dtype) - y[..., None]) / (math.sqrt(2.0) * sigma))
    return (u[..., 1:] - u[..., :-1]) / (u[..., -1:] - u[..., :1])


def first_argmax(q):
    """First index attaining the maximum along the last axis (strict >: the lowest index wins; numpy documents the first occurrence)."""
    return torch.as_tensor(np.argmax(np.asarray(q.detach(), np.float64), axis=-1), dtype=torch.long)


def hl_loss(logits, action, reward, terminal, gamma_n, K, on0, tg0, A, nb, vmin, vmax, sigma, value_rows=None, selector_rows=None,
            weights=None, discount=None, y=None, dtype=torch.float64):
    """The loss of the B transitions from the logits of their 2B rows ([states; next states], [2B][n_heads * A * nb]).
    Online head on0 + k at the taken action is regressed on head tg0 + k of the next states (no gradient through those).
    ``value_rows``: [B] logit rows of the next states that supply the bootstrap value (default: rows [B, 2B)).
    ``selector_rows``: [B] logit rows whose head on0 + k picks the action -- the first argmax of its expectations, the lowest index -- at
    which the value head's expectation is taken (default: the value head's own maximum).
    ``weights``: [B] loss weights on losses and dlogits, never on the priorities (default 1).
    ``discount``: [B], the row's discount in gamma_n's place (default gamma_n everywhere).
    ``y``: [B, K] scalars to project in the place of the targets (which are still returned, and still make the priorities).
    ``dtype``: the arithmetic's (float32: what a float32 evaluation of the same definition gives).
    Returns dict(losses [K], q [B, K], targets [B, K], priorities [B], dlogits [B, n_heads * A * nb], ce [B, K], p [B, K, nb])."""
    l = torch.as_tensor(logits, dtype=dtype)
    B = l.shape[0] // 2
    act = torch.as_tensor(np.asarray(action), dtype=torch.long)
    r = torch.as_tensor(np.asarray(reward), dtype=dtype)
    nt = 1.0 - torch.as_tensor(np.asarray(terminal), dtype=dtype)
    g = torch.full((B,), float(gamma_n), dtype=dtype) if discount is None else torch.as_tensor(np.asarray(discount), dtype=dtype)
    c = centres(nb, vmin, vmax, dtype)
    on = l[:B].reshape(B, -1, A, nb)
    nx = (l[B:] if value_rows is None else torch.as_tensor(value_rows, dtype=dtype)).detach().reshape(B, -1, A, nb)
    q_next = (torch.softmax(nx, -1) * c).sum(-1)[:, tg0 : tg0 + K]  # [B, K, A]
    if selector_rows is None:
        boot = q_next.max(-1).values
    else:
        sel = torch.as_tensor(selector_rows, dtype=dtype).detach().reshape(B, -1, A, nb)
        a_star = first_argmax((torch.softmax(sel, -1) * c).sum(-1)[:, on0 : on0 + K])
        boot = q_next.gather(-1, a_star[..., None])[..., 0]
    tg = r[:, None] + nt[:, None] * g[:, None] * boot  # [B, K]
    la = on[torch.arange(B)[:, None], torch.arange(on0, on0 + K)[None, :], act[:, None]]  # [B, K, nb]
    q = (torch.softmax(la, -1) * c).sum(-1)
    p = projection(tg if y is None else y, nb, vmin, vmax, sigma, dtype)
    ce = torch.logsumexp(la, -1) - (p * la).sum(-1)
    d = (torch.softmax(la, -1) - p).detach() / B
    wce = ce
    if weights is not None:
        w = torch.as_tensor(np.asarray(weights), dtype=dtype)
        d, wce = w[:, None, None] * d, w[:, None] * ce
    dl = torch.zeros(B, on.shape[1], A, nb, dtype=dtype)
    dl[torch.arange(B)[:, None], torch.arange(on0, on0 + K)[None, :], act[:, None]] = d
    td2 = (q - tg) ** 2
    return dict(losses=wce.mean(0), q=q, targets=tg, priorities=torch.sqrt(td2.mean(1).detach() + 1e-10), dlogits=dl.reshape(B, -1), ce=ce,
                p=p)
