"""float64 restatement of the C51 categorical projection loss of the histogram heads, written from the header text alone
(include/isdqn_hip.h, isdqn_net_config::categorical).  Torch, so that the gradient can also come from autograd.

Head layout (that of n_bins = nb): logit ((h * A) + a) * nb + j is atom j of action a of head h; eta = (v_max - v_min) / nb; the atoms
are the bin centres z_j = v_min + (j + 1/2) eta; Q_h(s, a) = sum_j softmax(l_{h,a})_j z_j."""
import numpy as np
import torch


def atoms(nb, vmin, vmax):
    eta = (vmax - vmin) / nb
    return vmin + (torch.arange(nb, dtype=torch.float64) + 0.5) * eta


def expectations(logits, nb, vmin, vmax):
    """[..., n * nb] logits -> [..., n] expectations sum_j softmax(l)_j z_j."""
    l = torch.as_tensor(logits, dtype=torch.float64)
    l = l.reshape(*l.shape[:-1], -1, nb)
    return (torch.softmax(l, -1) * atoms(nb, vmin, vmax)).sum(-1)


def first_argmax(q):
    """First index attaining the maximum along the last axis (strict >: the lowest index wins)."""
    return torch.as_tensor(np.argmax(np.asarray(q.detach(), np.float64), axis=-1), dtype=torch.long)


def positions(r, g, nb, vmin, vmax):
    """b_j = (clamp(r + g z_j, z_0, z_{nb-1}) - z_0) / eta for r, g of any (equal) shape: [..., nb], in [0, nb - 1]."""
    z = atoms(nb, vmin, vmax)
    eta = (vmax - vmin) / nb
    r = torch.as_tensor(r, dtype=torch.float64)[..., None]
    g = torch.as_tensor(g, dtype=torch.float64)[..., None]
    return ((r + g * z).clamp(z[0], z[-1]) - z[0]) / eta


def project_gather(p, b):
    """m_i = sum_j p_j max(0, 1 - |b_j - i|): THE definition.  p, b: [..., nb] -> [..., nb]."""
    nb = p.shape[-1]
    i = torch.arange(nb, dtype=torch.float64)
    wgt = (1.0 - (b[..., None, :] - i[:, None]).abs()).clamp(min=0.0)  # [..., i, j]
    return (wgt * p[..., None, :]).sum(-1)


def project_scatter(p, b):
    """The usual C51 projection: atom j gives p_j (u - b_j) to l = floor(b_j) and p_j (b_j - l) to u = l + 1; an atom that lands exactly
    on a support point (b_j = l) gives all of its mass to l -- the case the textbook ceil form loses."""
    nb = p.shape[-1]
    lo = b.floor().clamp(0, nb - 1)
    frac = b - lo
    up = (lo + 1).clamp(max=nb - 1)
    m = torch.zeros_like(p)
    m.scatter_add_(-1, lo.long(), p * (1.0 - frac))
    m.scatter_add_(-1, up.long(), p * frac)
    return m


def project_loop(p, b):
    """project_gather by plain loops on Python floats, for one row: an independent reading of the header."""
    nb = len(p)
    m = [0.0] * nb
    for i in range(nb):
        for j in range(nb):
            m[i] += float(p[j]) * max(0.0, 1.0 - abs(float(b[j]) - i))
    return m


def c51_loss(logits, action, reward, terminal, gamma_n, K, on0, tg0, A, nb, vmin, vmax, value_rows=None, selector_rows=None, weights=None):
    """The loss of the B transitions from the logits of their 2B rows ([states; next states], [2B][n_heads * A * nb]).  Online head
    on0 + k at the taken action is regressed on the projected distribution of head tg0 + k of `value_rows` ([B] rows of the next states;
    default: rows [B, 2B)) at a* = the first argmax of that head's expectations -- or, with `selector_rows` ([B] rows), of the
    expectations of head on0 + k of those.  No gradient flows through value or selector rows.  `weights`: [B] loss weights (default 1).
    Returns dict(q [B, K], targets [B, K], a_star [B, K], losses [K], priorities [B], dlogits [B, n_heads * A * nb], l [B, K],
    m [B, K, nb], p [B, K, nb], b [B, K, nb], la [B, K, nb] the online logits at the taken action, gap [B, K] = top-two gap of the deciding
    head's expectations, qmax = largest |expectation| among them)."""
    l = torch.as_tensor(logits, dtype=torch.float64)
    B = l.shape[0] // 2
    act = torch.as_tensor(np.asarray(action), dtype=torch.long)
    r = torch.as_tensor(np.asarray(reward, np.float64))
    nt = 1.0 - torch.as_tensor(np.asarray(terminal, np.float64))
    w = torch.ones(B, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights, np.float64))
    z = atoms(nb, vmin, vmax)
    on = l[:B].reshape(B, -1, A, nb)
    val = (l[B:] if value_rows is None else torch.as_tensor(value_rows, dtype=torch.float64)).detach().reshape(B, -1, A, nb)
    pv = torch.softmax(val, -1)
    vq = (pv * z).sum(-1)[:, tg0 : tg0 + K]  # [B, K, A]
    if selector_rows is None:
        dq = vq
    else:
        sel = torch.as_tensor(selector_rows, dtype=torch.float64).detach().reshape(B, -1, A, nb)
        dq = (torch.softmax(sel, -1) * z).sum(-1)[:, on0 : on0 + K]
    a_star = first_argmax(dq)  # [B, K]
    top = torch.sort(dq, dim=-1, descending=True).values
    gap = top[..., 0] - top[..., 1] if A > 1 else torch.full(top.shape[:-1], float("inf"), dtype=torch.float64)
    bi, ki = torch.arange(B)[:, None], torch.arange(K)[None, :]
    g = nt * gamma_n
    targets = r[:, None] + g[:, None] * vq[bi, ki, a_star]
    p = pv[bi, tg0 + ki, a_star]  # [B, K, nb]
    b = positions(r, g, nb, vmin, vmax)[:, None, :].expand(B, K, nb)
    m = project_gather(p, b)
    la = on[bi, on0 + ki, act[:, None]]  # [B, K, nb]
    q = (torch.softmax(la, -1) * z).sum(-1)
    ce = torch.logsumexp(la, -1) - (m * la).sum(-1)
    dl = torch.zeros(B, on.shape[1], A, nb, dtype=torch.float64)
    dl[bi, on0 + ki, act[:, None]] = (w[:, None, None] * (torch.softmax(la, -1) - m).detach()) / B
    td2 = (q - targets) ** 2
    return dict(q=q, targets=targets, a_star=a_star, losses=(w[:, None] * ce).mean(0), priorities=torch.sqrt(td2.mean(1).detach() + 1e-10),
                dlogits=dl.reshape(B, -1), l=ce, m=m, p=p, b=b, la=la.detach(), gap=gap, qmax=float(dq.abs().max()))


def gauss_bump(nb, vmin, vmax, mu, sigma=1.0):
    """-(z_j - mu)^2 / (2 sigma^2): added to a block's bias it makes the block's softmax a discretised Gaussian around mu."""
    return -((atoms(nb, vmin, vmax).numpy() - mu) ** 2) / (2.0 * sigma * sigma)

