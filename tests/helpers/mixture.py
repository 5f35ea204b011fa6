"""numpy / float64 restatement of the random ensemble mixture, written from the header text alone (include/isdqn_hip.h,
isdqn_mixture_draw / isdqn_batch_mixture):

    x        = Philox4x32-10(ctr = {h, 0x52454D00, lo32(c), hi32(c)}, key = {lo32(seed), hi32(seed)}), first word
    u_h      = (float)((x >> 8) + 1) 2^-24,   s = fp32 sum of u_h in ascending h,   alpha_h = u_h / s (fp32 division)
    Qmix(x, a) = sum_h alpha_h Q_h(x, a)
    q_b      = Qmix^online(s_b, a_b)
    a*       = first argmax_a Qmix^val(s'_b, a)    (double_q: of Qmix^online(s'_b, .), the value read from Qmix^val at a*)
    target_b = r_b + (1 - terminal_b) g_b Qmix^val(s'_b, a*)
    loss     = (1 / B) sum_b w_b l(q_b - target_b),   dL/dQ_h(s_b, a_b) = alpha_h l'(d_b) w_b / B

The draw is exact (float32 arithmetic in the header's order); everything behind it is float64.  Three wrong readings the tests must
be able to tell from it: ``variant`` = "online_only" (alpha on the online side, a uniform mixture on the value side), "max_first" (max_a
per head, mixed afterwards) and "no_alpha" (dL/dQ_h without the factor alpha_h)."""
import numpy as np

from tests.helpers.noisy import philox4x32_10

DOMAIN = 0x52454D00


def draw(H, seed, count):
    """alpha [H] float32, bit for bit what isdqn_mixture_draw leaves for (seed, count)."""
    x = philox4x32_10([np.arange(H), DOMAIN, count & 0xFFFFFFFF, (count >> 32) & 0xFFFFFFFF], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])[0]
    u = ((x >> np.uint32(8)).astype(np.uint32) + np.uint32(1)).astype(np.float32) * np.float32(2.0**-24)
    s = np.float32(0.0)
    for v in u:  # ascending h, one float32 rounding per add
        s = np.float32(s + v)
    return (u / s).astype(np.float32)


def _l(d, huber_delta):
    a = np.abs(d)
    if huber_delta > 0:
        return np.where(a <= huber_delta, 0.5 * d * d, huber_delta * (a - 0.5 * huber_delta)), np.clip(d, -huber_delta, huber_delta)
    return d * d, 2.0 * d


def mixture(rows, value_rows, alpha, action, reward, terminal, gamma_n, A, *, double_q=False, weights=None, discount=None, huber_delta=0.0,
            variant=None):
    """``rows``: float64 [2B][H * A], the online rows of the states then of the next states; ``value_rows``: [B][H * A], the value
    network's rows of the next states (None: rows[B:]).  Returns q_values, targets, losses (scalar), priorities, dout [B][H * A], dbh
    [H * A], a_star, gap (the two largest mixed values of the rows that select), qmax (the largest |value| any mixture reads)."""
    rows = np.asarray(rows, np.float64)
    B = rows.shape[0] // 2
    H = rows.shape[1] // A
    al = np.asarray(alpha, np.float64)
    on = rows[:B].reshape(B, H, A)
    nx = rows[B:].reshape(B, H, A)
    val = nx if value_rows is None else np.asarray(value_rows, np.float64).reshape(B, H, A)
    al_val = np.full(H, 1.0 / H) if variant == "online_only" else al
    mix = lambda x, w: np.einsum("h,bha->ba", w, x)
    w_b = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    g_b = np.full(B, float(gamma_n)) if discount is None else np.asarray(discount, np.float64)
    ar = np.arange(B)
    q = mix(on, al)[ar, action]
    vmix = mix(val, al_val)
    smix = mix(nx, al_val) if double_q else vmix
    a_star = smix.argmax(axis=1)  # (numpy: the first index of the maximum)
    v = vmix[ar, a_star]
    if variant == "max_first":
        v = np.einsum("h,bh->b", al, val.max(axis=2))
    targets = np.asarray(reward, np.float64) + (1.0 - np.asarray(terminal, np.float64)) * g_b * v
    d = q - targets
    l, dl = _l(d, float(huber_delta))
    g = dl * w_b / B
    dout = np.zeros((B, H, A))
    dout[ar, :, action] = g[:, None] * (np.ones(H) if variant == "no_alpha" else al)[None, :]
    top = np.sort(smix, axis=1)
    gap = top[:, -1] - top[:, -2] if A > 1 else np.full(B, np.inf)
    qmax = np.maximum(np.abs(on).max(axis=(1, 2)), np.maximum(np.abs(val).max(axis=(1, 2)), np.abs(nx).max(axis=(1, 2))))
    return dict(q_values=q, targets=targets, losses=float((w_b * l).sum() / B), priorities=np.sqrt(l + 1e-10), dout=dout.reshape(B, H * A),
                dbh=dout.reshape(B, H * A).sum(axis=0), a_star=a_star, gap=gap, qmax=qmax, d=d, w=w_b, g=g_b,
                nt=1.0 - np.asarray(terminal, np.float64), r=np.asarray(reward, np.float64), v=v)


def mean_heads_actions(q_rows, A):
    """first argmax_a of sum_h Q_h(row, a): float32 sums in ascending h, as ISDQN_ACT_MEAN_HEADS defines them."""
    q = np.asarray(q_rows, np.float32)
    n = q.shape[0]
    q = q.reshape(n, -1, A)
    s = np.zeros((n, A), np.float32)
    for h in range(q.shape[1]):
        s = (s + q[:, h]).astype(np.float32)
    return s.argmax(axis=1).astype(np.int32), s


# ---- the bounds of a float32 kernel against this float64 restatement on the same rows (tests/test_gpu_mixture.py) ----
RTOL = 1e-5  # the project's bound of a float32 kernel against float64 on the same inputs (tests/test_gpu_double_q.py)
EPS = 2.0**-23


def q_floor(H, qmax):
    """|Qmix_fp32 - Qmix_f64| <= (H + 2) 2^-23 max|row|: H products and at most H adds (partials and their combination) of relative
    error 2^-24 each on terms bounded by alpha_h |Q_h|, with sum_h alpha_h = 1 (up to its own rounding, inside the + 2)."""
    return (H + 2) * EPS * np.asarray(qmax, np.float64)


def bounds(ref, H, B, huber_delta=0.0):
    """Absolute floors of every compared quantity from the q floor e_b = q_floor(H, qmax_b), propagated through the formulas:
      target = r + nt g v          : e_t = e_b, the same floor (nt g <= 1 carries the mixture's error through; the three float32
                                     roundings of the target itself are 3 * 2^-24 (|r| + |g v|), which RTOL |target| covers unless r
                                     and g v cancel, and then |r| ~ |g v| <= max|row| and 3 * 2^-23 max|row| is below the floor for H >= 1)
      d = q - target               : e_d = e_b + e_t
      l = d^2 (Huber: <= the same) : e_l = (2 |d| + e_d) e_d;   loss = (1 / B) sum_b w_b l_b : sum_b w_b e_l / B
      priorities = sqrt(l + 1e-10) : e_l / (2 sqrt(l + 1e-10))
      dout = alpha_h l'(d) w / B   : |l''| <= 2, so 2 e_d w / B per unit alpha (alpha_h <= 1);   dbh: the sum of its rows' floors."""
    e_q = q_floor(H, ref["qmax"])
    e_t = e_q
    e_d = e_q + e_t
    e_l = (2.0 * np.abs(ref["d"]) + e_d) * e_d
    e_dout = 2.0 * e_d * ref["w"] / B
    return dict(q_values=e_q, targets=e_t, losses=float((ref["w"] * e_l).sum() / B), priorities=e_l / (2.0 * ref["priorities"]),
                dout=e_dout[:, None], dbh=float(e_dout.sum()))
