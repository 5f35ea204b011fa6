"""Shared helpers for the GPU parity tests: synthetic replay batches in both layouts (single frames +
id table for the HIP path, channel-last stacks for the oracle) and oracle/engine pairs that start
from identical parameters."""
import numpy as np
import torch

from oracle import network as onet
from oracle.isdqn import iSDQN as OracleAgent
from oracle.replay_buffer import ReplayElement


def make_frame_batch(B, n_actions, seed=0, h=84, w=84, stack=4, n_frames=None, zero_frac=0.1):
    """Random single frames + id table [B][2*stack] (-1 = zero frame) and the equivalent
    reference-layout batch (state/next_state (B,h,w,stack) uint8)."""
    rng = np.random.default_rng(seed)
    n_frames = n_frames or (3 * B + 8)
    frames = rng.integers(0, 256, size=(n_frames, h * w), dtype=np.uint8)
    ids = rng.integers(0, n_frames, size=(B, 2 * stack)).astype(np.int32)
    ids[rng.random(ids.shape) < zero_frac] = -1
    action = rng.integers(0, n_actions, B).astype(np.int32)
    reward = rng.normal(size=B).astype(np.float32)
    terminal = (rng.random(B) < 0.3).astype(np.uint8)

    def stacks(cols):
        out = np.zeros((B, h, w, stack), np.uint8)
        for b in range(B):
            for c in range(stack):
                if ids[b, cols + c] >= 0:
                    out[b, :, :, c] = frames[ids[b, cols + c]].reshape(h, w)
        return out

    ref = ReplayElement(state=stacks(0), action=action.astype(np.int64), reward=reward.astype(np.float64),
                        next_state=stacks(stack), is_terminal=terminal.astype(np.int64))
    return frames, ids, action, reward, terminal, ref


def perturbed_params(seed, obs, feats, arch, final_feature, layer_norm, scale=0.1, batch_norm=False):
    p = onet.init_params(seed, obs, feats, arch, final_feature, layer_norm, batch_norm=batch_norm)
    rng = np.random.default_rng(seed + 1)
    for m in p:
        for n in p[m]:
            if n != "kernel":  # move biases / LN params off their trivial init
                p[m][n] = (p[m][n] + rng.normal(0, scale, p[m][n].shape)).astype(np.float32)
    return p


def make_pair(feats, K, A, B, arch="cnn", obs=(84, 84, 4), layer_norm=True, precision="bf16x3", seed=0,
              lr=1e-3, gamma=0.99, n=1, adam_eps=1.5e-4, dtype=torch.float32, batch_norm=False):
    """``batch_norm``: both sides also start from the same (non-trivial) running averages."""
    from slimdqn._engine import QNetEngine

    params = perturbed_params(seed, obs, feats, arch, (1 + K) * A, layer_norm, batch_norm=batch_norm)
    oracle = OracleAgent(seed, obs, A, K, list(feats), layer_norm, batch_norm, arch, lr, gamma, n, 1, 1,
                         adam_eps=adam_eps, dtype=dtype, params=params)
    eng = QNetEngine(obs, A, 1 + K, feats, arch, layer_norm, B, gamma_n=gamma**n, learning_rate=lr,
                     adam_eps=adam_eps, precision=precision, batch_norm=batch_norm)
    stats = None
    if batch_norm:
        rng = np.random.default_rng(seed + 2)
        stats = {m: {"mean": rng.normal(0, 0.3, l["mean"].shape).astype(np.float32), "var": rng.uniform(0.5, 2.0, l["var"].shape).astype(np.float32)}
                 for m, l in onet.init_batch_stats(params).items()}
        oracle.batch_stats = onet.to_torch(stats, dtype)
    eng.import_flax(params, batch_stats=stats)
    return oracle, eng, params


def device_batch(eng, frames, ids, action, reward, terminal):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fr, idd, ac, rw, te = d(frames), d(ids), d(action), d(reward), d(terminal)
    batch = eng.make_batch(frames=fr, frame_stride=frames.shape[1], frame_ids=idd, action=ac, reward=rw, terminal=te)
    return batch


def masked_reference_grads(params, feats, K, A, ref, z_hip, layer_norm=True, gamma_n=0.99, huber_delta=0.0, with_scales=False):
    """float64 torch gradients of the iS-DQN loss (isdqn.py:92-109) in which every ReLU of the ONLINE half takes its
    pass/block decision from the HIP path's own pre-activations `z_hip[layer]` ([B, ...] float32, layer names Conv_0..2,
    Dense_0).  Why: a batch holds 10^5..10^7 ReLU inputs, a few of them within the forward's 1e-5 of zero; where the HIP
    mask differs from an independent forward's, the whole upstream gradient of that image changes by O(1), i.e. the leaves
    by O(1/B) -- as much as a missing image would.  With the decisions pinned, what is left is arithmetic, and the
    gradient comparison can be held to 1e-4 instead of 3e-3.  Returns a Flax-layout pytree of float64 arrays.

    ``with_scales``: also return, per element, the sum of the magnitudes of the terms that make up the gradient -- sum |dz| |x|
    for a weight, sum |dz| for a bias, sum |dy| |xhat| / sum |dy| for a LayerNorm scale / bias (the same float64 graph with
    absolute values): the scale against which a rounding error of the element is measured, however far below the leaf's
    largest entry the element itself lies."""
    import torch.nn.functional as F

    B = len(ref.action)
    P = {m: {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in d.items()} for m, d in params.items()}

    def same(size, k, s):
        out = -(-size // s)
        tot = max((out - 1) * s + k - size, 0)
        return tot // 2, tot - tot // 2

    saved = []  # (module, its input (padded, NCHW for a convolution), pre-activation z, LayerNorm name, xhat, LayerNorm output)

    def normalize(z):
        mean = z.mean(-1, keepdim=True)
        var = ((z * z).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
        return (z - mean) * torch.rsqrt(var + 1e-6)

    def ln(z, name):
        if not layer_norm:
            return z
        return normalize(z) * P[name]["scale"] + P[name]["bias"]

    def ln_saved(z, name):
        if not layer_norm:
            return z, None, None
        xhat = normalize(z)
        y = xhat * P[name]["scale"] + P[name]["bias"]
        y.retain_grad()
        return y, xhat, y

    def relu_with_hip_mask(y, z_name, ln_name):
        # online rows: decision from the HIP pre-activations; next-state rows (no gradient flows there): plain ReLU
        zh = torch.tensor(np.asarray(z_hip[z_name], np.float64)).reshape((B,) + tuple(y.shape[1:]))
        with torch.no_grad():
            keep_online = (ln(zh, ln_name) > 0).to(torch.float64)
        return torch.cat([y[:B] * keep_online, torch.relu(y[B:])])

    x = torch.tensor(np.concatenate([ref.state, ref.next_state]), dtype=torch.float64) / 255.0  # NHWC
    n_ln = 0
    for i, (k, s) in enumerate(((8, 4), (4, 2), (3, 1))):
        lo_h, hi_h = same(x.shape[1], k, s)
        lo_w, hi_w = same(x.shape[2], k, s)
        xp = F.pad(x.permute(0, 3, 1, 2), (lo_w, hi_w, lo_h, hi_h))
        zc = F.conv2d(xp, P[f"Conv_{i}"]["kernel"].permute(3, 2, 0, 1), P[f"Conv_{i}"]["bias"], stride=s)
        zc.retain_grad()
        y, xhat, yk = ln_saved(zc.permute(0, 2, 3, 1), f"LayerNorm_{n_ln}")
        saved.append((f"Conv_{i}", xp.detach(), zc, f"LayerNorm_{n_ln}", xhat, yk, s))
        x = relu_with_hip_mask(y, f"Conv_{i}", f"LayerNorm_{n_ln}")
        n_ln += 1
    h = x.reshape(2 * B, -1)
    n_dense = 0
    for width in feats[3:]:
        z = h @ P[f"Dense_{n_dense}"]["kernel"] + P[f"Dense_{n_dense}"]["bias"]
        z.retain_grad()
        y, xhat, yk = ln_saved(z, f"LayerNorm_{n_ln}")
        saved.append((f"Dense_{n_dense}", h.detach(), z, f"LayerNorm_{n_ln}", xhat, yk, None))
        h = relu_with_hip_mask(y, f"Dense_{n_dense}", f"LayerNorm_{n_ln}")
        n_ln += 1
        n_dense += 1
    zq = h @ P[f"Dense_{n_dense}"]["kernel"] + P[f"Dense_{n_dense}"]["bias"]
    zq.retain_grad()
    saved.append((f"Dense_{n_dense}", h.detach(), zq, None, None, None, None))
    q = zq.reshape(2 * B, 1 + K, A)
    act = torch.tensor(np.asarray(ref.action), dtype=torch.long)
    qv = q[:B, 1:, :][torch.arange(B), :, act]
    r = torch.tensor(np.asarray(ref.reward, np.float64))
    t = torch.tensor(np.asarray(ref.is_terminal, np.float64))
    tg = r[:, None] + (1 - t)[:, None] * gamma_n * q[B:, :K].max(-1).values
    d = qv - tg.detach()
    if huber_delta > 0:
        td = torch.where(d.abs() <= huber_delta, 0.5 * d * d, huber_delta * (d.abs() - 0.5 * huber_delta))
    else:
        td = d**2
    loss = td.mean(0).sum()
    loss.backward()
    grads = {m: {k: v.grad.numpy() for k, v in d.items()} for m, d in P.items()}
    if not with_scales:
        return grads
    scales = {}
    for mod, xin, z, ln_name, xhat, y, stride in saved:
        dz = z.grad.abs()
        w = torch.zeros_like(P[mod]["kernel"], requires_grad=True)
        if stride is not None:  # a convolution: the same correlation of |x| with |dz| gives sum |dz| |x| per tap
            za = F.conv2d(xin.abs(), w.permute(3, 2, 0, 1), stride=stride)
        else:
            za = xin.abs() @ w
        (gw,) = torch.autograd.grad((za * dz).sum(), [w])
        scales[mod] = {"kernel": gw.numpy(), "bias": dz.sum(dim=(0, 2, 3) if stride is not None else 0).numpy()}
        if xhat is not None:
            dy = y.grad.abs()
            red = tuple(range(dy.dim() - 1))
            scales[ln_name] = {"scale": (dy * xhat.detach().abs()).sum(red).numpy(), "bias": dy.sum(red).numpy()}
    return grads, scales


def hip_preactivations(eng, B):
    """The HIP path's own pre-activations of the online rows of the last forward, by layer (Conv_0..2, Dense_i; true
    channels only), in the form masked_reference_grads takes them.  Internal layout: [B][pixels][channels padded to 8]."""
    h = eng.observation_dim[0]
    z_hip = {}
    for i, (k, s) in enumerate(((8, 4), (4, 2), (3, 1))):
        h = -(-h // s)
        c = eng.features[i]
        cp = (c + 7) // 8 * 8
        z = eng.region(f"z/Conv_{i}").cpu().numpy()[: B * h * h * cp].reshape(B, -1, cp)
        z_hip[f"Conv_{i}"] = z[:, :, :c].reshape(B, -1)
    for j, c in enumerate(eng.features[3:]):
        cp = (c + 7) // 8 * 8
        z_hip[f"Dense_{j}"] = eng.region(f"z/Dense_{j}").cpu().numpy()[: B * cp].reshape(B, cp)[:, :c]
    return z_hip


# The engine's Adam hyper-parameters are float32 fields (include/isdqn_hip.h): 0.9 and 0.999 as float32 are the constants the
# kernels multiply by and the bias corrections are computed from (net_kernels.hip: pow_int((double)b1, t)).  1 - b is exact in
# float32 for both, so a float64 reference with the same two numbers differs from the kernels by rounding alone.
ADAM_B1, ADAM_B2 = float(np.float32(0.9)), float(np.float32(0.999))


def adam64(p0, m0, v0, g, t, lr, eps):
    """optax.adam on float64 copies (oracle/isdqn.py learn_on_batch, the same expression order): returns new p, m, v, the update
    u = m_hat / (sqrt(v_hat) + eps) and the denominator.  `t` is the step count after the increment."""
    p0, m0, v0, g = (np.asarray(a, np.float64) for a in (p0, m0, v0, g))
    c1, c2 = 1.0 - ADAM_B1 ** t, 1.0 - ADAM_B2 ** t
    m = ADAM_B1 * m0 + (1 - ADAM_B1) * g
    v = ADAM_B2 * v0 + (1 - ADAM_B2) * (g * g)
    den = np.sqrt(v / c2) + eps
    u = (m / c1) / den
    return p0 - lr * u, m, v, u, den


_U, _TINY = 2.0**-24, 2.0**-149  # float32 unit roundoff; denormal spacing, the absolute error floor of one rounding


def adam_bounds(p0, m0, v0, g, t, lr, eps):
    """float64 Adam and the error the kernels' float32 arithmetic may add (derivation, unit roundoff u = 2^-24):
      m = b1 m0 + (1 - b1) g: two products and a sum, each rounded once (-ffp-contract=off), 1 - b1 exact:
          |dm| <= u (b1 |m0| + (1 - b1) |g| + |m|)   (<= 2 ulps of the larger term), + a denormal floor per rounding;
      v = b2 v0 + ((1 - b2) g) g: three roundings of the g term:  |dv| <= u (b2 v0 + 2 (1 - b2) g^2 + v);
      p = p0 - lr (m inv_c1) rcp(sqrt(v inv_c2) + eps): given m and v, c1 / c2 / their reciprocals (float casts), the products,
          the eps sum (each 0.5 ulp), v_sqrt_f32 and v_rcp_f32 (1 ulp each) are about 9 u = 5.4e-7 relative to the step: bounded
          by 1e-6 |lr u| (ADVICE); the final p0 - lr u rounds to 0.5 ulp(p); and the float32 errors of m and v propagate to first
          order as lr dm / (c1 den) and lr |u| (dv / 2 v) (sqrt(v_hat) / den)."""
    p, m, v, u, den = adam64(p0, m0, v0, g, t, lr, eps)
    c1, c2 = 1.0 - float(np.float32(0.9)) ** t, 1.0 - float(np.float32(0.999)) ** t
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    g, m0, v0 = (np.asarray(a, np.float64) for a in (g, m0, v0))
    em = _U * (b1 * np.abs(m0) + (1 - b1) * np.abs(g) + np.abs(m)) + 3 * _TINY
    ev = _U * (b2 * v0 + 2 * (1 - b2) * g * g + v) + 4 * _TINY
    s = np.sqrt(v / c2)
    with np.errstate(divide="ignore", invalid="ignore"):
        dv_rel = np.where(v > 0, ev / (2 * v), 0.0)
    ep = (1e-6 * lr * np.abs(u) + 0.5 * np.spacing(np.abs(p).astype(np.float32)).astype(np.float64)
          + lr * em / (c1 * den) + lr * np.abs(u) * dv_rel * s / den)
    return (p, m, v, u), (ep, em, ev)
