"""float64 restatements of each stage of the BatchNorm learn path (csrc/batchnorm.h) on given operands, each with the error bound
the kernel's own fp32 arithmetic may use, and of the plan's BatchNorm sites (csrc/net_plan.h: BnSite).  torch float64 on the
device of the inputs, like bf16_model.py: nothing here needs a GPU.  tests/test_batchnorm_stages_host.py checks every function
against torch autograd and the oracle on the CPU; tests/test_gpu_batchnorm.py runs them on the HIP run's own tensors (cnn, fc), and
tests/test_gpu_impala_backward.py on the impala torso's sites (layers / site_layout with arch="impala").

Layout: a site's tensor is [N][P][Cp] -- rows, positions, channels padded to 8.  A spatial site (BatchNorm(axis=(1, 2)) on an image)
keeps one statistic per position p over the rows AND the C true channels; a feature site one per internal column p * Cp + c over
the rows.  Padded channels (c >= C) enter no sum and no count, and every stage writes exactly 0 there.

Bounds.  U, ROUNDING (units per fp32 operation), FLOOR and S8_STORE are bf16_model's.  A sum of n terms in the kernel's order is
within ROUNDING * depth * U * (sum of the magnitudes) of the exact one, depth the longest chain of additions one value goes
through (spatial_depth / feature_depth below, in the form of bf16_model.chain_depth); what is done to a term before it is added
(a product, the normalisation) counts on top.  Nothing is fitted: usage above 1.0 on the correct kernel names a missing term."""
import numpy as np
import torch

from tests.helpers import bf16_model as M

_ceil = lambda a, b: -(-a // b)
BN_EPS = float(np.float32(1e-5))
BN_MOMENTUM = float(np.float32(0.99))
BN_ONE_MINUS = float(np.float32(1.0) - np.float32(0.99))  # what `1.f - BN_MOMENTUM` is in fp32
CONVS = ((8, 4), (4, 2), (3, 1))
# fp32 operations on one normalised value xhat = (x - mean) * rsqrt(var + eps): the difference, var + eps, the hardware rsqrt
# (1 ulp = ROUNDING units), the product
XHAT_OPS = 4


# ------------------------------------------------------------------ the cases of the GPU stage test and their inputs
# The smallest shapes at which each loop and route of csrc/batchnorm.h can still go wrong (tests/test_gpu_batchnorm.py says what
# each one forces).  n_heads = 1: the single-head TF-DQN form (the head is regressed on its own stop-gradient target).
CASES = {
    "cnn-84x84x4-B40": dict(arch="cnn", obs=(84, 84, 4), feats=(8, 16, 8, 32), K=2, A=3, B=40, ln=True, n_heads=3),
    "cnn-52x60x2-B33-noln": dict(arch="cnn", obs=(52, 60, 2), feats=(16, 20, 12, 24), K=3, A=4, B=33, ln=False, n_heads=4),
    "cnn-headline-B8": dict(arch="cnn", obs=(84, 84, 4), feats=(32, 64, 64, 512), K=3, A=4, B=8, ln=True, n_heads=4),
    "fc-d6-B37": dict(arch="fc", obs=(6,), feats=(300, 24), K=1, A=4, B=37, ln=True, n_heads=1),
}
PARAM_SEED, BATCH_SEED = 3, 11


def case_inputs(case):
    """Parameters, running averages and the batch of a case, as gpu_helpers.make_pair(seed=PARAM_SEED, batch_norm=True) and
    make_frame_batch(seed=BATCH_SEED) make them: params / stats (Flax layout), then for a cnn frames / ids and for fc state /
    next_state, and action / reward / terminal."""
    from oracle import network as onet
    from tests.gpu_helpers import make_frame_batch, perturbed_params

    cfg = CASES[case]
    params = perturbed_params(PARAM_SEED, cfg["obs"], list(cfg["feats"]), cfg["arch"], cfg["n_heads"] * cfg["A"], cfg["ln"], batch_norm=True)
    rng = np.random.default_rng(PARAM_SEED + 2)
    stats = {m: {"mean": rng.normal(0, 0.3, l["mean"].shape).astype(np.float32), "var": rng.uniform(0.5, 2.0, l["var"].shape).astype(np.float32)}
             for m, l in onet.init_batch_stats(params).items()}
    out = dict(cfg=cfg, params=params, stats=stats)
    B, A = cfg["B"], cfg["A"]
    if cfg["arch"] == "cnn":
        h, w, stack = cfg["obs"]
        frames, ids, action, reward, terminal, _ = make_frame_batch(B, A, seed=BATCH_SEED, h=h, w=w, stack=stack)
        out.update(frames=frames, ids=ids)
    else:
        rng = np.random.default_rng(BATCH_SEED)
        d = cfg["obs"][0]
        out.update(state=rng.normal(size=(B, d)).astype(np.float32), next_state=rng.normal(size=(B, d)).astype(np.float32))
        action, reward = rng.integers(0, A, B).astype(np.int32), rng.normal(size=B).astype(np.float32)
        terminal = (rng.random(B) < 0.3).astype(np.uint8)
    out.update(action=action, reward=reward, terminal=terminal)
    return out


# ------------------------------------------------------------------ the plan's layers and sites, restated (net_plan.h)
def _same(size, k, s):
    out = _ceil(size, s)
    return out, max((out - 1) * s + k - size, 0) // 2


def impala_geometry(cfg):
    """the three Stacks of an impala case (impala_stages.geometry: H, W, Hp, Wp, pad, cin, cin_p, C, C_p)"""
    from tests.helpers import impala_stages as IS

    geo = IS.geometry(cfg["obs"], cfg["feats"])
    assert geo is not None, "the plan refuses this observation (the two sides need different pool padding)"
    return geo


def layers(cfg):
    """Hidden layers of a BatchNorm cnn / fc / impala plan in order: name, kind (0 conv, 1 dense, 2 the impala torso as one layer),
    LayerNorm name, c / cp (true / padded width), npix, conv k / s / hin / win / hout / wout / cin / cin_p, K (contraction length)
    and in_p (dense input width)."""
    out, n_ln, ln = [], 0, cfg["ln"]
    if cfg["arch"] == "impala":
        # the torso is ONE hidden layer (net_plan.h: the pseudo-layer "Impala", kind 2): the residual stream behind Stack_2 with the
        # top-level LayerNorm_0 and the ReLU behind it, in a conv layer's output geometry; the Dense layers follow it
        g = impala_geometry(cfg)[-1]
        co, cp, npix = g["C"], g["C_p"], g["Hp"] * g["Wp"]
        out.append(dict(name="Impala", kind=2, ln="LayerNorm_0" if ln else None, c=co, cp=cp, npix=npix, hout=g["Hp"], wout=g["Wp"]))
        n_ln += ln
        in_f, in_p, dense = npix * co, npix * cp, cfg["feats"][3:]
    elif cfg["arch"] == "cnn":
        h, w, c = cfg["obs"]
        cp = 8  # the input site's S8 rows: 8-padded channels
        for i, (k, s) in enumerate(CONVS):
            (ho, _), (wo, _) = _same(h, k, s), _same(w, k, s)
            co = int(cfg["feats"][i])
            out.append(dict(name=f"Conv_{i}", kind=0, ln=f"LayerNorm_{n_ln}" if ln else None, c=co, cp=_ceil(co, 8) * 8, npix=ho * wo, k=k, s=s,
                            hin=h, win=w, hout=ho, wout=wo, cin=c, cin_p=cp, K=k * k * cp))
            h, w, c, cp = ho, wo, co, _ceil(co, 8) * 8
            n_ln += ln
        in_f, in_p, dense = h * w * c, h * w * cp, cfg["feats"][3:]
    else:
        in_f = int(np.prod(cfg["obs"]))
        in_p, dense = _ceil(in_f, 8) * 8, cfg["feats"]
    for j, c in enumerate(dense):
        c = int(c)
        out.append(dict(name=f"Dense_{j}", kind=1, ln=f"LayerNorm_{n_ln}" if ln else None, c=c, cp=_ceil(c, 8) * 8, npix=1, K=in_p, in_p=in_p,
                        in_f=in_f))
        n_ln += ln
        in_f, in_p = c, _ceil(c, 8) * 8
    return out


def site_layout(cfg):
    """BatchNorm sites in Flax's call order: name ("BatchNorm_i"), region prefix "bn/<name>/", the hidden layer whose activation
    the site normalises (-1: the cnn's / impala's input x / 255), the region holding its input, spatial, P, C, Cp, G (statistic
    groups: P for a spatial site, P * Cp internal columns for a feature site) and the Flax shape of its scale / bias / mean / var.
    impala (net_plan.h: plan_impala_torso, place_bn_regions): the input site on bn/x0, then inside every Stack s the two block sites
    "Stack_s/BatchNorm_b" (layer -2 - (2 s + b), as BnSite.layer) on imp/s{s}/a1_{b} -- spatial, one statistic per pooled pixel --
    then the feature site behind the flatten on act/Impala and the Dense sites; the top-level sites count on their own
    (BatchNorm_0, BatchNorm_1, ...), the block sites are named inside their Stack."""
    out = []
    n_top = [0]

    def add(layer, src, spatial, P, C, Cp, shape, name=None):
        if name is None:
            name = f"BatchNorm_{n_top[0]}"
            n_top[0] += 1
        out.append(dict(name=name, prefix=f"bn/{name}/", layer=layer, src=src, spatial=bool(spatial), P=P, C=C, Cp=Cp, G=P if spatial else P * Cp,
                        flax_shape=shape))

    if cfg["arch"] == "impala":
        h, w, c = cfg["obs"]
        add(-1, "bn/x0", True, h * w, c, 8, (h, w))
        for s, g in enumerate(impala_geometry(cfg)):
            for b in range(2):
                add(-2 - (2 * s + b), f"imp/s{s}/a1_{b}", True, g["Hp"] * g["Wp"], g["C"], g["C_p"], (g["Hp"], g["Wp"]), name=f"Stack_{s}/BatchNorm_{b}")
        for i, L in enumerate(layers(cfg)):
            add(i, f"act/{L['name']}", False, L["npix"], L["c"], L["cp"], (L["npix"] * L["c"],))
        return out
    if cfg["arch"] == "cnn":
        h, w, c = cfg["obs"]
        add(-1, "bn/x0", True, h * w, c, 8, (h, w))
    for i, L in enumerate(layers(cfg)):
        if L["kind"] == 0:  # behind the first two ReLUs per position, behind the flatten per feature
            add(i, f"act/{L['name']}", i < 2, L["npix"], L["c"], L["cp"], (L["hout"], L["wout"]) if i < 2 else (L["npix"] * L["c"],))
        else:
            add(i, f"act/{L['name']}", False, 1, L["c"], L["cp"], (L["c"],))
    return out


# ------------------------------------------------------------------ summation depths
def spatial_depth(N, C):
    """bn_stats_spatial_kernel: a lane adds the C true channels of each of its ceil(N / 64) rows in sequence, then 6 shuffle levels"""
    return _ceil(N, 64) * C + 6


def feature_depth(N):
    """bn_stats_feature_kernel: a row slice adds its ceil(N / 8) rows in sequence, then the 8 slices in slice order"""
    return _ceil(N, 8) + 8


def _depth(N, spatial, C):
    return spatial_depth(N, C) if spatial else feature_depth(N)


def _true(x, C):
    """mask [Cp] of the true channels of x [N][P][Cp]"""
    return (torch.arange(x.shape[-1], device=x.device) < C).to(x.dtype)


def _sum(t, spatial):
    """the site's reduction of t [N][P][Cp] (padded channels already zero): [P] or [P * Cp]"""
    return t.sum(dim=(0, 2)) if spatial else t.sum(0).reshape(-1)


def _per_element(v, x, spatial):
    """a per-group vector [G] broadcast to x's shape [N][P][Cp]"""
    return v.reshape(1, -1, 1) if spatial else v.reshape(1, x.shape[1], x.shape[2])


# ------------------------------------------------------------------ stages
def bn_stats(x, spatial, C, rows=None, count=None, fast_variance=True):
    """mean, var = max(0, E[x^2] - E[x]^2) (flax's fast variance) of x [N][P][Cp] float64, and their bounds (d_mean, d_var).
    d_mean: the sum's depth + the reciprocal of the count and its product.  E[x^2]: one more, each square is rounded.  var: the
    cancellation 2 |mean| d_mean (+ d_mean^2), the rounding of mean^2 and of the difference.
    `rows` (a mask [N]), `count` and `fast_variance=False` build the wrong variants of the host test: rows that enter the sums,
    the divisor, var without its - mean^2."""
    N = x.shape[0]
    m = _true(x, C)
    xs = x * m
    if rows is not None:
        xs = xs * rows.to(x.dtype).reshape(-1, 1, 1)
    Mc = float(count if count is not None else (N * C if spatial else N))
    depth = _depth(N, spatial, C)
    mean, a1 = _sum(xs, spatial) / Mc, _sum(xs.abs(), spatial) / Mc
    e2 = _sum(xs * xs, spatial) / Mc
    var = (e2 - mean * mean if fast_variance else e2).clamp_min(0)
    d_mean = M.ROUNDING * (depth + 2) * M.U * a1 + M.FLOOR
    d_e2 = M.ROUNDING * (depth + 3) * M.U * e2 + M.FLOOR
    d_var = d_e2 + 2 * mean.abs() * d_mean + d_mean * d_mean + M.ROUNDING * M.U * (e2 + 2 * mean * mean) + M.FLOOR
    return mean, var, d_mean, d_var


def _mul(var, scale):
    return torch.rsqrt(var + BN_EPS) * scale


def bn_apply(x, mean, var, scale, bias, spatial, C, E_x=None):
    """y = (x - mean) * (rsqrt(var + eps) * scale) + bias on the true channels, 0 on the padded ones, and its bound: XHAT_OPS + 1
    operations on the product (the factor rsqrt * scale is one more), one on the sum with the bias, the S8 storage of y; E_x (an
    error bound of x, for a chain of stages) goes through the factor."""
    m = _true(x, C)
    mul = _per_element(_mul(var, scale), x, spatial)
    t = (x - _per_element(mean, x, spatial)) * mul
    y = (t + _per_element(bias, x, spatial)) * m
    E = (M.ROUNDING * M.U * ((XHAT_OPS + 1) * t.abs() + y.abs()) + M.S8_STORE * y.abs() + M.FLOOR) * m
    if E_x is not None:
        E = E + mul.abs() * E_x * m
    return y, E


def bn_backward(x, dy, mean, var, scale, spatial, C, E_dy=None, s1=None, s2=None, inv_m=None):
    """s1 = sum dy, s2 = sum dy * xhat (the gradients of bias and scale), dx = scale * rstd * (dy - s1 / M - xhat * s2 / M) with
    M = N * C (spatial) or N; padded channels of dx are 0.  Returns (s1, d_s1, s2, d_s2, dx, d_dx).
    Bounds: the sums as in bn_stats, each term of s2 after XHAT_OPS + 1 operations (xhat and the product); dx: about ten operations
    on three terms.  `E_dy`: an error bound of dy (a modelled data gradient), carried to first order into all three.
    `s1` / `s2`: the sums dx is computed from (the run's own, stage by stage); default: the ones computed here.
    `inv_m`: the wrong variant of the host test."""
    N = x.shape[0]
    m = _true(x, C)
    depth = _depth(N, spatial, C)
    rstd = _per_element(torch.rsqrt(var + BN_EPS), x, spatial)
    xhat = (x - _per_element(mean, x, spatial)) * rstd * m
    d = dy * m
    S1, S2 = _sum(d, spatial), _sum(d * xhat, spatial)
    d_s1 = M.ROUNDING * depth * M.U * _sum(d.abs(), spatial) + M.FLOOR
    d_s2 = M.ROUNDING * (depth + XHAT_OPS + 1) * M.U * _sum((d * xhat).abs(), spatial) + M.FLOOR
    if E_dy is not None:
        d_s1 = d_s1 + _sum(E_dy * m, spatial)
        d_s2 = d_s2 + _sum(E_dy * xhat.abs(), spatial)
    inv = float(inv_m) if inv_m is not None else 1.0 / (N * C if spatial else N)
    u1 = _per_element(S1 if s1 is None else s1, x, spatial) * inv
    u2 = _per_element(S2 if s2 is None else s2, x, spatial) * inv
    k = _per_element(scale, x, spatial) * rstd
    dx = k * (d - u1 - xhat * u2) * m
    d_dx = (M.ROUNDING * 10 * M.U * k.abs() * (d.abs() + u1.abs() + (xhat * u2).abs()) + M.FLOOR) * m
    if E_dy is not None:
        d_dx = d_dx + k.abs() * E_dy * m
    return S1, d_s1, S2, d_s2, dx, d_dx


def running(ra, batch, momentum=None):
    """0.99f * ra + (1 - 0.99f) * batch in fp32 with the kernel's constants (float32 numpy in, float32 out) and the bound of
    2 ulp of the result (two products and a sum, or a product and an fma).  `momentum`: the wrong variant of the host test."""
    ra, batch = np.asarray(ra, np.float32), np.asarray(batch, np.float32)
    mo = np.float32(BN_MOMENTUM if momentum is None else momentum)
    want = (mo * ra + (np.float32(1.0) - mo) * batch).astype(np.float32)
    return want, 2.0 * np.spacing(np.abs(want)).astype(np.float64)


# ------------------------------------------------------------------ a stage-free chain: layers on modelled operands
# |hi hi - x w| <= (2^-9 + 2^-9 + 2^-18) |x| |w| for one bf16 pass; three passes leave lo * lo and the roundings of the two lo halves
PASS_TRUNCATION = {1: 2.0**-8 + 2.0**-18, 3: 2.0**-16}


def exact_layer(op, x, E_x, w, passes, c):
    """A contraction on a MODELLED operand x (error bound E_x) and exact weights w: value = op(x, w) in float64, bound = the
    products the pass count leaves out (PASS_TRUNCATION, relative to S = op(|x|, |w|)) + the fp32 chain c + E_x through |w|."""
    v, S = op(x, w), op(x.abs(), w.abs())
    return v, PASS_TRUNCATION[passes] * S + M.bound(S, c) + op(E_x, w.abs()), S


# ------------------------------------------------------------------ the whole learn step in float64 (host test: inputs of the variants)
def reference_step(cfg, params, x_in, action, reward, terminal, gamma=0.99, n_heads=None):
    """The BatchNorm learn step of a cnn / fc case in float64 from exact operands, assembled from the stage functions above and
    bf16_model's contractions (a single exact pass): per site its input x [N][P][Cp], mean / var, out, the gradient dy w.r.t. its
    output with a bound E_dy (the data gradient's chain on these magnitudes), s1 / s2 / dx; per layer z, act, dz; q, q_values,
    targets and dL/dq.  x_in: cnn float64 [2B][h][w][8] (x / 255, padded channels 0), fc [2B][obs].  params: Flax layout."""
    L, sites = layers(cfg), site_layout(cfg)
    K, A, B = cfg["K"], cfg["A"], cfg["B"]
    n_heads = n_heads or 1 + K
    oh = 1 if n_heads >= 2 else 0
    N = 2 * B
    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    site_of = {s["layer"]: s for s in sites}
    out = dict(sites={}, layers={})

    def site_fwd(s, x):
        p = params[s["name"]]
        sc, bi = (pad_groups(s, t64(p[k])) for k in ("scale", "bias"))
        mean, var, d_mean, d_var = bn_stats(x, s["spatial"], s["C"])
        y, E_y = bn_apply(x, mean, var, sc, bi, s["spatial"], s["C"])
        out["sites"][s["name"]] = dict(x=x, mean=mean, var=var, d_mean=d_mean, d_var=d_var, out=y, E_out=E_y, scale=sc, bias=bi)
        return y

    cur = None
    if cfg["arch"] == "cnn":
        h, w, _ = cfg["obs"]
        cur = site_fwd(site_of[-1], x_in.reshape(N, h * w, 8))
    else:
        fc_in = x_in
    for i, l in enumerate(L):
        W, b = t64(params[l["name"]]["kernel"]), t64(params[l["name"]]["bias"])
        if l["kind"] == 0:
            xin = cur.reshape(N, l["hin"], l["win"], l["cin_p"])[..., : l["cin"]]
            z, _ = M.conv(1, (xin, None), (W, None), l["s"])
        else:
            xin = fc_in if cur is None else cur.reshape(N, -1, site_of[i - 1]["Cp"])[:, :, : site_of[i - 1]["C"]].reshape(N, -1)
            z, _ = M.dense(1, (xin, None), (W, None))
        z = z + b
        g, be = (t64(params[l["ln"]][k]) if l["ln"] else None for k in ("scale", "bias"))
        a, _ = M.ln_relu_fwd(z, g, be, torch.zeros_like(z), has_ln=l["ln"] is not None)
        a_p = torch.zeros(N, l["npix"], l["cp"], dtype=torch.float64)
        a_p[:, :, : l["c"]] = a.reshape(N, l["npix"], l["c"])
        out["layers"][l["name"]] = dict(xin=xin, z=z.reshape(N, l["npix"], l["c"]), act=a_p, W=W, gamma=g)
        cur = site_fwd(site_of[i], a_p)
    last = site_of[len(L) - 1]
    hid = cur.reshape(N, -1, last["Cp"])[:, :, : last["C"]].reshape(N, -1)
    head = f"Dense_{sum(l['kind'] == 1 for l in L)}"
    Wh = t64(params[head]["kernel"])
    q = hid @ Wh + t64(params[head]["bias"])
    a_idx = torch.as_tensor(np.asarray(action), dtype=torch.int64)
    cols = (torch.arange(K)[None, :] + oh) * A + a_idx[:, None]
    qv = q[:B].gather(1, cols)
    tg = M.bellman_targets(q[B:], t64(reward), t64(terminal), gamma, K, A)
    dout = torch.zeros(N, n_heads * A, dtype=torch.float64)
    dout[:B] = dout[:B].scatter(1, cols, 2.0 * (qv - tg) / B)
    out.update(q=q, q_values=qv, targets=tg, dout=dout, cols=cols, head_in=hid, head=head)
    # ---- backward
    dy, S = dout @ Wh.T, dout.abs() @ Wh.abs().T
    E = M.bound(S, M.chain_depth(_ceil(n_heads * A, 8) * 8, epilogue=3))
    for i in range(len(L) - 1, -1, -1):
        l, s = L[i], site_of[i]
        r = out["sites"][s["name"]]
        pad = lambda t: _pad_channels(t.reshape(N, s["P"], s["C"]), s["Cp"])
        dyp, Ep = pad(dy), pad(E)
        s1, d_s1, s2, d_s2, dx, d_dx = bn_backward(r["x"], dyp, r["mean"], r["var"], r["scale"], s["spatial"], s["C"], E_dy=Ep)
        r.update(dy=dyp, E_dy=Ep, s1=s1, d_s1=d_s1, s2=s2, d_s2=d_s2, dx=dx, d_dx=d_dx)
        lay = out["layers"][l["name"]]
        mask = (lay["act"][:, :, : l["c"]] > 0).double()
        dz, E_dz = M.ln_relu_bwd(lay["z"], lay["gamma"], mask, dx[:, :, : l["c"]], d_dx[:, :, : l["c"]], has_ln=l["ln"] is not None)
        lay.update(dz=dz, E_dz=E_dz, mask=mask)
        if l["kind"] == 0:
            dy, S = M.conv_dgrad(1, (dz, None), (lay["W"], None), (l["hin"], l["win"]), l["s"])
            E = M.bound(S, M.chain_depth(l["k"] ** 2 * l["cp"], epilogue=4))
        elif i > 0:
            dy, S = dz.reshape(N, -1) @ lay["W"].T, dz.reshape(N, -1).abs() @ lay["W"].abs().T
            E = M.bound(S, M.chain_depth(l["cp"], epilogue=3))
    if cfg["arch"] == "cnn":
        s = site_of[-1]
        r = out["sites"][s["name"]]
        dyp, Ep = (_pad_channels(t.reshape(N, s["P"], s["C"]), 8) for t in (dy, E))
        s1, d_s1, s2, d_s2, dx, d_dx = bn_backward(r["x"], dyp, r["mean"], r["var"], r["scale"], True, s["C"])  # (sums from the stored da)
        r.update(dy=dyp, E_dy=Ep, s1=s1, d_s1=d_s1, s2=s2, d_s2=d_s2, dx=dx, d_dx=d_dx)
    return out


def _pad_channels(t, Cp):
    out = torch.zeros(*t.shape[:-1], Cp, dtype=t.dtype, device=t.device)
    out[..., : t.shape[-1]] = t
    return out


def pad_groups(site, v):
    """a Flax-shaped scale / bias / mean / var of a site as its G internal groups (feature sites: column p * Cp + c, padded 0)"""
    v = torch.as_tensor(v).reshape(-1)
    if site["spatial"]:
        return v
    return _pad_channels(v.reshape(site["P"], site["C"]), site["Cp"]).reshape(-1)
