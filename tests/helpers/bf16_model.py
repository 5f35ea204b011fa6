"""float64 model of the engine's MFMA contractions at a given pass count, on the HIP run's own operands.

Precision (csrc/gemm_core.h): an fp32 operand x is split x = hi + lo, hi = bf16 nearest-even of x, lo = bf16 of x - hi.
  passes 1 (precision "bf16"):   hi*hi
  passes 2 (an exact operand):   hi*x + lo*x        (uint8 pixels: exact in bf16, so their lo plane is skipped)
  passes 3 ("bf16x3"):           hi*hi + lo*hi + hi*lo
Every bf16 product is exact in fp32, so the pass count fixes WHAT is summed; the kernel's only freedom is the fp32 rounding of
the sum.  Each model value therefore comes with S, the sum of the magnitudes of its terms, and the kernel must be within
c 2^-24 S of it, c the depth of its fp32 accumulation chain (see chain_depth).

Operands: S8 tensors (activations, pre-activation gradients, the weight mirror) are read back as their stored hi / lo halves;
fp32 operands a kernel rounds itself are split here with torch.bfloat16 (nearest-even, checked against rne_bf16_bits on the
host).  Everything is torch float64 on the device of the inputs: the helper needs no GPU, the GPU tests run it on one."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0**-24  # fp32 unit roundoff
FLOOR = 2.0**-126  # a flushed fp32 denormal: the absolute error floor of one operation
# The bf16 MFMA's internal sum of its 32 products is not documented.  Assumed: at most log2(32) fp32 levels (MFMA_TREE), and per
# fp32 operation 1 ulp rather than 1/2 (ROUNDING), in case an internal adder truncates.  Measured on the MI355X
# (tests/test_gpu_bf16_model.py, all cases), max |d| / (2^-24 S) against c = ROUNDING (MFMA_TREE + K steps + slabs + epilogue)
# = 18 .. 968: forward z 4.6, q 1.05, head-chain q_values 0.77, weight gradients 2.7 (conv) and 13.6 (dense, c = 80) -- every
# one below the K-step count alone, so both constants are conservative.
MFMA_TREE = 5
ROUNDING = 2
S8_STORE = 2.0**-17  # hi + lo of an S8 value against the fp32 value it was split from (|lo - (v - hi)| <= 2^-9 |v - hi|)


# ------------------------------------------------------------------ rounding and storage
def rne_bf16_bits(x):
    """Bit-level bf16 nearest-even of float32 values (numpy): the upper 16 bits after adding 0x7fff + the lowest kept bit.
    NaNs keep a quiet payload."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_bits_to_f64(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def split(x):
    """(hi, lo) float64 of fp32 values x as the kernels split them (split8 / s8_store_*): hi = bf16(x), lo = bf16(x - hi)."""
    x32 = torch.as_tensor(x).to(torch.float32)
    hi = x32.to(torch.bfloat16)
    lo = (x32 - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.to(torch.float64), lo.to(torch.float64)


def split_words(x):
    """The S8 image of a float32 buffer whose length is a multiple of 8 (what split_params_kernel / s8_store_group write),
    as int32 words: every 8 floats become 8 bf16 hi halves followed by 8 lo halves."""
    x32 = torch.as_tensor(x).to(torch.float32).reshape(-1, 8)
    hi = x32.to(torch.bfloat16)
    lo = (x32 - hi.to(torch.float32)).to(torch.bfloat16)
    return torch.stack([hi, lo], 1).contiguous().view(torch.int32).reshape(-1)


def s8_planes(region, rows, pitch):
    """(hi, lo) float64 [rows][pitch] of an S8 block stored [rows][pitch] (every 8 floats: 8 hi halves, then 8 lo halves)."""
    h = region[: rows * pitch].contiguous().view(torch.bfloat16).reshape(rows, pitch // 8, 2, 8).to(torch.float64)
    return h[:, :, 0].reshape(rows, pitch), h[:, :, 1].reshape(rows, pitch)


def s8_malformed(hi, lo):
    """Mask of S8 elements that are not a nearest-even split: |lo| must be at most half an ulp of hi (bf16: 8 significant bits).
    A truncating split leaves |lo| up to a whole ulp on about half of the elements."""
    a = hi.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    half_ulp = torch.where(a >= 2.0**-126, torch.exp2(e - 8), torch.full_like(a, 2.0**-134))
    return lo.abs() > half_ulp


# ------------------------------------------------------------------ contractions
def _terms(passes, a, b):
    """operand planes (hi, lo); lo None = exact operand.  The products the engine sums at `passes`."""
    (ah, al), (bh, bl) = a, b
    if passes == 1:
        return [(ah, bh)]
    if passes == 2:
        assert (al is None) != (bl is None), "two passes: exactly one operand is exact"
        return [(ah, bh), (al, bh)] if bl is None else [(ah, bh), (ah, bl)]
    assert passes == 3
    t = [(ah, bh)]
    if al is not None:
        t.append((al, bh))
    if bl is not None:
        t.append((ah, bl))
    return t


def contract(op, passes, a, b):
    """value = sum over the pass's products of op(a_part, b_part), S = the same with magnitudes.  op is bilinear."""
    val = mag = None
    for x, y in _terms(passes, a, b):
        v, m = op(x, y), op(x.abs(), y.abs())
        val = v if val is None else val + v
        mag = m if mag is None else mag + m
    return val, mag


def dense(passes, x, w):
    """x planes [N][in], w planes [in][out] (Flax layout): x @ w."""
    return contract(torch.matmul, passes, x, w)


def _same(size, k, s):
    out = -(-size // s)
    tot = max((out - 1) * s + k - size, 0)
    return out, tot // 2, tot - tot // 2


def _cols(x, k, s):
    """NHWC [N][H][W][C] -> im2col [N][Ho*Wo][C*k*k] with SAME padding (unfold order c, ky, kx)."""
    N, H, W, C = x.shape
    ho, lo_h, hi_h = _same(H, k, s)
    wo, lo_w, hi_w = _same(W, k, s)
    xp = F.pad(x.permute(0, 3, 1, 2), (lo_w, hi_w, lo_h, hi_h))
    return F.unfold(xp, k, stride=s).transpose(1, 2), ho, wo


def _wmat(w):
    kh, kw, cin, cout = w.shape
    return w.permute(2, 0, 1, 3).reshape(cin * kh * kw, cout)


def conv(passes, x, w, stride, chunk_elems=1 << 25):
    """SAME convolution: x planes NHWC [N][H][W][C], w planes HWIO -> [N][Ho*Wo][Cout] (pixel-major, the engine's row layout),
    as unfold + float64 matmul, in chunks of images."""
    k = w[0].shape[0]
    N, H, W, C = x[0].shape
    wm = tuple(None if p is None else _wmat(p) for p in w)
    _, ho, wo = _cols(x[0][:1], k, stride)
    step = max(1, chunk_elems // (ho * wo * C * k * k))
    vals, mags = [], []
    for i in range(0, N, step):
        xc = tuple(None if p is None else _cols(p[i : i + step], k, stride)[0] for p in x)
        v, m = contract(torch.matmul, passes, xc, wm)
        vals.append(v)
        mags.append(m)
    return torch.cat(vals), torch.cat(mags)


def conv_wgrad(passes, x, dz, k, stride, chunk_elems=1 << 25):
    """Weight gradient of a SAME convolution, HWIO: sum over images and output pixels of x patches times dz.
    x planes NHWC, dz planes [N][Ho*Wo][Cout]."""
    N, H, W, C = x[0].shape
    cout = dz[0].shape[-1]
    _, ho, wo = _cols(x[0][:1], k, stride)
    step = max(1, chunk_elems // (ho * wo * C * k * k))
    val = mag = 0
    for i in range(0, N, step):
        xc = tuple(None if p is None else _cols(p[i : i + step], k, stride)[0].reshape(-1, C * k * k).T for p in x)
        dc = tuple(None if p is None else p[i : i + step].reshape(-1, cout) for p in dz)
        v, m = contract(torch.matmul, passes, xc, dc)
        val, mag = val + v, mag + m
    to_hwio = lambda t: t.reshape(C, k, k, cout).permute(1, 2, 0, 3)
    return to_hwio(val), to_hwio(mag)


def conv_dgrad(passes, dz, w, hw, stride, chunk_elems=1 << 25):
    """Data gradient of a SAME convolution (the transposed convolution): dz planes [N][Ho*Wo][Cout], w planes HWIO, input
    size hw = (H, W) -> [N][H*W][Cin] (pixel-major), as a float64 matmul with the weights and a fold of the patches."""
    k, _, cin, cout = w[0].shape
    H, W = hw
    ho, lo_h, hi_h = _same(H, k, stride)
    wo, lo_w, hi_w = _same(W, k, stride)
    N = dz[0].shape[0]
    wt = tuple(None if p is None else _wmat(p).T for p in w)  # [Cout][Cin*k*k]

    def op(d, wm):  # bilinear in (d, wm); fold only sums, so magnitudes go through it unchanged
        cols = (d @ wm).transpose(1, 2)  # [n][Cin*k*k][Ho*Wo]
        img = F.fold(cols, (H + lo_h + hi_h, W + lo_w + hi_w), k, stride=stride)
        return img[:, :, lo_h : lo_h + H, lo_w : lo_w + W].permute(0, 2, 3, 1).reshape(d.shape[0], H * W, cin)

    step = max(1, chunk_elems // (ho * wo * cin * k * k))
    vals, mags = [], []
    for i in range(0, N, step):
        dc = tuple(None if p is None else p[i : i + step].reshape(-1, ho * wo, cout) for p in dz)
        v, m = contract(op, passes, dc, wt)
        vals.append(v)
        mags.append(m)
    return torch.cat(vals), torch.cat(mags)


def wgrad(passes, x, dz):
    """Dense weight gradient [in][out] = x^T dz, x planes [N][in], dz planes [N][out]."""
    return contract(torch.matmul, passes, tuple(None if p is None else p.T for p in x), dz)


# ------------------------------------------------------------------ bounds
def chain_depth(k, slabs=1, epilogue=2, block=32):
    """c of the bound |d| <= c 2^-24 S: the 32-product MFMA sum (MFMA_TREE levels, each relative to the magnitudes of its
    own K step: together at most MFMA_TREE S), the accumulator chain of ceil(k / block / slabs) K steps, the sequential sum
    of `slabs` split-K partials, and `epilogue` further fp32 operations -- each ROUNDING units.  k = 0: a plain fp32 sum
    of `slabs` terms."""
    steps = -(-k // (block * slabs)) if k else 0
    return ROUNDING * ((MFMA_TREE if k else 0) + steps + slabs + epilogue)


def bound(S, c):
    return c * U * S + c * FLOOR


def check(got, want, bnd, S=None, other=None, elementwise_control=True, label=""):
    """|got - want| <= bnd everywhere.  With `other` (the model of the same operands at the other pass count) also the negative
    control: the run is at least 4x closer to its own model than to the other one in the 2-norm, and (elementwise_control) the
    other model breaks the bound on at least half of the elements with a non-zero bound.  Returns (max |d| / bnd,
    max |d| / 2^-24 S when S is given, fraction of the other model outside the bound)."""
    got, want, bnd = (torch.as_tensor(t, dtype=torch.float64) for t in (got, want, bnd))
    d = (got - want).abs()
    pos = bnd > 0
    used = float((d[pos] / bnd[pos]).max()) if pos.any() else 0.0
    ratio = None
    if S is not None:
        S = torch.as_tensor(S, dtype=torch.float64)
        live = S > 0
        ratio = float((d[live] / (U * S[live])).max()) if live.any() else 0.0
    bad = d > bnd
    if bool(bad.any()):
        first = np.unravel_index(int(bad.reshape(-1).nonzero()[0]), tuple(bad.shape))
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.numel()} elements outside the bound (max |d| / bound = {used:.2f}, "
                             f"max |d| / 2^-24 S = {ratio}); first at {first}: got {float(got[first])!r} want {float(want[first])!r}")
    frac = None
    if other is not None:
        o = got - torch.as_tensor(other, dtype=torch.float64)
        n_own, n_other = float(torch.linalg.vector_norm(got - want)), float(torch.linalg.vector_norm(o))
        assert n_other >= 4 * n_own, f"{label}: negative control: |run - other passes| = {n_other:.3e} vs |run - own| = {n_own:.3e}"
        nz = bnd > 0
        frac = float((o.abs()[nz] > bnd[nz]).double().mean())
        if elementwise_control:
            assert frac >= 0.5, f"{label}: negative control: the other pass count breaks the bound on only {frac:.1%} of the elements"
    return used, ratio, frac


# ------------------------------------------------------------------ LayerNorm / ReLU
LN_EPS = 1e-6


def ln_stats(z):
    """mean, r = 1 / sqrt(var + eps), xhat over the last axis (the engine's var = max(E[z^2] - mean^2, 0))."""
    mean = z.mean(-1, keepdim=True)
    var = ((z * z).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
    r = torch.rsqrt(var + LN_EPS)
    return mean, var, r, (z - mean) * r


def ln_relu_bwd(z, gamma, mask, da, E_da, has_ln=True):
    """dz of y = relu(LayerNorm(z) gamma + beta) given dL/da (model) and its per-element error bound E_da; z [..., C] is the
    kernel's own fp32 z, mask its own ReLU decisions.  Returns (dz, bound): the bound carries E_da through the backward
    (first order) and adds the fp32 arithmetic of the LayerNorm backward itself -- its two row means (a chain of C + 8
    operations at most), r and xhat computed from E[z^2] - mean^2 (relative error C u (E[z^2] + mean^2) / (var + eps)) --
    and the S8 storage of dz."""
    if not has_ln:
        dz = da * mask
        return dz, (E_da + S8_STORE * dz.abs() + FLOOR) * mask  # blocked elements: exactly 0
    C = z.shape[-1]
    mean, var, r, xhat = ln_stats(z)
    A = gamma.abs() * mask
    g = da * gamma * mask
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xhat).mean(-1, keepdim=True)
    dz = r * (g - m1 - xhat * m2)
    ax = xhat.abs()
    ae = A * E_da
    prop = r * (ae + ae.mean(-1, keepdim=True) + ax * (ae * ax).mean(-1, keepdim=True))
    c_ln = ROUNDING * (C + 8)
    ga = g.abs()
    arith = c_ln * U * r * (ga + ga.mean(-1, keepdim=True) + ax * (ga * ax).mean(-1, keepdim=True))
    eps_r = c_ln * U * ((z * z).mean(-1, keepdim=True) + mean * mean) / (var + LN_EPS)
    eps_x = eps_r * ax + c_ln * U * r * z.abs().mean(-1, keepdim=True)
    stat = dz.abs() * eps_r + r * (eps_x * m2.abs() + ax * (ga * eps_x).mean(-1, keepdim=True))
    return dz, prop + arith + stat + S8_STORE * dz.abs() + c_ln * FLOOR


def ln_param_grads(z, mask, da, E_da, chain):
    """The LayerNorm scale / bias leaves of y = relu(LayerNorm(z) gamma + beta): (dgamma, E_dgamma, dbeta, E_dbeta) per channel, the
    sums over every leading axis of dy xhat and of dy, dy = mask da, xhat from the kernel's own fp32 z (ln_stats).  The bound of each is
    the sum of three terms: E_da carried through (sum mask E_da |xhat|, sum mask E_da); the fp32 error of xhat itself (eps_x, as
    derived in ln_relu_bwd) on sum |dy|, for the scale only; and a plain fp32 chain of `chain` additions -- the rows summed into one
    partial row plus the partial rows summed behind it, from the route -- on the magnitude sum of the terms (chain_depth(0, chain):
    the product dy xhat and the final store are its epilogue)."""
    C = z.shape[-1]
    mean, var, r, xhat = ln_stats(z)
    dy = da * mask
    ax, ady = xhat.abs(), dy.abs()
    c_ln = ROUNDING * (C + 8)
    eps_r = c_ln * U * ((z * z).mean(-1, keepdim=True) + mean * mean) / (var + LN_EPS)
    eps_x = eps_r * ax + c_ln * U * r * z.abs().mean(-1, keepdim=True)
    rows = lambda t: t.reshape(-1, C).sum(0)
    c = chain_depth(0, slabs=chain)
    Eg = rows(mask * E_da * ax) + rows(ady * eps_x) + bound(rows(ady * ax), c)
    Eb = rows(mask * E_da) + bound(rows(ady), c)
    return rows(dy * xhat), Eg, rows(dy), Eb


def ln_relu_fwd(z, gamma, beta, E_z, has_ln=True):
    """a = relu(LayerNorm(z) gamma + beta) (or relu(z)) of a model z with per-element error bound E_z, and the bound of the kernel's
    S8 activation against it: E_z carried through the normalisation (first order; relu is 1-Lipschitz), the fp32 arithmetic of
    the row statistics (a chain of C + 8 operations at most, relative to E[z^2] + mean^2 over var + eps) and of the affine map,
    and the S8 storage."""
    if not has_ln:
        a = z.clamp_min(0)
        return a, E_z + S8_STORE * a + FLOOR
    C = z.shape[-1]
    mean, var, r, xhat = ln_stats(z)
    y = xhat * gamma + beta
    a = y.clamp_min(0)
    ax, ag = xhat.abs(), gamma.abs()
    prop = ag * r * (E_z + E_z.mean(-1, keepdim=True) + ax * (E_z * ax).mean(-1, keepdim=True))
    c_ln = ROUNDING * (C + 8)
    eps_r = c_ln * U * ((z * z).mean(-1, keepdim=True) + mean * mean) / (var + LN_EPS)
    stat = ag * (eps_r * ax + c_ln * U * r * z.abs().mean(-1, keepdim=True))
    arith = ROUNDING * 4 * U * (ag * ax + beta.abs())
    return a, prop + stat + arith + S8_STORE * a + c_ln * FLOOR


def bellman_targets(q_next, reward, terminal, gamma_n, K, A):
    """r + (1 - term) gamma^n max_a q_next[k] for the K target heads k = 0 .. K - 1: [B][K]."""
    qn = q_next[:, : K * A].reshape(-1, K, A).max(-1).values
    return reward[:, None] + (1.0 - terminal[:, None]) * gamma_n * qn
