"""Plain restatements of what csrc/impala.h does BETWEEN the convolutions of the impala torso, and of the plan's geometry
(csrc/net_plan.h): the frame decode, the 3x3 / 2 SAME max-pool with its winners and its backward, the ReLU-mask + S8 conversion
with its column sums, the residual add.  torch on the device of the inputs (float64 wherever a sum is taken), like bf16_model.py:
nothing here needs a GPU, tests/test_impala_stages_host.py checks every function against torch / the oracle on the CPU, and the GPU
tests (tests/test_gpu_impala.py; tests/test_gpu_impala_backward.py for block_backward and what it is built from: one residual block
of impala_backward with every intermediate, every leaf and the bound each carries) run them on the HIP run's own tensors.

The tie rule of the pool: the winner of a window is the FIRST maximum in row-major window order (ky * 3 + kx) among the positions
inside the image -- what `vv[e] > best[e]` gives in imp_pool_fwd_kernel, what `a == ky * 3 + kx` reads back in
imp_pool_bwd_kernel, and what torch's CPU max_pool2d does (checked in the host test on an all-zero input)."""
import numpy as np
import torch

from tests.helpers import bf16_model as M

_ceil = lambda a, b: -(-a // b)
LN_MAX_BLOCKS = 256  # csrc: workgroups of the row-wise kernels (imp_blocks), 16 rows each
ROWS_PER_BLOCK = 16


# ------------------------------------------------------------------ geometry (net_plan.h: ImpalaStack, the impala regions)
def pool_same(size):
    """(output size, pad_lo) of the 3x3 / 2 SAME pool over `size`."""
    out = _ceil(size, 2)
    return out, max((out - 1) * 2 + 3 - size, 0) // 2


def geometry(obs, feats):
    """Per Stack: H, W (first convolution), Hp, Wp (behind the pool), pad, cin, cin_p, C, C_p.  None when the plan refuses the
    shape (the two sides need different pool padding in some Stack)."""
    h, w, c = obs
    c_p, out = 8, []
    for s in range(3):
        (hp, pad), (wp, pad_w) = pool_same(h), pool_same(w)
        if pad != pad_w:
            return None
        C = int(feats[s])
        out.append(dict(H=h, W=w, Hp=hp, Wp=wp, pad=pad, cin=c, cin_p=c_p, C=C, C_p=_ceil(C, 8) * 8))
        h, w, c, c_p = hp, wp, C, out[-1]["C_p"]
    return out


def wgrad_chain(B, npix, K):
    """(K steps of one accumulator, slabs) of an impala convolution's weight gradient on the generic engine: net_plan.h, the
    impala regions (gw_slabs), and launch_conv_wgrad / conv_wgrad_slabs."""
    ksteps = _ceil(B * npix, 32)
    sp = max(1, min(256 // _ceil(K, 64), ksteps))
    steps = _ceil(ksteps, sp)
    return steps, _ceil(ksteps, steps)


def row_blocks(rows):
    """workgroups of a row-wise kernel over `rows` rows, and the most rows one lane group walks (its sequential chain)."""
    blocks = min(_ceil(rows, ROWS_PER_BLOCK), LN_MAX_BLOCKS)
    return blocks, _ceil(_ceil(rows, ROWS_PER_BLOCK), blocks)


# ------------------------------------------------------------------ max-pool 3x3 / 2 SAME
def _padded_size(size):
    return (_ceil(size, 2) - 1) * 2 + 3


def pool_fwd(z, pad):
    """z [N][H][W][C] -> (values [N][Hp][Wp][C] in z's dtype, winners int64): -inf padding with `pad` rows / columns in front,
    winner = ky * 3 + kx of the first maximum in row-major window order (padding never wins: every window holds a real pixel)."""
    N, H, W, C = z.shape
    Hp, Wp = _ceil(H, 2), _ceil(W, 2)
    zp = torch.full((N, max(_padded_size(H), H + pad), max(_padded_size(W), W + pad), C), float("-inf"), dtype=z.dtype, device=z.device)
    zp[:, pad : pad + H, pad : pad + W] = z
    win = torch.stack([zp[:, ky : ky + 2 * Hp - 1 : 2, kx : kx + 2 * Wp - 1 : 2] for ky in range(3) for kx in range(3)])
    best = win.max(0).values
    k = torch.arange(9, device=z.device).reshape(9, 1, 1, 1, 1)
    first = torch.where(win == best, k, torch.full_like(k, 9)).min(0).values
    return best, first


def pool_ties(z, pad):
    """[N][Hp][Wp][C] number of window positions bit-equal to the window's maximum."""
    N, H, W, C = z.shape
    Hp, Wp = _ceil(H, 2), _ceil(W, 2)
    zp = torch.full((N, max(_padded_size(H), H + pad), max(_padded_size(W), W + pad), C), float("-inf"), dtype=z.dtype, device=z.device)
    zp[:, pad : pad + H, pad : pad + W] = z
    win = torch.stack([zp[:, ky : ky + 2 * Hp - 1 : 2, kx : kx + 2 * Wp - 1 : 2] for ky in range(3) for kx in range(3)])
    return (win == win.max(0).values).sum(0)


def pool_bwd(dp, arg, H, W, pad):
    """Scatter-add of dp [N][Hp][Wp][C] to the positions `arg` chose: (dz [N][H][W][C] float64, S = the same sum over |dp|,
    n = how many windows chose the pixel: at most 4)."""
    N, Hp, Wp, C = dp.shape
    dev = dp.device
    arg = arg.to(torch.int64)
    PH, PW = max(_padded_size(H), H + pad), max(_padded_size(W), W + pad)
    oy = torch.arange(Hp, device=dev).reshape(1, Hp, 1, 1)
    ox = torch.arange(Wp, device=dev).reshape(1, 1, Wp, 1)
    n = torch.arange(N, device=dev).reshape(N, 1, 1, 1)
    c = torch.arange(C, device=dev).reshape(1, 1, 1, C)
    flat = (((n * PH + 2 * oy + arg // 3) * PW + 2 * ox + arg % 3) * C + c).reshape(-1)
    d = dp.to(torch.float64).reshape(-1)
    crop = lambda t: t.reshape(N, PH, PW, C)[:, pad : pad + H, pad : pad + W]
    acc = lambda src: crop(torch.zeros(N * PH * PW * C, dtype=torch.float64, device=dev).scatter_add_(0, flat, src))
    inside = crop(torch.zeros(N * PH * PW * C, dtype=torch.float64, device=dev).scatter_add_(0, flat, torch.ones_like(d)))
    assert float(inside.sum()) == d.numel(), "a winner points into the padding"
    return acc(d), acc(d.abs()), inside.to(torch.int64)


# ------------------------------------------------------------------ frames, S8 conversion, residual add
def frames_to_x(frames, ids, h, w, stack, cin_p=8):
    """uint8 frames [n_frames][h * w] through an id table [n][stack] (-1: the zero frame) -> float32 [n][h][w][cin_p] =
    pixel / 255, the IEEE float32 quotient (imp_frames_kernel), channels >= stack zero."""
    frames, ids = torch.as_tensor(frames), torch.as_tensor(ids).to(torch.int64)
    n = ids.shape[0]
    x = torch.zeros(n, h, w, cin_p, dtype=torch.float32, device=frames.device)
    # the 256 quotients are taken on the CPU, where torch divides (on a GPU it multiplies by the reciprocal of a scalar divisor,
    # which is not the IEEE quotient for every pixel value), and looked up on the device of the frames
    lut = (torch.arange(256, dtype=torch.float32) / torch.tensor(255.0, dtype=torch.float32)).to(frames.device)
    px = lut[frames[ids.clamp_min(0).to(frames.device)].reshape(n, stack, h, w).to(torch.int64)]
    px = torch.where((ids >= 0).to(frames.device).reshape(n, stack, 1, 1), px, torch.zeros_like(px))
    x[..., :stack] = px.permute(0, 2, 3, 1)
    return x


def paired_ids(ids, stack):
    """the learn layout's table [B][2 * stack] as rows of the 2B images: states first, then next states"""
    ids = np.asarray(ids)
    return np.concatenate([ids[:, :stack], ids[:, stack : 2 * stack]])


def to_s8_masked(d, mask_hi=None):
    """imp_to_s8_kernel on d [rows][Cp] float32: v = d where the S8 activation's hi half is > 0 (None: everywhere), else 0.
    Returns (v float32, its S8 words, column sums of v in float64, column sums of |v|)."""
    v = torch.as_tensor(d).to(torch.float32)
    if mask_hi is not None:
        v = torch.where(mask_hi > 0, v, torch.zeros_like(v))
    v64 = v.to(torch.float64)
    return v, M.split_words(v), v64.sum(0), v64.abs().sum(0)


def residual_add(a, b):
    """imp_add_kernel: one float32 addition per element"""
    return torch.as_tensor(a).to(torch.float32) + torch.as_tensor(b).to(torch.float32)


# ------------------------------------------------------------------ the cases of tests/test_gpu_impala_backward.py
# The smallest shapes that still force each route (the first two are STAGE_CASES of tests/test_gpu_impala.py).
BACKWARD_CASES = {
    # 84x84: B 42 42 = 7056 rows, the row kernels' grid-stride loop twice
    "tiny-ln-B4": dict(arch="impala", obs=(84, 84, 4), feats=(8, 16, 16, 24), K=2, A=5, B=4, ln=True, bn=False),
    # C_p 16 / 24 / 16, a ragged last 16-row block, H != W
    "nonsquare-44x36x3-noln-B2": dict(arch="impala", obs=(44, 36, 3), feats=(12, 20, 9, 16), K=3, A=4, B=2, ln=False, bn=False),
    # Stacks 1 and 2 (C_p 40, 64) take launch_conv_fwd<64> and launch_conv_dgrad<64>
    "wide-20x20x2-ln-B3": dict(arch="impala", obs=(20, 20, 2), feats=(16, 40, 64, 24), K=2, A=4, B=3, ln=True, bn=False),
    # BatchNorm: the backward runs over the 2B = 4 rows, 4 * 1764 = 7056 rows of Stack 0's blocks: the loop twice
    "bn-84x84x4-noln-B2": dict(arch="impala", obs=(84, 84, 4), feats=(8, 16, 8, 32), K=2, A=3, B=2, ln=False, bn=True),
    # BatchNorm with LayerNorm, padded channels at every site, C = 3 < Cp = 8 at the input site
    "bn-44x36x3-ln-B3": dict(arch="impala", obs=(44, 36, 3), feats=(12, 20, 9, 16), K=3, A=4, B=3, ln=True, bn=True),
}
BACKWARD_RUNS = [(c, "bf16x3") for c in BACKWARD_CASES] + [(c, "bf16") for c in ("tiny-ln-B4", "wide-20x20x2-ln-B3", "bn-44x36x3-ln-B3")]


def conv_routes(geo):
    """Per Stack the template width of its convolutions' launches (csrc/impala.h): imp_conv_fwd takes launch_conv_fwd<32> for
    cout_p <= 32, else <64>; impala_backward's dgrad takes launch_conv_dgrad<32> for cin_p <= 32, else <64>.  Returns per Stack
    dict(fwd0, fwd_block, dgrad0, dgrad_block): Conv_0 maps cin_p -> C_p, the block convolutions C_p -> C_p."""
    bm = lambda p: 32 if p <= 32 else 64
    return [dict(fwd0=bm(g["C_p"]), fwd_block=bm(g["C_p"]), dgrad0=bm(g["cin_p"]), dgrad_block=bm(g["C_p"])) for g in geo]


# ------------------------------------------------------------------ one residual block of impala_backward
# A MODELLED fp32 tensor v (error bound E against the kernel's own fp32 tensor) that a kernel splits into S8 planes and contracts:
# the model contracts split(v).  Where the kernel's planes can differ from the model's at all (model_planes says where), they do
# so by, per element of the modelled operand and relative to the OTHER operand's whole magnitude (|hi| + |lo|):
#   three passes   |(hi + lo) - (hi' + lo')| <= E + U |v| (the model's own rounding to fp32) + 2 S8_STORE |v| (each side's lo half
#                  is rounded); and hi may differ from hi' by a whole bf16 ulp, at most 2^-7 |v| (+ E), which only the product
#                  hi * lo' sees: |lo'| <= 2^-8 |w| (half an ulp at the bottom of a binade), so 2^-15 |v| |w| more.  Together
#                  E + (6 S8_STORE + 2 U) |v|;
#   one pass       hi against hi': E + 2^-7 |v| -- a whole bf16 ulp, further than the two pass counts are apart.  Charged to every
#                  element, that would bury a single-pass chain; model_planes charges it only where hi can flip, which at one
#                  pass is about E / 2^-8 |v| of the elements, so the chain holds in single-pass bf16 as well.
# tests/test_impala_stages_host.py holds both to operands that sit exactly between two bf16 values.
SPLIT_MODEL = {3: 6 * M.S8_STORE + 2 * M.U, 1: 2.0**-7 + 2 * M.U}
DGRAD_EPILOGUE = 4  # launch_conv_dgrad's fp32 operations behind the K chain, as tests/test_gpu_batchnorm.py counts them


def model_planes(v, E, passes, split=M.split):
    """(planes, E_planes) of a modelled operand v whose kernel counterpart lies within E of it.  Rounding is monotone: where
    split(v - E) and split(v + E) are the same planes (the hi plane alone at one pass, which reads nothing else), every fp32 value
    between them splits to those planes too, so the kernel contracts exactly what the model does and that element carries no error
    at all.  Elsewhere the interval crosses a rounding boundary of hi or lo and the element carries E + SPLIT_MODEL |v|.
    `split`: the host test's exact variant passes (v, None) and E through."""
    if split is not M.split:
        return split(v), E
    below, above = split(v - E), split(v + E)
    stable = below[0] == above[0]
    if passes != 1:
        stable = stable & (below[1] == above[1])
    return split(v), torch.where(stable, torch.zeros_like(E), E + SPLIT_MODEL[passes] * v.abs())


def row_chain(rows):
    """fp32 additions one value of a row-wise kernel's column sum goes through (imp_to_s8_kernel's bpart, imp_lnrelu_bwd_kernel's
    lnpart, then adam_kernel's sum of the workgroups' partial rows): a lane's rows in sequence, the 16 row groups of its workgroup,
    the workgroups."""
    blocks, per_lane = row_blocks(rows)
    return per_lane + ROWS_PER_BLOCK + blocks


def dgrad_depth(cout_p):
    """c of launch_conv_dgrad<32 | 64, passes> on a 3x3 / 1 convolution: one accumulator over K = 9 cout_p (net_launch.h: Kc = T T cout_p,
    T = 3), no split-K."""
    return M.chain_depth(9 * cout_p, 1, DGRAD_EPILOGUE)


def wgrad_depth(n_img, npix, cin_p):
    """c of a block convolution's weight gradient on the generic engine (conv_wgrad_slabs), as the Conv_0 row of the forward test"""
    steps, slabs = wgrad_chain(n_img, npix, 9 * cin_p)
    return M.ROUNDING * (M.MFMA_TREE + steps + slabs + 2)


def _abs_planes(p):
    return (p[0].abs() if p[1] is None else p[0].abs() + p[1].abs(), None)


def column_sums(v, E_v, rows):
    """(sum, bound) over every leading axis of v [..., C]: the bias leaf of the convolution whose output gradient v is"""
    C = v.shape[-1]
    flat = lambda t: t.reshape(-1, C)
    return flat(v).sum(0), flat(E_v).sum(0) + M.bound(flat(v).abs().sum(0), M.ROUNDING * row_chain(rows))


def conv_leaves(passes, x, dz, E_dz, c_w, split=M.split):
    """kernel leaf of a 3x3 / 1 SAME convolution from its own input planes x [N][H][W][Cin] and a MODELLED output gradient dz
    [N][H][W][Cout] with bound E_dz: (gw HWIO, E_gw)."""
    N, H, W, C = dz.shape
    dp, E_p = model_planes(dz, E_dz, passes, split)
    flat = lambda p: tuple(None if t is None else t.reshape(N, H * W, C) for t in p)
    gw, S = M.conv_wgrad(passes, x, flat(dp), 3, 1)
    carried, _ = M.conv_wgrad(1, _abs_planes(x), (E_p.reshape(N, H * W, C), None), 3, 1)
    return gw, carried + M.bound(S, c_w)


def conv_data_gradient(passes, dz, E_dz, w, split=M.split):
    """data gradient of a 3x3 / 1 SAME convolution from a MODELLED output gradient dz [N][H][W][Cout] (bound E_dz) and the weights'
    planes w (HWIO): (da [N][H][W][Cin], E_da)."""
    N, H, W, C = dz.shape
    cin = w[0].shape[2]
    dp, E_p = model_planes(dz, E_dz, passes, split)
    flat = lambda p: tuple(None if t is None else t.reshape(N, H * W, C) for t in p)
    da, S = M.conv_dgrad(passes, flat(dp), w, (H, W), 1)
    carried, _ = M.conv_dgrad(1, (E_p.reshape(N, H * W, C), None), _abs_planes(w), (H, W), 1)
    E = carried + M.bound(S, dgrad_depth(-(-C // 8) * 8))
    return da.reshape(N, H, W, cin), E.reshape(N, H, W, cin)


def block_backward(passes, G, E_G, r, mask1, x1, a2, w1, w2, gamma, has_ln, bn=None, split=M.split):
    """Residual block b of impala_backward in the kernel's order, in float64, on true channels:
        stream = Conv_{2+2b}(a2) + r,  a2 = relu(Conv_{1+2b}(x1)),  x1 = [BatchNorm](a1),  a1 = relu([LayerNorm](r)).
    G [N][Hp][Wp][C]: the gradient of the stream above the block (a model) with its bound E_G; r: the block's own fp32 input;
    mask1: its own first ReLU decisions (a1 > 0); x1, a2: the own S8 planes the two convolutions read; w1, w2: the planes of the two
    kernels (HWIO); gamma: LayerNorm scale [C] (has_ln).  bn: dict(x = a1 [N][P][Cp] float64, mean, var, scale [P], s1, s2 = the
    run's own sums or None) -- the block's BatchNorm site between the first convolution's data gradient and the LayerNorm backward.
    Stages, each with its first-order bound (E carried through the contraction with magnitudes + the stage's own bound(S, c)):
        to_s8(G)            -> bias2 = column sums of G;                      planes of G (model_planes)
        wgrad, dgrad of Conv_{2+2b}: gw2 on own a2; da2
        to_s8(da2, a2 > 0)  -> v = da2 [a2 > 0], bias1 = column sums of v;   planes of v
        wgrad, dgrad of Conv_{1+2b}: gw1 on own x1; da1
        bn_backward         -> s1, s2, da1 <- dx (in place in the kernel)
        ln_relu_bwd         -> dz; ln_param_grads -> dgamma, dbeta;  G_out = G + dz (one fp32 addition)
    Returns a dict of every intermediate X with its bound E_X."""
    from tests.helpers import batchnorm_stages as BS

    N, Hp, Wp, C = G.shape
    C_p = -(-C // 8) * 8
    rows = N * Hp * Wp
    c_w = wgrad_depth(N, Hp * Wp, C_p)
    out = dict(G_in=G, E_G_in=E_G)
    out["bias2"], out["E_bias2"] = column_sums(G, E_G, rows)
    out["gw2"], out["E_gw2"] = conv_leaves(passes, a2, G, E_G, c_w, split)
    da2, E_da2 = conv_data_gradient(passes, G, E_G, w2, split)
    mask2 = (a2[0] > 0).to(G.dtype)
    v, E_v = da2 * mask2, E_da2 * mask2
    out.update(da2=da2, E_da2=E_da2, v=v, E_v=E_v, mask2=mask2)
    out["bias1"], out["E_bias1"] = column_sums(v, E_v, rows)
    out["gw1"], out["E_gw1"] = conv_leaves(passes, x1, v, E_v, c_w, split)
    da1, E_da1 = conv_data_gradient(passes, v, E_v, w1, split)
    out.update(da1=da1, E_da1=E_da1)
    if bn is not None:
        pad = lambda t: BS._pad_channels(t.reshape(N, Hp * Wp, C), C_p)
        dy, E_dy = pad(da1), pad(E_da1)
        s1, d_s1, s2, d_s2, _, _ = BS.bn_backward(bn["x"], dy, bn["mean"], bn["var"], bn["scale"], True, C, E_dy=E_dy)
        _, _, _, _, dx, d_dx = BS.bn_backward(bn["x"], dy, bn["mean"], bn["var"], bn["scale"], True, C, E_dy=E_dy, s1=bn.get("s1"), s2=bn.get("s2"))
        out.update(s1=s1, E_s1=d_s1, s2=s2, E_s2=d_s2)
        da1, E_da1 = dx[..., :C].reshape(N, Hp, Wp, C), d_dx[..., :C].reshape(N, Hp, Wp, C)
        out.update(dx=da1, E_dx=E_da1)
    mask1 = mask1.to(G.dtype)
    dz, E_dz = M.ln_relu_bwd(r, gamma, mask1, da1, E_da1, has_ln=has_ln)
    out.update(dz=dz, E_dz=E_dz, mask1=mask1)
    if has_ln:
        out["dgamma"], out["E_dgamma"], out["dbeta"], out["E_dbeta"] = M.ln_param_grads(r, mask1, da1, E_da1, row_chain(rows))
    G_out = G + dz
    out.update(G_out=G_out, E_G_out=E_G + E_dz + M.ROUNDING * M.U * G_out.abs())
    return out


# ------------------------------------------------------------------ structured frames (flat backgrounds, rectangles)
PALETTE = (0, 28, 74, 142, 200, 255)


def flat_frame_batch(B, n_actions, seed=0, h=44, w=44, stack=3, n_frames=None):
    """A replay batch in make_frame_batch's form whose frames look like Atari's: each single frame is one background value plus
    two or three axis-aligned constant rectangles (3 .. 8 pixels a side) from a small palette; sample 0's state is all zero frames
    (the padding in front of an episode).  Most 3x3 pool windows of the first convolution's output are then ties of bit-equal
    values."""
    from oracle.replay_buffer import ReplayElement

    rng = np.random.default_rng(seed)
    n_frames = n_frames or (2 * B + 4)
    frames = np.empty((n_frames, h, w), np.uint8)
    for f in frames:
        f[:] = rng.choice(PALETTE)
        for _ in range(int(rng.integers(2, 4))):
            rh, rw = (int(v) for v in rng.integers(3, 9, 2))
            y, x = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
            f[y : y + rh, x : x + rw] = rng.choice(PALETTE)
    frames = frames.reshape(n_frames, h * w)
    ids = rng.integers(0, n_frames, size=(B, 2 * stack)).astype(np.int32)
    ids[rng.random(ids.shape) < 0.1] = -1
    ids[0, :stack] = -1
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


def constant_neighbourhoods(images, pad):
    """[n][Hp][Wp] bool over the pool windows of the first Stack: the window's 3x3 positions lie inside the image with their own
    3x3 receptive fields, and that 5x5 neighbourhood of `images` [n][h][w][c] is constant in every channel.  The nine
    pre-pool values of such a window come from identical operands: a nine-way tie."""
    x = np.asarray(images).astype(np.int64)
    n, h, w, _ = x.shape
    Hp, Wp = _ceil(h, 2), _ceil(w, 2)
    out = np.zeros((n, Hp, Wp), bool)
    for oy in range(Hp):
        y0 = 2 * oy - pad - 1
        if y0 < 0 or y0 + 5 > h:
            continue
        for ox in range(Wp):
            x0 = 2 * ox - pad - 1
            if x0 < 0 or x0 + 5 > w:
                continue
            blk = x[:, y0 : y0 + 5, x0 : x0 + 5, :]
            out[:, oy, ox] = (blk == blk[:, :1, :1, :]).all(axis=(1, 2, 3))
    return out
