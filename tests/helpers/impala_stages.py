"""Plain restatements of what csrc/impala.h does BETWEEN the convolutions of the impala torso, and of the plan's geometry
(csrc/net_plan.h): the frame decode, the 3x3 / 2 SAME max-pool with its winners and its backward, the ReLU-mask + S8 conversion
with its column sums, the residual add.  torch on the device of the inputs (float64 wherever a sum is taken), like bf16_model.py:
nothing here needs a GPU, tests/test_impala_stages_host.py checks every function against torch / the oracle on the CPU, and the GPU
test (tests/test_gpu_impala.py) runs them on the HIP run's own tensors.

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
