"""tests/helpers/impala_stages.py against things that are not the code under test, no GPU: torch's max_pool2d and its autograd, the
oracle's restatement of the torso (oracle/network.py), the plan's own region sizes (isdqn_net_workspace_region builds the plan on
the host), and the plan's refusal of observations whose two sides need different pool padding.  The device side is
tests/test_gpu_impala.py: test_impala_stages_match_a_model_of_each_kernel_on_its_own_operands."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.helpers import bf16_model as M
from tests.helpers import impala_stages as IS

SIZES = [(84, 84), (42, 42), (21, 21), (11, 11), (44, 44), (9, 9), (8, 8), (22, 18)]


def _inputs(h, w, seed):
    """random, all-equal and piecewise-constant [2][h][w][5] float32 tensors"""
    rng = np.random.default_rng(seed)
    rnd = rng.normal(size=(2, h, w, 5)).astype(np.float32)
    flat = np.full((2, h, w, 5), -0.75, np.float32)
    pc = np.repeat(np.repeat(rng.normal(size=(2, -(-h // 4), -(-w // 3), 5)), 4, axis=1), 3, axis=2)[:, :h, :w].astype(np.float32)
    return {"random": torch.from_numpy(rnd), "all-equal": torch.from_numpy(flat), "piecewise-constant": torch.from_numpy(pc.copy())}


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool_forward_and_backward_against_torch(hw):
    h, w = hw
    (hp, pad), (wp, pad_w) = IS.pool_same(h), IS.pool_same(w)
    assert pad == pad_w
    for kind, z in _inputs(h, w, seed=h * 100 + w).items():
        want = onet._max_pool_same(z)
        val, arg = IS.pool_fwd(z, pad)
        assert val.dtype == z.dtype and tuple(val.shape) == (2, hp, wp, 5)
        assert torch.equal(val, want), kind  # bit for bit
        # the winner holds the maximum, lies inside the image, and no earlier window position holds it too
        iy = 2 * torch.arange(hp).reshape(1, hp, 1, 1) - pad + arg // 3
        ix = 2 * torch.arange(wp).reshape(1, 1, wp, 1) - pad + arg % 3
        assert int(iy.min()) >= 0 and int(iy.max()) < h and int(ix.min()) >= 0 and int(ix.max()) < w
        n, c = torch.arange(2).reshape(2, 1, 1, 1), torch.arange(5).reshape(1, 1, 1, 5)
        assert torch.equal(z[n, iy, ix, c], val)
        if kind == "all-equal":  # the first in-bounds position: 0 away from the padding, 4 = (1, 1) in the padded corner
            assert int(arg[0, 0, 0, 0]) == (4 if pad else 0) and int(arg[0, 1, 1, 0]) == 0
        ties = IS.pool_ties(z, pad)
        assert (int(ties.min()) >= 1) and (kind == "random" or float((ties >= 2).double().mean()) > 0.5)
        # backward: torch autograd through max_pool2d on the -inf-padded input
        zz = z.double().requires_grad_(True)
        dp = torch.from_numpy(np.random.default_rng(1).normal(size=(2, hp, wp, 5)))
        (onet._max_pool_same(zz) * dp).sum().backward()
        dz, S, cnt = IS.pool_bwd(dp, arg, h, w, pad)
        assert torch.equal(dz, zz.grad) or float((dz - zz.grad).abs().max()) <= 4 * 2.0**-52 * float(S.max()), kind
        assert int(cnt.max()) <= 4 and int(cnt.sum()) == dp.numel()
        assert torch.equal(S == 0, cnt == 0)
        assert float(dz[cnt == 0].abs().max() if bool((cnt == 0).any()) else 0.0) == 0.0


def test_torch_breaks_pool_ties_towards_the_first_position():
    """6x6 all-zero input: every window is a tie.  torch's CPU max_pool2d sends each window's gradient to its first in-bounds
    position in row-major order -- rows / columns 0, 2, 4 of the input (pad_lo = 0: window oy starts at row 2 oy) -- and so does
    pool_fwd."""
    z = torch.zeros(1, 6, 6, 1, dtype=torch.float64, requires_grad=True)
    onet._max_pool_same(z).sum().backward()
    want = torch.zeros(6, 6, dtype=torch.float64)
    want[0::2, 0::2] = 1.0
    assert torch.equal(z.grad[0, :, :, 0], want)
    val, arg = IS.pool_fwd(z.detach(), 0)
    assert int(arg.abs().max()) == 0
    dz, _, cnt = IS.pool_bwd(torch.ones(1, 3, 3, 1, dtype=torch.float64), arg, 6, 6, 0)
    assert torch.equal(dz[0, :, :, 0], want) and torch.equal(cnt[0, :, :, 0].double(), want)


def test_frames_to_x_is_the_oracle_input_rounded_to_float32():
    from tests.gpu_helpers import make_frame_batch

    frames, ids, _, _, _, ref = make_frame_batch(3, 4, seed=5, h=12, w=10, stack=3, zero_frac=0.3)
    x = IS.frames_to_x(torch.from_numpy(frames), IS.paired_ids(ids, 3), 12, 10, 3)
    assert x.dtype == torch.float32 and tuple(x.shape) == (6, 12, 10, 8)
    state = np.concatenate([ref.state, ref.next_state])
    want = (torch.from_numpy(state).to(torch.float64) / 255.0).to(torch.float32)  # oracle/network.py forward: x / 255
    assert torch.equal(x[..., :3], want) and float(x[..., 3:].abs().max()) == 0.0
    assert (ids == -1).any()
    # every uint8 / 255 in float32 is the correctly rounded quotient: the float32 division is what the float64 one rounds to
    v = torch.arange(256, dtype=torch.float32)
    assert torch.equal(v / torch.tensor(255.0), (v.double() / 255.0).float())


def test_masked_s8_conversion_and_the_residual_add():
    rng = np.random.default_rng(2)
    d = torch.from_numpy(rng.normal(size=(37, 16)).astype(np.float32))
    act = torch.from_numpy(np.maximum(rng.normal(size=(37, 16)), 0).astype(np.float32))
    hi, _ = M.split(act)
    v, words, cs, ca = IS.to_s8_masked(d, hi)
    want = torch.where(act > 0, d, torch.zeros_like(d))  # a select, as in the kernel: a blocked element is +0, never -0
    assert torch.equal(v, want) and torch.equal(words, M.split_words(want)) and not bool(torch.signbit(v[act <= 0]).any())
    assert np.allclose(cs.numpy(), (d.double() * (act > 0)).sum(0).numpy(), rtol=0, atol=1e-12) and bool((ca >= cs.abs()).all())
    v2, words2, _, _ = IS.to_s8_masked(d)
    assert torch.equal(v2, d) and torch.equal(words2, M.split_words(d))
    a, b = d, torch.from_numpy(rng.normal(size=(37, 16)).astype(np.float32))
    assert torch.equal(IS.residual_add(a, b), (a.double() + b.double()).float())  # one rounding of the exact sum


def _cfg(obs, feats, B=4, ln=True):
    from slimdqn import _hip

    cfg = _hip.NetConfig()
    cfg.arch = _hip.ARCH_IMPALA
    cfg.obs_h, cfg.obs_w, cfg.obs_c = obs
    cfg.n_features = len(feats)
    for i, f in enumerate(feats):
        cfg.features[i] = int(f)
    cfg.n_actions, cfg.n_heads, cfg.layer_norm, cfg.batch_size = 4, 3, int(ln), B
    return cfg


def _region_floats(cfg, name):
    from slimdqn import _hip

    off, size = ctypes.c_int64(), ctypes.c_int64()
    _hip.check(_hip.lib().isdqn_net_workspace_region(ctypes.byref(cfg), name.encode(), ctypes.byref(off), ctypes.byref(size)))
    return size.value // 4


@pytest.mark.parametrize("obs,feats,B", [((84, 84, 4), (8, 16, 16, 24), 4), ((44, 36, 3), (12, 20, 9, 16), 2), ((44, 44, 3), (8, 16, 16, 24), 3)])
def test_geometry_table_matches_the_plans_regions(obs, feats, B):
    cfg = _cfg(obs, feats, B)
    up = lambda n: -(-n // 64) * 64  # regions are sized in 256-byte granules
    geo = IS.geometry(obs, feats)
    assert geo is not None
    for s, g in enumerate(geo):
        assert g["cin_p"] == 8 if s == 0 else g["cin_p"] == geo[s - 1]["C_p"]
        assert _region_floats(cfg, f"imp/s{s}/xin") == up(2 * B * g["H"] * g["W"] * g["cin_p"])
        assert _region_floats(cfg, f"imp/s{s}/z0") == up(2 * B * g["H"] * g["W"] * g["C_p"])
        assert _region_floats(cfg, f"imp/s{s}/r0") == up(2 * B * g["Hp"] * g["Wp"] * g["C_p"])
        assert _region_floats(cfg, f"imp/s{s}/argmax") == up((2 * B * g["Hp"] * g["Wp"] * g["C_p"] + 3) // 4)
        assert _region_floats(cfg, f"imp/s{s}/dz0") == up(B * g["H"] * g["W"] * g["C_p"])
        # the weight-gradient slabs of Conv_0 and of a block convolution
        for k, (npix, cin_p) in ((0, (g["H"] * g["W"], g["cin_p"])), (3, (g["Hp"] * g["Wp"], g["C_p"]))):
            steps, slabs = IS.wgrad_chain(B, npix, 9 * cin_p)
            plan_slabs = max(1, min(256 // -(-9 * cin_p // 64), -(-B * npix // 32)))  # gw_slabs: the region holds that many
            assert _region_floats(cfg, f"imp/s{s}/gw{k}") == up(plan_slabs * g["C_p"] * 9 * cin_p)
            assert slabs <= plan_slabs and steps * slabs >= -(-B * npix // 32) > steps * (slabs - 1)
    # pool paddings the cases of the GPU test are meant to reach
    if obs == (84, 84, 4):
        assert [g["pad"] for g in geo] == [0, 0, 1] and [(g["Hp"], g["Wp"]) for g in geo] == [(42, 42), (21, 21), (11, 11)]
        assert IS.row_blocks(2 * B * 42 * 42) == (256, 4) and IS.row_blocks(B * 42 * 42) == (256, 2)  # the grid-stride loop runs twice
    if obs == (44, 36, 3):
        assert [(g["Hp"], g["Wp"]) for g in geo] == [(22, 18), (11, 9), (6, 5)] and [g["C_p"] for g in geo] == [16, 24, 16]
        assert (B * 6 * 5) % 16 != 0  # a ragged last 16-row block


def test_plan_refuses_sides_that_need_different_pool_padding():
    from slimdqn import _hip

    n, cnt = ctypes.c_int64(), ctypes.c_int32()
    bad = _cfg((44, 42, 3), (12, 20, 9, 16), 2)  # Stack_1 pools 22 (total padding 1: lo 0) and 21 (total 2: lo 1)
    assert IS.geometry((44, 42, 3), (12, 20, 9, 16)) is None
    assert _hip.lib().isdqn_net_param_layout(ctypes.byref(bad), ctypes.byref(n), None, 0, ctypes.byref(cnt)) == _hip.ERR_UNSUPPORTED
    assert "non-square" in _hip.last_error()
    wb = ctypes.c_int64()
    assert _hip.lib().isdqn_net_workspace_bytes(ctypes.byref(bad), ctypes.byref(wb)) == _hip.ERR_UNSUPPORTED
    ok = _cfg((44, 36, 3), (12, 20, 9, 16), 2)
    assert _hip.lib().isdqn_net_param_layout(ctypes.byref(ok), ctypes.byref(n), None, 0, ctypes.byref(cnt)) == 0 and n.value > 0
    assert _hip.lib().isdqn_net_workspace_bytes(ctypes.byref(ok), ctypes.byref(wb)) == 0 and wb.value > 0


def test_structured_frames_are_mostly_ties():
    """Case C of the GPU test, from the frames alone: at least half of the first Stack's pool windows see a 5x5 input neighbourhood
    that is constant in every channel (so their nine pre-pool values are bit-equal), one state is the all-zero image, and the
    frames are what the docstring says: a background and a few rectangles, i.e. few distinct values."""
    B, stack, h, w = 3, 3, 44, 44
    frames, ids, _, _, _, ref = IS.flat_frame_batch(B, 5, seed=11, h=h, w=w, stack=stack)
    assert frames.dtype == np.uint8 and frames.shape[1] == h * w
    assert all(len(np.unique(f)) <= 4 for f in frames) and any(len(np.unique(f)) >= 2 for f in frames)
    assert (ids[0, :stack] == -1).all() and int(ref.state[0].max()) == 0 and int(ref.state[1:].max()) > 0
    imgs = np.concatenate([ref.state, ref.next_state])
    const = IS.constant_neighbourhoods(imgs, IS.pool_same(h)[1])
    assert const.shape == (2 * B, 22, 22)
    assert const.mean() >= 0.5, const.mean()
    assert const[0].sum() == 20 * 20  # the all-zero image: every window whose neighbourhood lies inside the image
    # and the pool of a convolution of such an image really ties there: float64 conv of image 1 with random weights
    rng = np.random.default_rng(0)
    k = torch.from_numpy(rng.normal(size=(3, 3, stack, 4)))
    z = onet._conv_same(torch.from_numpy(imgs[1:2]).double() / 255.0, k, torch.zeros(4, dtype=torch.float64), 1)
    ties = IS.pool_ties(z, 0)
    assert bool((ties[0][torch.from_numpy(const[1])] == 9).all())
