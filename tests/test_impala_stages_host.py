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


# ---------------------------------------------------------------------------------------------------------------------------------
# The backward side (tests/test_gpu_impala_backward.py): block_backward against autograd, its bounds, the routes of the cases.
def _exact(t):
    return (t, None)


def _autograd_torso(ln, bn, seed=4, N=3, obs=(12, 12, 2), feats=(5, 6, 4)):
    """oracle/network.py's three Stacks in float64 under autograd on random inputs (training-mode BatchNorm on the batch statistics),
    with everything block_backward needs recorded: per Stack its input, per block r, a1, the first convolution's input x1, a2."""
    from tests.gpu_helpers import perturbed_params

    params = perturbed_params(seed, obs, list(feats) + [7], "impala", 4, ln, scale=0.3, batch_norm=bn)
    P = onet.to_torch(params, torch.float64, requires_grad=True)
    rng = np.random.default_rng(seed + 1)
    x = torch.from_numpy(rng.uniform(0, 1, size=(N,) + obs)).requires_grad_(True)
    cap, rec = {}, {}

    def inner(t, name):
        mean = t.mean(dim=(0, 3))
        var = torch.clamp((t * t).mean(dim=(0, 3)) - mean * mean, min=0.0)
        y = onet._batch_norm(t, P[name], None, False, True, None, name)
        rec[name] = dict(x=t.detach(), out=y.detach(), mean=mean.detach().reshape(-1), var=var.detach().reshape(-1))
        return y

    h = x
    for s in range(3):
        rec[f"in{s}"] = h.detach()
        h = onet._impala_stack(P, f"Stack_{s}", h, ln, cap, bn=inner if bn else None)
    cot = torch.from_numpy(rng.normal(size=tuple(h.shape)))
    (h * cot).sum().backward()
    return params, P, x, cap, rec, cot


def _chain(params, P, cap, rec, cot, ln, bn, passes, split, E_rel=0.0, feats=(5, 6, 4), obs=(12, 12, 2)):
    """the three Stacks' backward from block_backward, pool_bwd and bf16_model's contractions: {leaf: (value, bound)} and the input gradient"""
    from tests.helpers import batchnorm_stages as BS

    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    planes = lambda a: split(a) if split is not _exact else _exact(a)
    geo = IS.geometry(obs, feats)
    G, E = cot, E_rel * cot.abs()
    leaves, blocks = {}, []
    for s in (2, 1, 0):
        g = geo[s]
        C, C_p = g["C"], g["C_p"]
        for b in (1, 0):
            pre = f"Stack_{s}"
            r, a1, a2 = (cap[f"{pre}/{k}{b}"].detach() for k in ("r", "a1_", "a2_"))
            site = None
            x1 = a1
            if bn:
                q = rec[f"{pre}/BatchNorm_{b}"]
                x1 = q["out"]
                site = dict(x=BS._pad_channels(a1.reshape(a1.shape[0], -1, C), C_p), mean=q["mean"], var=q["var"],
                            scale=t64(params[f"{pre}/BatchNorm_{b}"]["scale"]).reshape(-1))
            res = IS.block_backward(passes, G, E, r, a1 > 0, planes(x1), planes(a2), planes(t64(params[f"{pre}/Conv_{1 + 2 * b}"]["kernel"])),
                                    planes(t64(params[f"{pre}/Conv_{2 + 2 * b}"]["kernel"])), t64(params[f"{pre}/LayerNorm_{b}"]["scale"]) if ln else None,
                                    ln, bn=site, split=split)
            blocks.append(res)
            leaves[f"{pre}/Conv_{2 + 2 * b}"] = dict(kernel=(res["gw2"], res["E_gw2"]), bias=(res["bias2"], res["E_bias2"]))
            leaves[f"{pre}/Conv_{1 + 2 * b}"] = dict(kernel=(res["gw1"], res["E_gw1"]), bias=(res["bias1"], res["E_bias1"]))
            if ln:
                leaves[f"{pre}/LayerNorm_{b}"] = dict(scale=(res["dgamma"], res["E_dgamma"]), bias=(res["dbeta"], res["E_dbeta"]))
            if bn:
                shape = (g["Hp"], g["Wp"])
                leaves[f"{pre}/BatchNorm_{b}"] = dict(scale=(res["s2"].reshape(shape), res["E_s2"].reshape(shape)),
                                                      bias=(res["s1"].reshape(shape), res["E_s1"].reshape(shape)))
            G, E = res["G_out"], res["E_G_out"]
        x_in = rec[f"in{s}"]
        W0 = t64(params[f"Stack_{s}/Conv_0"]["kernel"])
        z0 = onet._conv_same(x_in, W0, t64(params[f"Stack_{s}/Conv_0"]["bias"]), 1)
        _, arg = IS.pool_fwd(z0, g["pad"])
        dz0, _, _ = IS.pool_bwd(G, arg, g["H"], g["W"], g["pad"])
        N = dz0.shape[0]
        gw, _ = M.conv_wgrad(1, _exact(x_in), _exact(dz0.reshape(N, -1, C)), 3, 1)
        leaves[f"Stack_{s}/Conv_0"] = dict(kernel=(gw, torch.zeros_like(gw)), bias=(dz0.reshape(-1, C).sum(0), torch.zeros(C, dtype=torch.float64)))
        G, _ = M.conv_dgrad(1, _exact(dz0.reshape(N, -1, C)), _exact(W0), (g["H"], g["W"]), 1)
        G = G.reshape(N, g["H"], g["W"], g["cin"])
        E = torch.zeros_like(G)
    return leaves, G, blocks


@pytest.mark.parametrize("ln,bn", [(True, False), (False, False), (True, True), (False, True)], ids=["ln", "noln", "ln-bn", "noln-bn"])
def test_block_backward_chained_over_three_stacks_equals_autograd(ln, bn):
    """Every leaf of the three Stacks and the gradient of the torso's input, from block_backward on exact operands (one exact pass,
    no split) with the masks and pool winners of the float64 forward, against torch autograd through oracle.network._impala_stack."""
    params, P, x, cap, rec, cot = _autograd_torso(ln, bn)
    leaves, G, blocks = _chain(params, P, cap, rec, cot, ln, bn, 1, _exact)
    n_leaves = 0
    for mod, d in leaves.items():
        for leaf, (got, _) in d.items():
            want = P[mod][leaf].grad
            assert float(want.abs().max()) > 0, (mod, leaf)
            assert torch.allclose(got, want, rtol=1e-9, atol=1e-11 * float(want.abs().max())), (mod, leaf, float((got - want).abs().max()))
            n_leaves += 1
    assert n_leaves == 3 * (10 + (4 if ln else 0) + (4 if bn else 0))
    assert torch.allclose(G, x.grad, rtol=1e-9, atol=1e-11 * float(x.grad.abs().max()))
    assert set(leaves) == {m for m in P if m.startswith("Stack_")}


@pytest.mark.parametrize("ln,bn", [(True, False), (False, False), (True, True), (False, True)], ids=["ln", "noln", "ln-bn", "noln-bn"])
def test_block_backward_bounds_are_never_negative_and_zero_where_a_mask_blocks(ln, bn):
    """On split operands at three passes and at one, with a bound on the top gradient carried in: every bound of every stage is >= 0
    and finite; where the second ReLU blocks, v and its bound are exactly 0; without LayerNorm so are dz and its bound where the
    first ReLU blocks; a larger bound above gives a bound at least as large at every stage; and the value chain stays within a few
    2^-16 (three passes) / 2^-7 (one pass) of the exact one, so the bound's own inputs are the right tensors."""
    params, P, x, cap, rec, cot = _autograd_torso(ln, bn, seed=9)
    exact, G_exact, _ = _chain(params, P, cap, rec, cot, ln, bn, 1, _exact)
    for passes, tol in ((3, 2.0**-13), (1, 2.0**-4)):
        small, G_s, blocks_s = _chain(params, P, cap, rec, cot, ln, bn, passes, M.split, E_rel=1e-7)
        large, _, blocks_l = _chain(params, P, cap, rec, cot, ln, bn, passes, M.split, E_rel=1e-5)
        n_blocked = [0, 0]
        for res, res_l in zip(blocks_s, blocks_l):
            for k, v in res.items():
                if k.startswith("E_"):
                    assert bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0, k
                    assert bool((res_l[k] >= v).all()), k
            a2_blocks = res["mask2"] == 0
            assert float(res["v"][a2_blocks].abs().max()) == 0.0 and float(res["E_v"][a2_blocks].max()) == 0.0 and float(res["E_v"][~a2_blocks].min()) > 0.0
            n_blocked[0] += int(a2_blocks.sum())
            if not ln:
                blocked = res["mask1"] == 0
                n_blocked[1] += int(blocked.sum())
                if bool(blocked.any()):
                    assert float(res["dz"][blocked].abs().max()) == 0.0 and float(res["E_dz"][blocked].max()) == 0.0
                assert float(res["E_dz"][~blocked].min()) > 0.0
            assert bool((res["E_G_out"] >= res["E_G_in"]).all())
        assert n_blocked[0] > 0 and (ln or n_blocked[1] > 0)
        for mod, d in small.items():
            for leaf, (got, E) in d.items():
                want = exact[mod][leaf][0]
                assert float((got - want).abs().max()) <= tol * float(want.abs().max()), (passes, mod, leaf)
                assert float(E.min()) >= 0.0


def test_split_model_covers_the_planes_of_a_perturbed_operand():
    """SPLIT_MODEL: the planes of v and of v + e, |e| <= E, contracted with a weight's planes at `passes`, differ by at most
    (E + SPLIT_MODEL |v|) (|w_hi| + |w_lo|) per product -- on values that sit at bf16 rounding boundaries, where hi flips."""
    rng = np.random.default_rng(3)
    v = torch.from_numpy(rng.normal(size=4096))
    hi, _ = M.split(v)
    ulp = torch.exp2(torch.floor(torch.log2(hi.abs())) - 7)
    v = torch.cat([v, (hi + ulp / 2).float().double()])  # the second half: exactly between two bf16 values
    w = torch.from_numpy(rng.normal(size=v.shape))
    wp = M.split(w)
    for E_rel in (1e-7, 1e-5):
        E = E_rel * v.abs()
        for sign in (-1.0, 1.0):
            for passes in (3, 1):
                a = M.contract(torch.mul, passes, M.split(v), wp)[0]
                b = M.contract(torch.mul, passes, M.split(v + sign * E), wp)[0]
                _, Ep = IS.model_planes(v, E, passes)
                assert bool(((a - b).abs() <= Ep * (wp[0].abs() + wp[1].abs())).all()), (E_rel, sign, passes)
                # where model_planes charges nothing the products are the same bits; the values between two bf16 values are charged
                # (but for the few whose hi is a power of two, where the spacing towards zero halves and hi + ulp / 2 is no tie)
                assert bool((a[Ep == 0] == b[Ep == 0]).all()) and float((Ep[4096:] > 0).double().mean()) > 0.95
                if E_rel == 1e-7:  # random values: almost none within 1e-7 of a rounding boundary of hi (2^-8) or lo (2^-16)
                    assert float((Ep[:4096] == 0).double().mean()) > (0.9 if passes == 3 else 0.999)
    assert IS.SPLIT_MODEL[1] > 2.0**-9  # one pass: as far as the two pass counts are apart


@pytest.fixture(scope="module")
def backward_plans(tmp_path_factory):
    """{case: plan_dump's body} of the real plan of every case of the backward test, as the case runs (BatchNorm or not)"""
    import os

    from tests.helpers import plan_grid as pg

    exe = str(tmp_path_factory.mktemp("impala_backward") / "plan_dump")
    assert pg.compile_dumper(os.path.join(pg.ROOT, "is-dqn_amd", "csrc"), exe).wait() == 0
    cfgs = []
    for c in IS.BACKWARD_CASES.values():
        h, w, stack = c["obs"]
        cfgs.append(dict(pg.BASE_IMPALA, obs_h=h, obs_w=w, obs_c=stack, features=c["feats"], n_actions=c["A"], n_heads=1 + c["K"], layer_norm=int(c["ln"]),
                         batch_size=c["B"], batch_norm=int(c["bn"])))
    out = {}
    for case, (rc, body) in zip(IS.BACKWARD_CASES, pg.run_dumper(exe, cfgs)):
        assert rc == 0, f"{case}: refused: {body.strip()}"
        out[case] = body
    return out


@pytest.mark.parametrize("case", list(IS.BACKWARD_CASES))
def test_backward_cases_are_accepted_and_take_the_routes_they_exist_for(backward_plans, case):
    """The plan accepts every case; its Stacks' geometry is impala_stages.geometry; the widths that pick the launch templates
    (csrc/impala.h: cout_p <= 32 forward, cin_p <= 32 data gradient) are what conv_routes restates; the weight gradients' slabs are
    wgrad_chain's; Bb is B without BatchNorm and 2B with it."""
    cfg = IS.BACKWARD_CASES[case]
    fields = lambda l: {k: v for k, v in (t.split("=", 1) for t in l.split()[1:])}
    lines = backward_plans[case].splitlines()
    top = fields(next(l for l in lines if l.startswith("P ")))
    Bb = 2 * cfg["B"] if cfg["bn"] else cfg["B"]
    assert int(top["B"]) == cfg["B"] and int(top["Bb"]) == Bb and int(top["bn"]) == int(cfg["bn"])
    geo = IS.geometry(cfg["obs"], cfg["feats"])
    routes = IS.conv_routes(geo)
    for s, g in enumerate(geo):
        S = fields(next(l for l in lines if l.startswith(f"imp[{s}] ")))
        assert {k: int(S[k]) for k in ("H", "W", "Hp", "Wp", "cin", "cin_p", "C", "C_p")} == {k: g[k] for k in ("H", "W", "Hp", "Wp", "cin", "cin_p", "C", "C_p")}
        assert int(S["pool_pad"]) == g["pad"]
        for k in range(5):
            L = fields(next(l for l in lines if l.startswith(f"imp[{s}].conv[{k}] ")))
            cin_p, npix = (g["cin_p"], g["H"] * g["W"]) if k == 0 else (g["C_p"], g["Hp"] * g["Wp"])
            assert (int(L["cin_p"]), int(L["cout_p"]), int(L["npix"]), int(L["ksz"]), int(L["stride"])) == (cin_p, g["C_p"], npix, 3, 1)
            assert (32 if int(L["cout_p"]) <= 32 else 64) == (routes[s]["fwd0"] if k == 0 else routes[s]["fwd_block"])
            assert (32 if int(L["cin_p"]) <= 32 else 64) == (routes[s]["dgrad0"] if k == 0 else routes[s]["dgrad_block"])
            steps, slabs = IS.wgrad_chain(Bb, npix, 9 * cin_p)
            assert slabs <= int(L["gw_slabs"]) and steps * slabs >= -(-Bb * npix // 32) > steps * (slabs - 1)
    bns = [fields(l) for l in lines if l.startswith("bns[")]
    assert len(bns) == (9 if cfg["bn"] else 0)
    if cfg["bn"]:
        from tests.helpers import batchnorm_stages as BS

        regions = {t.split("=")[0]: int(t.split("=")[1].split("+")[0]) for l in lines if l.startswith("regions") for t in l.split()[1:]}
        for got, s in zip(bns, BS.site_layout(cfg)):
            assert got["name"] == s["name"] and int(got["layer"]) == s["layer"] and bool(int(got["spatial"])) == s["spatial"]
            assert (int(got["P"]), int(got["C"]), int(got["Cp"]), int(got["G"])) == (s["P"], s["C"], s["Cp"], s["G"])
            assert 4 * int(got["in_off"]) == regions[s["src"]] and 4 * int(got["out_off"]) == regions[s["prefix"] + "out"]  # floats / bytes
    # what each case is meant to force
    if case == "wide-20x20x2-ln-B3":
        assert [g["C_p"] for g in geo] == [16, 40, 64]
        assert routes[0] == dict(fwd0=32, fwd_block=32, dgrad0=32, dgrad_block=32)
        assert routes[1] == dict(fwd0=64, fwd_block=64, dgrad0=32, dgrad_block=64)  # Stack_1/Conv_0's data gradient reads 16 channels
        assert routes[2] == dict(fwd0=64, fwd_block=64, dgrad0=64, dgrad_block=64)
    else:
        assert all(v == 32 for r in routes for v in r.values())
    if case == "tiny-ln-B4":
        assert IS.row_blocks(Bb * 42 * 42) == (256, 2) and IS.row_chain(Bb * 42 * 42) == 2 + 16 + 256
    if case == "bn-84x84x4-noln-B2":
        assert Bb * 42 * 42 == 7056 and IS.row_blocks(Bb * 42 * 42) == (256, 2)
    if case == "nonsquare-44x36x3-noln-B2":
        assert (Bb * 6 * 5) % 16 != 0
