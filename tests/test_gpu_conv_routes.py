"""The cnn torso layer by layer at the frame sizes, stack depths and conv widths that select other kernels than the Atari frame does
(tests/helpers/conv_routes.py: the cases and the route each convolution takes, pinned on the host by tests/test_conv_routes_host.py).

Same method as tests/test_gpu_bf16_model.py: one run per (case, precision) -- loss_on_batch, a 2B-row forward, learn_on_batch with
grad_out -- then every stored tensor of every convolution against the float64 model of the one contraction that produced it, on the
run's own operands, within c 2^-24 S (bf16_model.chain_depth).  No new constant: a two-K-group forward sums its K steps in two
chains of half the length and adds them once (conv_img.h conv_fwd_img_kernel, KG == 2: K / 64 + 1 <= K / 32 steps), the generic
forward runs the same K / 32 steps, and a weight gradient's depth comes from the route that took it (conv_routes.wgrad_route: G
images per accumulator and `groups` slabs on the image kernel, the plan's slabs and their K steps on the generic engine).

The 100x100 run hands the frames over with a pitch of h * w + 5 bytes, the slack filled with 0xFF: a read across the end of a frame
shows in z/Conv_0.  Frame ids keep their -1 entries (zero frames).  No element is left out of any comparison.

At these widths (all multiples of 8) no layer has padded channels; the zero check of the padding is kept for widths that have.
Every case takes the image-resident data gradient (the generic one needs a dz image above 150 KB of LDS: a 160x160 frame), so the
`da` region is not read here."""
import numpy as np
import pytest
import torch

from tests.gpu_helpers import make_frame_batch, perturbed_params
from tests.helpers import bf16_model as M
from tests.helpers import conv_routes as R

pytestmark = pytest.mark.gpu

RUNS = [pytest.param(c, p, id=f"{c}-{p}") for c, p in R.RUNS]
GAMMA = 0.99
BATCH_SEED = 33  # the first seed from 29 up at which every case draws a zero frame (id -1): with six ids the smallest case often has none
_ceil = R._ceil

_CACHE = {}  # one run per (case, precision), kept while this module runs: every test reads the same step


@pytest.fixture(scope="module", autouse=True)
def _release_runs():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _run(case, precision):
    key = (case, precision)
    if key in _CACHE:
        return _CACHE[key]
    from slimdqn._engine import QNetEngine

    cfg = R.CASES[case]
    obs, feats, K, A, B = cfg["obs"], cfg["feats"], cfg["K"], cfg["A"], cfg["B"]
    h, w, stack = obs
    params = perturbed_params(17, obs, list(feats), "cnn", (1 + K) * A, True)
    eng = QNetEngine(obs, A, 1 + K, list(feats), "cnn", True, B, gamma_n=GAMMA, learning_rate=1e-3, adam_eps=1.5e-4, precision=precision)
    eng.import_flax(params)
    frames, ids, action, reward, terminal, ref = make_frame_batch(B, A, seed=BATCH_SEED, h=h, w=w, stack=stack, n_frames=B + 8)
    assert (ids < 0).any(), "the batch has no zero frame"
    pitch = h * w + cfg["slack"]
    table = np.full((frames.shape[0], pitch), 0xFF, np.uint8)
    table[:, : h * w] = frames
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fr = d(table)
    batch = eng.make_batch(frames=fr, frame_stride=pitch, frame_ids=d(ids), action=d(action), reward=d(reward), terminal=d(terminal))
    layers, head_in_p = R.layers(cfg)
    run = dict(cfg=cfg, precision=precision, layers=layers, x=d(np.concatenate([ref.state, ref.next_state])),  # [2B][h][w][stack] uint8
               routes=R.routes(cfg, precision), fields=R.plan_fields(cfg, B))
    eng.loss_on_batch(batch)
    torch.cuda.synchronize()
    run["p0"] = eng.export_flax()
    for L in layers:
        run[f"loss_act/{L['name']}"] = eng.region(f"act/{L['name']}").clone()
    # the forward-only path on the same 2B rows, and on its first n rows: every kernel here works per image
    both = d(np.concatenate([ids[:, :stack], ids[:, stack:]]))
    run["fwd_q"], run["fwd_act"] = {}, {}
    for n in sorted({1, 2, 3, 2 * B - 1, 2 * B}):
        run["fwd_q"][n] = eng.forward(frames=fr, frame_stride=pitch, frame_ids=both[:n].contiguous(), n_rows=n).clone()
        run["fwd_act"][n] = {f"act/{L['name']}": eng.region(f"act/{L['name']}")[: n * L["npix"] * L["cp"]].clone() for L in layers}
    heads = (torch.arange(2 * B, dtype=torch.int32, device="cuda") % K).contiguous()
    run["heads"] = heads
    run["best"] = eng.best_actions(frames=fr, frame_stride=pitch, frame_ids=both, idx_networks=heads).clone()
    g = torch.zeros_like(eng.params)
    losses = eng.learn_on_batch(batch, grad_out=g)
    torch.cuda.synchronize()
    run["losses"] = losses.clone()
    run["g"] = eng.internal_to_flax_grads(g)
    for L in layers:
        for r in ("act", "z", "dz"):
            run[f"{r}/{L['name']}"] = eng.region(f"{r}/{L['name']}").clone()
    del eng
    _CACHE[key] = run
    return run


def _passes(run):
    return (1, 3) if run["precision"] == "bf16" else (3, 1)


def _w(run, mod):
    return M.split(torch.from_numpy(np.asarray(run["p0"][mod]["kernel"])).cuda())


def _vec(run, mod, leaf):
    return torch.from_numpy(np.asarray(run["p0"][mod][leaf], np.float64)).cuda()


def _planes(run, key, L, rows):
    """own S8 tensor `key` of hidden layer L, rows [0, rows), true channels: planes [rows][npix][c]"""
    hi, lo = M.s8_planes(run[key], rows, L["npix"] * L["cp"])
    f = lambda t: t.reshape(rows, L["npix"], L["cp"])[:, :, : L["c"]]
    return f(hi), f(lo)


def _input_planes(run, i, rows, src=None):
    """planes of the input of layer i (i = len(layers): the head) over rows [0, rows): NHWC for a convolution, [rows][in] for a
    dense layer; `src`: the act tensors to read (default: the learn step's)"""
    layers = run["layers"]
    L = layers[i] if i < len(layers) else dict(kind=1)
    if i == 0:
        return run["x"][:rows].to(torch.float64), None  # uint8 pixels: exact
    below = layers[i - 1]
    P = _planes(src or run, f"act/{below['name']}", below, rows)
    if L["kind"] == 0:
        return tuple(p.reshape(rows, below["h"], below["w"], -1) for p in P)
    return tuple(p.reshape(rows, -1) for p in P)


def _forward_model(run, i, rows, passes, src=None):
    """(z, S, c) of hidden layer i (or the head, i = len(layers)) over rows [0, rows); `src`: the act tensors its input is read from"""
    cfg, layers = run["cfg"], run["layers"]
    xin = _input_planes(run, i, rows, src)
    if i == len(layers):  # the head GEMM + dense_post_kernel
        b, w = _vec(run, "Dense_1", "bias"), _w(run, "Dense_1")
        v, S = M.dense(passes, xin, w)
        in_p, nha_p = layers[-1]["cp"], _ceil((1 + cfg["K"]) * cfg["A"], 8) * 8
        return v + b, S + b.abs(), M.chain_depth(in_p, slabs=R.fwd_splits(2 * cfg["B"], nha_p, in_p, False))
    L = layers[i]
    b = _vec(run, L["name"], "bias")
    w = _w(run, L["name"])
    if L["kind"] == 0:
        p = passes if i else min(passes, 2)  # uint8 pixels: 3 passes are 2
        v, S = M.conv(p, xin, w, L["s"])
        c = M.chain_depth(L["K"])
        if i == 0:
            s = float(np.float32(1.0 / 255.0))
            v, S = v * s, S * s
        return v + b, S + b.abs(), c
    v, S = M.dense(passes, xin, w)
    fs = R.fwd_splits(2 * cfg["B"], L["cp"], L["in_p"], False)
    return v + b, S + b.abs(), M.chain_depth(L["in_p"], slabs=fs)


def _z(run, L, rows):
    return run[f"z/{L['name']}"][: rows * L["npix"] * L["cp"]].reshape(rows, L["npix"], L["cp"])[:, :, : L["c"]].double()


def _report(rows):
    print()
    for r in rows:
        print("  " + r)


N_HIDDEN = 4  # the three convolutions and the first Dense layer


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("case,precision", RUNS)
def test_the_run_and_its_routes(case, precision):
    """The step is finite, and every convolution takes the image-resident data gradient (this file reads no `da` region)."""
    run = _run(case, precision)
    assert np.isfinite(run["losses"].cpu().numpy()).all()
    assert all(r["dgrad"] is None or r["dgrad"]["kernel"] == "dgimg" for r in run["routes"])
    _report([f"{L['name']}: " + ", ".join(f"{k} {R.fmt(v)}" for k, v in r.items() if v) for L, r in zip(run["layers"], run["routes"])])


@pytest.mark.parametrize("case,precision", RUNS)
def test_forward_z_against_the_model(case, precision):
    """z/Conv_i (pre-LayerNorm fp32, online rows) of every convolution against its contraction on the layer below's own act (Conv_0:
    the uint8 pixels, scaled by 1 / 255) and the weights' nearest-even split, plus bias; z/Dense_0, which reads every pixel of
    Conv_2's act in the order the multi-tile kernels stored them.  Control: the other pass count (2 <-> 1 on Conv_0)."""
    run = _run(case, precision)
    own, other = _passes(run)
    B = run["cfg"]["B"]
    out = []
    for i, L in enumerate(run["layers"][:N_HIDDEN]):
        want, S, c = _forward_model(run, i, B, own)
        alt, _, _ = _forward_model(run, i, B, other)
        got = _z(run, L, B)
        want, S, alt = (t.reshape(got.shape) for t in (want, S, alt))
        # Dense_0 at these batch sizes is one tile split over up to 338 K slabs (conv_routes.fwd_splits), summed one after the other:
        # the worst case of that chain is looser than the difference the pass count makes, so its control holds in the 2-norm only
        used, ratio, frac = M.check(got, want, M.bound(S, c), S, alt, elementwise_control=L["kind"] == 0, label=f"z/{L['name']}")
        out.append(f"z/{L['name']}: c = {c}, max |d| / bound = {used:.3f}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
    _report(out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_hidden_activations_of_both_halves(case, precision):
    """act/<layer> of the three convolutions and Dense_0, rows [0, 2B): the online half through the float64 LayerNorm / ReLU of the
    layer's own z, the next-state half -- whose pre-activations are not stored -- through the model of the contraction on the layer
    below's own next-state act, carried through the LayerNorm (bf16_model.ln_relu_fwd: relu is 1-Lipschitz, so no element is left
    out).  Control on the next-state half: the other pass count, in the 2-norm.  loss_on_batch and the learn step wrote the same
    act bits for every convolution."""
    run = _run(case, precision)
    own, other = _passes(run)
    B = run["cfg"]["B"]
    out = []
    for i, L in enumerate(run["layers"][:N_HIDDEN]):
        shape = (B, L["npix"], L["c"])
        gamma, beta = (_vec(run, L["ln"], k) for k in ("scale", "bias"))
        hi, lo = _planes(run, f"act/{L['name']}", L, 2 * B)
        got = hi + lo
        z = _z(run, L, B)
        a, E = M.ln_relu_fwd(z, gamma, beta, torch.zeros_like(z))
        used_on, _, _ = M.check(got[:B], a, E, label=f"act/{L['name']} online")
        zm = []
        for p in (own, other):
            v, S, c = _forward_model(run, i, 2 * B, p)
            zm.append((v.reshape(2 * B, *shape[1:])[B:], M.bound(S, c).reshape(2 * B, *shape[1:])[B:]))
        a, E = M.ln_relu_fwd(zm[0][0], gamma, beta, zm[0][1])
        alt, _ = M.ln_relu_fwd(zm[1][0], gamma, beta, zm[1][1])
        used, _, frac = M.check(got[B:], a, E, None, alt, elementwise_control=False, label=f"act/{L['name']} next-state")
        out.append(f"act/{L['name']}: online max |d| / bound = {used_on:.3f}, next-state {used:.3f}, other passes outside: {frac:.0%}")
        if L["kind"] == 0:  # (Dense_0's act rows are rewritten by the learn step's head chain)
            n = 2 * B * L["npix"] * L["cp"]
            assert torch.equal(run[f"act/{L['name']}"][:n].view(torch.int32), run[f"loss_act/{L['name']}"][:n].view(torch.int32)), L["name"]
    _report(out)


def _dz_check(run, i, passes):
    """dz of convolution i (online rows) from the model of the data gradient of convolution i + 1 on its own dz planes, through the
    float64 LayerNorm / ReLU backward on the layer's own z and ReLU decisions (own act > 0)"""
    layers = run["layers"]
    B = run["cfg"]["B"]
    L, U_ = layers[i], layers[i + 1]
    dz = _planes(run, f"dz/{U_['name']}", U_, B)
    da, S = M.conv_dgrad(passes, dz, _w(run, U_["name"]), (L["h"], L["w"]), U_["s"])
    # every tap of every output channel at most (a class-split kernel sums ceil(k / s)^2 of them), then the epilogue
    E_da = M.bound(S, M.chain_depth(U_["k"] ** 2 * U_["cp"], epilogue=4))
    shape = (B, L["npix"], L["c"])
    z = _z(run, L, B)
    hi, lo = _planes(run, f"act/{L['name']}", L, B)
    mask = ((hi + lo) > 0).double()
    dzm, E = M.ln_relu_bwd(z, _vec(run, L["ln"], "scale"), mask, da.reshape(shape), E_da.reshape(shape))
    hi, lo = _planes(run, f"dz/{L['name']}", L, B)
    return hi + lo, dzm, E


@pytest.mark.parametrize("case,precision", RUNS)
def test_backward_dz_against_the_model(case, precision):
    """dz/Conv_1 and dz/Conv_0 under the convolutions' image-resident data gradients (one, two or three tiles per stride class):
    transposed SAME convolutions of the layer above's own dz with the weights' split, then the LayerNorm / ReLU backward.
    Control: the other pass count."""
    run = _run(case, precision)
    own, other = _passes(run)
    out = []
    for i in (1, 0):
        got, want, E = _dz_check(run, i, own)
        alt = _dz_check(run, i, other)[1]
        used, _, frac = M.check(got, want, E, None, alt, label=f"dz/Conv_{i}")
        out.append(f"dz/Conv_{i}: max |d| / bound = {used:.3f}, other passes outside: {frac:.0%}")
    _report(out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_weight_gradients_against_the_model(case, precision):
    """The kernel leaf of every convolution of g against the sum over the online rows of own input activations (Conv_0: pixels) x own
    dz at the pass count, within the chain of the route that took it; every bias against the sum of dz.  The control is asserted
    in the 2-norm (a worst-case chain over B x pixels products is looser than the difference the pass count makes)."""
    run = _run(case, precision)
    own, other = _passes(run)
    B = run["cfg"]["B"]
    out = []
    for i, L in enumerate(run["layers"][:3]):
        mod, route = L["name"], run["routes"][i]["wgrad"]
        dz = _planes(run, f"dz/{mod}", L, B)
        xin = _input_planes(run, i, B)

        def model(p):
            v, S = M.conv_wgrad(min(p, 2) if i == 0 else p, xin, dz, L["k"], L["s"])
            if i == 0:
                s = float(np.float32(1.0 / 255.0))
                v, S = v * s, S * s
            return v, S

        if route["kernel"] == "wgimg":  # G images per accumulator, one slab per group (conv_img.h conv_wgrad_img_kernel)
            steps, slabs = _ceil(route["G"] * L["npix"], 32), route["groups"]
        else:  # the plan's slabs of `steps` K steps each (net_launch.h launch_conv_wgrad)
            steps, slabs = route["steps"], route["slabs"]
        c = M.ROUNDING * (M.MFMA_TREE + steps + slabs + 2)
        want, S = model(own)
        alt, _ = model(other)
        got = torch.from_numpy(np.asarray(run["g"][mod]["kernel"], np.float64)).cuda()
        used, ratio, frac = M.check(got, want, M.bound(S, c), S, alt, elementwise_control=False, label=f"{mod}/kernel")
        out.append(f"{mod}/kernel [{R.fmt(route)}]: c = {c}, max |d| / bound = {used:.3f}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
        # bias: a plain fp32 sum of dz (hi + lo of the S8 value: within S8_STORE of the fp32 one); no pass count, no control
        dzv = (dz[0] + dz[1]).reshape(-1, dz[0].shape[-1])
        bw, bS = dzv.sum(0), dzv.abs().sum(0)
        gb = torch.from_numpy(np.asarray(run["g"][mod]["bias"], np.float64)).cuda()
        usedb, _, _ = M.check(gb, bw, M.bound(bS, M.chain_depth(0, slabs=dzv.shape[0], epilogue=4)) + M.S8_STORE * bS, label=f"{mod}/bias")
        out.append(f"{mod}/bias: max |d| / bound = {usedb:.3f}")
    _report(out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_s8_tensors_are_nearest_even_splits_and_padding_is_zero(case, precision):
    """Every stored activation / dz element of the convolutions is a nearest-even split (|lo| <= half an ulp of hi); channels above
    the true width are exactly 0 in act, z and dz."""
    run = _run(case, precision)
    B = run["cfg"]["B"]
    for L in run["layers"][:N_HIDDEN]:
        for r, rows in (("act", 2 * B), ("dz", B)):
            hi, lo = M.s8_planes(run[f"{r}/{L['name']}"], rows, L["npix"] * L["cp"])
            n = int(M.s8_malformed(hi, lo).sum())
            assert n == 0, f"{r}/{L['name']}: {n} elements are not a nearest-even split"
            pad = torch.stack([hi, lo]).reshape(2, rows, L["npix"], L["cp"])[..., L["c"]:]
            assert not bool(pad.any()), f"{r}/{L['name']}: padded channels are not zero"
        z = run[f"z/{L['name']}"][: B * L["npix"] * L["cp"]].reshape(B, L["npix"], L["cp"])[:, :, L["c"]:]
        assert not bool(z.any()), f"z/{L['name']}: padded channels are not zero"


def _order_depends_on_the_row_count(run):
    """The image kernels deal the 128-pixel tiles of eight images at a time to workgroups so that an image's tiles share an XCD
    (conv_img.h xcd_image_tile: taken when tiles > 1 and the launch has at least eight images), and a workgroup starts its K loop at
    step (blockIdx.x >> 3) % nsteps (conv_fwd_img_kernel, `rot`).  Tile (j, t) is workgroup j * T + t below eight images and
    (j / 8) * 8T + 8t + j % 8 from eight on: the same products in another fp32 order (the u8 pair kernel keeps that order on purpose:
    conv_u8_pair.h u8p_rotation).  Such a case is held to the model instead."""
    multi = any(r["fwd"]["kernel"] in ("u8img", "u8pair", "s8img") and r["fwd"]["tiles"] > 1 for r in run["routes"])
    return multi and 2 * run["cfg"]["B"] >= 8


@pytest.mark.parametrize("case,precision", RUNS)
def test_acting_forward_rows_against_the_model_at_every_row_count(case, precision):
    """eng.forward(n_rows = n), n in {1, 2, 3, 2B - 1, 2B}: act of the three convolutions and Dense_0 and the q rows, each against
    the model of its contraction on the same call's own act of the layer below, through the LayerNorm (as the next-state half of the
    learn step is checked).  Every convolution here takes the same kernel at an odd and an even image count (conv_routes: fwd ==
    fwd1; the S8 pair kernel that would differ needs one tile and K = 512 at two K groups), each kernel works per image, and the dense
    split-K factor is the plan's, not a function of n_rows: row r has the same bits at every n, except where the K order of a tile
    depends on the image count (_order_depends_on_the_row_count).  best_actions on the 2B rows is the argmax of head 1 + idx of
    those q rows."""
    run = _run(case, precision)
    own, _ = _passes(run)
    cfg, layers = run["cfg"], run["layers"]
    K, A, B = cfg["K"], cfg["A"], cfg["B"]
    assert all(r["fwd"] == r["fwd1"] for r in run["routes"])
    full = run["fwd_q"][2 * B]
    assert bool(torch.isfinite(full).all())
    exempt = _order_depends_on_the_row_count(run)
    out = []
    for n, q in run["fwd_q"].items():
        src = run["fwd_act"][n]
        assert q.shape == (n, (1 + K) * A)
        worst = 0.0
        for i, L in enumerate(layers):
            v, S, c = _forward_model(run, i, n, own, src)
            shape = (n, L["npix"], L["c"])
            a, E = M.ln_relu_fwd(v.reshape(shape), _vec(run, L["ln"], "scale"), _vec(run, L["ln"], "bias"), M.bound(S, c).reshape(shape))
            hi, lo = _planes(src, f"act/{L['name']}", L, n)
            used, _, _ = M.check(hi + lo, a, E, label=f"n_rows = {n}: act/{L['name']}")
            worst = max(worst, used)
        v, S, c = _forward_model(run, len(layers), n, own, src)
        usedq, _, _ = M.check(q.double(), v, M.bound(S, c), S, label=f"n_rows = {n}: q")
        same = torch.equal(q.view(torch.int32), full[:n].view(torch.int32))
        out.append(f"n_rows = {n}: act max |d| / bound = {worst:.3f}, q {usedq:.3f}, bits of the 2B-row forward: {same}, "
                   f"max |q - q(2B)| = {float((q - full[:n]).abs().max()):.2e}")
        if not exempt:
            assert same, f"n_rows = {n}: rows differ from the 2B-row forward's"
    _report(out)
    rows = torch.arange(2 * B, device="cuda")
    qh = full.reshape(2 * B, 1 + K, A)[rows, 1 + run["heads"].long()]
    top = torch.sort(qh, descending=True).values
    assert bool((top[:, 0] > top[:, 1]).all()), "a tie between the two largest q values: pick another seed"
    assert torch.equal(run["best"].long(), qh.argmax(-1))
