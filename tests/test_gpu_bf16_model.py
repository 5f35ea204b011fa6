"""Single-pass bf16 (and bf16x3) layer by layer against a float64 model of each contraction on the run's own operands
(tests/helpers/bf16_model.py).

Each case runs loss_on_batch, then learn_on_batch(grad_out=g), and reads the workspace.  Every stored tensor is compared with the
model of the contraction that produced it -- operands read back from the same run (S8 hi / lo halves, the weights' nearest-even
split), at the pass count of the run -- within c 2^-24 S, S the magnitude sum of the terms, c the fp32 accumulation depth
(bf16_model.chain_depth: ROUNDING x (MFMA_TREE + K steps + slabs + epilogue)).  Negative control: the same operands at the other
pass count (3 for a bf16 run, 1 for a bf16x3 run; 2 <-> 1 for Conv_0's uint8 pixels) must be 4x further away in the 2-norm and,
where the bound is tight enough, break it on at least half of the elements.

Measured on the MI355X over all cases (max |d| / 2^-24 S against c, 18 .. 968; the constants behind c and these values are in
bf16_model.py next to MFMA_TREE / ROUNDING): z 4.6, q 1.05 (loss path) and 1.05 (forward-only path), q_values 0.77, weight
gradients 2.7 (conv) and 13.6 (dense, c = 80).  Against composite bounds (max |d| / bound): targets 0.03, dz under a dense layer
0.47, dz under a convolution 0.49, dz under the head chain 0.93, next-state activations 0.62, online activations 0.70 with a
LayerNorm and 0.998 without one (B1030-noln: relu(z) is exact, so the S8 storage of the activation, bounded by its worst case
2^-17 |a|, is all that is left), Adam p / m / v 1.0 / 0.48 / 0.66 (gpu_helpers.adam_bounds: p's own half-ulp rounding).
Negative control, smallest share of elements the other pass count puts outside the bound: forward z 87 %, q / q_values 96 %,
dz 64 %, targets 66 %.  Weight gradients sum B x pixels products, and a next-state activation's LayerNorm spreads a contraction's
error over its row: there a worst-case bound is looser than the 1 / sqrt(n) difference the pass count makes, so the control holds
in the 2-norm only (elementwise 0 % .. 100 % and 33 % .. 52 %).

Mutations each of which fails at least one of these tests: split8 / s8_store_quad truncating hi (44 tests), the bf16 dense
forward running 3 passes (9), DenseDgradLN<1, 128> skipping its last K step (3: c5, B512, B1030), the S = 4 head chain
dropping the last transition of a partial workgroup (B1030's head test), round8 truncating (21), the bf16 convolution data
gradients running 3 passes (6: dz of every cnn case).

Not covered here: the LayerNorm scale / bias leaves of g at these sizes.  Their model (bf16_model.ln_param_grads: sum dy xhat and
sum dy, bounded by a plain chain over the partial rows of the route that wrote them) and every Dense route the widths above do not
select -- the four ln_bwd_small forms and ln_bwd_wide up to its 4096 columns, with and without a LayerNorm and with grid-stride rows;
two hidden Dense layers behind the torso, DenseDgradLN at a ragged K; the generic head path in a learn step and in a gradient-only
pass; the head chain at its widest; dense_post_kernel's second column pass and its slab tail; the big dense data gradient; a head
with no hidden layer -- are held stage by stage in tests/test_gpu_dense_routes.py (cases and routes: tests/helpers/dense_routes.py,
where _head_chain and _dense_dgrad_ln of this file now live).
The impala torso in bf16 and bf16x3 is covered stage by stage, with the same model and bounds, in
tests/test_gpu_impala.py (test_impala_stages_match_a_model_of_each_kernel_on_its_own_operands), the BatchNorm cnn and fc networks
in tests/test_gpu_batchnorm.py (test_batchnorm_stages_match_a_model_of_each_kernel_on_its_own_operands).  Every cnn case here runs
at the Atari frame (84x84x4): the convolution kernels that other frame sizes, stack depths and conv widths select -- several tiles per
image or per stride class, the u8 pair kernel's loop over halves, the generic fallbacks behind the LDS checks -- are held to the same
model in tests/test_gpu_conv_routes.py (cases and routes: tests/helpers/conv_routes.py).  Still uncovered in bf16: the BatchNorm
sites inside the impala torso ("Stack_s/BatchNorm_b"; they reuse the six kernels of csrc/batchnorm.h)."""
import numpy as np
import pytest
import torch

from tests.gpu_helpers import adam_bounds, device_batch, make_frame_batch, perturbed_params
from tests.helpers import bf16_model as M
from tests.helpers import conv_routes as R
from tests.helpers import dense_routes as D

pytestmark = pytest.mark.gpu

HEADLINE = (32, 64, 64, 512)
CASES = {
    "c5-bf16": dict(arch="cnn", feats=HEADLINE, K=32, A=4, B=1024, ln=True),  # head chain S = 4; DenseDgradLN<1, 128>
    "c2-bf16": dict(arch="cnn", feats=HEADLINE, K=9, A=9, B=256, ln=True),  # head chain S = 1; DenseDgradLN<1, 128, 2>
    "B512": dict(arch="cnn", feats=HEADLINE, K=3, A=4, B=512, ln=True),  # S = 2
    "B1030-ragged-noln": dict(arch="cnn", feats=HEADLINE, K=2, A=3, B=1030, ln=False),  # S = 4, a partial last workgroup
    "B131": dict(arch="cnn", feats=HEADLINE, K=3, A=4, B=131, ln=True),  # ragged weight-gradient image groups
    "small": dict(arch="cnn", feats=(7, 9, 11, 13), K=3, A=5, B=6, ln=True),  # small and ragged tiles
    "fc-lunar": dict(arch="fc", feats=(100, 100), K=1, A=4, B=32, ln=True),  # observations rounded in the kernel
    "fc-wide": dict(arch="fc", feats=(300, 600), K=3, A=5, B=1000, ln=True),  # head chain COLS = 2, S = 2
    "fc-cols4": dict(arch="fc", feats=(64, 1288), K=2, A=3, B=40, ln=True),  # head chain COLS = 4 (1288: ragged)
}
RUNS = [pytest.param(c, "bf16", id=f"{c}-bf16" if not c.endswith("-bf16") else c) for c in CASES] + [
    pytest.param(c, "bf16x3", id=f"{c}-bf16x3") for c in ("small", "B131", "fc-lunar", "fc-cols4")]
GAMMA = 0.99
# the geometry and the plan's tiling decisions, restated once for this file and tests/test_gpu_conv_routes.py
FC_OBS, CONVS, _ceil = R.FC_OBS, R.CONVS, R._ceil
_layers, _fwd_splits, _dense_wgrad_slabs, _conv_wgrad_chain = R.layers, R.fwd_splits, R.dense_wgrad_slabs, R.conv_wgrad_chain


# the selection code, restated (net_plan.h, learn_step.h): tests/helpers/dense_routes.py holds it for this file and tests/test_gpu_dense_routes.py
_dense_dgrad_ln, _head_chain = D._dense_dgrad_ln, D._head_chain


# ------------------------------------------------------------------ one run
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

    cfg = CASES[case]
    feats, K, A, B, arch, ln = cfg["feats"], cfg["K"], cfg["A"], cfg["B"], cfg["arch"], cfg["ln"]
    obs = (84, 84, 4) if arch == "cnn" else FC_OBS
    params = perturbed_params(17, obs, list(feats), arch, (1 + K) * A, ln)
    eng = QNetEngine(obs, A, 1 + K, list(feats), arch, ln, B, gamma_n=GAMMA, learning_rate=1e-3, adam_eps=1.5e-4, precision=precision)
    eng.import_flax(params)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if arch == "cnn":
        frames, ids, action, reward, terminal, ref = make_frame_batch(B, A, seed=29, n_frames=B + 64)
        batch = device_batch(eng, frames, ids, action, reward, terminal)
        x = np.concatenate([ref.state, ref.next_state])  # [2B][84][84][4] uint8
    else:
        rng = np.random.default_rng(29)
        st, nx = (rng.normal(size=(B, FC_OBS[0])).astype(np.float32) for _ in range(2))
        action, reward = rng.integers(0, A, B).astype(np.int32), rng.normal(size=B).astype(np.float32)
        terminal = (rng.random(B) < 0.3).astype(np.uint8)
        batch = eng.make_batch(state=d(st), next_state=d(nx), action=d(action), reward=d(reward), terminal=d(terminal))
        x = np.concatenate([st, nx])
    eng.loss_on_batch(batch)
    torch.cuda.synchronize()
    run = dict(cfg=cfg, precision=precision, x=torch.from_numpy(x).cuda(), action=action, reward=reward, terminal=terminal,
               q=eng.region("q").clone(), loss_qv=eng.q_values.clone(), loss_tg=eng.targets.clone(), loss_losses=eng.losses.clone())
    run["p0"] = eng.export_flax()
    # the learn step's head chain applies the last hidden layer's LayerNorm / ReLU itself and rewrites its act rows: a few hi
    # halves may round the other way than dense_post_kernel's, so the loss path's q is checked on the act it read
    last = _layers(cfg)[0][-1]["name"]
    run["loss_act"] = eng.region(f"act/{last}").clone()
    # the forward-only path (head GEMM + dense_post_kernel) on the same 2B rows, with the same parameters
    if arch == "cnn":
        both = torch.from_numpy(np.concatenate([ids[:, :4], ids[:, 4:]]).copy()).cuda()
        run["fwd_q"] = eng.forward(frames=batch._keep[0], frame_stride=frames.shape[1], frame_ids=both, n_rows=2 * B).clone()
    else:
        run["fwd_q"] = eng.forward(obs=d(x), n_rows=2 * B).clone()
    torch.cuda.synchronize()
    run["fwd_act"] = eng.region(f"act/{last}").clone()
    run["p0_internal"] = eng.params.clone()
    for t in (eng.q_values, eng.targets, eng.priorities):  # whatever the learn step leaves unwritten shows as NaN, not as loss_on_batch's value
        t.fill_(float("nan"))
    g = torch.zeros_like(eng.params)
    eng.learn_on_batch(batch, grad_out=g)
    torch.cuda.synchronize()
    layers, head_in_p = _layers(cfg)
    run.update(g_internal=g.clone(), adam_m=eng.adam_m.clone(), adam_v=eng.adam_v.clone(), adam_count=int(eng.adam_count.item()))
    run.update(layers=layers, head_in_p=head_in_p, nha_p=_ceil((1 + K) * A, 8) * 8, qv=eng.q_values.clone(), tg=eng.targets.clone(),
               losses=eng.losses.clone(), prio=eng.priorities.clone(), dout=eng.region("dout").clone(), g=eng.internal_to_flax_grads(g),
               mirror=eng.region("wsplit").clone().view(torch.int32), params_after=eng.params.clone())
    for L in layers:
        for r in ("act", "z", "dz"):
            run[f"{r}/{L['name']}"] = eng.region(f"{r}/{L['name']}").clone()
    del eng
    _CACHE[key] = run
    return run


def _passes(run):
    return (1, 3) if run["precision"] == "bf16" else (3, 1)


def _w(run, mod, src="p0"):
    return M.split(torch.from_numpy(np.asarray(run[src][mod]["kernel"])).cuda())


def _vec(run, mod, leaf):
    return torch.from_numpy(np.asarray(run["p0"][mod][leaf], np.float64)).cuda()


def _act(run, L, rows, key=None):
    """own S8 output of hidden layer L, rows [0, rows), true channels: planes [rows][npix][c]."""
    hi, lo = M.s8_planes(run[key or f"act/{L['name']}"], rows, L["npix"] * L["cp"])
    f = lambda t: t.reshape(rows, L["npix"], L["cp"])[:, :, : L["c"]]
    return f(hi), f(lo)


def _input_planes(run, i, rows, key=None):
    """planes of the input of hidden layer i over rows [0, rows): NHWC for a convolution, [rows][in] for a dense layer"""
    layers = run["layers"]
    L = layers[i] if i < len(layers) else dict(kind=1)  # i = len(layers): the head
    if i == 0:
        x = run["x"][:rows]
        if L["kind"] == 0:
            return x.to(torch.float64), None  # uint8 pixels: exact
        return M.split(x)
    P = _act(run, layers[i - 1], rows, key)
    if L["kind"] == 0:
        h = layers[i - 1]["h"]
        return tuple(p.reshape(rows, h, h, -1) for p in P)
    return tuple(p.reshape(rows, -1) for p in P)


def _forward_model(run, i, rows, passes, key=None):
    """(z, S, c) of hidden layer i (or the head, i = len(layers)) over rows [0, rows); `key`: the region holding its input"""
    cfg, layers = run["cfg"], run["layers"]
    N2 = 2 * cfg["B"]
    if i < len(layers):
        L = layers[i]
        mod = L["name"]
    else:
        mod, L = f"Dense_{sum(l['kind'] == 1 for l in layers)}", None
    b = _vec(run, mod, "bias")
    xin = _input_planes(run, i, rows, key)
    w = _w(run, mod)
    if L is not None and L["kind"] == 0:
        p = passes if i else min(passes, 2)  # uint8 pixels: 3 passes are 2
        v, S = M.conv(p, xin, w, L["s"])
        c = M.chain_depth(L["K"])
        if i == 0:
            s = float(np.float32(1.0 / 255.0))
            v, S = v * s, S * s
        return v + b, S + b.abs(), c
    v, S = M.dense(passes, xin, w)
    in_p = L["in_p"] if L is not None else run["head_in_p"]
    out_p = L["cp"] if L is not None else run["nha_p"]
    fs = _fwd_splits(N2, out_p, in_p, cfg["arch"] == "fc" and i == 0)
    return v + b, S + b.abs(), M.chain_depth(in_p, slabs=fs)


def _report(rows):
    print()
    for r in rows:
        print("  " + r)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("case,precision", RUNS)
def test_selected_instantiations(case, precision):
    """The instantiations each case is meant to reach, from the selection code restated on the host."""
    cfg = CASES[case]
    layers, hid_p = _layers(cfg)
    K, A, B = cfg["K"], cfg["A"], cfg["B"]
    hc = _head_chain(cfg, hid_p, _ceil((1 + K) * A, 8) * 8, K, 1 if precision == "bf16" else 3)
    assert hc is not None, "head chain skipped"
    want_S = 4 if B >= 1024 else 2 if B >= 512 else 1
    assert hc[0] == want_S
    if case == "fc-wide":
        assert hc[1] == 2
    if case == "fc-cols4":
        assert hc[1] == 4
    if case == "c5-bf16":
        assert _dense_dgrad_ln(cfg, layers) == 1  # DenseDgradLN<1, 128>: one K group
    if case == "c2-bf16":
        assert _dense_dgrad_ln(cfg, layers) == 2  # DenseDgradLN<1, 128, 2>
    if case == "B131":  # the image-resident weight gradients of Conv_1 / Conv_2 take G = 2 images per group: the last group holds one
        for L in layers[1:3]:
            steps, slabs = _conv_wgrad_chain(B, L)
            G = (B + 127) // 128
            assert G == 2 and B % G == 1 and slabs == _ceil(B, G)
    run = _run(case, precision)
    assert np.isfinite(run["losses"].cpu().numpy()).all()


@pytest.mark.parametrize("case,precision", RUNS)
def test_forward_layers_against_the_model(case, precision):
    """z/<layer> (pre-LayerNorm fp32, online rows) of every hidden layer against its contraction on the layer below's own act and
    the weights' nearest-even split, plus bias; the q rows of loss_on_batch (both halves) against the head row on own act."""
    run = _run(case, precision)
    own, other = _passes(run)
    B = run["cfg"]["B"]
    out = []
    for i, L in enumerate(run["layers"]):
        want, S, c = _forward_model(run, i, B, own)
        alt, _, _ = _forward_model(run, i, B, other)
        got = run[f"z/{L['name']}"][: B * L["npix"] * L["cp"]].reshape(B, L["npix"], L["cp"])[:, :, : L["c"]].double()
        want, S, alt = (t.reshape(got.shape) for t in (want, S, alt))
        used, ratio, frac = M.check(got, want, M.bound(S, c), S, alt, label=f"z/{L['name']}")
        out.append(f"z/{L['name']}: c = {c}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
    nha = (1 + run["cfg"]["K"]) * run["cfg"]["A"]
    n = len(run["layers"])
    want, S, c = _forward_model(run, n, 2 * B, own, "loss_act")
    alt, _, _ = _forward_model(run, n, 2 * B, other, "loss_act")
    got = run["q"][: 2 * B * run["nha_p"]].reshape(2 * B, run["nha_p"])[:, :nha].double()
    used, ratio, frac = M.check(got, want, M.bound(S, c), S, alt, label="q")
    out.append(f"q: c = {c}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
    _report(out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_forward_only_path_against_the_model(case, precision):
    """eng.forward on the same 2B rows with the same parameters (head GEMM + dense_post_kernel): its q against the head model on
    the act rows that forward wrote, within the head GEMM's chain; control: the other pass count."""
    run = _run(case, precision)
    own, other = _passes(run)
    B, n = run["cfg"]["B"], len(run["layers"])
    want, S, c = _forward_model(run, n, 2 * B, own, "fwd_act")
    alt, _, _ = _forward_model(run, n, 2 * B, other, "fwd_act")
    _, ratio, frac = M.check(run["fwd_q"].double(), want, M.bound(S, c), S, alt, label="forward q")
    _report([f"forward q: c = {c}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}"])


@pytest.mark.parametrize("case,precision", RUNS)
def test_hidden_activations_of_both_halves(case, precision):
    """act/<layer> of every hidden layer, rows [0, 2B): the online half through the float64 LayerNorm / ReLU of the layer's own z
    (only the normalisation's arithmetic is left), the next-state half -- whose pre-activations are not stored -- through the
    model of the contraction on the layer below's own next-state act, carried through the LayerNorm (bf16_model.ln_relu_fwd).
    Control on the next-state half: the other pass count, in the 2-norm."""
    run = _run(case, precision)
    own, other = _passes(run)
    B = run["cfg"]["B"]
    out = []
    for i, L in enumerate(run["layers"]):
        shape = (B, L["npix"], L["c"])
        gamma, beta = (_vec(run, L["ln"], k) if L["ln"] else None for k in ("scale", "bias"))
        hi, lo = M.s8_planes(run[f"act/{L['name']}"], 2 * B, L["npix"] * L["cp"])
        got = (hi + lo).reshape(2 * B, L["npix"], L["cp"])[:, :, : L["c"]]
        z = run[f"z/{L['name']}"][: B * L["npix"] * L["cp"]].reshape(B, L["npix"], L["cp"])[:, :, : L["c"]].double()
        a, E = M.ln_relu_fwd(z, gamma, beta, torch.zeros_like(z), has_ln=L["ln"] is not None)
        used_on, _, _ = M.check(got[:B], a, E, label=f"act/{L['name']} online")
        zm = []
        for p in (own, other):
            v, S, c = _forward_model(run, i, 2 * B, p)
            zm.append((v.reshape(2 * B, *shape[1:])[B:], M.bound(S, c).reshape(2 * B, *shape[1:])[B:]))
        a, E = M.ln_relu_fwd(zm[0][0], gamma, beta, zm[0][1], has_ln=L["ln"] is not None)
        alt, _ = M.ln_relu_fwd(zm[1][0], gamma, beta, zm[1][1], has_ln=L["ln"] is not None)
        used, _, frac = M.check(got[B:], a, E, None, alt, elementwise_control=False, label=f"act/{L['name']} next-state")
        out.append(f"act/{L['name']}: online max |d| / bound = {used_on:.3f}, next-state {used:.3f}, other passes outside: {frac:.0%}")
    _report(out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_adam_step_against_float64(case, precision):
    """The learn step's Adam update (first step from zero moments: adam_kernel and the fused-Adam GEMM epilogue, whichever each
    tensor takes at this size) against float64 Adam applied to the gradient it reported, element by element within the float32
    rounding that gpu_helpers.adam_bounds derives; the count advances to 1."""
    run = _run(case, precision)
    assert run["adam_count"] == 1
    p0, g = (run[k].cpu().numpy() for k in ("p0_internal", "g_internal"))
    zero = np.zeros_like(p0)
    (p, m, v, _), (ep, em, ev) = adam_bounds(p0, zero, zero, g, 1, 1e-3, 1.5e-4)
    out = []
    for name, got, want, bound in (("m", run["adam_m"], m, em), ("v", run["adam_v"], v, ev), ("p", run["params_after"], p, ep)):
        r = np.abs(got.cpu().numpy().astype(np.float64) - want) / bound
        i = int(np.argmax(r))
        assert r[i] <= 1.0, f"{name}[{i}]: got {float(got[i])!r} want {want[i]!r} bound {bound[i]:.3e} g {g[i]!r}"
        out.append(f"{name}: max |d| / bound = {r[i]:.3f}")
    assert np.count_nonzero(run["params_after"].cpu().numpy() != p0) > 0.5 * np.count_nonzero(g)
    _report(out)


def _head(run, passes):
    """model q of all 2B rows at `passes`, its bound, and the online q of the taken actions / the Bellman targets with bounds"""
    cfg = run["cfg"]
    K, A, B = cfg["K"], cfg["A"], cfg["B"]
    n = len(run["layers"])
    q, S, _ = _forward_model(run, n, 2 * B, passes)
    hid_p = run["head_in_p"]
    c = M.chain_depth(hid_p, slabs=8)  # head chain: K steps dealt over 8 waves, then the 8 wave partials
    E = M.bound(S, c)
    a = torch.from_numpy(run["action"].astype(np.int64)).cuda()
    cols = (torch.arange(K, device=a.device)[None, :] + 1) * A + a[:, None]
    qv, Eqv = q[:B].gather(1, cols), E[:B].gather(1, cols)
    r = torch.from_numpy(run["reward"].astype(np.float64)).cuda()
    t = torch.from_numpy(run["terminal"].astype(np.float64)).cuda()
    tg = M.bellman_targets(q[B:], r, t, GAMMA, K, A)
    # max is 1-Lipschitz in the max norm: where the two largest are within the bound either is accepted
    Eq = E[B:, : K * A].reshape(B, K, A).max(-1).values
    Etg = GAMMA * Eq + M.ROUNDING * 3 * M.U * (r.abs()[:, None] + GAMMA * tg.abs()) + M.FLOOR
    return qv, Eqv, S[:B].gather(1, cols), tg, Etg


@pytest.mark.parametrize("case,precision", RUNS)
def test_head_losses_and_priorities(case, precision):
    """q_values and targets of the learn step (the head chain) against the head model on own act, the Bellman target over the
    model's next-state q; dL/dq ("dout"), the per-head losses and the priorities in float64 from the run's own q_values / targets;
    loss_on_batch's q_values / targets from the q rows it wrote."""
    run = _run(case, precision)
    own, other = _passes(run)
    K, B = run["cfg"]["K"], run["cfg"]["B"]
    qv, Eqv, Sqv, tg, Etg = _head(run, own)
    aqv, _, _, atg, _ = _head(run, other)
    out = []
    _, ratio, frac = M.check(run["qv"].double(), qv, Eqv, Sqv, aqv, label="q_values")
    out.append(f"q_values: max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
    used, _, frac = M.check(run["tg"].double(), tg, Etg, None, atg, elementwise_control=False, label="targets")
    out.append(f"targets: max |d| / bound = {used:.2f}, other passes outside: {frac:.0%}")
    # float64 from the run's own q_values / targets (no pass count enters: no control)
    td = run["qv"].double() - run["tg"].double()
    want = torch.zeros(B, run["nha_p"], dtype=torch.float64, device=td.device)
    a = torch.from_numpy(run["action"].astype(np.int64)).cuda()
    cols = (torch.arange(K, device=a.device)[None, :] + 1) * run["cfg"]["A"] + a[:, None]
    want.scatter_(1, cols, 2.0 * td / B)
    got = run["dout"][: B * run["nha_p"]].reshape(B, -1).double()
    M.check(got, want, M.ROUNDING * 3 * M.U * want.abs() + M.FLOOR, label="dout")
    lw = (td * td).mean(0)
    M.check(run["losses"].double(), lw, M.bound(lw, M.chain_depth(0, slabs=B, epilogue=3)), label="losses")
    arg = (td * td).sum(1) / K + 1e-10
    pw = arg.sqrt()
    M.check(run["prio"].double(), pw, M.ROUNDING * (K + 4) * M.U * arg / (2 * pw) + 1e-300, label="priorities")
    # loss_on_batch reads its q_values off the q rows it wrote (checked in test_forward_layers_against_the_model)
    q = run["q"][: 2 * B * run["nha_p"]].reshape(2 * B, -1)
    assert torch.equal(run["loss_qv"], q[:B].gather(1, cols))
    r = torch.from_numpy(run["reward"].astype(np.float64)).cuda()
    t = torch.from_numpy(run["terminal"].astype(np.float64)).cuda()
    ltg = M.bellman_targets(q[B:].double(), r, t, GAMMA, K, run["cfg"]["A"])
    M.check(run["loss_tg"].double(), ltg, M.ROUNDING * 3 * M.U * (r.abs()[:, None] + ltg.abs()) + M.FLOOR, label="loss_on_batch targets")
    _report(out)


def _dz_check(run, i, passes):
    """dz of hidden layer i (online rows) from the model of its da, through the float64 LayerNorm / ReLU backward on the layer's own
    z and ReLU decisions (own act > 0).  The head chain's da = dL/dq W_head is an fp32 AXPY on the fp32 master weights
    (net_kernels.hip head_chain_kernel), so that one is modelled as a plain fp32 sum and has no pass count."""
    cfg, layers = run["cfg"], run["layers"]
    B = cfg["B"]
    L, up = layers[i], i + 1
    if up == len(layers):  # below the head: the head chain
        nha = (1 + cfg["K"]) * cfg["A"]
        dq = run["dout"][: B * run["nha_p"]].reshape(B, -1)[:, :nha].double()
        W = _vec(run, f"Dense_{sum(l['kind'] == 1 for l in layers)}", "kernel")
        da, S = dq @ W.T, dq.abs() @ W.abs().T
        E_da = M.bound(S, M.chain_depth(0, slabs=cfg["K"] + 1))
    elif layers[up]["kind"] == 0:  # a convolution's data gradient (conv_dgrad_img with the LayerNorm backward fused, or ConvDgrad)
        U_ = layers[up]
        hi, lo = M.s8_planes(run[f"dz/{U_['name']}"], B, U_["npix"] * U_["cp"])
        dz = tuple(p.reshape(B, U_["npix"], U_["cp"])[:, :, : U_["c"]] for p in (hi, lo))
        da, S = M.conv_dgrad(passes, dz, _w(run, U_["name"]), (L["h"], L["h"]), U_["s"])
        # every tap of every output channel at most (a class-split kernel sums ceil(k / s)^2 of them), then the epilogue
        E_da = M.bound(S, M.chain_depth(U_["k"] ** 2 * U_["cp"], epilogue=4))
    else:  # a dense layer's data gradient on the MFMA engine (DenseDgradLN below the torso)
        U_ = layers[up]
        dz = M.s8_planes(run[f"dz/{U_['name']}"], B, U_["cp"])
        dz = tuple(p[:, : U_["c"]] for p in dz)
        w = _w(run, U_["name"])
        da, S = M.dense(passes, dz, tuple(p.T for p in w))
        E_da = M.bound(S, M.chain_depth(U_["cp"], epilogue=3))
    shape = (B, L["npix"], L["c"])
    z = run[f"z/{L['name']}"][: B * L["npix"] * L["cp"]].reshape(B, L["npix"], L["cp"])[:, :, : L["c"]].double()
    hi, lo = _act(run, L, B)
    mask = ((hi + lo) > 0).double()
    gamma = _vec(run, L["ln"], "scale") if L["ln"] else None
    dzm, E = M.ln_relu_bwd(z, gamma, mask, da.reshape(shape), E_da.reshape(shape), has_ln=L["ln"] is not None)
    hi, lo = M.s8_planes(run[f"dz/{L['name']}"], B, L["npix"] * L["cp"])
    got = (hi + lo).reshape(B, L["npix"], L["cp"])[:, :, : L["c"]]
    return got, dzm, E


@pytest.mark.parametrize("case,precision", RUNS)
def test_backward_dz_against_the_model(case, precision):
    """dz/<layer> of every hidden layer: the last one under the head chain, the layer under the first dense one (cnn: Conv_2
    through DenseDgradLN; fc: the dense chain), and Conv_1 / Conv_0 under the convolutions' data gradients (transposed SAME
    convolutions of own dz with the weights' split).  Control: the other pass count, where one enters (not through the head
    chain's fp32 AXPY)."""
    run = _run(case, precision)
    own, other = _passes(run)
    layers = run["layers"]
    out = []
    for i in range(len(layers) - 1, -1, -1):
        got, want, E = _dz_check(run, i, own)
        alt = _dz_check(run, i, other)[1] if i + 1 < len(layers) else None
        used, _, frac = M.check(got, want, E, None, alt, label=f"dz/{layers[i]['name']}")
        out.append(f"dz/{layers[i]['name']}: max |d| / bound = {used:.3f}" + (f", other passes outside: {frac:.0%}" if alt is not None else
                                                                             " (head chain AXPY: no pass count)"))
    _report(out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_weight_gradients_against_the_model(case, precision):
    """Every kernel leaf of g against sum over the online rows of own input activations x own dz at the pass count, every bias
    against sum dz.  Weight gradients sum B x pixels products: a worst-case chain of that length is looser than the difference
    the pass count makes (which averages as 1 / sqrt(n)), so there the control is asserted in the 2-norm and its elementwise
    fraction only reported."""
    run = _run(case, precision)
    own, other = _passes(run)
    cfg, layers = run["cfg"], run["layers"]
    B = cfg["B"]
    out = []
    nh = sum(l["kind"] == 1 for l in layers)
    for i in range(len(layers) + 1):
        head = i == len(layers)
        L = layers[i] if not head else None
        mod = L["name"] if not head else f"Dense_{nh}"
        if head:
            nha = (1 + cfg["K"]) * cfg["A"]
            dz = M.split(run["dout"][: B * run["nha_p"]].reshape(B, -1)[:, :nha])  # fp32 dL/dq, split by the kernel
        else:
            hi, lo = M.s8_planes(run[f"dz/{mod}"], B, L["npix"] * L["cp"])
            dz = tuple(p.reshape(B, L["npix"], L["cp"])[:, :, : L["c"]] for p in (hi, lo))
        xin = _input_planes(run, i, B)
        if L is not None and L["kind"] == 0:
            def model(p):
                v, S = M.conv_wgrad(min(p, 2) if i == 0 else p, xin, dz, L["k"], L["s"])
                if i == 0:
                    s = float(np.float32(1.0 / 255.0))
                    v, S = v * s, S * s
                return v, S
            steps, slabs = _conv_wgrad_chain(B, L)
            c = M.ROUNDING * (M.MFMA_TREE + steps + slabs + 2)
        else:
            dz2 = tuple(p.reshape(B, -1) for p in dz)
            model = lambda p: M.wgrad(p, xin, dz2)
            in_p = L["in_p"] if L is not None else run["head_in_p"]
            out_p = L["cp"] if L is not None else run["nha_p"]
            c = M.chain_depth(B, slabs=_dense_wgrad_slabs(B, in_p, out_p))
        want, S = model(own)
        alt, _ = model(other)
        got = torch.from_numpy(np.asarray(run["g"][mod]["kernel"], np.float64)).cuda()
        used, ratio, frac = M.check(got, want, M.bound(S, c), S, alt, elementwise_control=False, label=f"{mod}/kernel")
        out.append(f"{mod}/kernel: c = {c}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
        # bias: a plain fp32 sum of dz (hi + lo of the S8 value: within S8_STORE of the fp32 one); no pass count, no control
        dzv = (dz[0] + dz[1]).reshape(-1, dz[0].shape[-1])
        bw, bS = dzv.sum(0), dzv.abs().sum(0)
        gb = torch.from_numpy(np.asarray(run["g"][mod]["bias"], np.float64)).cuda()
        M.check(gb, bw, M.bound(bS, M.chain_depth(0, slabs=dzv.shape[0], epilogue=4)) + M.S8_STORE * bS, label=f"{mod}/bias")
    _report(out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_s8_tensors_and_mirror_are_nearest_even_splits(case, precision):
    """After the step the weight mirror equals a fresh nearest-even split of the fp32 parameters, bit for bit (a kernel that reads
    a stale mirror fails this or the forward check); every stored activation / dz element is a nearest-even split (|lo| <= half
    an ulp of hi: a truncating split leaves a whole ulp on about half of them)."""
    run = _run(case, precision)
    want = M.split_words(run["params_after"])
    got = run["mirror"][: want.numel()]
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{bad.numel()} mirror words differ from a nearest-even split, first at {int(bad[0])}"
    B = run["cfg"]["B"]
    for L in run["layers"]:
        for r, rows in (("act", 2 * B), ("dz", B)):
            hi, lo = M.s8_planes(run[f"{r}/{L['name']}"], rows, L["npix"] * L["cp"])
            n = int(M.s8_malformed(hi, lo).sum())
            assert n == 0, f"{r}/{L['name']}: {n} elements are not a nearest-even split"
