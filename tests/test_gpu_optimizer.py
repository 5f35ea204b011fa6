"""The optimizer and the first layer's weight gradient, element by element against float64.

1. Adam (gemm_core.h adam_element: hardware v_sqrt_f32 / v_rcp_f32, precomputed 1 / (1 - b^t)) through the product learn path, from
   planted moments and step counts, in both kernels that run it: adam_kernel (slab reduction, then the update) and the fused-Adam
   epilogue of the dense weight-gradient GEMM (net_problems.h AdamFuse).
2. The S8 weight mirror both write (s8_store_quad) equals a fresh split of the parameters, bit for bit; gradient-only passes
   leave parameters, moments, count and mirror alone.
3. Every leaf's gradient against the float64 gradient with the HIP path's own ReLU decisions, element-wise against the sum of
   magnitudes of its terms, and for a systematic scale / offset bias.
4. The K = 1 fixture's first Adam step against the float64 step on those pinned decisions: where the fixture's Conv_0 offset
   comes from (docs/NOTEBOOK.md)."""
import os

import numpy as np
import pytest
import torch

from tests.gpu_helpers import adam_bounds as _adam_bounds
from tests.gpu_helpers import device_batch, hip_preactivations, make_frame_batch, make_pair, masked_reference_grads

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Which kernel updates which tensor (net_plan.h: dense weight-gradient slabs s = 1 from 128 output tiles of 128 x 128, else 256 / tiles
# capped at ceil(B / 32) K steps; net_kernels.hip weight_gradient: fused Adam when effective_splits(B, s) == 1 and the input is not the
# caller's fp32 observations; the head takes the head chain in every learn step with a ReLU hidden layer up to 2048 wide):
#   headline, B = 32 and B = 64: Dense_0 (512 x 7744 after SAME padding: 4 x 61 = 244 tiles, s = 1) -> FUSED epilogue at both sizes
#     (one and two K steps of the contraction inside the one slab); the head (Dense_1) -> head chain, slabs + adam_kernel at both;
#     conv kernels, every bias and LayerNorm parameter -> adam_kernel.  (The fused GEMM with update = 0 -- no head chain, so the head
#     too -- runs in test_gradient_only_passes_change_nothing.)  The mutation that drops the lo half of the fused epilogue's mirror
#     store fails both headline cases on exactly Dense_0's 1 982 464 lo words.
#   fc 8 -> 100 -> 100 -> 8, B = 32: Dense_0 (fp32 observations) -> slabs + adam_kernel; Dense_1 (104 x 104, one tile) -> FUSED;
#     Dense_2 (head chain) -> adam_kernel
OPT_CONFIGS = [
    pytest.param(dict(arch="cnn", feats=(32, 64, 64, 512), K=9, A=9, B=32, eps=1.5e-4), id="headline-B32"),
    pytest.param(dict(arch="cnn", feats=(32, 64, 64, 512), K=9, A=9, B=64, eps=1.5e-4), id="headline-B64-two-ksteps"),
    pytest.param(dict(arch="fc", feats=(100, 100), K=1, A=4, B=32, eps=1e-8), id="lunar-lander-eps1e-8"),
]
# 0 and 1: the first steps; 9: c1, c2 far from both 0 and 1; 12.5 M: a full Atari run (b2^t underflows, c1 = c2 = 1)
T0S = [0, 1, 9, 12_500_000]
LR = 1e-3


def _engine(cfg, seed=3):
    from slimdqn._engine import QNetEngine
    from tests.gpu_helpers import perturbed_params

    feats, K, A, B, eps = cfg["feats"], cfg["K"], cfg["A"], cfg["B"], cfg["eps"]
    if cfg["arch"] == "cnn":
        oracle, eng, params = make_pair(feats, K, A, B, seed=seed, lr=LR, adam_eps=eps)
        frames, ids, action, reward, terminal, ref = make_frame_batch(B, A, seed=seed + 20, n_frames=B + 64)
        return eng, device_batch(eng, frames, ids, action, reward, terminal)
    obs = (8,)
    params = perturbed_params(seed, obs, feats, "fc", (1 + K) * A, True)
    eng = QNetEngine(obs, A, 1 + K, feats, "fc", True, B, gamma_n=0.99, learning_rate=LR, adam_eps=eps)
    eng.import_flax(params)
    rng = np.random.default_rng(seed)
    d = lambda a: torch.from_numpy(a).cuda()
    batch = eng.make_batch(state=d(rng.normal(size=(B, 8)).astype(np.float32)), next_state=d(rng.normal(size=(B, 8)).astype(np.float32)),
                           action=d(rng.integers(0, A, B).astype(np.int32)), reward=d(rng.normal(size=B).astype(np.float32)),
                           terminal=d((rng.random(B) < 0.2).astype(np.uint8)))
    return eng, batch


def _real(eng):
    """True where an internal parameter element is a real Flax element (not channel / row padding)."""
    mask = np.zeros(eng.n_param_floats, bool)
    for info in eng.infos:
        shape = tuple(info.flax_shape[: info.ndim])
        mask[info.offset : info.offset + info.size] = eng._to_internal(info, np.ones(shape, np.float32)) != 0
    return mask


def _plant(g_pre, real, t, eps, rng):
    """m, v by element index, six classes in turn (real elements only; padding keeps m = v = 0, so it never moves):
    0: v = 0, m != 0          1: v denormal (1e-40)       2: sqrt(v_hat) = eps from v alone (the eps-dominated denominator)
    3: v = 1e4 (tiny step)    4: m against the sign of the gradient, 4x its size     5: ordinary moments"""
    n = g_pre.size
    a = np.abs(g_pre) + 1e-9
    cls = np.arange(n) % 6
    m = (rng.normal(size=n) * a).astype(np.float32)
    v = np.zeros(n, np.float32)
    c2 = 1.0 - float(np.float32(0.999)) ** t
    v[cls == 1] = 1e-40
    v[cls == 2] = eps * eps * c2 / float(np.float32(0.999))
    v[cls == 3] = 1e4
    m[cls == 4] = -4.0 * g_pre[cls == 4]
    v[cls == 4] = (2.0 * g_pre[cls == 4] ** 2).astype(np.float32)
    m[cls == 5] = (0.3 * g_pre[cls == 5] + 0.1 * m[cls == 5]).astype(np.float32)
    v[cls == 5] = (g_pre[cls == 5] ** 2 + 1e-8).astype(np.float32)
    m[~real] = 0.0
    v[~real] = 0.0
    assert np.all(np.abs(v[(cls == 1) & real]) < np.finfo(np.float32).tiny)  # really denormal in float32
    return m, v


def _bits(t):
    return t.detach().clone().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("cfg", OPT_CONFIGS)
def test_adam_element_update_and_mirror_match_float64(cfg):
    """(1) Adam through learn_on_batch from planted (m, v, t): p, m, v per element against float64 Adam on the gradient the update
    consumed (grad_out is written from the registers the update reads), within the float32 rounding derived in _adam_bounds;
    adam_count advances by one.  (2) After every step the mirror the optimizer wrote is bit-identical to rebuild_mirror()'s split of
    the new parameters over the whole buffer, padding included (split_params_kernel writes every group of 8: both define it)."""
    eng, batch = _engine(cfg)
    eps = cfg["eps"]
    real = _real(eng)
    g_pre = torch.zeros_like(eng.params)
    eng.grad_on_batch(batch, g_pre)
    g_pre = g_pre.cpu().numpy()
    rng = np.random.default_rng(11)
    worst = {}
    for t0 in T0S:
        m0, v0 = _plant(g_pre, real, t0 + 1, eps, rng)
        eng.adam_m.copy_(torch.from_numpy(m0))
        eng.adam_v.copy_(torch.from_numpy(v0))
        eng.adam_count.fill_(t0)
        p0 = eng.params.cpu().numpy().copy()
        grad = torch.zeros_like(eng.params)
        eng.learn_on_batch(batch, grad_out=grad)
        torch.cuda.synchronize()
        g = grad.cpu().numpy()
        assert np.isfinite(g).all()
        assert int(eng.adam_count.item()) == t0 + 1
        (p, m, v, u), (ep, em, ev) = _adam_bounds(p0, m0, v0, g, t0 + 1, LR, eps)
        got_p, got_m, got_v = (x.cpu().numpy().astype(np.float64) for x in (eng.params, eng.adam_m, eng.adam_v))
        for name, got, want, bound in (("m", got_m, m, em), ("v", got_v, v, ev), ("p", got_p, p, ep)):
            r = np.abs(got - want) / bound
            i = int(np.argmax(r))
            worst[(t0, name)] = float(r[i])
            assert r[i] <= 1.0, (f"t0={t0} {name}[{i}] (class {i % 6}, real {real[i]}): got {got[i]!r} want {want[i]!r} "
                                 f"err {abs(got[i] - want[i]):.3e} bound {bound[i]:.3e} g {g[i]!r} m0 {m0[i]!r} v0 {v0[i]!r}")
        assert np.count_nonzero(got_p[real] != p0[real]) > 0.5 * real.sum()  # the planted moments move most elements
        mirror = _bits(eng.region("wsplit"))
        eng.rebuild_mirror()
        fresh = _bits(eng.region("wsplit"))
        bad = np.flatnonzero(mirror != fresh)
        assert bad.size == 0, f"t0={t0}: {bad.size} mirror words differ from a fresh split, first at float {bad[0]}"
    print("worst |err| / bound:", {f"{k[0]}/{k[1]}": round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("cfg", OPT_CONFIGS[:1] + OPT_CONFIGS[2:])
def test_gradient_only_passes_change_nothing(cfg):
    """grad_on_batch (update = 0: at B = 32 Dense_0 and the head run the fused-Adam GEMM with its stores switched off) leaves the
    parameters, both moments, the count and the mirror bit-identical, with non-trivial moments planted."""
    eng, batch = _engine(cfg)
    real = _real(eng)
    rng = np.random.default_rng(5)
    m0, v0 = _plant(rng.normal(size=eng.n_param_floats).astype(np.float32) * 1e-3, real, 8, cfg["eps"], rng)
    eng.adam_m.copy_(torch.from_numpy(m0))
    eng.adam_v.copy_(torch.from_numpy(v0))
    eng.adam_count.fill_(7)
    eng.rebuild_mirror()
    before = [_bits(t) for t in (eng.params, eng.adam_m, eng.adam_v, eng.adam_count, eng.region("wsplit"))]
    grad = torch.zeros_like(eng.params)
    eng.grad_on_batch(batch, grad)
    torch.cuda.synchronize()
    assert np.abs(grad.cpu().numpy()).max() > 0
    after = [_bits(t) for t in (eng.params, eng.adam_m, eng.adam_v, eng.adam_count, eng.region("wsplit"))]
    for name, b, a in zip(("params", "adam_m", "adam_v", "adam_count", "mirror"), before, after):
        assert np.array_equal(a, b), name


# Gradient error model of the bf16x3 path.  Operands are split a = a_hi + a_lo (+ a residual below 2^-17 |a|, RNE) and the
# products a_hi b_hi + a_hi b_lo + a_lo b_hi are exact in the fp32 MFMA accumulator (the dropped a_lo b_lo is below 2^-18 |a b|);
# a sum of n of them in fp32 adds ~n' 2^-24 of its magnitude sum (n' the depth of the accumulation chains: K steps of 32, then
# the slab reduction).  So where both operands are exact, an element is within ~2^-16 of S = sum |dz| |x|, its terms' magnitude sum:
#   Conv_0's kernel: the frames are uint8 (exact in bf16: Conv_0 runs two passes), decoded by one fp32 multiply by fl(1/255) after
#     the sum; dz of Conv_0 is S8 (hi + lo of the fp32 value).  C_CONV0 = 2^-16.            measured max |d| / S: 3.4e-6 (K1), 7e-7
#   biases (sums of dz alone) and the upstream dz's own error (the chain above, each layer ~2^-16 of ITS magnitude sums, with
#     cancellation between them): C_ELEM = 2^-12.                                           measured max |d| / S: 1.1e-4 (Dense_0/bias, K1)
#   every other leaf reads an operand the forward computed (activations, xhat), whose own error is relative to the forward's
#     magnitude sums, not to |x|: near a ReLU edge an activation of 1e-7 may carry 1e-6.  No per-element scale of the gradient graph
#     bounds that, so those leaves keep the leaf-maximum bound of test_large_batch_kernel_variants (1e-4 of max |g|).
# None of these roundings prefers a sign: over a leaf of n elements the errors d_i average out, so the scale bias
# alpha = <d, g> / <g, g> and the offset beta = mean(d) / rms(g) are zero up to their spread
#   sd(alpha) = sqrt(sum (e_i g_i)^2) / <g, g>,  sd(beta) = sqrt(sum e_i^2) / (n rms(g)),  e_i = C S_i / sqrt(3)
# plus what IS common to every leaf: the float32 TD errors q - target (the forward's ~2e-5 on q, relative to TD errors of order 1)
# scale ALL gradients by one factor -- measured alpha -6e-6 .. +7e-6 with one sign per batch across all 18 leaves -- and fl(1/255)
# is (1/255)(1 - 2^-25.3).  Bound: 6 sd + SYSTEMATIC, SYSTEMATIC = 2^-15.  A Conv_0 decode scale off by 2^-12 (2.4e-4) moves its
# alpha by that much: its bound is 4.5e-5 - 7.1e-5 here (measured with that mutation: alpha = +2.4e-4 .. +2.5e-4).
C_CONV0, C_ELEM, SYSTEMATIC = 2.0**-16, 2.0**-12, 2.0**-15


def _elem_scale(mod, leaf):
    """the per-element constant C of the module comment (None: the leaf is held to 1e-4 of its maximum instead)"""
    if mod == "Conv_0" and leaf == "kernel":
        return C_CONV0
    if leaf == "bias" and not mod.startswith("LayerNorm"):
        return C_ELEM
    return None


GRAD_CASES = [
    pytest.param("K1", id="K1-fixture-B4"),
    pytest.param(32, id="headline-B32"),
    pytest.param(131, id="headline-B131-ragged-wgrad-groups"),
]


def _k1_agent():
    from tests.test_gpu_golden import _agent

    g = np.load(os.path.join(GOLD, "network_K1.npz"))
    agent, batch, K, A, B = _agent(g)
    return g, agent, batch, K, A, B


def _grad_case(case):
    """(engine, HIP gradient of one learn step, reference-layout batch, initial params, feats, K, A, B, lr, eps)"""
    from oracle import network as onet

    if case == "K1":
        g, agent, batch, K, A, B = _k1_agent()
        eng = agent._engine
        params = onet.init_params(int(g["seed"]), (84, 84, 4), [32, 64, 64, 512], "cnn", (1 + K) * A, True)
        grad = torch.zeros_like(eng.params)
        eng.learn_on_batch(agent._c_batch(eng, batch), grad_out=grad)
        return eng, grad, batch, params, (32, 64, 64, 512), K, A, B, float(g["lr"]), float(g["adam_eps"])
    feats, K, A, B = (32, 64, 64, 512), 3, 4, case
    oracle, eng, params = make_pair(feats, K, A, B, seed=7)
    frames, ids, action, reward, terminal, ref = make_frame_batch(B, A, seed=23, n_frames=B + 64)
    grad = torch.zeros_like(eng.params)
    eng.learn_on_batch(device_batch(eng, frames, ids, action, reward, terminal), grad_out=grad)
    return eng, grad, ref, params, feats, K, A, B, 1e-3, 1.5e-4


@pytest.mark.parametrize("case", GRAD_CASES)
def test_weight_gradients_elementwise_and_unbiased_against_float64(case):
    """(3) Conv_0's weight gradient (at these sizes the image-group kernel, conv_img.h conv_wgrad_img_kernel<.., U8 = true>: K = 256
    taps x 4 planes, one image per group, one slab per image reduced by adam_kernel) and every other leaf: |g_hip - g_ref| <=
    C * sum |dz| |x| element by element where the model gives one (_elem_scale), and the scale / offset bias alpha, beta of every
    leaf within the model's bound (comment above)."""
    eng, grad, ref, params, feats, K, A, B, lr, eps = _grad_case(case)
    torch.cuda.synchronize()
    z_hip = hip_preactivations(eng, B)
    want, scale = masked_reference_grads(params, feats, K, A, ref, z_hip, layer_norm=True, gamma_n=0.99, with_scales=True)
    got = eng.internal_to_flax_grads(grad)
    rows = []
    for mod in want:
        for leaf in want[mod]:
            gr = np.asarray(want[mod][leaf], np.float64).reshape(-1)
            gh = np.asarray(got[mod][leaf], np.float64).reshape(-1)
            S = np.asarray(scale[mod][leaf], np.float64).reshape(-1)
            d = gh - gr
            c = _elem_scale(mod, leaf)
            r = np.abs(d) / (c * S + 1e-30) if c else np.abs(d) / (1e-4 * np.abs(gr).max())
            e = (c or C_ELEM) * S / np.sqrt(3.0)
            gg = float(gr @ gr)
            rms = np.sqrt(gg / gr.size)
            alpha, beta = float(d @ gr) / gg, float(d.mean()) / rms
            a_bound = 6 * np.sqrt(float(((e * gr) ** 2).sum())) / gg + SYSTEMATIC
            b_bound = 6 * np.sqrt(float((e * e).sum())) / (gr.size * rms) + SYSTEMATIC
            rows.append((f"{mod}/{leaf}", "S" if c else "max", float(r.max()), alpha, a_bound, beta, b_bound))
    print(f"\n{case}: leaf  (element bound against)  max |d| / bound  alpha (bound)  beta (bound)")
    for name, kind, rmax, alpha, ab, beta, bb in rows:
        print(f"  {name} ({kind}): {rmax:.3f}  {alpha:+.2e} ({ab:.1e})  {beta:+.2e} ({bb:.1e})")
    for name, kind, rmax, alpha, ab, beta, bb in rows:
        assert abs(alpha) <= ab, f"{name}: scale bias alpha {alpha:.3e} > {ab:.3e}"
        assert abs(beta) <= bb, f"{name}: offset beta {beta:.3e} > {bb:.3e}"
        assert rmax <= 1.0, f"{name}: element error {rmax:.3f} of its bound ({kind})"


def _masks_of_the_float64_forward(params, ref, B):
    """The ReLU decisions of an independent float64 forward (what the fixture generator's oracle decided), online rows only."""
    import torch.nn.functional as F

    P = {m: {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in d.items()} for m, d in params.items()}
    x = torch.tensor(np.asarray(ref.state), dtype=torch.float64) / 255.0
    out = {}

    def ln(z, name):
        mean = z.mean(-1, keepdim=True)
        var = ((z * z).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
        return (z - mean) * torch.rsqrt(var + 1e-6) * P[name]["scale"] + P[name]["bias"]

    for i, (k, s) in enumerate(((8, 4), (4, 2), (3, 1))):
        size = x.shape[1]
        o = -(-size // s)
        tot = max((o - 1) * s + k - size, 0)
        xp = F.pad(x.permute(0, 3, 1, 2), (tot // 2, tot - tot // 2, tot // 2, tot - tot // 2))
        z = F.conv2d(xp, P[f"Conv_{i}"]["kernel"].permute(3, 2, 0, 1), P[f"Conv_{i}"]["bias"], stride=s).permute(0, 2, 3, 1)
        y = ln(z, f"LayerNorm_{i}")
        out[f"Conv_{i}"] = (y > 0).numpy().reshape(B, -1)
        x = torch.relu(y)
    z = x.reshape(B, -1) @ P["Dense_0"]["kernel"] + P["Dense_0"]["bias"]
    out["Dense_0"] = (ln(z, "LayerNorm_3") > 0).numpy()
    return out


def _hip_masks(params, z_hip):
    out = {}
    for name, ln_name in (("Conv_0", "LayerNorm_0"), ("Conv_1", "LayerNorm_1"), ("Conv_2", "LayerNorm_2"), ("Dense_0", "LayerNorm_3")):
        z = np.asarray(z_hip[name], np.float64)
        c = params[ln_name]["scale"].shape[0]
        zz = z.reshape(z.shape[0], -1, c)
        mean = zz.mean(-1, keepdims=True)
        var = np.maximum((zz * zz).mean(-1, keepdims=True) - mean * mean, 0)
        y = (zz - mean) / np.sqrt(var + 1e-6) * params[ln_name]["scale"] + params[ln_name]["bias"]
        out[name] = (y > 0).reshape(z.shape[0], -1)
    return out


def test_k1_first_adam_step_matches_the_mask_pinned_float64_step():
    """(4a) The K = 1 fixture's first learn step against float64 Adam applied to the float64 gradient with the HIP path's own ReLU
    decisions (mask-pinned): every leaf element within lr * dg * eps / (|g| + eps)^2, dg the gradient bound above (Adam's first step is lr g / (|g| +
    eps), whose slope in g is at most lr eps / (|g| + eps)^2) plus the Adam arithmetic of _adam_bounds; every leaf's sum within
    4 tol sqrt(n), tol = 0.02 lr (the bound test_gpu_golden held before it was loosened).
    (4b) The fixture was generated by a float64 forward that takes its own ReLU decisions: the decisions that differ from the HIP
    path's are counted, and the fixture's Conv_0 sum gap is shown to be the pinned step's own distance from the fixture."""
    from oracle.make_golden_network import SMALL

    g, agent, batch, K, A, B = _k1_agent()
    eng = agent._engine
    from oracle import network as onet

    params = onet.init_params(int(g["seed"]), (84, 84, 4), [32, 64, 64, 512], "cnn", (1 + K) * A, True)
    lr, eps = float(g["lr"]), float(g["adam_eps"])
    grad = torch.zeros_like(eng.params)
    eng.learn_on_batch(agent._c_batch(eng, batch), grad_out=grad)
    torch.cuda.synchronize()
    z_hip = hip_preactivations(eng, B)
    gref, scale = masked_reference_grads(params, [32, 64, 64, 512], K, A, batch, z_hip, layer_norm=True, gamma_n=float(g["gamma"]),
                                         with_scales=True)
    got = eng.export_flax()
    tol = 0.02 * lr
    lines = []
    for mod in gref:
        for leaf in gref[mod]:
            p0 = np.asarray(params[mod][leaf], np.float64)
            gr = np.asarray(gref[mod][leaf], np.float64)
            zero = np.zeros_like(gr)
            (p, _, _, _), (ep, _, _) = _adam_bounds(p0, zero, zero, gr, 1, lr, eps)
            c = _elem_scale(mod, leaf)
            dg = c * np.asarray(scale[mod][leaf]) if c else 1e-4 * np.abs(gr).max()  # the gradient bounds of the test above
            bound = lr * dg * eps / (np.abs(gr) + eps) ** 2 + ep
            d = np.asarray(got[mod][leaf], np.float64) - p
            assert np.all(np.abs(d) <= bound), (mod, leaf, float(np.abs(d).max()), float(bound.reshape(-1)[np.argmax(np.abs(d))]))
            s_hip, s_pin = float(got[mod][leaf].astype(np.float64).sum()), float(p.sum())
            assert abs(s_hip - s_pin) < 4 * tol * np.sqrt(p.size), (mod, leaf, s_hip - s_pin)
            if mod in SMALL and leaf == "kernel":
                s_fix = float(g[f"f64/after1/{mod}/{leaf}/sum"])
                # the fixture's gap is the pinned step's own distance from it (what test_gpu_golden's 0.5 tol n sum bound absorbs)
                assert abs((s_hip - s_fix) - (s_pin - s_fix)) < 4 * tol * np.sqrt(p.size), (mod, "fixture gap")
                lines.append(f"{mod}: hip - fixture {s_hip - s_fix:+.3e}, pinned - fixture {s_pin - s_fix:+.3e}, hip - pinned "
                             f"{s_hip - s_pin:+.2e} (bound {4 * tol * np.sqrt(p.size):.2e})")
    flips = {n: int((a != b).sum()) for (n, a), b in zip(_hip_masks(params, z_hip).items(), _masks_of_the_float64_forward(params, batch, B).values())}
    print("\nK1 first step:", *lines, f"ReLU decisions that differ from the float64 forward: {flips}", sep="\n  ")
