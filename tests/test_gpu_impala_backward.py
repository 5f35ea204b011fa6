"""The impala torso's backward and its BatchNorm sites, stage by stage on the run's own operands (csrc/impala.h: impala_backward;
csrc/batchnorm.h).  tests/test_gpu_impala.py holds the torso's forward, the pool backward and Conv_0's leaves to a float64 model of
each kernel; this file holds what lies between the top of a Stack and its pool: imp_to_s8_kernel with a ReLU mask, the SAME-padded
3x3 data gradients launch_conv_dgrad<32 | 64, passes>, imp_lnrelu_bwd_kernel and its in-place accumulation into the stream
gradient, the kernel and bias leaves of Conv_1 .. Conv_4, the block LayerNorms' leaves, and -- with BatchNorm -- the seven torso
sites forward and backward, Stack_0/Conv_0's data gradient, the running averages and the acting forward.

One run per (case, precision), cached for the module (impala_stages.BACKWARD_CASES / BACKWARD_RUNS: the smallest shapes that still
force each route; tests/test_impala_stages_host.py holds them to the real plan through plan_dump -- the plan accepts wide-20x20x2 as
written, Stacks 1 and 2 take launch_conv_fwd<64> and launch_conv_dgrad<64>):
  tiny-ln-B4 (84x84x4, 8/16/16/24)        7056 rows: the row kernels' grid-stride loop twice           bf16x3, bf16
  nonsquare-44x36x3-noln-B2               C_p 16 / 24 / 16, a ragged last 16-row block, H != W         bf16x3
  wide-20x20x2-ln-B3 (16/40/64/24)        C_p 40 and 64: the <64> forward and data-gradient templates  bf16x3, bf16
  bn-84x84x4-noln-B2 (8/16/8/32)          BatchNorm; the 2B-row backward has 7056 rows                 bf16x3
  bn-44x36x3-ln-B3 (12/20/9/16)           BatchNorm + LayerNorm, C < Cp at every site (3 / 8 at input) bf16x3, bf16
Without BatchNorm: loss_on_batch, grad_on_batch(batch, g).  With it: loss_on_batch, learn_on_batch(batch, grad_out=g), then the acting
forward of all 2B rows and of row 3 alone.  The workspace is copied after each call; every row reads those copies.

What impala_backward leaves in place (read off csrc/impala.h): dz/Impala; the stream gradient at each Stack's pool output, g_pool(s) =
imp/s2/dr for s = 2 and the head of imp/s{s+1}/da for s < 2; imp/s{s}/dzs (last written as the split of dz0); gw{k}, bpart{k},
lnpart{b}; every bn/<site>/dbias, dscale, mean, var, out; with BatchNorm imp/s0/da as Stack_0/Conv_0's data gradient left it.  da
and dzs inside a Stack are rewritten and the stream gradient is accumulated in place, so each Stack is ONE chain between two stored
anchors -- top: float(dz/Impala) for s = 2, else the model of Stack_{s+1}/Conv_0's data gradient on the run's own imp/s{s+1}/dzs;
bottom: the run's own g_pool(s) -- and never crosses a Stack (below g_pool the dz0 row of tests/test_gpu_impala.py takes over).

test_impala_backward_chains_match_a_model_of_each_stage, per Stack, block 1 then block 0 (impala_stages.block_backward: float64
models of to_s8_masked, bf16_model.conv_wgrad / conv_dgrad at the run's pass count, batchnorm_stages.bn_backward,
bf16_model.ln_relu_bwd, the in-place +=; every bound first order: E carried through the contraction with magnitudes, + the stage's
own bound(S, c), c from the route -- data gradient K = 9 cout_p with no split, weight gradient conv_wgrad_slabs' K steps and slabs,
column sums per-lane rows + 16 row groups + workgroups; a modelled operand that is split again carries an error only where
[v - E, v + E] crosses a rounding boundary of its planes: impala_stages.model_planes):
  Conv_{2+2b} bias leaf     ~ column sums of the stream gradient            (Stack 2, block 1: of dz/Impala itself -- no pass count, no control)
  Conv_{2+2b} kernel leaf   ~ conv_wgrad(own a2_b planes, split(stream gradient))
  Conv_{1+2b} bias, kernel  ~ the same behind the run's own ReLU mask a2_b > 0 (hi half), on own a1_b (BatchNorm: own bn/<site>/out)
  bn/Stack_s/BatchNorm_b/dbias, dscale ~ bn_backward(own a1_b, da, own mean / var, scale), E_dy carried; dx from the run's own sums;
                              the scale and bias leaves of g equal the two regions bit for bit
  Stack_s/LayerNorm_b leaves ~ bf16_model.ln_param_grads(own r_b, own mask a1_b > 0, da, E_da, chain)
  g_pool(s), after block 0  ~ the chain's stream gradient within the carried bound; padded channels exactly 0
  control of every row: the same chain at the other pass count at least 4x further away in the 2-norm.
And one row outside the chains: dz/Impala ~ ln_relu_bwd(own z/Impala, own act/Impala > 0, da), da the model of Dense_0's data gradient on
the run's own dz/Dense_0, with BatchNorm through the feature site behind the flatten (its dbias / dscale rows, dx on its own sums).
Every row is asserted in both precisions.  A bound carried through six single-pass stages would say nothing if every split of a
modelled operand were charged a bf16 ulp; model_planes charges it only where hi can flip, and the single-pass chains then hold with
the margins below.

test_impala_batchnorm_sites_forward_backward_running_and_acting (the three BatchNorm runs; every operand the run's own):
  forward, 2B rows: bn/x0 == split_words(uint8 / 255) bit for bit; every site's mean, var ~ bn_stats(own input), out ~ bn_apply(own
  input, own mean / var), padded channels 0, well-formed S8 (all nine sites: input, six block sites, flatten, Dense_0); z0 of
  Stack 0 ~ conv(own input-site out) + bias; every a2_b ~ relu(conv(own block-site out) + bias)
  imp/s0/da as left ~ conv_dgrad(own imp/s0/dzs, split(W)), other pass count outside the bound on >= 50 % of the elements
  input site dbias, dscale ~ s1, s2 of bn_backward(own bn/x0, own imp/s0/da)
  every site: scale / bias leaves of g == dscale / dbias regions bit for bit; running mean / var after the step within 2 ulp
  acting forward, 2B rows and row 3 alone: every site's out ~ bn_apply(own input, updated running averages); q ~ the head on the
  last site's out, other pass count outside the bound on >= 50 % of the elements.

Measured on the MI355X (max |d| / bound over the runs; control = smallest |run - other passes| / |run - own| in the 2-norm, asserted
>= 4; share = smallest share of elements the other pass count leaves outside the bound):
  row                        bf16x3 (5 runs)              bf16 (3 runs)
  Conv_{2+2b} bias           0.029, control 810x          0.021, control 7499x
  Conv_{2+2b} kernel         0.242, control 1222x         0.104, control 1200x
  Conv_{1+2b} bias           0.012, control 1002x         0.007, control 1218x
  Conv_{1+2b} kernel         0.136, control 912x          0.072, control 164x
  block site dbias / dscale  0.003 / 0.003, control 1231x 0.003 / 0.003, control 140x
  LayerNorm_b scale / bias   0.001 / 0.001, control 622x  0.002 / 0.005, control 159x
  g_pool                     0.125 (no LayerNorm), 0.002 (LayerNorm), control 1365x      0.047, control 465x
  dz/Impala                  0.740 (no LayerNorm: S8 storage), 0.383, control 879x, share 95 %   0.372, control 945x, share 93 %
  feature site dbias / dscale 0.030 / 0.041               0.026 / 0.053
  site mean / var / out      0.107 / 0.077 / 0.955 (S8 storage's worst case)             the same
  z0 on the input site's out 0.139, control 27684x, share 100 %                          0.076, share 100 %
  a2_b on the block site's out 0.704 (S8 storage), control 621x, share 37 % (behind a ReLU: 2-norm only)   0.655, control 828x
  imp/s0/da as left          0.144, control 27835x, share 100 %                          0.056, share 100 %
  input site dbias / dscale  0.089 / 0.078                0.094 / 0.066
  running mean / var         0.000 of 2 ulp (bit-equal to the fp32 expression)           the same
  acting out / q             0.955 / 0.053, q control 30033x, share 97 %                 0.952 / 0.042, share 100 %
Reported, not asserted: the elementwise control on the chain rows.  The share of elements the other pass count leaves outside the
carried bound is 0 % on every leaf (sums over thousands of rows) and on g_pool with LayerNorm, 5 .. 44 % on g_pool without (behind a
ReLU); ln_relu_bwd's worst-case row-statistics terms put the carried bound above the 2^-9 the pass counts differ by.  No nearer
anchor exists (da and the stream gradient are rewritten in place), so g_pool's control is the 2-norm (>= 465x), like the leaves'.
No row is above 1 and no kernel defect was found.
Times: the slowest run is tiny-ln-B4-bf16x3 at 1.4 s (it pays the process's first launches), every other run 0.06 .. 0.10 s, the file
4.3 s; the yardstick -- the slowest run of test_impala_stages_match_a_model_of_each_kernel_on_its_own_operands on the same machine -- is 1.7 s.

Mutations (arithmetic only, scratch copies of csrc/impala.h, one library each, one run of this file each; none is committed).  Failing
runs of this file, the first rows that fail / what fails in tests/test_gpu_impala.py and the impala tests of tests/test_gpu_batchnorm.py:
  imp_to_s8_kernel ignores its mask              all 8 chain runs: Conv_{1+2b} bias and kernel of every block, then everything below /
                                                 the oracle test (4 shapes), flat-frames stage run, both BatchNorm oracle shapes
  imp_lnrelu_bwd_kernel stores out without base  all 8 chain runs: g_pool and every leaf below the first block / the same 7
  the same kernel adds dg without the xhat factor the 6 LayerNorm chain runs: the six LayerNorm_b scale leaves / oracle test (3 LayerNorm
                                                 shapes), flat-frames run, the LayerNorm BatchNorm shape
  <64> data gradient at the other pass count     wide-20x20x2 in bf16x3 AND bf16 (2-norm control of the rows below Stack 2's first
                                                 data gradient; Conv_3 leaves outside the bound) / the reference-widths oracle shape,
                                                 bf16x3 only: before this file nothing ran launch_conv_dgrad<64, 1>
  bn_site_backward(apply = false) at a block site the 3 BatchNorm chain runs: g_pool and every leaf below / both BatchNorm oracle shapes
  input site's sums over half the rows           the 3 site runs: BatchNorm_0 dbias and dscale, nothing else / both BatchNorm oracle shapes
So in bf16x3 the end-to-end comparisons (2e-4 per leaf against pinned decisions, 5e-2 of a leaf's largest entry with BatchNorm) also
see mutations this gross; what they cannot do is name the stage, run in single-pass bf16, or see an error inside their tolerance."""
import ctypes

import numpy as np
import pytest
import torch

from tests.gpu_helpers import device_batch, make_frame_batch, make_pair
from tests.helpers import batchnorm_stages as BS
from tests.helpers import bf16_model as M
from tests.helpers import impala_stages as IS

pytestmark = pytest.mark.gpu

RUNS = [pytest.param(c, p, id=f"{c}-{p}") for c, p in IS.BACKWARD_RUNS]
BN_RUNS = [pytest.param(c, p, id=f"{c}-{p}") for c, p in IS.BACKWARD_RUNS if IS.BACKWARD_CASES[c]["bn"]]
PARAM_SEED, BATCH_SEED = 3, 7
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_runs():
    yield
    _CACHE.clear()


class _Snap:
    """the workspace as one call left it: regions by name, as QNetEngine.region reads them"""

    def __init__(self, eng):
        self.eng, self.ws = eng, eng.workspace.clone()

    def region(self, name):
        from slimdqn import _hip

        off, size = ctypes.c_int64(), ctypes.c_int64()
        _hip.check(self.eng.lib.isdqn_net_workspace_region(ctypes.byref(self.eng.cfg), name.encode(), ctypes.byref(off), ctypes.byref(size)))
        return self.ws[off.value // 4 : (off.value + size.value) // 4]


def _run(case, precision):
    """One run per (case, precision): loss_on_batch, then grad_on_batch(batch, g) -- with BatchNorm learn_on_batch(batch, grad_out=g)
    and the acting forward of all 2B rows and of row 3 alone -- and the workspace as each call left it."""
    key = (case, precision)
    if key in _CACHE:
        return _CACHE[key]
    cfg = IS.BACKWARD_CASES[case]
    feats, obs, K, A, B, ln, bn = (cfg[k] for k in ("feats", "obs", "K", "A", "B", "ln", "bn"))
    _, eng, params = make_pair(feats, K, A, B, arch="impala", obs=obs, layer_norm=ln, seed=PARAM_SEED, lr=1e-3, precision=precision, batch_norm=bn)
    frames, ids, action, reward, terminal, _ = make_frame_batch(B, A, seed=BATCH_SEED, h=obs[0], w=obs[1], stack=obs[2])
    batch = device_batch(eng, frames, ids, action, reward, terminal)
    run = dict(case=case, precision=precision, cfg=cfg, eng=eng, params=params, frames=frames, ids=ids, N=2 * B if bn else B,
               passes=(3, 1) if precision == "bf16x3" else (1, 3), geo=IS.geometry(obs, feats))
    run["p_before"] = eng.params.clone()
    eng.loss_on_batch(batch)
    g = torch.zeros_like(eng.params)
    if bn:
        torch.cuda.synchronize()
        assert torch.equal(eng.params.view(torch.int32), run["p_before"].view(torch.int32)), "loss_on_batch changed the parameter buffer"
        eng.learn_on_batch(batch, grad_out=g)
    else:
        eng.grad_on_batch(batch, g)
    torch.cuda.synchronize()
    run.update(g=g, hip_g=eng.internal_to_flax_grads(g), learn=_Snap(eng), p_after=eng.params.clone())
    if bn:
        stack = obs[2]
        dev = eng.params.device
        flat_ids = np.concatenate([ids[:, :stack], ids[:, stack:]], 0).copy()
        fwd = lambda rows: eng.forward(frames=batch._keep[0], frame_stride=frames.shape[1],
                                       frame_ids=torch.from_numpy(flat_ids[rows].copy()).to(dev), n_rows=len(flat_ids[rows]))
        run["acting"] = []
        for rows in (slice(0, 2 * B), slice(3, 4)):
            q = fwd(rows).double()
            torch.cuda.synchronize()
            run["acting"].append((rows, q, _Snap(eng)))
        run["p1"] = eng.export_flax()
    _CACHE[key] = run
    return run


class _Rows:
    """Every comparison goes through bf16_model.check; a failing row is kept and the test fails at its end with all of them, so one
    run names every stage that is off.  Per row: max |d| / bound, and against the same chain at the other pass count the ratio
    |run - other| / |run - own| (2-norm; asserted >= 4 by check) and the share of elements the other model leaves outside the bound
    (asserted >= 50 % where `elementwise`)."""

    def __init__(self, tag):
        self.tag, self.usage, self.report, self.failures = tag, {}, [], []

    def check(self, row, label, got, want, bnd, S=None, alt=None, elementwise=False):
        got, want, bnd = (torch.as_tensor(t, dtype=torch.float64) for t in (got, want, bnd))
        assert got.shape == want.shape == bnd.shape, (label, got.shape, want.shape, bnd.shape)
        d = (got - want).abs()
        pos = bnd > 0
        used = float((d[pos] / bnd[pos]).max()) if bool(pos.any()) else 0.0
        if bool((d[~pos] > 0).any()):
            used = float("inf")
        ctrl = share = None
        if alt is not None:
            o = (got - torch.as_tensor(alt, dtype=torch.float64)).abs()
            ctrl = float(torch.linalg.vector_norm(o)) / max(float(torch.linalg.vector_norm(d)), 1e-300)
            share = float((o[pos] > bnd[pos]).double().mean()) if bool(pos.any()) else 0.0
        try:
            M.check(got, want, bnd, S, alt, elementwise_control=elementwise, label=label)
        except AssertionError as e:
            self.failures.append(str(e))
        u = self.usage.setdefault(row, [0.0, float("inf"), 1.0])
        u[0] = max(u[0], used)
        if ctrl is not None:
            u[1], u[2] = min(u[1], ctrl), min(u[2], share)
        self.report.append(f"{label}: max |d| / bound = {used:.3f}" + (f", |run - other| / |run - own| = {ctrl:.1f}, other passes outside: {share:.0%}"
                                                                      if ctrl is not None else ""))

    def require(self, ok, message):
        if not ok:
            self.failures.append(message)

    def finish(self):
        print()
        for line in self.report:
            print("  " + line)
        for row, (used, ctrl, share) in self.usage.items():
            print(f"  USAGE {self.tag} {row}: max |d| / bound = {used:.3f}" + (f", control >= {ctrl:.1f}x, other passes outside >= {share:.0%}"
                                                                            if ctrl != float("inf") else ""))
        assert not self.failures, f"{len(self.failures)} rows failed:\n" + "\n".join(self.failures)


def _tools(run):
    eng, params, snap = run["eng"], run["params"], run["learn"]
    dev = eng.params.device
    vec = lambda mod, leaf: torch.from_numpy(np.asarray(params[mod][leaf], np.float64)).to(dev)
    wsplit = lambda mod: M.split(torch.from_numpy(np.asarray(params[mod]["kernel"])).to(dev))
    leaf = lambda mod, name: torch.from_numpy(np.asarray(run["hip_g"][mod][name], np.float64)).to(dev)
    return dev, vec, wsplit, leaf


def _s8(rows_, snap, name, n_rows, pitch, c, shape):
    """planes (hi, lo) of the first n_rows rows of an S8 tensor, true channels, shaped: well-formed words, padded channels 0"""
    hi, lo = M.s8_planes(snap.region(name), n_rows, pitch)
    rows_.require(int(M.s8_malformed(hi, lo).sum()) == 0, f"{name}: elements that are not a nearest-even split")
    hi, lo = hi.reshape(*shape, pitch), lo.reshape(*shape, pitch)
    if c < pitch:
        rows_.require(float(hi[..., c:].abs().max()) == 0.0 and float(lo[..., c:].abs().max()) == 0.0, f"{name}: padded channels are not 0")
    return hi[..., :c], lo[..., :c]


def _site_groups(run, site, leaf, src):
    """the G internal groups of a site's scale / bias / mean / var in a parameter-shaped buffer"""
    offs = run.setdefault("offs", {i.name.decode(): int(i.offset) for i in run["eng"].infos})
    o = offs[f"{site['name']}/{leaf}"]
    return src[o : o + site["G"]]


def _block_site(run, s, b, N):
    """the operands of a block's BatchNorm site for block_backward: its own input a1 [N][P][Cp], own batch statistics and sums"""
    snap = run["learn"]
    site = next(t for t in run["sites"] if t["name"] == f"Stack_{s}/BatchNorm_{b}")
    P_, Cp = site["P"], site["Cp"]
    x = sum(M.s8_planes(snap.region(site["src"]), N * P_, Cp)).reshape(N, P_, Cp)
    reg = lambda name: snap.region(site["prefix"] + name)[: site["G"]].double()
    return site, dict(x=x, mean=reg("mean"), var=reg("var"), scale=_site_groups(run, site, "scale", run["p_before"]).double(), s1=reg("dbias"), s2=reg("dscale"))


def _stack_chain(run, rows_, s, p):
    """Stack s between its two anchors at p passes: the top gradient (dz/Impala for s = 2, else the model of Stack_{s+1}/Conv_0's data
    gradient on the run's own imp/s{s+1}/dzs), then block 1 and block 0 through impala_stages.block_backward on the run's own forward
    tensors.  Returns [block 1, block 0]."""
    dev, vec, wsplit, _ = _tools(run)
    snap, geo, N, cfg = run["learn"], run["geo"], run["N"], run["cfg"]
    g = geo[s]
    Hp, Wp, C, C_p = g["Hp"], g["Wp"], g["C"], g["C_p"]
    small = N * Hp * Wp
    if s == 2:
        G = sum(_s8(rows_, snap, "dz/Impala", small, C_p, C, (N, Hp, Wp)))
        E = torch.zeros_like(G)
    else:
        n = geo[s + 1]
        dzs = _s8(rows_, snap, f"imp/s{s + 1}/dzs", N * n["H"] * n["W"], n["C_p"], n["C"], (N, n["H"] * n["W"]))
        G, S = M.conv_dgrad(p, dzs, wsplit(f"Stack_{s + 1}/Conv_0"), (n["H"], n["W"]), 1)
        G, E = G.reshape(N, Hp, Wp, C), M.bound(S, IS.dgrad_depth(n["C_p"])).reshape(N, Hp, Wp, C)
    out = []
    for b in (1, 0):
        pre = f"imp/s{s}/"
        r = snap.region(pre + f"r{b}")[: small * C_p].reshape(N, Hp, Wp, C_p)[..., :C].double()
        a1 = _s8(rows_, snap, pre + f"a1_{b}", small, C_p, C, (N, Hp, Wp))
        a2 = _s8(rows_, snap, pre + f"a2_{b}", small, C_p, C, (N, Hp, Wp))
        x1, site = a1, None
        if cfg["bn"]:
            st, site = _block_site(run, s, b, N)
            x1 = _s8(rows_, snap, st["prefix"] + "out", small, C_p, C, (N, Hp, Wp))
        gamma = vec(f"Stack_{s}/LayerNorm_{b}", "scale") if cfg["ln"] else None
        res = IS.block_backward(p, G, E, r, a1[0] > 0, x1, a2, wsplit(f"Stack_{s}/Conv_{1 + 2 * b}"), wsplit(f"Stack_{s}/Conv_{2 + 2 * b}"), gamma,
                                cfg["ln"], bn=site)
        out.append(res)
        G, E = res["G_out"], res["E_G_out"]
    return out


@pytest.mark.parametrize("case,precision", RUNS)
def test_impala_backward_chains_match_a_model_of_each_stage(case, precision):
    """See the module docstring: per Stack one chain of float64 stage models between two anchors the run itself stored, every leaf
    and the bottom anchor within the carried bound, the same chain at the other pass count as the negative control."""
    run = _run(case, precision)
    cfg, geo, N, snap = run["cfg"], run["geo"], run["N"], run["learn"]
    own, other = run["passes"]
    rows_ = _Rows(f"{case}-{precision}")
    dev, vec, wsplit, leaf = _tools(run)
    if cfg["bn"]:
        run["sites"] = BS.site_layout(dict(cfg, n_heads=1 + cfg["K"]))
    ln, bn = cfg["ln"], cfg["bn"]

    for s in (2, 1, 0):
        g = geo[s]
        Hp, Wp, C, C_p = g["Hp"], g["Wp"], g["C"], g["C_p"]
        mine, alt = _stack_chain(run, rows_, s, own), _stack_chain(run, rows_, s, other)
        for b, res, res_o in zip((1, 0), mine, alt):
            top = s == 2 and b == 1  # the operands of these rows are the run's own: dz/Impala and a2_1
            k2, k1 = f"Stack_{s}/Conv_{2 + 2 * b}", f"Stack_{s}/Conv_{1 + 2 * b}"
            # the bias leaf above the top anchor of Stack 2 sums dz/Impala itself: no pass count enters, so no control
            rows_.check("Conv_2+2b/bias", f"s{s}/Conv_{2 + 2 * b}/bias", leaf(k2, "bias"), res["bias2"], res["E_bias2"], None,
                        None if top else res_o["bias2"])
            rows_.check("Conv_2+2b/kernel", f"s{s}/Conv_{2 + 2 * b}/kernel", leaf(k2, "kernel"), res["gw2"], res["E_gw2"], None, res_o["gw2"])
            rows_.check("Conv_1+2b/bias", f"s{s}/Conv_{1 + 2 * b}/bias", leaf(k1, "bias"), res["bias1"], res["E_bias1"], None, res_o["bias1"])
            rows_.check("Conv_1+2b/kernel", f"s{s}/Conv_{1 + 2 * b}/kernel", leaf(k1, "kernel"), res["gw1"], res["E_gw1"], None, res_o["gw1"])
            if bn:
                site = next(t for t in run["sites"] if t["name"] == f"Stack_{s}/BatchNorm_{b}")
                reg = lambda name: snap.region(site["prefix"] + name)[: site["G"]]
                rows_.check("BatchNorm_b/dbias", f"{site['name']}/dbias", reg("dbias").double(), res["s1"], res["E_s1"], None, res_o["s1"])
                rows_.check("BatchNorm_b/dscale", f"{site['name']}/dscale", reg("dscale").double(), res["s2"], res["E_s2"], None, res_o["s2"])
                for lf, name in (("scale", "dscale"), ("bias", "dbias")):
                    rows_.require(torch.equal(_site_groups(run, site, lf, run["g"]).view(torch.int32), reg(name).view(torch.int32)),
                                  f"{site['name']}/{lf} of g is not the {name} region")
            if ln:
                mod = f"Stack_{s}/LayerNorm_{b}"
                rows_.check("LayerNorm_b/scale", f"s{s}/LayerNorm_{b}/scale", leaf(mod, "scale"), res["dgamma"], res["E_dgamma"], None, res_o["dgamma"])
                rows_.check("LayerNorm_b/bias", f"s{s}/LayerNorm_{b}/bias", leaf(mod, "bias"), res["dbeta"], res["E_dbeta"], None, res_o["dbeta"])
        # the bottom anchor: what the two blocks left of the stream gradient, as the pool backward reads it
        g_pool = snap.region("imp/s2/dr" if s == 2 else f"imp/s{s + 1}/da")[: N * Hp * Wp * C_p].reshape(N, Hp, Wp, C_p)
        rows_.require(float(g_pool[..., C:].abs().max() if C < C_p else 0.0) == 0.0, f"g_pool({s}): padded channels are not 0")
        rows_.check("g_pool", f"s{s}/g_pool", g_pool[..., :C].double(), mine[1]["G_out"], mine[1]["E_G_out"], None, alt[1]["G_out"])

    # ---- the row under the first Dense: dz/Impala from the model of Dense_0's data gradient on the run's own dz/Dense_0
    T = geo[2]
    P_, C, C_p = T["Hp"] * T["Wp"], T["C"], T["C_p"]
    d0, d0_p = int(cfg["feats"][3]), -(-int(cfg["feats"][3]) // 8) * 8
    z = snap.region("z/Impala")[: N * P_ * C_p].reshape(N, P_, C_p)[..., :C].double()
    act = _s8(rows_, snap, "act/Impala", N * P_, C_p, C, (N, P_))
    got = sum(_s8(rows_, snap, "dz/Impala", N * P_, C_p, C, (N, P_)))
    gamma = vec("LayerNorm_0", "scale") if ln else None

    def under_dense(p):
        dz = tuple(t[:, :d0] for t in M.s8_planes(snap.region("dz/Dense_0"), N, d0_p))
        da, S = M.dense(p, dz, tuple(t.T for t in wsplit("Dense_0")))
        da, E_da = da.reshape(N, P_, C), M.bound(S, M.chain_depth(d0_p, epilogue=3)).reshape(N, P_, C)
        if bn:  # through the feature site behind the flatten, on the run's own sums
            site = next(t for t in run["sites"] if t["src"] == "act/Impala")
            x = sum(M.s8_planes(snap.region("act/Impala"), N * P_, C_p)).reshape(N, P_, C_p)
            reg = lambda name: snap.region(site["prefix"] + name)[: site["G"]].double()
            scale = _site_groups(run, site, "scale", run["p_before"]).double()
            dy, E_dy = BS._pad_channels(da, C_p), BS._pad_channels(E_da, C_p)
            s1, d_s1, s2, d_s2, _, _ = BS.bn_backward(x, dy, reg("mean"), reg("var"), scale, False, C, E_dy=E_dy)
            _, _, _, _, dx, d_dx = BS.bn_backward(x, dy, reg("mean"), reg("var"), scale, False, C, E_dy=E_dy, s1=reg("dbias"), s2=reg("dscale"))
            if p == own:
                rows_.check("feature site dbias", f"{site['name']}/dbias", reg("dbias"), s1, d_s1)
                rows_.check("feature site dscale", f"{site['name']}/dscale", reg("dscale"), s2, d_s2)
            da, E_da = dx[..., :C], d_dx[..., :C]
        return M.ln_relu_bwd(z, gamma, ((act[0] + act[1]) > 0).double(), da, E_da, has_ln=ln)

    want, E = under_dense(own)
    rows_.check("dz/Impala", "dz/Impala", got, want, E, None, under_dense(other)[0])
    rows_.finish()


@pytest.mark.parametrize("case,precision", BN_RUNS)
def test_impala_batchnorm_sites_forward_backward_running_and_acting(case, precision):
    """BatchNorm cases only; every row's operands are the run's own, so every row is asserted in both precisions.  See the module
    docstring for the rows."""
    from tests.helpers.conv_routes import fwd_splits

    run = _run(case, precision)
    cfg, geo, N2, snap, eng = run["cfg"], run["geo"], run["N"], run["learn"], run["eng"]
    own, other = run["passes"]
    rows_ = _Rows(f"{case}-{precision}")
    dev, vec, wsplit, leaf = _tools(run)
    sites = run["sites"] = BS.site_layout(dict(cfg, n_heads=1 + cfg["K"]))
    layers = BS.layers(dict(cfg, n_heads=1 + cfg["K"]))
    h, w, stack = cfg["obs"]
    B, A, K = cfg["B"], cfg["A"], cfg["K"]
    nha = (1 + K) * A
    nha_p = -(-nha // 8) * 8
    frames, ids = run["frames"], run["ids"]
    x0 = IS.frames_to_x(torch.from_numpy(frames).to(dev), IS.paired_ids(ids, stack), h, w, stack)

    def site_planes(sn, s, which, n):
        name = s["src"] if which == "src" else s["prefix"] + "out"
        hi, lo = M.s8_planes(sn.region(name), n, s["P"] * s["Cp"])
        rows_.require(int(M.s8_malformed(hi, lo).sum()) == 0, f"{name}: elements that are not a nearest-even split")
        return tuple(t.reshape(n, s["P"], s["Cp"]) for t in (hi, lo))

    def conv_row(row, label, x, mod, got, relu, src=None):
        wt = wsplit(mod) if src is None else M.split(torch.from_numpy(np.asarray(src[mod]["kernel"])).to(dev))
        b = vec(mod, "bias") if src is None else torch.from_numpy(np.asarray(src[mod]["bias"], np.float64)).to(dev)
        c = M.chain_depth(9 * (-(-x[0].shape[-1] // 8) * 8), 1, 2)
        v, S = M.conv(own, x, wt, 1)
        alt, _ = M.conv(other, x, wt, 1)
        want, alt, S = v + b, alt + b, S + b.abs()
        bnd = M.bound(S, c)
        if relu:
            want, alt = want.clamp_min(0), alt.clamp_min(0)
            bnd = bnd + M.S8_STORE * want + M.FLOOR
        rows_.check(row, label, got, want.reshape(got.shape), bnd.reshape(got.shape), S.reshape(got.shape), alt.reshape(got.shape), elementwise=not relu)

    # ---------------------------------------------------------------- forward, all 2B rows
    rows_.require(torch.equal(snap.region("bn/x0")[: N2 * h * w * 8].view(torch.int32), M.split_words(x0)), "bn/x0 is not the S8 split of uint8 / 255")
    outs = {}
    for s in sites:
        x = sum(site_planes(snap, s, "src", N2))
        mean, var, d_mean, d_var = BS.bn_stats(x, s["spatial"], s["C"])
        reg = lambda name: snap.region(s["prefix"] + name)[: s["G"]].double()
        rows_.check("mean", f"{s['name']}/mean", reg("mean"), mean, d_mean)
        rows_.check("var", f"{s['name']}/var", reg("var"), var, d_var)
        y, E = BS.bn_apply(x, reg("mean"), reg("var"), _site_groups(run, s, "scale", run["p_before"]).double(),
                           _site_groups(run, s, "bias", run["p_before"]).double(), s["spatial"], s["C"])
        out = outs[s["name"]] = site_planes(snap, s, "out", N2)
        if s["C"] < s["Cp"]:
            rows_.require(all(float(t[..., s["C"]:].abs().max()) == 0.0 for t in out), f"{s['name']}/out: padded channels are not 0")
        rows_.check("out", f"{s['name']}/out", sum(out), y, E)
    g0 = geo[0]
    z0 = snap.region("imp/s0/z0")[: N2 * h * w * g0["C_p"]].reshape(N2, h * w, g0["C_p"])
    xin = tuple(t.reshape(N2, h, w, 8)[..., :stack] for t in outs["BatchNorm_0"])
    conv_row("z0", "s0/z0 on the input site's out", xin, "Stack_0/Conv_0", z0[..., : g0["C"]].double(), False)
    for s, g in enumerate(geo):
        for b in range(2):
            shape = (N2, g["Hp"], g["Wp"])
            x1 = tuple(t.reshape(*shape, g["C_p"])[..., : g["C"]] for t in outs[f"Stack_{s}/BatchNorm_{b}"])
            a2 = sum(_s8(rows_, snap, f"imp/s{s}/a2_{b}", N2 * g["Hp"] * g["Wp"], g["C_p"], g["C"], (N2, g["Hp"] * g["Wp"])))
            conv_row("a2", f"s{s}/a2_{b} on the block site's out", x1, f"Stack_{s}/Conv_{1 + 2 * b}", a2, True)

    # ---------------------------------------------------------------- Stack_0/Conv_0's data gradient and the input site's sums
    s_in = sites[0]
    dzs = _s8(rows_, snap, "imp/s0/dzs", N2 * h * w, g0["C_p"], g0["C"], (N2, h * w))
    da, S = M.conv_dgrad(own, dzs, wsplit("Stack_0/Conv_0"), (h, w), 1)
    alt, _ = M.conv_dgrad(other, dzs, wsplit("Stack_0/Conv_0"), (h, w), 1)
    own_da = snap.region("imp/s0/da")[: N2 * h * w * 8].reshape(N2, h * w, 8).double()
    pad = lambda t: BS._pad_channels(t.reshape(N2, h * w, stack), 8)
    rows_.check("imp/s0/da as left", "imp/s0/da (data gradient into Stack_0/Conv_0's input)", own_da, pad(da), pad(M.bound(S, IS.dgrad_depth(g0["C_p"]))),
                pad(S), pad(alt), elementwise=True)
    x = sum(site_planes(snap, s_in, "src", N2))
    reg = lambda name: snap.region(s_in["prefix"] + name)[: s_in["G"]].double()
    s1, d_s1, s2, d_s2, _, _ = BS.bn_backward(x, own_da, reg("mean"), reg("var"), _site_groups(run, s_in, "scale", run["p_before"]).double(), True, stack)
    rows_.check("input site dbias", "BatchNorm_0/dbias (own da)", reg("dbias"), s1, d_s1)
    rows_.check("input site dscale", "BatchNorm_0/dscale (own da)", reg("dscale"), s2, d_s2)
    # an input site summed over B rows' worth of inv_m, or a da already divided: s1 / s2 above are plain sums, so any factor shows

    # ---------------------------------------------------------------- leaves of g, running averages
    for s in sites:
        for lf, name in (("scale", "dscale"), ("bias", "dbias")):
            rows_.require(torch.equal(_site_groups(run, s, lf, run["g"]).view(torch.int32), snap.region(s["prefix"] + name)[: s["G"]].view(torch.int32)),
                          f"{s['name']}/{lf} of g is not the {name} region")
        for lf in ("mean", "var"):
            want, ulp2 = BS.running(_site_groups(run, s, lf, run["p_before"]).cpu().numpy(), snap.region(s["prefix"] + lf)[: s["G"]].cpu().numpy())
            got = _site_groups(run, s, lf, run["p_after"]).cpu().numpy().astype(np.float64)
            rows_.check(f"running {lf}", f"{s['name']} running {lf}", torch.from_numpy(got), torch.from_numpy(want.astype(np.float64)), torch.from_numpy(ulp2))

    # ---------------------------------------------------------------- acting: each site on the updated running averages
    p1, after = run["p1"], run["p_after"]
    head = f"Dense_{len(layers) - 1}"
    for rows, q, sn in run["acting"]:
        n = len(range(N2)[rows])
        tag = f"acting ({n} rows)"
        rows_.require(torch.equal(sn.region("bn/x0")[: n * h * w * 8].view(torch.int32), M.split_words(x0[rows])), f"{tag}: bn/x0")
        cur = None
        for s in sites:
            x = sum(site_planes(sn, s, "src", n))
            y, E = BS.bn_apply(x, *(_site_groups(run, s, k, after).double() for k in ("mean", "var", "scale", "bias")), s["spatial"], s["C"])
            cur = site_planes(sn, s, "out", n)
            if s["C"] < s["Cp"]:
                rows_.require(all(float(t[..., s["C"]:].abs().max()) == 0.0 for t in cur), f"{tag} {s['name']}/out: padded channels are not 0")
            rows_.check("acting out", f"{tag} {s['name']}/out", sum(cur), y, E)
        last = sites[-1]
        xin = tuple(t[:, :, : last["C"]].reshape(n, -1) for t in cur)
        wt = M.split(torch.from_numpy(np.asarray(p1[head]["kernel"])).to(dev))
        b = torch.from_numpy(np.asarray(p1[head]["bias"], np.float64)).to(dev)
        c = M.chain_depth(last["Cp"], slabs=fwd_splits(N2, nha_p, last["Cp"], False))
        v, S = M.dense(own, xin, wt)
        alt, _ = M.dense(other, xin, wt)
        rows_.check("acting q", f"{tag} q on the last site's out", q, v + b, M.bound(S + b.abs(), c), S + b.abs(), alt + b, elementwise=True)
    rows_.finish()
