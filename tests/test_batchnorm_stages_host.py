"""tests/helpers/batchnorm_stages.py against things that are not the code under test, no GPU: torch float64 autograd of the same
formulas, the oracle's BatchNorm network (oracle/network.py), the engine's own parameter layout and workspace regions
(isdqn_net_param_layout / isdqn_net_workspace_region are host arithmetic), and -- on the exact inputs of the GPU cases -- that each
wrong variant of a stage lands far outside the bound the GPU test holds that stage to.  The device side is
tests/test_gpu_batchnorm.py: test_batchnorm_stages_match_a_model_of_each_kernel_on_its_own_operands."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.helpers import batchnorm_stages as BS
from tests.helpers import bf16_model as M
from tests.helpers import impala_stages as IS

_up = lambda n, g: -(-n // g) * g


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize("spatial,N,P,C,Cp", [(True, 70, 5, 3, 8), (True, 9, 4, 8, 8), (False, 19, 3, 5, 8), (False, 74, 1, 16, 16)])
def test_stage_functions_agree_with_float64_autograd(spatial, N, P, C, Cp):
    rng = np.random.default_rng(N * 10 + C)
    G = P if spatial else P * Cp
    x = torch.zeros(N, P, Cp, dtype=torch.float64)
    x[..., :C] = torch.from_numpy(rng.normal(0.4, 1.3, size=(N, P, C)))
    dyw = torch.zeros_like(x)
    dyw[..., :C] = torch.from_numpy(rng.normal(size=(N, P, C)))
    scale, bias = (torch.from_numpy(rng.normal(1.0, 0.3, size=G)) for _ in range(2))
    xa, sa, ba = (t.clone().requires_grad_(True) for t in (x, scale, bias))
    xt = xa[..., :C]
    red = (0, 2) if spatial else (0,)
    mean = xt.mean(dim=red)
    var = ((xt * xt).mean(dim=red) - mean * mean).clamp_min(0)
    if spatial:
        sc, bi, mu, vv = (t.reshape(1, P, 1) for t in (sa, ba, mean, var))
    else:
        sc, bi = (t.reshape(1, P, Cp)[..., :C] for t in (sa, ba))
        mu, vv = mean[None], var[None]
    y = (xt - mu) * (torch.rsqrt(vv + BS.BN_EPS) * sc) + bi
    (y * dyw[..., :C]).sum().backward()

    m, v, d_mean, d_var = BS.bn_stats(x, spatial, C)
    want_mean = mean if spatial else BS._pad_channels(mean, Cp).reshape(-1)
    want_var = var if spatial else BS._pad_channels(var, Cp).reshape(-1)
    assert torch.allclose(m, want_mean.detach(), rtol=1e-12, atol=1e-14) and torch.allclose(v, want_var.detach(), rtol=1e-12, atol=1e-14)
    assert bool((d_mean > 0).all()) and bool((d_var >= 2 * m.abs() * d_mean).all())  # the cancellation term is in the bound
    yy, E = BS.bn_apply(x, m, v, scale, bias, spatial, C)
    assert torch.allclose(yy[..., :C], y.detach(), rtol=1e-12, atol=1e-13)
    assert float(yy[..., C:].abs().max() if C < Cp else 0.0) == 0.0 and float(E[..., C:].abs().max() if C < Cp else 0.0) == 0.0
    assert bool((E[..., :C] >= M.S8_STORE * yy[..., :C].abs()).all())
    s1, d_s1, s2, d_s2, dx, d_dx = BS.bn_backward(x, dyw, m, v, scale, spatial, C)
    keep = torch.ones(G, dtype=torch.bool) if spatial else (torch.arange(Cp) < C).repeat(P)
    assert torch.allclose(s1[keep], ba.grad[keep], rtol=1e-11, atol=1e-12) and torch.allclose(s2[keep], sa.grad[keep], rtol=1e-11, atol=1e-12)
    assert float(s1[~keep].abs().max() if bool((~keep).any()) else 0.0) == 0.0
    assert torch.allclose(dx, xa.grad, rtol=1e-10, atol=1e-12)
    assert float(dx[..., C:].abs().max() if C < Cp else 0.0) == 0.0 and bool((d_dx[..., :C] > 0).all()) and bool((d_s1[keep] > 0).all())
    # a carried input error widens every bound, the run's own sums replace the computed ones
    E_dy = torch.full_like(x, 1e-7)
    _, e1, _, e2, dx2, e3 = BS.bn_backward(x, dyw, m, v, scale, spatial, C, E_dy=E_dy, s1=s1, s2=s2)
    assert torch.equal(dx2, dx) and bool((e1[keep] > d_s1[keep]).all()) and bool((e2[keep] > d_s2[keep]).all()) and bool((e3[..., :C] > d_dx[..., :C]).all())
    # summation depths, from the kernels' loops
    assert BS.spatial_depth(80, 4) == 2 * 4 + 6 and BS.spatial_depth(18, 8) == 8 + 6 and BS.feature_depth(74) == 10 + 8 and BS.feature_depth(16) == 2 + 8


def test_running_average_uses_the_float32_constants():
    ra = np.array([0.3, -1.5, 2.0, 0.0], np.float32)
    b = np.array([0.1, 0.25, -0.7, 1e-3], np.float32)
    want, ulp2 = BS.running(ra, b)
    exact = BS.BN_MOMENTUM * ra.astype(np.float64) + BS.BN_ONE_MINUS * b.astype(np.float64)
    assert want.dtype == np.float32 and np.all(np.abs(want.astype(np.float64) - exact) <= ulp2)
    assert BS.BN_MOMENTUM != 0.99 and abs(BS.BN_MOMENTUM - 0.99) < 1e-7 and abs(BS.BN_ONE_MINUS - 0.01) < 1e-7 and BS.BN_EPS == float(np.float32(1e-5))
    assert np.all(ulp2 == 2.0 * np.spacing(np.abs(want)).astype(np.float64))


SMALL = {
    "cnn": dict(arch="cnn", obs=(20, 16, 2), feats=(5, 6, 7, 9), K=2, A=3, B=3, ln=True, n_heads=3),
    "fc": dict(arch="fc", obs=(5,), feats=(12, 7), K=1, A=4, B=6, ln=False, n_heads=2),
}


@pytest.mark.parametrize("kind", list(SMALL))
def test_reference_step_agrees_with_the_oracle_network(kind):
    """forward values, the BatchNorm scale / bias gradients and the moved running averages of batchnorm_stages.reference_step
    against oracle/network.py's BatchNorm network under float64 autograd"""
    from tests.gpu_helpers import perturbed_params

    cfg = SMALL[kind]
    K, A, B = cfg["K"], cfg["A"], cfg["B"]
    params = perturbed_params(5, cfg["obs"], list(cfg["feats"]), cfg["arch"], cfg["n_heads"] * A, cfg["ln"], batch_norm=True)
    rng = np.random.default_rng(8)
    stats = {m: {"mean": rng.normal(0, 0.3, l["mean"].shape).astype(np.float32), "var": rng.uniform(0.5, 2.0, l["var"].shape).astype(np.float32)}
             for m, l in onet.init_batch_stats(params).items()}
    action, reward, terminal = rng.integers(0, A, B), rng.normal(size=B), (rng.random(B) < 0.3).astype(np.float64)
    if kind == "cnn":
        h, w, c = cfg["obs"]
        raw = rng.integers(0, 256, size=(2 * B, h, w, c)).astype(np.uint8)
        x_or = torch.from_numpy(raw)
        x_in = BS._pad_channels(torch.from_numpy(raw).double() / 255.0, 8)
    else:
        x_or = torch.from_numpy(rng.normal(size=(2 * B, cfg["obs"][0])))
        x_in = x_or.clone()
    ref = BS.reference_step(cfg, params, x_in, action, reward, terminal, n_heads=cfg["n_heads"])
    P = onet.to_torch(params, torch.float64, requires_grad=True)
    cap, new = {}, {}
    q = onet.forward(P, x_or, cfg["feats"], cfg["arch"], cfg["ln"], capture=cap, batch_norm=True, batch_stats=onet.to_torch(stats, torch.float64),
                     use_running_average=False, new_stats=new)
    assert torch.allclose(ref["q"], q.detach(), rtol=1e-9, atol=1e-11)
    qq = q.reshape(2 * B, 1 + K, A)
    qv = qq[:B, 1:][torch.arange(B), :, torch.as_tensor(action)]
    tg = torch.as_tensor(reward)[:, None] + (1 - torch.as_tensor(terminal))[:, None] * 0.99 * qq[B:, :K].max(-1).values
    ((qv - tg.detach()) ** 2).mean(0).sum().backward()
    assert torch.allclose(ref["targets"], tg.detach(), rtol=1e-9, atol=1e-11)
    for s in BS.site_layout(cfg):
        r = ref["sites"][s["name"]]
        unpad = (lambda v: v.reshape(s["flax_shape"])) if s["spatial"] else (lambda v: v.reshape(s["P"], s["Cp"])[:, : s["C"]].reshape(s["flax_shape"]))
        y = cap[s["name"]].detach().reshape(2 * B, s["P"], s["C"])
        assert torch.allclose(r["out"][..., : s["C"]], y, rtol=1e-9, atol=1e-11), s["name"]
        for leaf, key in (("scale", "s2"), ("bias", "s1")):
            want = P[s["name"]][leaf].grad
            assert float(want.abs().max()) > 0
            assert torch.allclose(unpad(r[key]), want, rtol=1e-7, atol=1e-10 * float(want.abs().max())), (s["name"], leaf)
        for leaf in ("mean", "var"):
            ra, batch = stats[s["name"]][leaf].reshape(-1), unpad(r[leaf]).reshape(-1).numpy().astype(np.float32)
            got, _ = BS.running(ra, batch)
            want = new[s["name"]][leaf].reshape(-1).numpy()
            # (the oracle moves them in float64 with 0.99 and 0.01; the kernel's 1 - 0.99f is 1e-6 below 0.01)
            assert np.all(np.abs(got - want) <= 2e-6 * (np.abs(ra) + 0.01 * np.abs(batch))), (s["name"], leaf)


# ------------------------------------------------------------------ layout
def _net_cfg(cfg):
    from slimdqn import _hip

    c = _hip.NetConfig()
    c.arch = {"cnn": _hip.ARCH_CNN, "impala": _hip.ARCH_IMPALA, "fc": _hip.ARCH_FC}[cfg["arch"]]
    if cfg["arch"] != "fc":
        c.obs_h, c.obs_w, c.obs_c = cfg["obs"]
    else:
        c.obs_h = c.obs_w = 1
        c.obs_c = cfg["obs"][0]
    c.n_features = len(cfg["feats"])
    for i, f in enumerate(cfg["feats"]):
        c.features[i] = int(f)
    c.n_actions, c.n_heads, c.layer_norm, c.batch_size, c.batch_norm = cfg["A"], cfg["n_heads"], int(cfg["ln"]), cfg["B"], 1
    return c


@pytest.mark.parametrize("case", list(BS.CASES))
def test_site_layout_matches_the_engines_parameter_layout_and_regions(case):
    from slimdqn import _hip

    cfg = BS.CASES[case]
    c = _net_cfg(cfg)
    n, cnt = ctypes.c_int64(), ctypes.c_int32()
    _hip.check(_hip.lib().isdqn_net_param_layout(ctypes.byref(c), ctypes.byref(n), None, 0, ctypes.byref(cnt)))
    infos = (_hip.TensorInfo * cnt.value)()
    _hip.check(_hip.lib().isdqn_net_param_layout(ctypes.byref(c), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)))
    by_name = {i.name.decode(): i for i in infos if i.kind >= 5}
    sites = BS.site_layout(cfg)
    assert len(by_name) == 4 * len(sites)
    N2 = 2 * cfg["B"]

    def region_floats(name):
        off, size = ctypes.c_int64(), ctypes.c_int64()
        _hip.check(_hip.lib().isdqn_net_workspace_region(ctypes.byref(c), name.encode(), ctypes.byref(off), ctypes.byref(size)))
        return size.value // 4

    for s in sites:
        for kind, leaf in ((5, "scale"), (6, "bias"), (7, "mean"), (8, "var")):
            i = by_name[f"{s['name']}/{leaf}"]
            assert i.kind == kind and list(i.dims)[:4] == [s["G"], s["P"], s["C"], s["Cp"]], (s["name"], leaf, list(i.dims))
            assert tuple(i.flax_shape[: i.ndim]) == tuple(s["flax_shape"]) and i.size == _up(s["G"], 8)
            assert (i.ndim == 2) == s["spatial"]
        assert region_floats(s["prefix"] + "out") == _up(N2 * s["P"] * s["Cp"], 64)
        assert region_floats(s["src"]) == _up(N2 * s["P"] * s["Cp"], 64)
        for r in ("mean", "var", "dbias", "dscale"):
            assert region_floats(s["prefix"] + r) == _up(_up(s["G"], 8), 64)
    for l in BS.layers(cfg):
        for r in ("act", "z", "dz"):  # with BatchNorm the backward runs over all 2B rows
            assert region_floats(f"{r}/{l['name']}") == _up(N2 * l["npix"] * l["cp"], 64)
    if cfg["arch"] == "fc":
        assert region_floats("bn/x0") == _up(N2 * cfg["obs"][0], 64)
    assert region_floats("dout") == _up(N2 * _up(cfg["n_heads"] * cfg["A"], 8), 64)
    # what each case is meant to force
    if case == "cnn-84x84x4-B40":
        assert N2 == 80 and 64 < N2 < 128  # the lane loop's second iteration, partly filled
    if case == "cnn-52x60x2-B33-noln":
        assert [(s["C"], s["Cp"]) for s in sites[:3]] == [(2, 8), (16, 16), (20, 24)] and (sites[3]["C"], sites[3]["Cp"], sites[3]["spatial"]) == (12, 16, False)
        assert [s["P"] for s in sites[:3]] == [52 * 60, 13 * 15, 7 * 8]
    if case == "cnn-headline-B8":
        assert sites[-1]["G"] == 512 and sites[3]["G"] == 11 * 11 * 64
    if case == "fc-d6-B37":
        assert N2 == 74 and N2 % 8 == 2 and sites[0]["G"] == 304 and 256 < 304 < 512 and cfg["n_heads"] == 1


@pytest.mark.parametrize("case", list(IS.BACKWARD_CASES))
def test_impala_site_layout_matches_the_oracle_the_parameter_layout_and_the_regions(case):
    """Every case of tests/test_gpu_impala_backward.py, planned with BatchNorm: the sites' names and Flax shapes are the oracle's
    (init_params(..., batch_norm=True), init_batch_stats) in Flax's call order, and name / kind / dims / region sizes are the
    engine's own (host arithmetic of the plan: plan_impala_torso, place_bn_regions)."""
    from slimdqn import _hip

    cfg = dict(IS.BACKWARD_CASES[case], n_heads=1 + IS.BACKWARD_CASES[case]["K"])
    sites = BS.site_layout(cfg)
    params = onet.init_params(0, cfg["obs"], list(cfg["feats"]), "impala", cfg["n_heads"] * cfg["A"], cfg["ln"], batch_norm=True)
    stats = onet.init_batch_stats(params)
    assert [s["name"] for s in sites] == [m for m in params if m.rsplit("/", 1)[-1].startswith("BatchNorm_")] == list(stats)
    assert [s["name"] for s in sites] == ["BatchNorm_0"] + [f"Stack_{s}/BatchNorm_{b}" for s in range(3) for b in range(2)] + [
        f"BatchNorm_{1 + j}" for j in range(len(cfg["feats"]) - 2)]
    for s in sites:
        for leaf in ("scale", "bias"):
            assert params[s["name"]][leaf].shape == tuple(s["flax_shape"]), (s["name"], leaf)
        for leaf in ("mean", "var"):
            assert stats[s["name"]][leaf].shape == tuple(s["flax_shape"]), (s["name"], leaf)
    geo = IS.geometry(cfg["obs"], cfg["feats"])
    assert [s["src"] for s in sites[:8]] == ["bn/x0"] + [f"imp/s{s}/a1_{b}" for s in range(3) for b in range(2)] + ["act/Impala"]
    assert [s["layer"] for s in sites] == [-1] + [-2 - k for k in range(6)] + list(range(len(cfg["feats"]) - 2))
    assert [s["spatial"] for s in sites] == [True] * 7 + [False] * (len(sites) - 7)
    assert [(s["P"], s["C"], s["Cp"]) for s in sites[1:7]] == [(g["Hp"] * g["Wp"], g["C"], g["C_p"]) for g in geo for _ in range(2)]
    assert (sites[7]["P"], sites[7]["C"], sites[7]["Cp"]) == (geo[2]["Hp"] * geo[2]["Wp"], geo[2]["C"], geo[2]["C_p"])

    c = _net_cfg(cfg)
    n, cnt = ctypes.c_int64(), ctypes.c_int32()
    _hip.check(_hip.lib().isdqn_net_param_layout(ctypes.byref(c), ctypes.byref(n), None, 0, ctypes.byref(cnt)))
    infos = (_hip.TensorInfo * cnt.value)()
    _hip.check(_hip.lib().isdqn_net_param_layout(ctypes.byref(c), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)))
    by_name = {i.name.decode(): i for i in infos if i.kind >= 5}
    assert len(by_name) == 4 * len(sites)
    N2 = 2 * cfg["B"]

    def region_floats(name):
        off, size = ctypes.c_int64(), ctypes.c_int64()
        _hip.check(_hip.lib().isdqn_net_workspace_region(ctypes.byref(c), name.encode(), ctypes.byref(off), ctypes.byref(size)))
        return size.value // 4

    for s in sites:
        for kind, leaf in ((5, "scale"), (6, "bias"), (7, "mean"), (8, "var")):
            i = by_name[f"{s['name']}/{leaf}"]
            assert i.kind == kind and list(i.dims)[:4] == [s["G"], s["P"], s["C"], s["Cp"]], (s["name"], leaf, list(i.dims))
            assert tuple(i.flax_shape[: i.ndim]) == tuple(s["flax_shape"]) and i.size == _up(s["G"], 8)
        assert region_floats(s["prefix"] + "out") == _up(N2 * s["P"] * s["Cp"], 64)
        assert region_floats(s["src"]) == _up(N2 * s["P"] * s["Cp"], 64)
        for r in ("mean", "var", "dbias", "dscale"):
            assert region_floats(s["prefix"] + r) == _up(_up(s["G"], 8), 64)
    for l in BS.layers(cfg):
        for r in ("act", "z", "dz"):  # with BatchNorm the backward runs over all 2B rows
            assert region_floats(f"{r}/{l['name']}") == _up(N2 * l["npix"] * l["cp"], 64)
    for s, g in enumerate(geo):  # and so does the torso's: its gradient regions hold 2B images
        assert region_floats(f"imp/s{s}/dz0") == _up(N2 * g["H"] * g["W"] * g["C_p"], 64)
        assert region_floats(f"imp/s{s}/da") == _up(N2 * max(g["H"] * g["W"] * g["cin_p"], g["Hp"] * g["Wp"] * g["C_p"]), 64)
    if case == "bn-84x84x4-noln-B2":
        assert IS.row_blocks(N2 * 42 * 42) == (256, 2)  # the 2B-row backward's grid-stride loop runs twice
    if case == "bn-44x36x3-ln-B3":
        assert all(s["C"] < s["Cp"] for s in sites[:8]) and (sites[0]["C"], sites[0]["Cp"]) == (3, 8)


# ------------------------------------------------------------------ the GPU cases separate the references from wrong variants
_REF = {}


def _reference(case):
    if case not in _REF:
        inp = BS.case_inputs(case)
        cfg = inp["cfg"]
        if cfg["arch"] == "cnn":
            h, w, stack = cfg["obs"]
            x_in = IS.frames_to_x(torch.from_numpy(inp["frames"]), IS.paired_ids(inp["ids"], stack), h, w, stack).double()
        else:
            x_in = torch.from_numpy(np.concatenate([inp["state"], inp["next_state"]])).double()
        ref = BS.reference_step(cfg, inp["params"], x_in, inp["action"].astype(np.int64), inp["reward"].astype(np.float64),
                                inp["terminal"].astype(np.float64), n_heads=cfg["n_heads"])
        _REF[case] = (inp, ref)
    return _REF[case]


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    yield
    _REF.clear()


def _outside(got, want, bnd, affected=None):
    """share of the affected elements that lie more than 4x outside the bound"""
    far = (got - want).abs() > 4 * bnd
    if affected is not None:
        far = far[affected]
    return float(far.double().mean()) if far.numel() else 0.0


def _variant_shares(case, variant):
    """{compared tensor: share of its affected elements more than 4x outside its bound}; empty: the variant does not apply"""
    inp, ref = _reference(case)
    cfg = inp["cfg"]
    N, B = 2 * cfg["B"], cfg["B"]
    L = {l["name"]: l for l in BS.layers(cfg)}
    names = [l["name"] for l in BS.layers(cfg)]
    out = {}
    for s in BS.site_layout(cfg):
        r, sp, C = ref["sites"][s["name"]], s["spatial"], s["C"]
        rows = torch.arange(N)
        if variant == "divisor N * Cp" and sp and C < s["Cp"]:
            m, v, _, _ = BS.bn_stats(r["x"], sp, C, count=N * s["Cp"])
            out[s["name"] + "/mean"], out[s["name"] + "/var"] = _outside(m, r["mean"], r["d_mean"]), _outside(v, r["var"], r["d_var"])
        if variant == "spatial rows n >= 64 dropped" and sp and N > 64:
            m, v, _, _ = BS.bn_stats(r["x"], sp, C, rows=rows < 64)
            out[s["name"] + "/mean"], out[s["name"] + "/var"] = _outside(m, r["mean"], r["d_mean"]), _outside(v, r["var"], r["d_var"])
        if variant == "feature row slice 7 dropped" and not sp:
            m, v, _, _ = BS.bn_stats(r["x"], sp, C, rows=rows % 8 != 7)
            keep = (torch.arange(s["Cp"]) < C).repeat(s["P"])  # (padded columns: 0 either way)
            out[s["name"] + "/mean"] = _outside(m, r["mean"], r["d_mean"], keep)
            out[s["name"] + "/var"] = _outside(v, r["var"], r["d_var"], keep)
        if variant == "var without - mean^2":
            _, v, _, _ = BS.bn_stats(r["x"], sp, C, fast_variance=False)
            keep = torch.ones(s["G"], dtype=torch.bool) if sp else (torch.arange(s["Cp"]) < C).repeat(s["P"])
            out[s["name"] + "/var"] = _outside(v, r["var"], r["d_var"], keep)
        if variant == "inv_m = 1 / N on a spatial site" and sp and s["layer"] >= 0:
            l = L[names[s["layer"]]]
            lay = ref["layers"][l["name"]]
            _, _, _, _, dx, _ = BS.bn_backward(r["x"], r["dy"], r["mean"], r["var"], r["scale"], sp, C, inv_m=1.0 / N)
            dz, _ = M.ln_relu_bwd(lay["z"], lay["gamma"], lay["mask"], dx[:, :, :C], r["d_dx"][:, :, :C], has_ln=l["ln"] is not None)
            out["dz/" + l["name"]] = _outside(dz, lay["dz"], lay["E_dz"], lay["mask"] > 0)
        if variant == "xhat from the running averages":
            ra_mean, ra_var = (BS.pad_groups(s, torch.from_numpy(inp["stats"][s["name"]][k]).double()) for k in ("mean", "var"))
            _, _, s2, _, _, _ = BS.bn_backward(r["x"], r["dy"], ra_mean, ra_var, r["scale"], sp, C)
            keep = torch.ones(s["G"], dtype=torch.bool) if sp else (torch.arange(s["Cp"]) < C).repeat(s["P"])
            out[s["name"] + "/dscale"] = _outside(s2, r["s2"], r["d_s2"], keep)
        if variant == "momentum 0.9":
            for leaf in ("mean", "var"):
                ra = BS.pad_groups(s, torch.from_numpy(inp["stats"][s["name"]][leaf])).numpy()
                batch = r[leaf].numpy().astype(np.float32)
                want, ulp2 = BS.running(ra, batch)
                got, _ = BS.running(ra, batch, momentum=0.9)
                keep = torch.ones(s["G"], dtype=torch.bool) if sp else (torch.arange(s["Cp"]) < C).repeat(s["P"])
                out[f"{s['name']} running {leaf}"] = _outside(torch.from_numpy(got.astype(np.float64)), torch.from_numpy(want.astype(np.float64)),
                                                              torch.from_numpy(ulp2), keep)
    if variant == "next-state rows of dL/dq not zeroed":  # the GPU test leaves 1.0 there before the step; the rows' bound is 0
        stale = ref["dout"].clone()
        stale[B:] = 1.0
        out["dout"] = _outside(stale[B:], ref["dout"][B:], torch.zeros_like(stale[B:]))
    return out


VARIANTS = ["divisor N * Cp", "spatial rows n >= 64 dropped", "feature row slice 7 dropped", "inv_m = 1 / N on a spatial site",
            "xhat from the running averages", "var without - mean^2", "momentum 0.9", "next-state rows of dL/dq not zeroed"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_gpu_case_inputs_separate_the_reference_from_a_wrong_variant(variant):
    """On the generated frames and parameters of every GPU case the variant applies to, at least a quarter of the affected elements
    of at least one compared tensor lie more than 4x outside the bound the GPU test holds that tensor to."""
    applied = 0
    for case in BS.CASES:
        shares = _variant_shares(case, variant)
        if not shares:
            continue
        applied += 1
        best = max(shares, key=shares.get)
        print(f"  {variant} | {case}: {best} {shares[best]:.0%} of the affected elements > 4x outside its bound")
        assert shares[best] >= 0.25, (variant, case, shares)
    assert applied >= 1, f"no GPU case reaches the variant {variant!r}"
    if variant in ("spatial rows n >= 64 dropped", "divisor N * Cp"):
        assert applied >= 2


def test_reference_step_bounds_hold_the_reference_to_itself():
    """dL/dq of the reference: rows [B, 2B) zero and one non-zero per transition and regressed head (the single-head case: at head 0)"""
    for case in ("fc-d6-B37",):
        inp, ref = _reference(case)
        B = inp["cfg"]["B"]
        assert float(ref["dout"][B:].abs().max()) == 0.0 and int((ref["dout"][:B] != 0).sum()) == B * inp["cfg"]["K"]
        assert bool((ref["cols"] < inp["cfg"]["A"]).all())
