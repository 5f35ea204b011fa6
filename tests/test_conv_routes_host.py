"""The cases of tests/test_gpu_conv_routes.py, held on the host: the plan-level half of tests/helpers/conv_routes.py against the real
plan (tests/helpers/plan_dump.cpp), the launch-level half as a literal table of the route every convolution of every case takes, the
coverage of the kernels and paths the cases exist for, and the float64 model of the three contractions (tests/helpers/bf16_model.py)
against torch's conv2d and its autograd at these geometries.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import bf16_model as M
from tests.helpers import conv_routes as R
from tests.helpers import plan_grid as pg

CSRC = os.path.join(pg.ROOT, "is-dqn_amd", "csrc")
PRECISION = {"bf16x3": 0, "bf16": 1}  # include/isdqn_hip.h ISDQN_PRECISION_*
RUN_IDS = [f"{c}-{p}" for c, p in R.RUNS]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(case, precision): [{field: value} per layer]} of the real plan of every run"""
    exe = str(tmp_path_factory.mktemp("conv_routes") / "plan_dump")
    assert pg.compile_dumper(CSRC, exe).wait() == 0
    cfgs = []
    for case, prec in R.RUNS:
        c = R.CASES[case]
        h, w, stack = c["obs"]
        cfgs.append(dict(pg.BASE, obs_h=h, obs_w=w, obs_c=stack, features=c["feats"], n_actions=c["A"], n_heads=1 + c["K"], layer_norm=1,
                         batch_size=c["B"], precision=PRECISION[prec]))
    out = {}
    for run, (rc, body) in zip(R.RUNS, pg.run_dumper(exe, cfgs)):
        assert rc == 0, f"{run}: refused: {body.strip()}"
        rows = [l for l in body.splitlines() if l.startswith("L[")]
        out[run] = [{k: v for k, v in (t.split("=", 1) for t in l.split()[1:])} for l in rows]
    return out


@pytest.mark.parametrize("case,precision", R.RUNS, ids=RUN_IDS)
def test_plan_fields_equal_the_real_plan(plans, case, precision):
    """Every configuration is accepted, and the plan's own tiling decisions are what conv_routes.plan_fields computes."""
    cfg = R.CASES[case]
    layers, _ = R.layers(cfg)
    real = plans[(case, precision)]
    assert len(real) == len(layers) + 1  # the head
    for L, want, got in zip(layers, R.plan_fields(cfg, cfg["B"]), real):
        assert got["name"] == L["name"] and int(got["kind"]) == 0
        for k, v in want.items():
            assert (int(got[k]) if k in got else None) == v, f"{L['name']}.{k}: plan {got.get(k)}, restated {v}"
        for k, mine in (("hin", "hin"), ("win", "win"), ("cin", "cin"), ("cin_p", "cin_p"), ("hout", "h"), ("wout", "w"), ("cout", "c"),
                        ("cout_p", "cp"), ("ksz", "k"), ("stride", "s"), ("pad", "pad"), ("K", "K"), ("is_u8", "u8")):
            assert int(got[k]) == int(L[mine]), f"{L['name']}.{k}"
    d0 = real[len(R.CONVS)]
    assert int(d0["kind"]) == 1 and int(d0["in_p"]) == layers[3]["in_p"]


# The route of every convolution of every run: forward at n_img = 2B / at n_img = 1, data gradient, weight gradient.
# (conv_routes.fmt: kernel<mt, passes[, KG2 | u8]>; generic<BM, passes>(why); tiles per image / per stride class; the generic weight
# gradient's slabs and K steps per slab)
ROUTES = {
    ("100x100", "bf16x3"): [
        ("u8img<2,2> tiles=5", "u8img<2,2> tiles=5", None, "generic(lds) slabs=59 steps=2"),
        ("s8img<4,3,KG2> tiles=2", "s8img<4,3,KG2> tiles=2", "dgimg<2,3> tiles=2+2+2+2", "generic(lds) slabs=32 steps=1"),
        ("s8img<4,3,KG2> tiles=2", "s8img<4,3,KG2> tiles=2", "dgimg<4,3> tiles=2", "wgimg<4,9,3> G=1 groups=6")],
    ("100x100", "bf16"): [
        ("u8img<2,1> tiles=5", "u8img<2,1> tiles=5", None, "wgimg<2,4,1,u8> G=1 groups=6"),
        ("s8img<4,1> tiles=2", "s8img<4,1> tiles=2", "dgimg<2,1> tiles=2+2+2+2", "wgimg<4,8,1> G=1 groups=6"),
        ("s8img<4,1> tiles=2", "s8img<4,1> tiles=2", "dgimg<4,1> tiles=2", "wgimg<4,9,1> G=1 groups=6")],
    ("160x120", "bf16x3"): [
        ("u8pair<2> tiles=10", "u8pair<2> tiles=10", None, "generic(lds) slabs=57 steps=2"),
        ("s8img<4,3,KG2> tiles=3", "s8img<4,3,KG2> tiles=3", "dgimg<2,3> tiles=3+3+3+3", "generic(lds) slabs=29 steps=1"),
        ("s8img<4,3,KG2> tiles=3", "s8img<4,3,KG2> tiles=3", "dgimg<4,3> tiles=3", "generic(lds) slabs=15 steps=2")],
    ("128x128-w64", "bf16x3"): [
        ("u8img<4,2> tiles=8", "u8img<4,2> tiles=8", None, "generic(lds) slabs=64 steps=2"),
        ("generic<64,3>(lds)", "generic<64,3>(lds)", "dgimg<4,3> tiles=2+2+2+2", "generic(lds) slabs=16 steps=2"),
        ("s8img<4,3,KG2> tiles=2", "s8img<4,3,KG2> tiles=2", "dgimg<4,3> tiles=2", "generic(lds) slabs=16 steps=2")],
    ("128x128-w64", "bf16"): [
        ("u8img<4,1> tiles=8", "u8img<4,1> tiles=8", None, "generic(lds) slabs=64 steps=2"),
        ("s8img<4,1,KG2> tiles=2", "s8img<4,1,KG2> tiles=2", "dgimg<4,1> tiles=2+2+2+2", "generic(lds) slabs=16 steps=2"),
        ("s8img<4,1> tiles=2", "s8img<4,1> tiles=2", "dgimg<4,1> tiles=2", "wgimg<4,9,1> G=1 groups=4")],
    ("64x64x3", "bf16x3"): [
        ("u8img<2,2> tiles=2", "u8img<2,2> tiles=2", None, "generic(u8ntw3) slabs=48 steps=1"),
        ("s8img<4,3> tiles=1", "s8img<4,3> tiles=1", "dgimg<2,3> tiles=1+1+1+1", "wgimg<4,8,3> G=1 groups=6"),
        ("s8img<4,3> tiles=1", "s8img<4,3> tiles=1", "dgimg<4,3> tiles=1", "wgimg<4,9,3> G=1 groups=6")],
    ("84-w64-48-24", "bf16x3"): [
        ("u8img<4,2> tiles=4", "u8img<4,2> tiles=4", None, "generic(lds) slabs=35 steps=2"),
        ("generic<64,3>(lds)", "generic<64,3>(lds)", "dgimg<4,3> tiles=1+1+1+1", "generic(lds) slabs=10 steps=2"),
        ("s8img<2,3> tiles=1", "s8img<2,3> tiles=1", "dgimg<4,3> tiles=1", "generic(plan) slabs=19 steps=1")],
    ("84-w64-48-24", "bf16"): [
        ("u8img<4,1> tiles=4", "u8img<4,1> tiles=4", None, "wgimg<4,4,1,u8> G=1 groups=5"),
        ("s8img<4,1,KG2> tiles=1", "s8img<4,1,KG2> tiles=1", "dgimg<4,1> tiles=1+1+1+1", "wgimg<4,4,1> G=1 groups=5"),
        ("s8img<2,1> tiles=1", "s8img<2,1> tiles=1", "dgimg<4,1> tiles=1", "generic(plan) slabs=19 steps=1")],
    ("40x40x2", "bf16x3"): [
        ("u8img<2,2> tiles=1", "u8img<2,2> tiles=1", None, "wgimg<2,2,2,u8> G=1 groups=7"),
        ("s8img<2,3> tiles=1", "s8img<2,3> tiles=1", "dgimg<2,3> tiles=1+1+1+1", "wgimg<2,4,3> G=1 groups=7"),
        ("s8img<4,3> tiles=1", "s8img<4,3> tiles=1", "dgimg<2,3> tiles=1", "generic(plan) slabs=6 steps=1")],
    ("8x8x1", "bf16x3"): [
        ("u8img<2,2> tiles=1", "u8img<2,2> tiles=1", None, "generic(plan) slabs=1 steps=1"),
        ("generic<32,3>(cin8)", "generic<32,3>(cin8)", "dgimg<2,3> tiles=1+1+1+1", "generic(plan) slabs=1 steps=1"),
        ("generic<32,3>(cin8)", "generic<32,3>(cin8)", "dgimg<2,3> tiles=1", "generic(plan) slabs=1 steps=1")],
}


@pytest.mark.parametrize("case,precision", R.RUNS, ids=RUN_IDS)
def test_route_table_is_literal(case, precision):
    got = [tuple(None if r[k] is None else R.fmt(r[k]) for k in ("fwd", "fwd1", "dgrad", "wgrad")) for r in R.routes(R.CASES[case], precision)]
    assert got == ROUTES[(case, precision)]


def test_headline_routes_are_the_known_ones():
    """The restatement on the Atari frame at the headline widths gives the kernels DESIGN.md names for it: the u8 pair kernel, the S8
    pair kernel on an even image count and its two-K-group twin on an odd one, one tile per image and per stride class."""
    cfg = dict(arch="cnn", feats=(32, 64, 64, 512), ln=True, B=32)
    got = [tuple(None if r[k] is None else R.fmt(r[k]) for k in ("fwd", "fwd1", "dgrad", "wgrad")) for r in R.routes(cfg, "bf16x3")]
    assert got == [("u8pair<2> tiles=4", "u8pair<2> tiles=4", None, "wgimg<2,4,2,u8> G=1 groups=32"),
                   ("s8pair", "s8img<4,3,KG2> tiles=1", "dgimg<2,3> tiles=1+1+1+1", "wgimg<4,8,3> G=1 groups=32"),
                   ("s8img<4,3> tiles=1", "s8img<4,3> tiles=1", "dgimg<4,3> tiles=1", "wgimg<4,9,3> G=1 groups=32")]


def test_the_cases_reach_every_route_they_exist_for():
    """Each kernel form or path that no test at the Atari frame reaches is reached by at least one convolution of one run."""
    seen = []
    for case, prec in R.RUNS:
        cfg = R.CASES[case]
        layers, _ = R.layers(cfg)
        for L, r in zip(layers, R.routes(cfg, prec)):
            seen.append((case, prec, L, r))
    any_ = lambda f: any(f(c, p, L, r) for c, p, L, r in seen)
    f, d, w = (lambda r: r["fwd"]), (lambda r: r["dgrad"] or {}), (lambda r: r["wgrad"])
    want = {
        "S8 image forward, 2 tiles, ragged last tile": lambda c, p, L, r: f(r)["kernel"] == "s8img" and f(r)["tiles"] == 2 and L["npix"] == 169,
        "S8 image forward, 3 tiles": lambda c, p, L, r: f(r)["kernel"] == "s8img" and f(r)["tiles"] == 3,
        "S8 image forward, one K group, several tiles": lambda c, p, L, r: f(r)["kernel"] == "s8img" and f(r)["tiles"] > 1 and f(r)["kg"] == 1,
        "S8 image forward, two K groups, several tiles": lambda c, p, L, r: f(r)["kernel"] == "s8img" and f(r)["tiles"] > 1 and f(r)["kg"] == 2,
        "image data gradient, several tiles per class, 4 classes": lambda c, p, L, r: d(r).get("kernel") == "dgimg" and d(r)["tiles"] in ([2] * 4, [3] * 4),
        "image data gradient, several tiles, 1 class": lambda c, p, L, r: d(r).get("kernel") == "dgimg" and d(r)["tiles"] in ([2], [3]),
        "u8 one-tile kernel, odd tile count": lambda c, p, L, r: f(r)["kernel"] == "u8img" and f(r)["tiles"] == 5,
        "u8 one-tile kernel, 64 channels, 2 passes": lambda c, p, L, r: f(r)["kernel"] == "u8img" and f(r)["mt"] == 4 and f(r)["passes"] == 2,
        "u8 one-tile kernel, 64 channels, 1 pass": lambda c, p, L, r: f(r)["kernel"] == "u8img" and f(r)["mt"] == 4 and f(r)["passes"] == 1,
        "u8 one-tile kernel, 64 channels on the four tiles of the Atari frame": lambda c, p, L, r: f(r)["kernel"] == "u8img" and f(r)["mt"] == 4 and f(r)["tiles"] == 4,
        "u8 one-tile kernel, three stacked frames": lambda c, p, L, r: f(r)["kernel"] == "u8img" and L["K"] == 192,
        "u8 pair kernel, more than four tiles, ragged last half": lambda c, p, L, r: f(r)["kernel"] == "u8pair" and f(r)["tiles"] == 10 and L["npix"] % 256 == 176,
        "generic forward at 64 input channels (lds)": lambda c, p, L, r: f(r)["kernel"] == "generic" and f(r)["why"] == "lds" and L["cin_p"] == 64,
        "the same layer on the image kernel in bf16": lambda c, p, L, r: p == "bf16" and L["K"] == 1024 and f(r)["kernel"] == "s8img" and f(r)["kg"] == 2,
        "generic weight gradient (lds), uint8 pixels": lambda c, p, L, r: w(r)["kernel"] == "generic" and w(r)["why"] == "lds" and L["u8"],
        "generic weight gradient (lds), K = 512 / 576 / 1024": lambda c, p, L, r: w(r)["kernel"] == "generic" and w(r)["why"] == "lds" and L["K"] in (512, 576, 1024),
        "generic weight gradient, uint8 pixels with ntw 3": lambda c, p, L, r: w(r)["kernel"] == "generic" and w(r)["why"] == "u8ntw3",
        "wgimg<4,4,1,u8>": lambda c, p, L, r: w(r)["kernel"] == "wgimg" and w(r)["u8"] and w(r)["mt"] == 4 and w(r)["ntw"] == 4,
        "wgimg<2,2,2,u8>": lambda c, p, L, r: w(r)["kernel"] == "wgimg" and w(r)["u8"] and w(r)["mt"] == 2 and w(r)["ntw"] == 2,
        "wgimg<2,4,3>": lambda c, p, L, r: w(r)["kernel"] == "wgimg" and not w(r)["u8"] and w(r)["mt"] == 2 and w(r)["ntw"] == 4 and w(r)["passes"] == 3,
        "a non-square frame with multi-tile layers": lambda c, p, L, r: L["h"] != L["w"] and L["npix"] > 128,
        "a frame pitch above h * w": lambda c, p, L, r: R.CASES[c]["slack"] > 0,
        "the smallest observation: one output pixel": lambda c, p, L, r: L["hin"] == 1 and L["npix"] == 1 and d(r).get("kernel") == "dgimg",
        "a data gradient over a 24-channel dz": lambda c, p, L, r: d(r).get("kernel") == "dgimg" and d(r)["mt"] == 4 and L["c"] == 24,
    }
    missing = [k for k, fn in want.items() if not any_(fn)]
    assert not missing, missing
    # the u8 / ntw 3 fall-through leaves the generic engine the plan's raised slab count, not the image kernel's groups
    cfg = R.CASES["64x64x3"]
    fields = R.plan_fields(cfg, cfg["B"])[0]
    r = R.routes(cfg, "bf16x3")[0]["wgrad"]
    assert fields["wgi_groups"] == 6 and fields["gw_slabs"] == 48 and r["slabs"] == 48 != fields["wgi_groups"]


# ------------------------------------------------------------------ the model at these geometries
def _same_pad(x, k, s):
    """explicit SAME padding of NCHW x, as oracle/network.py pads"""
    H, W = x.shape[2:]
    pads = []
    for size in (W, H):
        out = -(-size // s)
        tot = max((out - 1) * s + k - size, 0)
        pads += [tot // 2, tot - tot // 2]
    return F.pad(x, pads)


SHAPES = [  # (input h, w, cin, cout, k, s): the three layers of the non-square, the two-tile, the three-frame and the smallest case
    (160, 120, 4, 3, 8, 4), (40, 30, 3, 5, 4, 2), (20, 15, 5, 3, 3, 1),
    (100, 100, 4, 3, 8, 4), (25, 25, 3, 5, 4, 2), (13, 13, 5, 3, 3, 1),
    (64, 64, 3, 2, 8, 4), (16, 16, 2, 3, 4, 2),
    (8, 8, 1, 2, 8, 4), (2, 2, 2, 3, 4, 2), (1, 1, 3, 2, 3, 1),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_contractions_against_conv2d_in_float64(shape):
    """bf16_model.conv / conv_wgrad / conv_dgrad at three passes are hi*hi + lo*hi + hi*lo: against torch's float64 conv2d with the
    explicit SAME padding of oracle/network.py, and its autograd, they differ by what the split drops -- bf16 keeps 8 significant
    bits, so |lo| <= 2^-8 |x|: the lo*lo term is at most 2^-16 |a| |b|, and lo's own rounding (2^-9 |lo| per operand) adds 2 x 2^-17,
    together 2^-15 of the magnitude sum -- and on operands that are exact in bf16 by float64 rounding alone."""
    h, w, cin, cout, k, s = shape
    g = torch.Generator().manual_seed(h * 1000 + w + cin)
    N = 3
    for exact in (True, False):
        x = torch.randn(N, h, w, cin, generator=g, dtype=torch.float64).float()
        wt = torch.randn(k, k, cin, cout, generator=g, dtype=torch.float64).float()
        ho, wo = -(-h // s), -(-w // s)
        dz = torch.randn(N, ho * wo, cout, generator=g, dtype=torch.float64).float()
        if exact:
            x, wt, dz = (t.to(torch.bfloat16).float() for t in (x, wt, dz))
        xs, ws, ds = M.split(x), M.split(wt), M.split(dz)
        x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
        w64 = wt.double().permute(3, 2, 0, 1).requires_grad_(True)  # HWIO -> OIHW
        y = F.conv2d(_same_pad(x64, k, s), w64, stride=s)
        assert tuple(y.shape) == (N, cout, ho, wo)
        cot = dz.double().reshape(N, ho, wo, cout).permute(0, 3, 1, 2)
        gx, gw = torch.autograd.grad(y, (x64, w64), cot)
        tol = lambda S: (1e-12 if exact else 2.0**-15) * S + 1e-300
        v, S = M.conv(3, xs, ws, s)
        want = y.detach().permute(0, 2, 3, 1).reshape(N, ho * wo, cout)
        assert bool(((v - want).abs() <= tol(S)).all()), "conv"
        v, S = M.conv_wgrad(3, xs, ds, k, s)
        assert bool(((v - gw.permute(2, 3, 1, 0)).abs() <= tol(S)).all()), "conv_wgrad"
        v, S = M.conv_dgrad(3, ds, ws, (h, w), s)
        assert bool(((v - gx.permute(0, 2, 3, 1).reshape(N, h * w, cin)).abs() <= tol(S)).all()), "conv_dgrad"


def test_geometry_general_layers_keep_the_atari_frame():
    """conv_routes.layers without an obs is the 84x84x4 restatement tests/test_gpu_bf16_model.py has always used."""
    cfg = dict(arch="cnn", feats=(7, 9, 11, 13), ln=True)
    ls, in_p = R.layers(cfg)
    assert [(L["name"], L["h"], L["w"], L["npix"], L["K"], L["cp"]) for L in ls[:3]] == [
        ("Conv_0", 21, 21, 441, 256, 8), ("Conv_1", 11, 11, 121, 128, 16), ("Conv_2", 11, 11, 121, 144, 16)]
    assert ls[3]["in_p"] == 121 * 16 and in_p == 16
    assert R.layers(dict(arch="fc", feats=(100, 100), ln=False))[0][0]["in_p"] == 8
    assert np.all([L["ln"] is None for L in R.layers(dict(arch="fc", feats=(100, 100), ln=False))[0]])
