"""The cases of tests/test_gpu_dense_routes.py, held on the host: the plan-level half of tests/helpers/dense_routes.py against the real
plan (tests/helpers/plan_dump.cpp), the launch-level half as a literal table of the route every Dense layer of every case takes, the
coverage of the kernels and paths the cases exist for, the widths the plan refuses because no kernel runs them, and the float64
model of the LayerNorm parameter leaves (bf16_model.ln_param_grads) against torch's autograd.  No GPU."""
import os

import pytest
import torch

from tests.helpers import bf16_model as M
from tests.helpers import dense_routes as D
from tests.helpers import plan_grid as pg

CSRC = os.path.join(pg.ROOT, "is-dqn_amd", "csrc")
PRECISION = {"bf16x3": 0, "bf16": 1}  # include/isdqn_hip.h ISDQN_PRECISION_*
ALL = {**D.CASES, **D.HOST_ONLY}
RUNS = D.RUNS + [(c, "bf16") for c in D.HOST_ONLY]
RUN_IDS = [f"{c}-{p}" for c, p in RUNS]


def _config(cfg, precision):
    base = dict(pg.BASE_FC if cfg["arch"] == "fc" else pg.BASE, features=tuple(cfg["feats"]), n_actions=cfg["A"], n_heads=1 + cfg["K"],
                layer_norm=int(cfg["ln"]), batch_size=cfg["B"], precision=PRECISION[precision])
    if cfg["arch"] == "fc":
        return dict(base, obs_c=cfg["obs"][0])
    h, w, stack = cfg["obs"]
    return dict(base, obs_h=h, obs_w=w, obs_c=stack)


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dense_routes") / "plan_dump")
    assert pg.compile_dumper(CSRC, exe).wait() == 0
    return exe


def _layer_rows(body):
    rows = [l for l in body.splitlines() if l.startswith("L[")]
    return [{k: v for k, v in (t.split("=", 1) for t in l.split()[1:])} for l in rows]


@pytest.fixture(scope="module")
def plans(dumper):
    """{(case, precision): [{field: value} per layer]} of the real plan of every run"""
    out = {}
    for run, (rc, body) in zip(RUNS, pg.run_dumper(dumper, [_config(ALL[c], p) for c, p in RUNS])):
        assert rc == 0, f"{run}: refused: {body.strip()}"
        out[run] = _layer_rows(body)
    return out


@pytest.mark.parametrize("case,precision", RUNS, ids=RUN_IDS)
def test_plan_fields_equal_the_real_plan(plans, case, precision):
    """Every configuration is accepted, and the plan's own decisions for its Dense layers -- fwd_narrow, fwd_splits, gw_slabs,
    part_rows, the widths -- are what dense_routes.plan_fields computes."""
    cfg = ALL[case]
    hidden, dense = D.dense_layers(cfg)
    real = plans[(case, precision)]
    assert len(real) == len(hidden) + 1
    for L, want in zip(dense, D.plan_fields(cfg)):
        got = real[L["i"]]
        assert got["name"] == L["name"] and int(got["kind"]) == 1 and int(got["is_head"]) == int(L["head"])
        for k, v in want.items():
            assert int(got[k]) == v, f"{L['name']}.{k}: plan {got[k]}, restated {v}"
    if cfg["arch"] == "cnn":  # the convolution under the first Dense: its partial rows hold DenseDgradLN's
        i = dense[0]["i"] - 1
        assert int(real[i]["part_rows"]) == D.part_rows(cfg, hidden, i) >= D.conv2_ln(cfg)["parts"]


# The route of every Dense layer of every run (dense_routes.fmt), the head last:
#   forward: kernel, the plan's split factor, the slabs dense_post_kernel (or the head chain) sums, dense_post_kernel's column passes,
#            who finishes the row in a learn step;
#   head: the chain's <S, COLS> or generic-head; hidden: the LayerNorm / ReLU backward that writes its dz, the most rows summed into
#         one partial row, the partial rows, who sums them;
#   the data gradient it runs for the layer below; its weight gradient (fused into Adam, or slabs x K steps each).
ROUTES = {
    ("fc-ladder", "bf16x3"): [
        ("unpadded x1 slabs=1 passes=1 dense_post", "small<8> rows=32 parts=2 by=adam", "none", "slabs=2x1"),
        ("plain_narrow x1 slabs=1 passes=1 dense_post", "small<16> rows=16 parts=3 by=adam", "narrow", "slabs=2x1"),
        ("plain_narrow x2 slabs=2 passes=1 dense_post", "small<32> rows=8 parts=5 by=adam", "narrow", "slabs=2x1"),
        ("plain_big x4 slabs=4 passes=1 dense_post", "small<64> rows=4 parts=10 by=adam", "narrow", "slabs=2x1"),
        ("plain_big x7 slabs=7 passes=1 dense_post", "wide cols=2 rows=1 parts=37 by=adam", "narrow", "slabs=2x1"),
        ("plain_big x9 slabs=9 passes=2 dense_post", "wide cols=3 rows=1 parts=37 by=adam", "narrow", "slabs=2x1"),
        ("plain_big x17 slabs=17 passes=1 chain", "chain rows=1 parts=37 by=adam", "narrow", "slabs=2x1"),
        ("plain_big x3 slabs=3 passes=1 dense_post", "chain<S=1,COLS=1>", "none", "slabs=2x1")],
    ("fc-ladder-relu", "bf16x3"): [
        ("unpadded x1 slabs=1 passes=1 dense_post", "small<8> rows=32 parts=1 by=adam", "none", "slabs=1x1"),
        ("plain_narrow x1 slabs=1 passes=1 dense_post", "small<16> rows=16 parts=1 by=adam", "narrow", "fused-adam"),
        ("plain_narrow x2 slabs=2 passes=1 dense_post", "small<32> rows=8 parts=1 by=adam", "narrow", "fused-adam"),
        ("plain_big x4 slabs=4 passes=1 dense_post", "small<64> rows=4 parts=2 by=adam", "narrow", "fused-adam"),
        ("plain_big x7 slabs=7 passes=1 dense_post", "wide cols=2 rows=1 parts=5 by=adam", "narrow", "fused-adam"),
        ("plain_big x9 slabs=9 passes=2 dense_post", "wide cols=3 rows=1 parts=5 by=adam", "narrow", "fused-adam"),
        ("plain_big x17 slabs=17 passes=1 chain", "chain rows=1 parts=5 by=adam", "narrow", "fused-adam"),
        ("plain_big x3 slabs=3 passes=1 dense_post", "chain<S=1,COLS=1>", "none", "slabs=1x1")],
    ("fc-rows", "bf16x3"): [
        ("unpadded x1 slabs=1 passes=1 dense_post", "small<64> rows=12 parts=256 by=adam", "none", "slabs=66x1"),
        ("plain_big x7 slabs=7 passes=1 dense_post", "small<32> rows=16 parts=256 by=adam", "narrow", "slabs=66x1"),
        ("plain_big x4 slabs=4 passes=1 chain", "chain rows=4 parts=525 by=adam", "narrow", "slabs=66x1"),
        ("plain_big x1 slabs=1 passes=1 dense_post", "chain<S=4,COLS=1>", "none", "slabs=66x1")],
    ("fc-2048", "bf16x3"): [
        ("unpadded x1 slabs=1 passes=1 dense_post", "small<8> rows=32 parts=1 by=adam", "none", "slabs=1x1"),
        ("plain_narrow x1 slabs=1 passes=4 dense_post", "wide cols=8 rows=1 parts=9 by=adam", "narrow", "fused-adam"),
        ("plain_big x64 slabs=64 passes=1 dense_post", "generic-head", "narrow", "fused-adam")],
    ("fc-2048", "bf16"): [
        ("unpadded x1 slabs=1 passes=1 dense_post", "small<8> rows=32 parts=1 by=adam", "none", "slabs=1x1"),
        ("plain_narrow x1 slabs=1 passes=4 chain", "chain rows=1 parts=9 by=adam", "narrow", "fused-adam"),
        ("plain_big x64 slabs=64 passes=1 dense_post", "chain<S=1,COLS=4>", "none", "slabs=1x1")],
    ("fc-4096", "bf16x3"): [
        ("unpadded x1 slabs=1 passes=1 dense_post", "small<8> rows=32 parts=1 by=adam", "none", "slabs=1x1"),
        ("plain_narrow x1 slabs=1 passes=8 dense_post", "wide cols=16 rows=1 parts=3 by=adam", "narrow", "fused-adam"),
        ("plain_big x128 slabs=128 passes=1 dense_post", "generic-head", "narrow", "fused-adam")],
    ("fc-dgrad-big", "bf16"): [
        ("unpadded x1 slabs=1 passes=2 dense_post", "wide cols=4 rows=13 parts=256 by=adam", "none", "slabs=25x4"),
        ("plain_big x10 slabs=8 passes=1 chain", "chain rows=4 parts=800 by=adam", "big", "slabs=25x4"),
        ("plain_big x2 slabs=2 passes=1 dense_post", "chain<S=4,COLS=1>", "none", "slabs=100x1")],
    ("fc-dgrad-big-3072", "bf16"): [
        ("unpadded x1 slabs=1 passes=2 dense_post", "wide cols=4 rows=12 parts=256 by=adam", "none", "slabs=32x3"),
        ("plain_big x10 slabs=8 passes=1 chain", "chain rows=4 parts=768 by=adam", "narrow", "slabs=32x3"),
        ("plain_big x2 slabs=2 passes=1 dense_post", "chain<S=4,COLS=1>", "none", "slabs=96x1")],
    ("cnn-2dense", "bf16x3"): [
        ("plain_big x50 slabs=50 passes=1 dense_post", "small<32> rows=8 parts=1 by=adam", "DenseDgradLN kg=1 ksteps=4", "fused-adam"),
        ("plain_big x4 slabs=4 passes=1 chain", "chain rows=1 parts=7 by=adam", "narrow", "fused-adam"),
        ("plain_big x7 slabs=7 passes=1 dense_post", "chain<S=1,COLS=1>", "none", "slabs=1x1")],
    ("fc-headonly", "bf16x3"): [
        ("unpadded x1 slabs=1 passes=1 dense_post", "generic-head", "none", "slabs=1x1")],
}
ROUTES[("fc-ladder", "bf16")] = ROUTES[("fc-ladder", "bf16x3")]  # (no route of the ladder depends on the precision)
ROUTES[("cnn-2dense", "bf16")] = ROUTES[("cnn-2dense", "bf16x3")]
# fc-ladder through grad_on_batch: no head chain, so the last hidden layer and the head take the generic path
LADDER_GRAD_ONLY_TAIL = [
    ("plain_big x17 slabs=17 passes=1 dense_post", "small<32> rows=8 parts=5 by=adam", "narrow", "slabs=2x1"),
    ("plain_big x3 slabs=3 passes=1 dense_post", "generic-head", "narrow", "slabs=2x1")]


@pytest.mark.parametrize("case,precision", RUNS, ids=RUN_IDS)
def test_route_table_is_literal(case, precision):
    assert [D.fmt(r) for r in D.routes(ALL[case], precision)] == ROUTES[(case, precision)]


def test_gradient_only_ladder_takes_the_generic_head_path():
    for precision in D.PRECISIONS["fc-ladder"]:
        got = [D.fmt(r) for r in D.routes(D.CASES["fc-ladder"], precision, update=False)]
        assert got[:-2] == ROUTES[("fc-ladder", precision)][:-2] and got[-2:] == LADDER_GRAD_ONLY_TAIL


def test_conv_under_the_first_dense_is_fused():
    cfg = D.CASES["cnn-2dense"]
    assert D.conv2_ln(cfg) == dict(kernel="fused", rows=7, parts=25, by="reduce_rows")
    hidden, _ = D.dense_layers(cfg)
    assert D._dense_dgrad_ln(cfg, hidden) == 1 and hidden[3]["cp"] == 104 and hidden[3]["cp"] % 32 == 8  # three K steps and a ragged one


def test_head_chain_decisions_hold_under_todays_lds_formula():
    """_head_chain counts 8 bytes of per-pair state where head_chain.h now counts 12: no run here is close enough to the 150 KB limit
    for that to change its decision, and fc-2048 sits on both sides of the limit by the precision alone."""
    for case, precision in RUNS:
        cfg = ALL[case]
        hidden, dense = D.dense_layers(cfg)
        if not hidden or hidden[-1]["kind"] != 1:
            continue
        head, passes = dense[-1], 3 if precision == "bf16x3" else 1
        hc = D._head_chain(cfg, head["in_p"], head["cp"], cfg["K"], passes)
        if head["in_p"] > D.HC_THREADS * D.HC_MAX_COLS:
            assert hc is None
            continue
        S = 4 if cfg["B"] >= 1024 else 2 if cfg["B"] >= 512 else 1
        fits = D.head_chain_lds_bytes(head["in_p"], head["cp"], cfg["K"], passes, S) <= 150 * 1024
        assert (hc is not None) == fits, (case, precision)
    cfg = D.CASES["fc-2048"]
    assert D.head_chain_lds_bytes(2048, 16, 2, 1, 1) <= 150 * 1024 < D.head_chain_lds_bytes(2048, 16, 2, 3, 1)


def test_the_cases_reach_every_route_they_exist_for():
    """Each kernel form or path that the stage-level tests at the headline widths do not reach is reached by at least one Dense
    layer of one run: a case that stops selecting its route fails here."""
    seen = []
    for case, prec in RUNS:
        cfg = ALL[case]
        _, dense = D.dense_layers(cfg)
        for L, r in zip(dense, D.routes(cfg, prec)):
            seen.append((case, prec, cfg, L, r))
    seen += [("fc-ladder/grad", "bf16x3", D.CASES["fc-ladder"], L, r)
             for L, r in zip(D.dense_layers(D.CASES["fc-ladder"])[1], D.routes(D.CASES["fc-ladder"], "bf16x3", update=False))]
    any_ = lambda f: any(f(c, p, cfg, L, r) for c, p, cfg, L, r in seen)
    ln = lambda r: r.get("ln") or {}
    small = lambda tpr, **kw: lambda c, p, cfg, L, r: ln(r).get("kernel") == "small" and ln(r)["tpr"] == tpr and all(f(cfg, L, r) for f in kw.values())
    want = {
        "small<8> with padded channels": small(8, a=lambda cfg, L, r: L["c"] < L["cp"]),
        "small<16> at its edge": small(16, a=lambda cfg, L, r: L["cp"] == 64),
        "small<32> at its edge": small(32, a=lambda cfg, L, r: L["cp"] == 128),
        "small<64> with idle lanes": small(64, a=lambda cfg, L, r: L["cp"] == 200),
        "small<64> grid-stride": small(64, a=lambda cfg, L, r: ln(r)["parts"] == 256 and ln(r)["rows"] > 4),
        "small<32> grid-stride": small(32, a=lambda cfg, L, r: ln(r)["parts"] == 256 and ln(r)["rows"] > 8),
        "small<8..64> without LayerNorm": lambda c, p, cfg, L, r: not cfg["ln"] and {ln(x).get("tpr") for x in D.routes(cfg, p)} >= {8, 16, 32, 64},
        "wide without LayerNorm": lambda c, p, cfg, L, r: not cfg["ln"] and ln(r).get("kernel") == "wide",
        "wide, 2 and 3 ragged columns": lambda c, p, cfg, L, r: ln(r).get("kernel") == "wide" and ln(r)["cols"] == 3 and L["cp"] % 256,
        "wide at 8 columns (generic head at 2048)": lambda c, p, cfg, L, r: ln(r).get("kernel") == "wide" and ln(r)["cols"] == 8,
        "wide at its limit": lambda c, p, cfg, L, r: ln(r).get("kernel") == "wide" and ln(r)["cols"] == D.LN_WIDE_MAX_COLS,
        "wide grid-stride": lambda c, p, cfg, L, r: ln(r).get("kernel") == "wide" and ln(r)["parts"] == 256 and ln(r)["rows"] > 1,
        "chain": lambda c, p, cfg, L, r: ln(r).get("kernel") == "chain",
        "chain at its widest": lambda c, p, cfg, L, r: r.get("head") == dict(kernel="chain", S=1, cols=4) and L["in_p"] == 2048,
        "chain S = 4 on a 16-wide row": lambda c, p, cfg, L, r: r.get("head", {}).get("S") == 4 and L["in_p"] == 16,
        "generic head in a learn step": lambda c, p, cfg, L, r: c != "fc-ladder/grad" and r.get("head") == dict(kernel="generic") and r["dgrad"],
        "generic head in a gradient-only pass": lambda c, p, cfg, L, r: c == "fc-ladder/grad" and r.get("head") == dict(kernel="generic"),
        "the head straight on the observations": lambda c, p, cfg, L, r: L["head"] and L["unpadded"],
        "DenseDgradLN with a ragged K step": lambda c, p, cfg, L, r: (r["dgrad"] or {}).get("kernel") == "DenseDgradLN" and L["cp"] % 32,
        "narrow data gradient": lambda c, p, cfg, L, r: (r["dgrad"] or {}).get("kernel") == "narrow",
        "big data gradient": lambda c, p, cfg, L, r: (r["dgrad"] or {}).get("kernel") == "big" and c in D.CASES,
        "unpadded forward, unaligned rows": lambda c, p, cfg, L, r: r["fwd"]["kernel"] == "unpadded" and L["in_f"] % 8,
        "plain_narrow forward": lambda c, p, cfg, L, r: r["fwd"]["kernel"] == "plain_narrow",
        "plain_big forward": lambda c, p, cfg, L, r: r["fwd"]["kernel"] == "plain_big",
        "dense_post second column pass": lambda c, p, cfg, L, r: r["fwd"]["passes"] == 2 and r["fwd"]["post"] == "dense_post" and not L["unpadded"],
        "dense_post 16-slab loop and a masked tail": lambda c, p, cfg, L, r: r["fwd"]["slabs"] == 17,
        "dense_post eight 16-slab loops, no tail": lambda c, p, cfg, L, r: r["fwd"]["slabs"] == 128,
        "fused-Adam weight gradient": lambda c, p, cfg, L, r: r["wgrad"]["kernel"] == "fused-adam",
        "slab weight gradient": lambda c, p, cfg, L, r: r["wgrad"]["kernel"] == "slabs" and r["wgrad"]["slabs"] > 1,
    }
    missing = [k for k, fn in want.items() if not any_(fn)]
    assert not missing, missing
    assert D.conv2_ln(D.CASES["cnn-2dense"])["kernel"] == "fused"


# ------------------------------------------------------------------ the plan refuses what no kernel runs
def _refusal_configs():
    out = []
    for precision in (0, 1):
        for name, base, feats in (("fc", pg.BASE_FC, lambda w: (8, w)), ("cnn", dict(pg.BASE, batch_size=3), lambda w: (32, 64, 64, w)),
                                  ("cnn, second Dense", dict(pg.BASE, batch_size=3), lambda w: (32, 64, 64, 32, w))):
            for ln in (1, 0):
                for w in (4096, 4097, 4104, 8192):
                    out.append((f"{name} width {w} ln {ln} precision {precision}", w <= D.HIDDEN_MAX,
                                dict(base, features=feats(w), layer_norm=ln, precision=precision, n_heads=2, n_actions=2)))
        for name, base in (("fc", pg.BASE_FC), ("cnn", pg.BASE)):
            for heads, actions in ((16, 341), (51, 107), (8, 683), (100, 82)):  # 5456, 5457, 5464, 8200 outputs
                out.append((f"{name} head {heads}x{actions} precision {precision}", heads * actions <= D.HEAD_MAX,
                            dict(base, n_heads=heads, n_actions=actions, precision=precision)))
            out.append((f"{name} dueling head 16 x (340 + 1) precision {precision}", True, dict(base, dueling=1, n_heads=16, n_actions=340, precision=precision)))
            out.append((f"{name} dueling head 16 x (341 + 1) precision {precision}", False, dict(base, dueling=1, n_heads=16, n_actions=341, precision=precision)))
    return out


def test_plan_refuses_the_widths_no_kernel_runs(dumper):
    """A hidden Dense above 4096 columns (ln_bwd_wide_kernel holds 256 * LN_WIDE_MAX_COLS; net_launch.h keeps its own check as a
    backstop) and a scalar head row above 5456 columns (dense_post_kernel's 64 KB of LDS) are refused when the plan is built, for
    fc and cnn in both precisions, with or without LayerNorm: no network exists whose forward or learn step would fail half-way.
    4096 and 5456 themselves are accepted."""
    cfgs = _refusal_configs()
    for (name, accepted, _), (rc, body) in zip(cfgs, pg.run_dumper(dumper, [c for _, _, c in cfgs])):
        if accepted:
            assert rc == 0, f"{name}: refused: {body.strip()}"
        else:
            assert rc != 0 and body.strip() == "bad dense width", f"{name}: rc {rc} {body.strip()[:80]!r}"


def test_accepted_widths_fit_the_row_kernels(dumper):
    """At the accepted limits the launch-side limits hold: 16 columns per thread of ln_bwd_wide_kernel, and dense_post_kernel's three
    staged rows within 64 KB."""
    cfgs = [dict(pg.BASE_FC, features=(8, 4096)), dict(pg.BASE_FC, n_heads=16, n_actions=341)]
    for rc, body in pg.run_dumper(dumper, cfgs):
        assert rc == 0
        for l in _layer_rows(body):
            if int(l["kind"]) == 1:
                assert 3 * int(l["out_p"]) * 4 <= 64 * 1024
                assert int(l["is_head"]) or int(l["out_p"]) <= 256 * D.LN_WIDE_MAX_COLS


# ------------------------------------------------------------------ the model of the LayerNorm parameter leaves
@pytest.mark.parametrize("shape", [(5, 21), (37, 200), (3, 7, 64)], ids=str)
def test_ln_param_grads_against_autograd(shape):
    """bf16_model.ln_param_grads is the float64 gradient of sum(cot * relu(LayerNorm(z) gamma + beta)) with respect to gamma and beta
    with the ReLU decisions it is given; its bounds are positive and grow with E_da."""
    g = torch.Generator().manual_seed(sum(shape))
    z = torch.randn(*shape, generator=g, dtype=torch.float64)
    C = shape[-1]
    gamma = (1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    da = torch.randn(*shape, generator=g, dtype=torch.float64)
    xhat = M.ln_stats(z)[3]
    y = torch.relu(xhat * gamma + beta)
    gg, gb = torch.autograd.grad((y * da).sum(), (gamma, beta))
    mask = (y > 0).double().detach()
    dg, Eg, db, Eb = M.ln_param_grads(z, mask, da, torch.zeros_like(da), chain=shape[0] + 1)
    assert torch.allclose(dg, gg, rtol=1e-12, atol=1e-12) and torch.allclose(db, gb, rtol=1e-12, atol=1e-12)
    assert bool((Eg > 0).all()) and bool((Eb > 0).all())
    _, Eg2, _, Eb2 = M.ln_param_grads(z, mask, da, torch.full_like(da, 1e-3), chain=shape[0] + 1)
    live = mask.reshape(-1, C).sum(0) > 0
    assert bool((Eg2 >= Eg).all()) and bool((Eb2[live] > Eb[live] + 0.9e-3).all())
