"""The C51 categorical projection loss (include/isdqn_hip.h, isdqn_net_config::categorical) without a GPU: the float64 restatement of
tests/helpers/categorical.py -- gather form against the scatter form against a plain loop, the projection's properties, autograd --,
the struct layout and the header's definition, the workspace plan with the option off, the C ABI's refusals, the flag, the agents'
refusals and the entry points."""
import argparse
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from tests.helpers import categorical as c51


def _case(seed, B, n_heads, A, nb, scale=1.0, reward_scale=4.0):
    rng = np.random.default_rng(seed)
    rows = rng.normal(0, scale, (2 * B, n_heads * A * nb)).astype(np.float32).astype(np.float64)
    return (rows, rng.integers(0, A, B), (rng.normal(size=B) * reward_scale).astype(np.float32), (rng.random(B) < 0.3).astype(np.uint8),
            rng.uniform(0.2, 1.0, B).astype(np.float32))


# ------------------------------------------------------------------ 1. the projection
@pytest.mark.parametrize("nb,vmin,vmax", [(2, -1.0, 1.0), (51, -10.2, 10.2), (64, -8.0, 8.0), (65, -3.0, 5.0)])
def test_gather_form_equals_scatter_form_equals_a_plain_loop(nb, vmin, vmax):
    rng = np.random.default_rng(nb)
    n = 40
    p = torch.softmax(torch.from_numpy(rng.normal(0, 2, (n, nb))), -1)
    r = torch.from_numpy(rng.normal(0, 0.6 * (vmax - vmin), n))
    g = torch.from_numpy(np.where(rng.random(n) < 0.3, 0.0, 0.99))
    z = c51.atoms(nb, vmin, vmax)
    r[0], g[0] = z[nb // 2], 0.0  # an atom exactly on a support point: the l == u case of the textbook form
    r[1], g[1] = 0.5 * (z[0] + z[1]), 0.0  # halfway between two atoms
    b = c51.positions(r, g, nb, vmin, vmax)
    assert float(b.min()) >= 0.0 and float(b.max()) <= nb - 1 + 1e-12  # ((z_{nb-1} - z_0) / eta rounds: nb - 1 to an ulp or two)
    assert (b == 0).all(-1).any() and ((b - (nb - 1)).abs() < 1e-12).all(-1).any()  # rows clamped at either end
    mg, ms = c51.project_gather(p, b), c51.project_scatter(p, b)
    assert float((mg - ms).abs().max()) < 1e-14
    assert float((mg.sum(-1) - 1).abs().max()) < 1e-13
    for row in (0, 1, 5, n - 1):
        np.testing.assert_allclose(mg[row].numpy(), c51.project_loop(p[row].numpy(), b[row].numpy()), rtol=1e-12, atol=1e-16)
    onehot = torch.zeros(nb, dtype=torch.float64)
    onehot[nb // 2] = 1.0
    assert torch.equal(mg[0], onehot) or float((mg[0] - onehot).abs().max()) < 1e-13
    assert abs(float(mg[1][0]) - 0.5) < 1e-12 and abs(float(mg[1][1]) - 0.5) < 1e-12


def test_the_projection_preserves_the_mean_of_unclamped_rows():
    nb, vmin, vmax = 51, -10.2, 10.2
    rng = np.random.default_rng(3)
    z = c51.atoms(nb, vmin, vmax)
    p = torch.softmax(torch.from_numpy(rng.normal(0, 2, (30, nb))), -1)
    r = torch.from_numpy(rng.uniform(-0.1, 0.1, 30))
    g = torch.full((30,), 0.99, dtype=torch.float64)
    tz = r[:, None] + g[:, None] * z
    assert float(tz.min()) > float(z[0]) and float(tz.max()) < float(z[-1])  # nothing clamps
    m = c51.project_gather(p, c51.positions(r, g, nb, vmin, vmax))
    np.testing.assert_allclose((m * z).sum(-1).numpy(), (p * tz).sum(-1).numpy(), rtol=0, atol=1e-13)


def test_terminal_rows_put_all_mass_on_the_neighbours_of_r_and_r_beyond_an_end_on_the_end_atom():
    nb, vmin, vmax = 51, -10.2, 10.2
    eta = (vmax - vmin) / nb
    z = c51.atoms(nb, vmin, vmax)
    rng = np.random.default_rng(4)
    p = torch.softmax(torch.from_numpy(rng.normal(0, 2, (4, nb))), -1)
    r = torch.tensor([1.2345, -3.3, -50.0, 77.0], dtype=torch.float64)
    m = c51.project_gather(p, c51.positions(r, torch.zeros(4, dtype=torch.float64), nb, vmin, vmax))
    for row in (0, 1):
        lo = int(np.floor((float(r[row]) - float(z[0])) / eta))
        assert abs(float(m[row, lo] + m[row, lo + 1]) - 1.0) < 1e-13 and float(m[row, lo]) > 0 and float(m[row, lo + 1]) > 0
        assert abs(float((m[row] * z).sum()) - float(r[row])) < 1e-12
        assert int((m[row] > 0).sum()) == 2
    assert float(m[2, 0]) == pytest.approx(1.0, abs=1e-14) and int((m[2] > 0).sum()) == 1
    assert float(m[3, nb - 1]) == pytest.approx(1.0, abs=1e-14) and int((m[3] > 0).sum()) == 1


# ------------------------------------------------------------------ 2. the loss: plain loops, autograd
def _loss_loops(rows, action, reward, terminal, gamma_n, K, on0, tg0, A, nb, vmin, vmax, value_rows=None, selector_rows=None, weights=None):
    """c51_loss by plain loops over (transition, pair) on Python floats: an independent reading of the header."""
    import math

    rows = np.asarray(rows, np.float64)
    B = rows.shape[0] // 2
    eta = (vmax - vmin) / nb
    z = [vmin + (j + 0.5) * eta for j in range(nb)]
    on = rows[:B].reshape(B, -1, A, nb)
    val = (rows[B:] if value_rows is None else np.asarray(value_rows, np.float64)).reshape(B, -1, A, nb)
    sel = None if selector_rows is None else np.asarray(selector_rows, np.float64).reshape(B, -1, A, nb)

    def softmax(l):
        mx = max(l)
        e = [math.exp(x - mx) for x in l]
        s = sum(e)
        return [x / s for x in e], mx + math.log(s)

    q, tg, a_star, l = np.zeros((B, K)), np.zeros((B, K)), np.zeros((B, K), np.int64), np.zeros((B, K))
    dl = np.zeros((B, on.shape[1], A, nb))
    for b in range(B):
        wb = 1.0 if weights is None else float(weights[b])
        g = (1.0 - float(terminal[b])) * gamma_n
        for k in range(K):
            decide = val[b, tg0 + k] if sel is None else sel[b, on0 + k]
            qs = [sum(pj * zj for pj, zj in zip(softmax(list(decide[a]))[0], z)) for a in range(A)]
            best = 0
            for a in range(1, A):
                if qs[a] > qs[best]:
                    best = a
            a_star[b, k] = best
            p, _ = softmax(list(val[b, tg0 + k, best]))
            tg[b, k] = float(reward[b]) + g * sum(pj * zj for pj, zj in zip(p, z))
            bj = [(min(max(float(reward[b]) + g * zj, z[0]), z[-1]) - z[0]) / eta for zj in z]
            m = c51.project_loop(p, bj)
            la = list(on[b, on0 + k, int(action[b])])
            sm, lse = softmax(la)
            q[b, k] = sum(pj * zj for pj, zj in zip(sm, z))
            l[b, k] = lse - sum(mi * li for mi, li in zip(m, la))
            dl[b, on0 + k, int(action[b])] = [wb * (si - mi) / B for si, mi in zip(sm, m)]
    wv = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    return dict(q=q, targets=tg, a_star=a_star, losses=(wv[:, None] * l).mean(0), priorities=np.sqrt(((q - tg) ** 2).mean(1) + 1e-10),
                dlogits=dl.reshape(B, -1), l=l)


@pytest.mark.parametrize("shape", [(5, 3, 4, 2, -1.0, 1.0), (4, 2, 3, 7, -3.0, 3.0), (3, 1, 5, 33, -10.0, 10.0)])
def test_vectorised_helper_equals_the_plain_loops(shape):
    B, K, A, nb, vmin, vmax = shape
    n_heads = 1 + K if K > 1 else 1
    on0 = 1 if n_heads > 1 else 0
    rows, a, r, t, w = _case(B + nb, B, n_heads, A, nb, reward_scale=0.4 * (vmax - vmin))
    g = float(np.float32(0.99))
    for extra in (dict(), dict(weights=w), dict(selector_rows=rows[B:][::-1].copy()), dict(value_rows=rows[:B] * 0.5)):
        v = c51.c51_loss(rows, a, r, t, g, K, on0, 0, A, nb, vmin, vmax, **extra)
        l = _loss_loops(rows, a, r, t, g, K, on0, 0, A, nb, vmin, vmax, **extra)
        assert np.array_equal(v["a_star"].numpy(), l["a_star"])
        for name in ("q", "targets", "losses", "priorities", "dlogits", "l"):
            np.testing.assert_allclose(v[name].detach().numpy(), l[name], rtol=1e-12, atol=1e-14, err_msg=name)
    np.testing.assert_allclose(c51.expectations(rows, nb, vmin, vmax).numpy(),
                               (torch.softmax(torch.from_numpy(rows).reshape(2 * B, -1, nb), -1) * c51.atoms(nb, vmin, vmax)).sum(-1).numpy(), rtol=1e-15)


def test_selector_rows_decide_and_an_exact_tie_takes_the_first_index():
    B, K, A, nb = 6, 2, 4, 9
    rows, a, r, t, _ = _case(1, B, 1 + K, A, nb)
    sel = np.zeros_like(rows[B:]).reshape(B, 1 + K, A, nb)
    bump = c51.gauss_bump(nb, -5.0, 5.0, 2.0)
    sel[:, :, 1] = bump
    sel[:, :, 3] = bump
    dq = c51.c51_loss(rows, a, r, t, 0.97, K, 1, 0, A, nb, -5.0, 5.0, selector_rows=sel.reshape(B, -1))
    assert (dq["a_star"] == 1).all()
    plain = c51.c51_loss(rows, a, r, t, 0.97, K, 1, 0, A, nb, -5.0, 5.0)
    ex = c51.expectations(rows[B:], nb, -5.0, 5.0).reshape(B, 1 + K, A)[:, :K]
    assert torch.equal(plain["a_star"], ex.argmax(-1))


def test_gradient_equals_autograd_and_no_gradient_flows_through_any_target_term():
    B, K, A, nb, heads = 7, 3, 4, 11, 4
    rows_np, a, r, t, w = _case(11, B, heads, A, nb)
    rows = torch.tensor(rows_np, requires_grad=True)
    ref = c51.c51_loss(rows, a, r, t, float(np.float32(0.99)), K, 1, 0, A, nb, -4.0, 4.0, weights=w)
    ref["losses"].sum().backward()
    g = rows.grad.numpy()
    # heads 1 and 2 supply the distributions of pairs 1 and 2 and are learned in pairs 0 and 1: still nothing in the next-state rows,
    # and one block of nb non-zeros per (transition, pair) at (1 + k, a_b)
    assert (g[B:] == 0).all()
    np.testing.assert_allclose(g[:B], ref["dlogits"].numpy(), rtol=1e-12, atol=2e-16)
    nz = (g[:B].reshape(B, heads, A, nb) != 0).any(-1)
    assert nz.sum() == B * K and not nz[:, 0].any()
    for k in range(K):
        assert nz[np.arange(B), 1 + k, a].all()


# ------------------------------------------------------------------ 3. the C ABI's configuration
def test_config_struct_gains_categorical_between_batch_norm_and_n_bins_and_the_header_defines_it(tmp_path):
    import subprocess

    from slimdqn import _hip

    names = [f[0] for f in _hip.NetConfig._fields_]
    i = names.index("batch_norm")
    assert names[i : i + 5] == ["batch_norm", "categorical", "n_bins", "n_quantiles", "hl_min"] and names[-2:] == ["hl_sigma", "double_q"]
    j = names.index("huber_delta")
    assert names[j : j + 5] == ["huber_delta", "munchausen_tau", "munchausen_alpha", "munchausen_clip", "batch_norm"]
    assert _hip.NetConfig().categorical == 0  # built without it: off
    header = open(os.path.join(ROOT, "include", "isdqn_hip.h")).read()
    body = header[header.index("typedef struct isdqn_net_config") : header.index("} isdqn_net_config;")]
    fields = re.findall(r"^\s+(?:int32_t|float)\s+([^;]+);", body, flags=re.M)
    flat = [re.sub(r"\[.*\]", "", x).strip() for f in fields for x in f.split(",")]
    assert flat == names
    text = body[body.index("int32_t categorical;") : body.index("int32_t n_bins;")]
    for phrase in ("0: off", "1: on", "Anything else", "the FIRST index attaining max_a", "p_j   = softmax(l^val_v(s', a*))_j",
                   "g     = (1 - terminal) * gamma^n", "Tz_j  = min(max(r + g * z_j, z_0), z_{nb-1})", "b_j   = (Tz_j - z_0) / eta",
                   "m_i   = sum_j p_j * max(0, 1 - |b_j - i|)", "summed in ascending j", "logsumexp(l^on_o(s, a_b)) - sum_i m_i",
                   "losses[k] = (1 / B) sum_b w_b l_bk", "w_b (softmax(l^on)_i - m_i) / B", "No gradient flows through p, a* or any target term",
                   "z_j = c_j = hl_min + (j + 1/2) eta", "the online expectation", "sqrt(mean_k (q - target)^2 + 1e-10)", "not the cross-entropy",
                   "hl_sigma is ignored", "ISDQN_ERR_ARG", "ISDQN_ERR_UNSUPPORTED", "5456", "[-10.2, 10.2]"):
        assert phrase in text, phrase
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "isdqn_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(isdqn_net_config), offsetof(isdqn_net_config, batch_norm),'
                   ' offsetof(isdqn_net_config, categorical), offsetof(isdqn_net_config, n_bins)); return 0; }\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses
    exe = tmp_path / "layout"
    subprocess.check_call([hipcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_bn, o_c, o_nb = (int(x) for x in subprocess.check_output([str(exe)]).split())
    N = _hip.NetConfig
    assert size == ctypes.sizeof(N) and (o_bn, o_c, o_nb) == (N.batch_norm.offset, N.categorical.offset, N.n_bins.offset)
    assert o_c == o_bn + 4 and o_nb == o_c + 4 and N.double_q.offset + 4 == size


@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


def _fill(c, n_bins=0, double_q=0, n_heads=4, n_actions=9, batch_norm=0, tau=0.0, huber=0.0, n_quantiles=0, sigma=0.3):
    from slimdqn import _hip

    c.arch = _hip.ARCH_CNN
    c.obs_h, c.obs_w, c.obs_c = 84, 84, 4
    c.n_features = 4
    for i, f in enumerate((32, 64, 64, 512)):
        c.features[i] = f
    c.n_actions, c.n_heads, c.layer_norm, c.batch_size = n_actions, n_heads, 1, 32
    c.precision = _hip.PRECISION_BF16X3
    c.gamma_n, c.learning_rate, c.adam_b1, c.adam_b2, c.adam_eps = 0.99, 1e-4, 0.9, 0.999, 1e-8
    c.huber_delta = huber
    c.batch_norm = batch_norm
    c.n_bins = n_bins
    c.n_quantiles = n_quantiles
    if n_bins:
        c.hl_min, c.hl_max, c.hl_sigma = -10.0, 10.0, sigma
    c.double_q = double_q
    c.munchausen_tau, c.munchausen_alpha, c.munchausen_clip = tau, 0.9, -1.0
    return c


def _cfg(categorical=0, **kw):
    from slimdqn import _hip

    c = _fill(_hip.NetConfig(), **kw)
    c.categorical = categorical
    return c


def _region_table(lib, cfg, names):
    out = {}
    for n in names:
        off, size = ctypes.c_int64(), ctypes.c_int64()
        rc = lib.isdqn_net_workspace_region(ctypes.byref(cfg), n.encode(), ctypes.byref(off), ctypes.byref(size))
        out[n] = (off.value, size.value) if rc == 0 else None
    return out


def _bytes(lib, cfg):
    b = ctypes.c_int64()
    return lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)), b.value


REGIONS = ["q", "logits", "dout", "da", "slab", "q_values", "targets", "dbh", "adam_consts", "loss_partials", "wsplit", "q_target", "logits_target",
           "act/Conv_0", "z/Conv_1", "dz/Conv_2", "act/Dense_0", "red/Dense_0", "part/Dense_0", "gw/Conv_0", "gw/Dense_0", "gw/Dense_1"]
# (configuration, workspace bytes, crc32 of the json of [(region, byte offset, byte size)] over REGIONS) of the headline network at
# B = 32, recorded from the library as it was before the field existed
OFF_CASES = [(dict(), 70920448, 528501311), (dict(n_bins=51), 79239424, 3654524767), (dict(double_q=1), 70925568, 3598022443),
             (dict(n_bins=51, double_q=1), 79480064, 3377133642), (dict(tau=0.03), 70930688, 3294758429),
             (dict(n_heads=1, huber=1.0), 70808832, 1256237255), (dict(n_quantiles=51, huber=1.0), 79239424, 3654524767)]


@pytest.mark.parametrize("kw,bytes_before,crc_before", OFF_CASES)
def test_workspace_plan_with_the_option_off_is_the_plan_without_the_field(lib, kw, bytes_before, crc_before):
    import zlib

    from slimdqn import _hip

    never = _fill(_hip.NetConfig(), **kw)  # a configuration that never set the field
    off = _cfg(0, **kw)
    (rc0, b0), (rc1, b1) = _bytes(lib, never), _bytes(lib, off)
    assert rc0 == rc1 == _hip.OK and b0 == b1 == bytes_before
    r0, r1 = _region_table(lib, never, REGIONS), _region_table(lib, off, REGIONS)
    tab = [(n, r0[n][0], r0[n][1]) if r0[n] is not None else (n, None, None) for n in REGIONS]
    assert zlib.crc32(json.dumps(tab).encode()) == crc_before
    assert r0 == r1 and r0["q"] is not None and (r0["logits"] is None) == ("n_bins" not in kw and "n_quantiles" not in kw)
    n0, n1 = ctypes.c_int64(), ctypes.c_int64()
    cnt = ctypes.c_int32()
    assert lib.isdqn_net_param_layout(ctypes.byref(never), ctypes.byref(n0), None, 0, ctypes.byref(cnt)) == _hip.OK
    assert lib.isdqn_net_param_layout(ctypes.byref(off), ctypes.byref(n1), None, 0, ctypes.byref(cnt)) == _hip.OK
    assert n0.value == n1.value


@pytest.mark.parametrize("kw", [dict(n_bins=51), dict(n_bins=51, double_q=1), dict(n_bins=2, n_heads=1)])
def test_the_categorical_plan_is_the_histogram_plan(lib, kw):
    """The option switches the loss kernel and nothing else: same workspace, same regions, same parameters; hl_sigma may be 0."""
    from slimdqn import _hip

    hist, cat = _cfg(0, **kw), _cfg(1, **kw, sigma=0.0)
    (rc0, b0), (rc1, b1) = _bytes(lib, hist), _bytes(lib, cat)
    assert rc0 == rc1 == _hip.OK and b0 == b1
    assert _region_table(lib, hist, REGIONS) == _region_table(lib, cat, REGIONS)
    assert _bytes(lib, _cfg(0, **kw, sigma=0.0))[0] == _hip.ERR_ARG  # HL-Gauss still needs its sigma


def test_every_refusal_returns_its_code_and_names_the_field(lib):
    from slimdqn import _hip

    table = [
        (dict(categorical=2, n_bins=51), _hip.ERR_ARG, b"categorical"),
        (dict(categorical=-1, n_bins=51), _hip.ERR_ARG, b"categorical"),
        (dict(categorical=2), _hip.ERR_ARG, b"categorical"),
        (dict(categorical=1), _hip.ERR_ARG, b"categorical"),  # n_bins = 0
        (dict(categorical=1, n_quantiles=32, huber=1.0), _hip.ERR_ARG, b"categorical"),
        (dict(categorical=1, n_bins=51, tau=0.03), _hip.ERR_UNSUPPORTED, b"categorical"),
        # refused exactly as the histogram heads refuse them: the same code and the same message as with categorical = 0
        (dict(categorical=1, n_bins=51, huber=1.0), _hip.ERR_ARG, None),
        (dict(categorical=1, n_bins=51, batch_norm=1), _hip.ERR_UNSUPPORTED, None),
        (dict(categorical=1, n_bins=2, n_heads=66, n_actions=2), _hip.ERR_UNSUPPORTED, None),  # K = 65 regressed heads
        (dict(categorical=1, n_bins=32, n_heads=10, n_actions=18), _hip.ERR_UNSUPPORTED, None),  # 5760 outputs > 5456
        (dict(categorical=1, n_bins=1), _hip.ERR_ARG, None),
        (dict(categorical=1, n_bins=257), _hip.ERR_ARG, None),
    ]
    for kw, code, word in table:
        rc, _ = _bytes(lib, _cfg(**kw))
        msg = bytes(lib.isdqn_last_error())
        assert rc == code, (kw, rc)
        if word is not None:
            assert word in msg, (kw, msg)
        else:
            rc0, _ = _bytes(lib, _cfg(**dict(kw, categorical=0)))
            assert rc0 == code and bytes(lib.isdqn_last_error()) == msg, (kw, msg)
    ok = [dict(categorical=1, n_bins=2), dict(categorical=1, n_bins=256, n_heads=2, n_actions=5), dict(categorical=1, n_bins=51, double_q=1),
          dict(categorical=1, n_bins=51, sigma=0.0), dict(categorical=1, n_bins=200, n_heads=1), dict(categorical=1, n_bins=2, n_heads=65, n_actions=2),
          dict(categorical=1, n_bins=31, n_heads=4, n_actions=44)]  # 5456 outputs
    for kw in ok:
        assert _bytes(lib, _cfg(**kw))[0] == _hip.OK, kw


# ------------------------------------------------------------------ 4. the flag
def _parse(argv, algo="isdqn"):
    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    getattr(pa, f"add_{algo}_arguments")(parser)
    names = pa.add_engine_arguments(parser)
    return vars(parser.parse_args(["-en", "x_Game", "-s", "1"] + argv)), names, parser


def test_the_flag_its_default_and_histogram_loss_kwargs():
    from experiments.base import parser_argument as pa

    p, names, parser = _parse([])
    assert "categorical" in names and p["categorical"] is False
    assert "categorical" not in pa.histogram_loss_kwargs(p)  # without -cat: the keywords of before the flag
    for algo in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn"):
        kw = pa.histogram_loss_kwargs(_parse(["-hl", "-cat", "-nb", "51", "-minn", "-10.2", "-maxn", "10.2"], algo=algo)[0])
        assert kw == dict(n_bins=51, min_value=-10.2, max_value=10.2, sigma=3.0, categorical=True)
    assert pa.histogram_loss_kwargs(_parse(["-hl", "--categorical"])[0])["categorical"] is True
    assert pa.histogram_loss_kwargs(_parse(["-hl"])[0]) == dict(n_bins=50, min_value=-100.0, max_value=100.0, sigma=3.0)
    help_text = " ".join(parser.format_help().split())
    cat = help_text[help_text.index("--categorical"):][:500]
    assert "C51" in cat and "-hl" in cat and "-10.2" in cat


def test_parameters_json_keeps_the_reference_groups(tmp_path):
    """Like -hl, which it modifies, -cat stays out of parameters.json."""
    from experiments.base.utils import prepare_logs

    for env, algo in (("atari", "isdqn"), ("atari", "dqn"), ("lunar_lander", "tfdqn")):
        p = prepare_logs(env, algo, ["-en", f"b{algo}_Game", "-dw", "-s", "1", "-hl", "-cat", "-nb", "51"], root=str(tmp_path))
        assert p["categorical"] is True and p["histogram_loss"] is True
        on = json.load(open(tmp_path / env / "exp_output" / f"b{algo}_Game" / "parameters.json"))
        plain_p = prepare_logs(env, algo, ["-en", f"a{algo}_Game", "-dw", "-s", "1"], root=str(tmp_path))
        plain = json.load(open(tmp_path / env / "exp_output" / f"a{algo}_Game" / "parameters.json"))
        assert plain_p["categorical"] is False
        for stored in (on, plain):
            assert not any("categorical" in k for k in list(stored[algo]) + list(stored["shared_parameters"]))
        assert set(on[algo]) == set(plain[algo]) and set(on["shared_parameters"]) == set(plain["shared_parameters"])


@pytest.mark.parametrize("env,algo,extra", [("atari", "isdqn", []), ("atari", "isdqn", ["-qr"]), ("atari", "isdqn", ["-hl", "-mq"]),
                                            ("atari", "dqn", []), ("atari", "tfdqn", ["-hl", "-mq"]), ("lunar_lander", "dqn", ["-qr"]),
                                            ("atari", "analysisdqn", []), ("atari", "analysistfdqn", ["-qr"])])
def test_cat_without_hl_or_with_qr_or_mq_is_refused_before_anything_is_written(tmp_path, env, algo, extra):
    from experiments.base.utils import prepare_logs
    from slimdqn import _engine

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, ["-en", "c_Game", "-dw", "-s", "1", "-cat"] + extra, root=str(tmp_path))
    assert "categorical" in str(e.value)
    assert str(e.value) in (_engine.CATEGORICAL_NEEDS_HISTOGRAM, _engine.CATEGORICAL_QUANTILE_REFUSED, _engine.CATEGORICAL_MUNCHAUSEN_REFUSED)
    assert not (tmp_path / env).exists()  # before the output directory is created
    prepare_logs(env, algo, ["-en", "c_Game", "-dw", "-s", "1", "-cat", "-hl"], root=str(tmp_path))


def test_entry_points_pass_the_keyword_to_their_agents():
    base = os.path.join(ROOT, "is-dqn_amd", "experiments")
    for rel in ("atari/isdqn.py", "atari/dqn.py", "atari/analysisdqn.py", "lunar_lander/isdqn.py", "lunar_lander/dqn.py",
                "atari/tfdqn.py", "atari/analysistfdqn.py", "lunar_lander/tfdqn.py"):
        src = open(os.path.join(base, rel)).read()
        assert "**histogram_loss_kwargs(p)" in src, rel  # (-cat travels in these keywords)


# ------------------------------------------------------------------ 5. the agents
def test_agents_take_the_keyword_and_refuse_the_three_combinations_before_an_engine_is_built():
    from slimdqn import _engine
    from slimdqn._engine import QNetEngine
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    for f in (QNetEngine.__init__, DQN.__init__, iSDQN.__init__, TFDQN.__init__):
        assert inspect.signature(f).parameters["categorical"].default is False
    isd = lambda **kw: iSDQN(0, (84, 84, 4), 4, 2, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    ana = lambda **kw: AnalysisDQN(0, (84, 84, 4), 4, 2, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    dqn = lambda **kw: DQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    tf = lambda **kw: TFDQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    atf = lambda **kw: AnalysisTFDQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    eng = lambda **kw: QNetEngine((84, 84, 4), 4, 3, [8, 8, 8, 16], "cnn", True, 4, **kw)
    # raised before an engine is built (no GPU here: building one would raise something else)
    for make in (isd, ana, dqn, tf, atf, eng):
        with pytest.raises(ValueError) as e:
            make(categorical=True)
        assert str(e.value) == _engine.CATEGORICAL_NEEDS_HISTOGRAM
        with pytest.raises(ValueError) as e:
            make(categorical=True, n_quantiles=16)
        assert str(e.value) == _engine.CATEGORICAL_QUANTILE_REFUSED
        with pytest.raises(ValueError) as e:
            make(categorical=True, n_bins=51, n_quantiles=16)
        assert str(e.value) == _engine.CATEGORICAL_QUANTILE_REFUSED
        with pytest.raises(ValueError) as e:
            make(categorical=True, n_bins=51, munchausen_tau=0.03)
        assert str(e.value) == _engine.CATEGORICAL_MUNCHAUSEN_REFUSED
    for msg in (_engine.CATEGORICAL_NEEDS_HISTOGRAM, _engine.CATEGORICAL_QUANTILE_REFUSED, _engine.CATEGORICAL_MUNCHAUSEN_REFUSED):
        assert "categorical" in msg
