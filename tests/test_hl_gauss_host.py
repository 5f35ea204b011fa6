"""CPU checks of the HL-Gauss histogram loss option: the CLI flags (the reference's add_histogram_loss_parameters,
experiments/base/parser_argument.py:199-228, plus -hl), the float64 restatement the GPU tests compare against
(tests/helpers/hl_gauss.py), and the host-only parameter layout / validation of the C ABI."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.helpers import hl_gauss as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parser():
    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    pa.add_isdqn_arguments(parser)
    pa.add_engine_arguments(parser)
    return parser


BASE_ARGV = ["-en", "x_Game", "-s", "1"]


def test_parser_histogram_flags_keep_the_reference_names_types_and_defaults():
    p = vars(_parser().parse_args(BASE_ARGV))
    assert p["histogram_loss"] is False
    assert p["n_bins"] == 50 and isinstance(p["n_bins"], int)
    # (the reference writes the three float defaults as the ints -100, 100 and 3, which argparse passes through as they are)
    assert (p["min_value"], p["max_value"], p["sigma"]) == (-100, 100, 3)
    q = vars(_parser().parse_args(BASE_ARGV + ["-hl", "-nb", "51", "-minn", "-10", "-maxn", "10.5", "-sigma", "0.3"]))
    assert (q["histogram_loss"], q["n_bins"], q["min_value"], q["max_value"], q["sigma"]) == (True, 51, -10.0, 10.5, 0.3)
    assert all(isinstance(q[k], float) for k in ("min_value", "max_value", "sigma"))
    q = vars(_parser().parse_args(BASE_ARGV + ["--histogram_loss", "--n_bins", "7", "--min_value", "1", "--max_value", "2", "--sigma", "4"]))
    assert (q["histogram_loss"], q["n_bins"], q["min_value"], q["max_value"], q["sigma"]) == (True, 7, 1.0, 2.0, 4.0)


def test_short_flags_n_nb_and_nbi_are_three_options():
    p = vars(_parser().parse_args(BASE_ARGV + ["-n", "3", "-nb", "51", "-nbi", "4"]))
    assert (p["update_horizon"], p["n_bins"], p["n_bellman_iterations"]) == (3, 51, 4)


def test_histogram_flags_are_engine_extras_and_off_means_zero_bins():
    from experiments.base import parser_argument as pa

    engine = pa.add_engine_arguments(argparse.ArgumentParser())
    assert {"histogram_loss", "n_bins", "min_value", "max_value", "sigma"} <= set(engine)
    isdqn = pa.add_isdqn_arguments(argparse.ArgumentParser())
    assert not {"n_bins", "min_value", "max_value", "sigma"} & set(isdqn)
    off = vars(_parser().parse_args(BASE_ARGV + ["-nb", "51"]))
    assert pa.histogram_loss_kwargs(off) == dict(n_bins=0, min_value=-100.0, max_value=100.0, sigma=3.0)
    on = vars(_parser().parse_args(BASE_ARGV + ["-hl", "-nb", "51"]))
    assert pa.histogram_loss_kwargs(on)["n_bins"] == 51


# ------------------------------------------------------------------ the float64 projection
NB, VMIN, VMAX = 51, -10.0, 10.0
ETA = (VMAX - VMIN) / NB
SIGMA = 0.75 * ETA


def test_projection_is_a_distribution():
    y = torch.tensor([-50.0, -10.0, -9.9, -3.3, 0.0, 0.123, 7.5, 10.0, 1e6], dtype=torch.float64)
    p = hl.projection(y, NB, VMIN, VMAX, SIGMA)
    assert p.shape == (9, NB)
    assert (p >= 0).all()
    assert torch.allclose(p.sum(-1), torch.ones(9, dtype=torch.float64), atol=1e-12)


def test_projection_mean_is_the_target_on_a_centre_inside_the_support():
    c = hl.centres(NB, VMIN, VMAX)
    for j in (10, 20, 25, 33, 40):
        p = hl.projection(c[j], NB, VMIN, VMAX, SIGMA)
        assert abs(float((p * c).sum()) - float(c[j])) < 1e-9, j


def test_target_far_outside_the_support_is_finite_after_the_clamp():
    for y in (-1e30, -1e4, 1e4, 1e30):
        p = hl.projection(torch.tensor(y, dtype=torch.float64), NB, VMIN, VMAX, SIGMA)
        assert torch.isfinite(p).all() and abs(float(p.sum()) - 1.0) < 1e-12
    # in float32 without the clamp the normaliser underflows: the reason for the clamp
    e = hl.edges(NB, VMIN, VMAX).float()
    u = torch.special.erf((e - 1e4) / (2 ** 0.5 * SIGMA))
    assert float(u[-1] - u[0]) == 0.0


def test_softmax_minus_p_is_the_autograd_gradient_of_the_cross_entropy():
    rng = np.random.default_rng(0)
    B, K, A, n_heads = 5, 3, 4, 4
    logits = torch.tensor(rng.normal(0, 1.5, (2 * B, n_heads * A * NB)), dtype=torch.float64, requires_grad=True)
    action = rng.integers(0, A, B)
    reward = rng.normal(0, 20, B)  # some targets outside [v_min, v_max]
    terminal = (rng.random(B) < 0.4).astype(np.uint8)
    out = hl.hl_loss(logits, action, reward, terminal, 0.97, K, 1, 0, A, NB, VMIN, VMAX, SIGMA)
    out["losses"].sum().backward()
    g = logits.grad
    assert torch.allclose(g[:B], out["dlogits"], rtol=1e-12, atol=1e-15)
    assert (g[B:] == 0).all()  # next-state rows carry no gradient
    # losses[k] = mean_b CE = mean_b (logsumexp(l) - sum_j p_j l_j), and CE >= entropy of the target histogram
    p = hl.projection(out["targets"], NB, VMIN, VMAX, SIGMA)
    ent = -(p * torch.log(p.clamp_min(1e-300))).sum(-1)
    assert (out["ce"] >= ent - 1e-12).all()
    # the expectation of the online head at the taken action is q
    ex = hl.expectations(logits[:B].detach(), NB, VMIN, VMAX).reshape(B, n_heads, A)
    assert torch.allclose(out["q"], ex[torch.arange(B)[:, None], torch.arange(1, 1 + K)[None, :], torch.as_tensor(action)[:, None]])


# ------------------------------------------------------------------ the helper's keyword arguments
def _rows_case(seed, B, K, A, nb, n_heads):
    rng = np.random.default_rng(seed)
    return dict(rows=torch.tensor(rng.normal(0, 1.5, (2 * B, n_heads * A * nb)), dtype=torch.float64),
                value_rows=torch.tensor(rng.normal(0, 1.5, (B, n_heads * A * nb)), dtype=torch.float64),
                action=rng.integers(0, A, B), reward=rng.normal(0, 8, B), terminal=(rng.random(B) < 0.4).astype(np.uint8),
                weights=rng.uniform(0.2, 1.7, B), discount=rng.uniform(0.3, 0.99, B))


@pytest.mark.parametrize("A", [1, 4])
def test_keyword_defaults_leave_the_result_unchanged_and_equal_double_q(A):
    """With every keyword at its default the result is the bits of the call without them; selector_rows / value_rows / weights give
    what tests/helpers/double_q.py gives with ``hist`` -- an independent writing of the same definition."""
    from tests.helpers import double_q as dq

    B, K, n_heads, nb = 6, 3, 4, 17
    c = _rows_case(3, B, K, A, nb, n_heads)
    args = (c["action"], c["reward"], c["terminal"], 0.97, K, 1, 0, A, nb, VMIN, VMAX, SIGMA)
    plain = hl.hl_loss(c["rows"], *args)
    same = hl.hl_loss(c["rows"], *args, value_rows=None, selector_rows=None, weights=None, discount=None, y=None)
    ones = hl.hl_loss(c["rows"], *args, value_rows=c["rows"][B:], weights=np.ones(B), discount=np.full(B, 0.97), y=plain["targets"])
    for k in ("losses", "q", "targets", "priorities", "dlogits", "ce"):
        assert torch.equal(plain[k], same[k]) and torch.equal(plain[k], ones[k]), k
    hist = dict(nb=nb, vmin=VMIN, vmax=VMAX, sigma=SIGMA)
    for vr in (None, c["value_rows"]):
        want = dq.double_q(c["rows"], c["action"], c["reward"], c["terminal"], 0.97, K, 1, 0, A, value_rows=vr, weights=c["weights"], hist=hist)
        got = hl.hl_loss(c["rows"], *args, value_rows=vr, selector_rows=c["rows"][B:], weights=c["weights"])
        for mine, theirs in (("targets", "targets"), ("q", "q"), ("losses", "losses"), ("priorities", "priorities"), ("dlogits", "dq")):
            np.testing.assert_allclose(got[mine].numpy(), want[theirs], rtol=1e-13, atol=1e-15, err_msg=mine)
        if A > 1:  # the selector bites: a* leaves the value head's own greedy action somewhere
            assert (want["a_star"] != want["greedy"]).any()
            assert not torch.equal(got["targets"], hl.hl_loss(c["rows"], *args, value_rows=vr)["targets"])


def test_selector_takes_the_first_of_two_equal_expectations():
    B, K, A, n_heads, nb = 3, 1, 3, 2, 5
    c = _rows_case(5, B, K, A, nb, n_heads)
    sel = c["rows"][B:].clone().reshape(B, n_heads, A, nb)
    sel[:, 1, 0] = 0.0
    sel[:, 1, 0, 0] = 30.0  # a poor action 0 (all mass on the lowest bin), then two bit-equal better ones
    sel[:, 1, 2] = sel[:, 1, 1]
    val = c["value_rows"].reshape(B, n_heads, A, nb)
    got = hl.hl_loss(c["rows"], c["action"], c["reward"], c["terminal"], 0.9, K, 1, 0, A, nb, VMIN, VMAX, SIGMA, value_rows=c["value_rows"],
                     selector_rows=sel.reshape(B, -1))
    want = torch.as_tensor(c["reward"]) + (1.0 - torch.as_tensor(c["terminal"], dtype=torch.float64)) * 0.9 * hl.expectations(val[:, 0, 1], nb, VMIN, VMAX)[:, 0]
    assert torch.allclose(got["targets"][:, 0], want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("A", [1, 4])
def test_dlogits_is_autograd_of_the_helpers_own_loss_with_every_keyword(A):
    B, K, n_heads, nb = 5, 2, 3, 9
    c = _rows_case(7, B, K, A, nb, n_heads)
    rows = c["rows"].clone().requires_grad_(True)
    y = torch.tensor(np.random.default_rng(1).uniform(VMIN - 3, VMAX + 3, (B, K)))
    for kw in (dict(), dict(y=y)):
        rows.grad = None
        out = hl.hl_loss(rows, c["action"], c["reward"], c["terminal"], 0.97, K, 1, 0, A, nb, VMIN, VMAX, SIGMA, value_rows=c["value_rows"],
                         selector_rows=rows[B:], weights=c["weights"], discount=c["discount"], **kw)
        out["losses"].sum().backward()
        assert torch.allclose(rows.grad[:B], out["dlogits"], rtol=1e-12, atol=1e-15)
        assert (rows.grad[B:] == 0).all()
        assert torch.allclose(out["p"].sum(-1), torch.ones(B, K, dtype=torch.float64), atol=1e-12)
    # per-row discount and y are what they say: the targets follow the discount, the projection follows y
    nt = 1.0 - torch.as_tensor(c["terminal"], dtype=torch.float64)
    base = hl.hl_loss(rows.detach(), c["action"], c["reward"], c["terminal"], 1.0, K, 1, 0, A, nb, VMIN, VMAX, SIGMA)
    disc = hl.hl_loss(rows.detach(), c["action"], c["reward"], c["terminal"], 1.0, K, 1, 0, A, nb, VMIN, VMAX, SIGMA, discount=c["discount"])
    r = torch.as_tensor(c["reward"])[:, None]
    assert torch.allclose(disc["targets"] - r, (base["targets"] - r) * torch.as_tensor(c["discount"])[:, None] * nt[:, None], rtol=1e-13, atol=1e-15)
    assert torch.equal(out["p"], hl.projection(y, nb, VMIN, VMAX, SIGMA)) and torch.equal(out["targets"], hl.hl_loss(
        rows.detach(), c["action"], c["reward"], c["terminal"], 0.97, K, 1, 0, A, nb, VMIN, VMAX, SIGMA, value_rows=c["value_rows"],
        selector_rows=rows[B:].detach(), discount=c["discount"])["targets"])


def test_float32_evaluation_of_the_helper_stays_float32_and_close():
    B, K, A, n_heads, nb = 4, 2, 3, 3, 64
    c = _rows_case(9, B, K, A, nb, n_heads)
    rows = c["rows"].float().double()
    args = (c["action"], c["reward"].astype(np.float32), c["terminal"], 0.97, K, 1, 0, A, nb, -8.0, 8.0, 0.75 * 0.25)
    lo, hi = hl.hl_loss(rows, *args, dtype=torch.float32), hl.hl_loss(rows, *args)
    assert lo["dlogits"].dtype == torch.float32 and lo["losses"].dtype == torch.float32 and hi["dlogits"].dtype == torch.float64
    assert float((lo["dlogits"].double() - hi["dlogits"]).abs().max()) < 1e-6 and float((lo["losses"].double() - hi["losses"]).abs().max()) < 1e-5


# ------------------------------------------------------------------ C ABI, host-only
@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


def _cfg(n_bins=51, hl_min=-10.0, hl_max=10.0, sigma=0.3, huber=0.0, bn=0, arch="cnn"):
    from slimdqn import _hip

    cfg = _hip.NetConfig()
    if arch == "cnn":
        cfg.arch, cfg.obs_h, cfg.obs_w, cfg.obs_c = _hip.ARCH_CNN, 84, 84, 4
        feats = (32, 64, 64, 512)
    else:
        cfg.arch, cfg.obs_h, cfg.obs_w, cfg.obs_c = _hip.ARCH_FC, 1, 1, 8
        feats = (100, 100)
    cfg.n_features = len(feats)
    for i, f in enumerate(feats):
        cfg.features[i] = f
    cfg.n_actions, cfg.n_heads, cfg.layer_norm, cfg.batch_size = 9, 10, 1, 256
    cfg.huber_delta, cfg.batch_norm = huber, bn
    cfg.n_bins, cfg.hl_min, cfg.hl_max, cfg.hl_sigma = n_bins, hl_min, hl_max, sigma
    return cfg


def _layout(lib, cfg):
    from slimdqn import _hip

    n, cnt = ctypes.c_int64(), ctypes.c_int32()
    rc = lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), None, 0, ctypes.byref(cnt))
    if rc:
        return rc, None
    infos = (_hip.TensorInfo * cnt.value)()
    assert lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)) == 0
    return rc, {i.name.decode(): i for i in infos}


@pytest.mark.parametrize("arch", ["cnn", "fc"])
def test_param_layout_of_histogram_heads(lib, arch):
    rc, infos = _layout(lib, _cfg(arch=arch))
    assert rc == 0
    head = infos["Dense_1/kernel"] if arch == "cnn" else infos["Dense_2/kernel"]
    F = 512 if arch == "cnn" else 100
    assert tuple(head.flax_shape[:2]) == (F, 10 * 9 * 51)
    bias = infos["Dense_1/bias"] if arch == "cnn" else infos["Dense_2/bias"]
    assert bias.flax_shape[0] == 10 * 9 * 51
    # n_bins = 0 keeps the scalar head, whatever the other three fields hold
    rc, infos0 = _layout(lib, _cfg(n_bins=0, hl_min=0.0, hl_max=0.0, sigma=0.0, arch=arch))
    assert rc == 0
    head0 = infos0["Dense_1/kernel"] if arch == "cnn" else infos0["Dense_2/kernel"]
    assert tuple(head0.flax_shape[:2]) == (F, 90)


def test_workspace_regions_of_histogram_heads(lib):
    from slimdqn import _hip

    def size(cfg, name):
        off, sz = ctypes.c_int64(), ctypes.c_int64()
        rc = lib.isdqn_net_workspace_region(ctypes.byref(cfg), name.encode(), ctypes.byref(off), ctypes.byref(sz))
        return rc, sz.value

    nlog_p = (10 * 9 * 51 + 7) // 8 * 8
    cfg = _cfg()
    assert size(cfg, "logits") == (0, 512 * nlog_p * 4)
    assert size(cfg, "q")[1] == (512 * 96 * 4 + 255) // 256 * 256
    assert size(cfg, "dout")[1] == (256 * nlog_p * 4 + 255) // 256 * 256
    assert size(_cfg(n_bins=0), "logits")[0] == _hip.ERR_ARG  # no logit rows without the histogram loss


@pytest.mark.parametrize("kw, rc", [
    (dict(n_bins=1), "ERR_ARG"),
    (dict(n_bins=257), "ERR_ARG"),
    (dict(n_bins=-3), "ERR_ARG"),
    (dict(hl_min=5.0, hl_max=5.0), "ERR_ARG"),
    (dict(hl_min=5.0, hl_max=-5.0), "ERR_ARG"),
    (dict(sigma=0.0), "ERR_ARG"),
    (dict(sigma=-1.0), "ERR_ARG"),
    (dict(huber=1.0), "ERR_ARG"),
    (dict(bn=1), "ERR_UNSUPPORTED"),
    (dict(n_bins=2), "OK"),
    (dict(n_bins=60, arch="fc"), "OK"),  # 10 * 9 * 60 = 5400 logits
    (dict(n_bins=61, arch="fc"), "ERR_UNSUPPORTED"),  # 5490: wider than the head row the forward stages in LDS
])
def test_param_layout_validates_the_histogram_settings(lib, kw, rc):
    from slimdqn import _hip

    got, _ = _layout(lib, _cfg(**kw))
    assert got == getattr(_hip, rc)
