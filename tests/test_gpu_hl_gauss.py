"""The HL-Gauss histogram loss on the GPU (include/isdqn_hip.h, isdqn_net_config::n_bins; csrc/hl_gauss.h) against the float64
restatement of tests/helpers/hl_gauss.py: the loss kernel on the HIP run's own logits, the whole path against float64 logits of the
oracle network, gradients and Adam, acting on expectations, shift_params on whole histograms, the single-head baselines, run-to-run
bit identity, the captured multi-step replay and the Atari entry point with -hl."""
import json

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.gpu_helpers import ADAM_B1, ADAM_B2, adam64, make_frame_batch, perturbed_params
from tests.helpers import hl_gauss as hl

pytestmark = pytest.mark.gpu

NB, VMIN, VMAX = 51, -10.0, 10.0
SIGMA = 0.75 * (VMAX - VMIN) / NB
TOL = {"bf16x3": dict(q=1e-3, loss=1e-3, grad=3e-3), "bf16": dict(q=8e-2, loss=5e-2, grad=2.5e-1)}
FC_OBS = (8,)


def _engine(feats, A, n_heads, B, arch="cnn", obs=(84, 84, 4), ln=True, precision="bf16x3", seed=0, lr=1e-3, gamma_n=0.99):
    from slimdqn._engine import QNetEngine

    params = perturbed_params(seed, obs, feats, arch, n_heads * A * NB, ln)
    eng = QNetEngine(obs, A, n_heads, feats, arch, ln, B, gamma_n=gamma_n, learning_rate=lr, adam_eps=1.5e-4, precision=precision,
                     n_bins=NB, min_value=VMIN, max_value=VMAX, sigma=SIGMA)
    eng.import_flax(params)
    return eng, params


class _Batch:
    """One batch in both forms: the engine's C batch and the float64 network input [states; next states]."""

    def __init__(self, eng, arch, obs, B, A, seed, reward_scale=15.0):
        rng = np.random.default_rng(seed + 100)
        if arch == "fc":
            s = rng.normal(size=(B, obs[0])).astype(np.float32)
            ns = rng.normal(size=(B, obs[0])).astype(np.float32)
            self.action = rng.integers(0, A, B).astype(np.int32)
            self.terminal = (rng.random(B) < 0.3).astype(np.uint8)
            self.x_state, self.x_next = torch.from_numpy(s), torch.from_numpy(ns)
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            self.reward = (rng.normal(size=B) * reward_scale).astype(np.float32)
            self.cb = eng.make_batch(state=d(s), next_state=d(ns), action=d(self.action), reward=d(self.reward), terminal=d(self.terminal))
        else:
            frames, ids, action, _, terminal, ref = make_frame_batch(B, A, seed=seed, h=obs[0], w=obs[1], stack=obs[2])
            self.action, self.terminal = action, terminal
            self.reward = (rng.normal(size=B) * reward_scale).astype(np.float32)  # some targets outside [v_min, v_max]
            self.x_state, self.x_next = torch.from_numpy(ref.state), torch.from_numpy(ref.next_state)
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            self.fr, self.ids, self.stride = d(frames), d(ids), frames.shape[1]
            self.cb = eng.make_batch(frames=self.fr, frame_stride=self.stride, frame_ids=self.ids, action=d(action), reward=d(self.reward),
                                     terminal=d(terminal))

    def obs_kw(self, rows):
        """forward / best_actions keywords for the first `rows` states"""
        if hasattr(self, "fr"):
            stack = self.ids.shape[1] // 2
            ids = self.ids[:rows, :stack].contiguous()
            return dict(frames=self.fr, frame_stride=self.stride, frame_ids=ids)
        return dict(obs=self.x_state[:rows].cuda())


def _logits(eng, B):
    """the HIP run's own logit rows [2B][n_heads * A * nb] (region "logits": [2B][padded to 8])"""
    nlog = eng.n_heads * eng.n_actions * NB
    nlog_p = (nlog + 7) // 8 * 8
    return eng.region("logits")[: 2 * B * nlog_p].reshape(2 * B, nlog_p)[:, :nlog].double().cpu()


def _oracle_logits(params, b, feats, arch, ln, target_params=None):
    p = onet.to_torch(params, torch.float64)
    on = onet.forward(p, b.x_state, feats, arch, ln)
    nx = onet.forward(onet.to_torch(target_params, torch.float64) if target_params is not None else p, b.x_next, feats, arch, ln)
    return torch.cat([on, nx])


def _ref(eng, logits, b, K=None, on0=None, tg0=0):
    K = eng.n_regressed if K is None else K
    on0 = (1 if eng.n_heads >= 2 else 0) if on0 is None else on0
    return hl.hl_loss(logits, b.action, b.reward, b.terminal, float(eng.cfg.gamma_n), K, on0, tg0, eng.n_actions, NB, VMIN, VMAX, SIGMA)


def _close(a, b, rtol=1e-5, atol=1e-7):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


# ------------------------------------------------------------------ 1. the loss kernel on the HIP run's own logits
@pytest.mark.parametrize("shape", [
    pytest.param(((32, 64, 64, 512), 9, 9, 12, "cnn"), id="headline-K9-A9-B12"),
    pytest.param(((7, 9, 11, 13), 3, 5, 6, "cnn"), id="tiny-B6"),
    pytest.param(((16, 16), 2, 3, 11, "fc"), id="fc-B11-ragged"),
])
def test_loss_kernel_matches_float64_on_the_hip_logits(shape):
    feats, K, A, B, arch = shape
    obs = FC_OBS if arch == "fc" else (84, 84, 4)
    eng, _ = _engine(feats, A, 1 + K, B, arch=arch, obs=obs)
    b = _Batch(eng, arch, obs, B, A, seed=5)
    losses = eng.learn_on_batch(b.cb).clone()
    torch.cuda.synchronize()
    ref = _ref(eng, _logits(eng, B), b)
    assert (ref["targets"].abs() > VMAX).any() and b.terminal.any()  # the clamp and terminal rows are exercised
    _close(losses.cpu(), ref["losses"])
    _close(eng.q_values.cpu(), ref["q"])
    _close(eng.targets.cpu(), ref["targets"])
    _close(eng.priorities.cpu(), ref["priorities"])
    nlog = eng.n_heads * A * NB
    dout = eng.region("dout").reshape(-1)[: B * ((nlog + 7) // 8 * 8)].reshape(B, -1).double().cpu()
    _close(dout[:, :nlog], ref["dlogits"])
    assert (dout[:, nlog:] == 0).all()


# ------------------------------------------------------------------ 2. the whole path against float64 logits of the oracle network
E2E = [
    pytest.param(((7, 9, 11, 13), 3, 5, 6, "cnn", True, "bf16x3"), id="cnn-ln"),
    pytest.param(((16, 20, 5, 24), 2, 3, 5, "cnn", False, "bf16x3"), id="cnn-noln"),
    pytest.param(((32, 64, 64, 512), 9, 9, 8, "cnn", True, "bf16x3"), id="cnn-headline-B8"),
    pytest.param(((32, 32), 2, 4, 9, "fc", True, "bf16x3"), id="fc-ln"),
    pytest.param(((8, 16, 16, 24), 2, 5, 4, "impala", True, "bf16x3"), id="impala-ln"),
    pytest.param(((7, 9, 11, 13), 3, 5, 6, "cnn", True, "bf16"), id="cnn-ln-bf16"),
]


@pytest.mark.parametrize("shape", E2E)
def test_loss_on_batch_matches_float64_oracle_logits(shape):
    feats, K, A, B, arch, ln, prec = shape
    obs = FC_OBS if arch == "fc" else (84, 84, 4)
    eng, params = _engine(feats, A, 1 + K, B, arch=arch, obs=obs, ln=ln, precision=prec, seed=2)
    b = _Batch(eng, arch, obs, B, A, seed=9)
    losses = eng.loss_on_batch(b.cb).cpu().numpy()
    ref = _ref(eng, _oracle_logits(params, b, feats, arch, ln), b)
    t = TOL[prec]
    assert np.abs(eng.q_values.cpu().numpy() - ref["q"].numpy()).max() < t["q"] * max(1.0, float(ref["q"].abs().max()))
    assert np.abs(eng.targets.cpu().numpy() - ref["targets"].numpy()).max() < t["q"] * max(1.0, float(ref["targets"].abs().max()))
    assert np.abs(losses - ref["losses"].numpy()).max() < t["loss"] * max(1.0, float(ref["losses"].abs().max()))


# ------------------------------------------------------------------ 3. gradients and Adam
def _s8_values(region: torch.Tensor, rows, pitch):
    """fp32 values of an S8 activation block [rows][pitch] (every 8 floats: 8 bf16 hi halves, then 8 lo halves)."""
    u16 = region.cpu().numpy()[: rows * pitch].view(np.uint16).reshape(rows, pitch // 8, 2, 8)
    f = lambda h: (h.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return (f(u16[:, :, 0]) + f(u16[:, :, 1])).reshape(rows, pitch)


@pytest.mark.parametrize("shape", [
    pytest.param(((7, 9, 11, 13), 3, 5, 6, "cnn"), id="cnn-tiny"),
    pytest.param(((32, 32), 2, 4, 9, "fc"), id="fc"),
])
def test_learn_gradients_and_adam_of_histogram_heads(shape):
    feats, K, A, B, arch = shape
    obs = FC_OBS if arch == "fc" else (84, 84, 4)
    lr = 1e-3
    eng, params = _engine(feats, A, 1 + K, B, arch=arch, obs=obs, seed=4, lr=lr)
    b = _Batch(eng, arch, obs, B, A, seed=13)
    p0 = eng.params.clone()
    g = torch.zeros_like(eng.params)
    eng.learn_on_batch(b.cb, grad_out=g)
    torch.cuda.synchronize()
    hip_g = eng.internal_to_flax_grads(g)
    head = f"Dense_{len(feats) - (3 if arch == 'cnn' else 0)}"
    hid = f"Dense_{len(feats) - (3 if arch == 'cnn' else 0) - 1}"
    # (a) head leaves against float64 dlogits^T . act from the HIP run's own logits and hidden activations
    ref = _ref(eng, _logits(eng, B), b)
    F = feats[-1]
    act = _s8_values(eng.region(f"act/{hid}"), B, (F + 7) // 8 * 8)[:, :F]
    dl = ref["dlogits"].numpy()
    for leaf, want in (("kernel", act.T @ dl), ("bias", dl.sum(0))):
        got = np.asarray(hip_g[head][leaf], np.float64)
        e = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert e <= 1e-4, (leaf, e)
    # (b) every leaf against float64 autograd of the oracle forward
    pt = onet.to_torch(params, torch.float64, requires_grad=True)
    logits = torch.cat([onet.forward(pt, b.x_state, feats, arch, True), onet.forward(pt, b.x_next, feats, arch, True).detach()])
    _ref(eng, logits, b)["losses"].sum().backward()
    for mod in pt:
        for leaf, t in pt[mod].items():
            want = t.grad.numpy()
            got = np.asarray(hip_g[mod][leaf], np.float64)
            e = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
            assert e <= 10 * TOL["bf16x3"]["grad"], (mod, leaf, e)
    # (c) Adam on the head leaves: one optax step from zero moments with the HIP gradient
    for info in eng.infos:
        if info.name.decode().startswith(head + "/"):
            sl = slice(info.offset, info.offset + info.size)
            pn, m, v, _, _ = adam64(p0[sl].cpu().numpy(), 0.0, 0.0, g[sl].cpu().numpy(), 1, lr, 1.5e-4)
            _close(eng.params[sl].cpu(), pn, rtol=1e-6, atol=1e-9)
            _close(eng.adam_m[sl].cpu(), m, rtol=1e-6, atol=1e-12)
            _close(eng.adam_v[sl].cpu(), v, rtol=1e-5, atol=1e-15)
    assert int(eng.adam_count.item()) == 1 and (ADAM_B1, ADAM_B2) == (float(np.float32(0.9)), float(np.float32(0.999)))


# ------------------------------------------------------------------ 4. acting on expectations, shift_params on whole histograms
@pytest.mark.parametrize("arch", ["cnn", "fc"])
def test_forward_best_actions_and_shift(arch):
    feats = (7, 9, 11, 13) if arch == "cnn" else (32, 32)
    obs = FC_OBS if arch == "fc" else (84, 84, 4)
    K, A, B = 3, 5, 8
    eng, params = _engine(feats, A, 1 + K, B, arch=arch, obs=obs, seed=6)
    b = _Batch(eng, arch, obs, B, A, seed=21)
    q = eng.forward(n_rows=B, **b.obs_kw(B)).double().cpu()
    torch.cuda.synchronize()
    ex = hl.expectations(_logits(eng, B)[:B], NB, VMIN, VMAX)
    assert q.shape == (B, (1 + K) * A)
    _close(q, ex, rtol=1e-5, atol=1e-6)
    qo = hl.expectations(_oracle_logits(params, b, feats, arch, True)[:B], NB, VMIN, VMAX)
    assert (q - qo).abs().max() < 1e-3 * max(1.0, float(qo.abs().max()))
    idx = torch.tensor([i % K for i in range(B)], dtype=torch.int32, device="cuda")
    acts = eng.best_actions(idx_networks=idx, **b.obs_kw(B)).cpu().numpy()
    for i in range(B):
        row = ex[i].reshape(1 + K, A)[1 + i % K]
        top = torch.sort(row, descending=True).values
        if float(top[0] - top[1]) < 1e-4:
            continue
        assert acts[i] == int(row.argmax())
        one = dict(obs=b.x_state[i : i + 1].cuda()) if arch == "fc" else dict(frames=b.fr, frame_stride=b.stride,
                                                                            frame_ids=b.ids[i : i + 1, : obs[2]].contiguous())
        assert int(eng.best_action(idx_network=i % K, **one).item()) == int(row.argmax())
    # shift_params: head k <- head k + 1 on whole histograms, the last head unchanged
    before = eng.export_flax()
    flat_before = eng.params.clone()
    eng.shift_params()
    after = eng.export_flax()
    head = f"Dense_{len(feats) - (3 if arch == 'cnn' else 0)}"
    w = A * NB
    for leaf in ("kernel", "bias"):
        x0, x1 = before[head][leaf], after[head][leaf]
        assert np.array_equal(x1[..., :-w], x0[..., w:])
        assert np.array_equal(x1[..., -w:], x0[..., -w:])
        shifted = np.concatenate([x0[..., w:], x0[..., -w:]], axis=-1)
        assert np.array_equal(x1, shifted)
    for mod in before:
        if mod != head:
            for leaf in before[mod]:
                assert np.array_equal(before[mod][leaf], after[mod][leaf])
    assert not torch.equal(flat_before, eng.params)


# ------------------------------------------------------------------ 5. single-head baselines
@pytest.mark.parametrize("arch", ["cnn", "fc"])
def test_dqn_target_forms_and_tfdqn(arch):
    feats = (7, 9, 11, 13) if arch == "cnn" else (32, 32)
    obs = FC_OBS if arch == "fc" else (84, 84, 4)
    A, B = 4, 7
    eng, params = _engine(feats, A, 1, B, arch=arch, obs=obs, seed=8)
    tparams = perturbed_params(31, obs, feats, arch, A * NB, True)
    tgt = torch.zeros_like(eng.params)
    eng.import_flax(tparams, target=tgt)
    b = _Batch(eng, arch, obs, B, A, seed=17)
    # TF-DQN: the single head regressed on itself (same parameters for the next states)
    losses = eng.loss_on_batch(b.cb).cpu().numpy()
    ref = _ref(eng, _oracle_logits(params, b, feats, arch, True), b, K=1, on0=0)
    assert np.abs(losses - ref["losses"].numpy()).max() < 1e-3 * max(1.0, float(ref["losses"].abs().max()))
    assert np.abs(eng.targets.cpu().numpy() - ref["targets"].numpy()).max() < 1e-3 * max(1.0, float(ref["targets"].abs().max()))
    # DQN: next states through the target parameters, loss and learn forms
    ref_t = _ref(eng, _oracle_logits(params, b, feats, arch, True, target_params=tparams), b, K=1, on0=0)
    losses = eng.loss_on_batch_target(b.cb, tgt).cpu().numpy()
    assert np.abs(losses - ref_t["losses"].numpy()).max() < 1e-3 * max(1.0, float(ref_t["losses"].abs().max()))
    assert np.abs(eng.q_values.cpu().numpy() - ref_t["q"].numpy()).max() < 1e-3 * max(1.0, float(ref_t["q"].abs().max()))
    losses = eng.learn_on_batch_target(b.cb, tgt).clone()
    torch.cuda.synchronize()
    own = _ref(eng, _logits(eng, B), b, K=1, on0=0)
    _close(losses.cpu(), own["losses"])
    _close(eng.priorities.cpu(), own["priorities"])
    assert np.abs(losses.cpu().numpy() - ref_t["losses"].numpy()).max() < 1e-3 * max(1.0, float(ref_t["losses"].abs().max()))


def test_agents_carry_the_histogram_settings():
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    kw = dict(n_bins=NB, min_value=VMIN, max_value=VMAX, sigma=SIGMA)
    a = iSDQN(0, (84, 84, 4), 4, 2, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    assert a.network.final_feature == 3 * 4 * NB
    assert a.get_model()["params"]["params"]["Dense_1"]["kernel"].shape == (16, 3 * 4 * NB)
    d = DQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    assert d.network.final_feature == 4 * NB and d._engine.n_bins == NB
    t = TFDQN(0, (84, 84, 4), 4, [8, 8, 8, 16], True, False, "cnn", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw)
    assert t.network.final_feature == 4 * NB and t._engine.cfg.hl_sigma == np.float32(SIGMA)


# ------------------------------------------------------------------ 6. determinism and the captured replay
def test_two_learn_steps_are_bit_identical_from_identical_state():
    feats, K, A, B = (32, 64, 64, 512), 9, 9, 32
    runs = []
    for _ in range(2):
        eng, _ = _engine(feats, A, 1 + K, B, seed=1)
        b = _Batch(eng, "cnn", (84, 84, 4), B, A, seed=3)
        ls = [eng.learn_on_batch(b.cb).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.stack(ls), eng.priorities.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


class _Replica:
    """bench.Replica's training state (synthetic prefilled replay, headline widths) with histogram heads."""

    def __init__(self, seed=3, capacity=4096, B=32, K=3, A=9, prioritized=False):
        from slimdqn._engine import QNetEngine
        from slimdqn.sample_collection.replay_buffer import ReplayBuffer
        from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

        self.prioritized = prioritized
        sampler = PrioritizedSamplingDistribution(seed, capacity, device="cuda:0") if prioritized else UniformSamplingDistribution(seed, device="cuda:0")
        self.rb = ReplayBuffer(sampler, B, capacity, stack_size=4, update_horizon=1, gamma=0.99, device="cuda:0")
        pri = np.random.default_rng(seed).uniform(0.1, 2.0, capacity) if prioritized else None
        self.rb.prefill_synthetic(capacity, (84, 84), A, seed=seed, p_terminal=0.005, priorities=pri)
        self.eng = QNetEngine((84, 84, 4), A, 1 + K, (32, 64, 64, 512), "cnn", True, B, gamma_n=0.99, learning_rate=6.25e-5, adam_eps=1.5e-4,
                              device="cuda:0", n_bins=NB, min_value=VMIN, max_value=VMAX, sigma=SIGMA)
        self.eng.init_params(seed)
        torch.cuda.synchronize()

    def step(self):
        batch = self.rb.sample()
        cb = self.eng.make_batch(frames=batch.frames, frame_stride=batch.frame_stride, frame_ids=batch.frame_ids, action=batch.action,
                                 reward=batch.reward, terminal=batch.is_terminal)
        self.eng.learn_on_batch(cb)
        if self.prioritized:
            self.rb.update_device(batch, self.eng.priorities)


@pytest.mark.parametrize("prioritized", [False, True])
def test_graph_replay_equals_eager_steps(prioritized):
    from slimdqn._graph import GraphedUpdate

    S, n_replays = 4, 2
    eager, graphed = _Replica(prioritized=prioritized), _Replica(prioritized=prioritized)
    assert torch.equal(eager.eng.params, graphed.eng.params)
    g = GraphedUpdate(graphed.rb, graphed.eng, prioritized, S)
    for _ in range(S * n_replays):
        eager.step()
    for _ in range(n_replays):
        g.run()
    torch.cuda.synchronize()
    for name in ("params", "adam_m", "adam_v", "adam_count", "losses_accum"):
        a, b = getattr(eager.eng, name), getattr(graphed.eng, name)
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} elements differ between eager and graph replay"
    assert torch.isfinite(eager.eng.losses_accum).all() and (eager.eng.losses_accum > 0).all()


# ------------------------------------------------------------------ 7. the Atari entry point with -hl
def test_entry_point_with_the_histogram_loss(tmp_path):
    from experiments.atari.isdqn import run

    argv = ["-en", "hl_Synthetic", "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "200", "-bs", "8", "-n", "1", "-horizon", "50",
            "-at", "cnn", "-ne", "2", "-ntspe", "60", "-utd", "4", "-nis", "20", "-ed", "100", "-nbi", "2", "-ln", "-tuf", "16",
            "-env", "synthetic", "-hl", "-nb", "51", "-minn", "-10", "-maxn", "10", "-sigma", "0.3"]
    gathered = run(argv, root=str(tmp_path))
    assert len(gathered) == 2
    out = tmp_path / "atari" / "exp_output" / "hl_Synthetic"
    # (the engine group's flags, -hl and the four histogram flags among them, stay out of parameters.json like -hd and -prec: it holds
    # the reference's groups, which the comparisons between runs read)
    params = json.load(open(out / "parameters.json"))
    assert params["isdqn"]["n_bellman_iterations"] == 2 and "n_bins" not in params["shared_parameters"]
    res = json.load(open(out / "isdqn" / "episode_returns_and_lengths" / "1.json"))
    assert len(res["episode_returns"]) == 2
    import pickle

    model = pickle.load(open(out / "isdqn" / "models" / "1", "rb"))["params"]
    assert model["params"]["Dense_1"]["kernel"].shape == (16, 3 * 9 * 51)
    assert all(np.isfinite(v).all() for leaves in model["params"].values() for v in leaves.values())
