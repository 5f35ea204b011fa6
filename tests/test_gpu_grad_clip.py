"""Clipping of the gradient by its global norm in front of Adam (include/isdqn_hip.h, isdqn_net_config::max_grad_norm;
csrc/grad_clip.h), on the device, against the float64 reference of tests/helpers/grad_clip.py.

Cases -- the smallest networks that reach each route of the learn step's optimizer tail:
  fc            obs 8 -> 100 -> 100, K = 1, A = 4, B = 32, eps 1e-8: Dense_1 is fused into Adam with the option off (the bypass is taken),
                every tensor is a single tile
  headline-B32  cnn (32, 64, 64, 512), K = 9, A = 9: Dense_0 is fused with the option off, conv slabs (one per image for Conv_0), the head
  headline-B64  chain's head slabs, tens of thousands of partial sums in the finalize kernel; B = 64: two K steps in the one Dense_0 slab
  duel          fc (100, 100), K = 3, A = 4, B = 32, dueling = 1: the live mask in the norm, the head outside the head chain
  hist          fc (100, 100), K = 3, A = 4, B = 32, n_bins = 11: the generic head route at the logit width, large gradients
  dqn           fc (100, 100), one head, through learn_on_batch_target / grad_on_batch with target parameters

Tolerances.  The device accumulates exact float64 squares of the fp32 gradient (24 x 24 bits fit 53) and rounds the float64 norm and
scale to fp32 once: 2^-24 relative; the tests allow 2^-23.  The float64 sums themselves (10^4 .. 10^6 terms, any order) differ by
< 1e-12 relative: nothing against 2^-23.  The update is held to tests.gpu_helpers.adam_bounds on the gradient Adam consumed,
fl32(grad_out * fl32(scale)): the bounds tests/test_gpu_optimizer.py derives, unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from tests.gpu_helpers import adam_bounds, make_frame_batch, masked_reference_grads, hip_preactivations, perturbed_params
from tests.helpers import dueling as du
from tests.helpers import grad_clip as gc
from tests.test_gpu_optimizer import _bits, _plant, _real

pytestmark = pytest.mark.gpu

REL = 2.0**-23
LR = 1e-3
INF = float("inf")
HEADLINE, FC = (32, 64, 64, 512), (100, 100)
CASES = ["fc", "headline-B32", "headline-B64", "duel", "hist", "dqn"]


class Case:
    """One engine (clipping on at threshold ``c``, or off with c = 0) and one batch; ``weights``: loss_weights of the batch."""

    def __init__(self, name, c=INF, weights=None, lr=LR):
        from slimdqn._engine import QNetEngine

        self.name = name
        d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        gkw = dict(gamma_n=0.99, learning_rate=lr, max_grad_norm=c)
        self.target = None
        self.params_tree = self.ref = None
        if name.startswith("headline"):
            self.B, self.K, self.A, self.eps = int(name.split("B")[1]), 9, 9, 1.5e-4
            self.params_tree = perturbed_params(3, (84, 84, 4), HEADLINE, "cnn", (1 + self.K) * self.A, True)
            eng = QNetEngine((84, 84, 4), self.A, 1 + self.K, HEADLINE, "cnn", True, self.B, adam_eps=self.eps, **gkw)
            eng.import_flax(self.params_tree)
            frames, ids, action, reward, terminal, self.ref = make_frame_batch(self.B, self.A, seed=23, n_frames=self.B + 64)
            self.batch = eng.make_batch(frames=d(frames), frame_stride=frames.shape[1], frame_ids=d(ids), action=d(action), reward=d(reward),
                                        terminal=d(terminal), loss_weights=d(weights))
        else:
            self.B, self.A = 32, 4
            self.K, self.eps, kw, dueling = {"fc": (1, 1e-8, {}, False), "duel": (3, 1.5e-4, {}, True),
                                             "hist": (3, 1.5e-4, dict(n_bins=11, min_value=-10.0, max_value=10.0, sigma=0.75 * 20 / 11), False),
                                             "dqn": (0, 1.5e-4, {}, False)}[name]
            H, w = 1 + self.K, kw.get("n_bins", 1)
            out = du.raw_width(H, self.A, w) if dueling else H * self.A * w
            p = perturbed_params(3, (8,), FC, "fc", out, True)
            if dueling:
                p = du.mask_head(p, "Dense_2", FC[-1], H, self.A, w)
            eng = QNetEngine((8,), self.A, H, FC, "fc", True, self.B, adam_eps=self.eps, dueling=dueling, **kw, **gkw)
            eng.import_flax(p)
            if name == "dqn":
                self.target = torch.zeros_like(eng.params)
                eng.import_flax(perturbed_params(5, (8,), FC, "fc", out, True), target=self.target)
            rng = np.random.default_rng(3)
            f32 = lambda a: a.astype(np.float32)
            self.batch = eng.make_batch(state=d(f32(rng.normal(size=(self.B, 8)))), next_state=d(f32(rng.normal(size=(self.B, 8)))),
                                        action=d(rng.integers(0, self.A, self.B).astype(np.int32)), reward=d(f32(rng.normal(size=self.B))),
                                        terminal=d((rng.random(self.B) < 0.2).astype(np.uint8)), loss_weights=d(weights))
        self.eng = eng
        self.real = _real(eng)
        self.live = self.real.copy()  # real elements that are part of the norm
        if eng.dueling:
            info = eng.head_kernel_info()
            self.structural = int(info.offset) + du.structural_indices(FC[-1], int(info.dims[1]), eng.n_heads, self.A, 1)
            self.live[self.structural] = False

    def grad(self):
        """gradient-only pass: the call's own grad_out"""
        g = torch.zeros_like(self.eng.params)
        self.eng.grad_on_batch(self.batch, g, target_params=self.target)
        torch.cuda.synchronize()
        return g.cpu().numpy()

    def step(self):
        """one update step; returns the reduced gradient it consumed (the DQN form's debug entry does not exist: its gradient comes
        from the gradient-only pass on the same state, whose norm the step must then reproduce bit for bit)"""
        eng = self.eng
        if self.target is not None:
            g = self.grad()
            n_pre = _bits(eng.grad_clip[:1])
            eng.learn_on_batch_target(self.batch, self.target)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(eng.grad_clip[:1]), n_pre), "the update step's norm differs from the gradient-only pass's"
            return g
        g = torch.zeros_like(eng.params)
        eng.learn_on_batch(self.batch, grad_out=g)
        torch.cuda.synchronize()
        return g.cpu().numpy()

    def clip(self):
        return self.eng.grad_clip.cpu().numpy().copy()

    def state(self):
        e = self.eng
        return [_bits(t) for t in (e.params, e.adam_m, e.adam_v, e.adam_count, e.region("wsplit"))]


def _norm64(g, mask=None):
    g = np.asarray(g, np.float64)
    return gc.global_norm([g if mask is None else g[mask]])


def _first_norm(case):
    """fp32 norm of a gradient-only pass on the current state (the threshold does not enter the norm)"""
    case.grad()
    n0 = np.float32(case.clip()[0])
    assert np.isfinite(n0) and n0 > 0
    return n0


# ------------------------------------------------------------------ 1. norm and scale
@pytest.mark.parametrize("name", CASES)
def test_norm_and_scale_equal_the_float64_norm_of_the_calls_own_gradient(name):
    case = Case(name)
    n0 = _first_norm(case)
    rows = []
    for label, c in (("0.5n", np.float32(0.5) * n0), ("2n", np.float32(2.0) * n0), ("inf", np.float32(INF))):
        case.eng.set_max_grad_norm(float(c))
        g = case.grad()
        assert np.isfinite(g).all()
        n_dev, s_dev = (float(x) for x in case.clip()[:2])
        n64 = _norm64(g)
        assert np.all(g[~case.real] == 0), "a padding element carries a gradient"
        for mask in (case.real, case.live):  # (grad_out is masked under dueling; float64 sums of the same terms in another grouping)
            assert abs(_norm64(g, mask) - n64) <= 1e-12 * n64
        s64 = gc.clip_scale(n64, float(c))
        rows.append((label, n_dev, n64, abs(n_dev - n64) / n64, s_dev, s64))
        assert abs(n_dev - n64) <= REL * n64, (label, n_dev, n64)
        assert abs(s_dev - s64) <= REL * s64, (label, s_dev, s64)
        if label != "0.5n":
            assert np.float32(s_dev).view(np.int32) == np.float32(1.0).view(np.int32), (label, s_dev)
        else:
            assert 0.49 < s_dev < 0.51
            # the wrong readings, on this very gradient: what Adam would consume leaves the tolerance under every one of them
            leaves = [g[i.offset : i.offset + i.size] for i in case.eng.infos]
            want = gc.clipped(leaves, float(c))
            for wname in ("per_leaf_norms", "l1_norm", "clip_by_value"):
                got = gc.WRONG[wname](leaves, float(c))
                worst = max(float(np.abs(a - b).max()) / float(np.abs(b).max()) for a, b in zip(got, want) if np.abs(b).max() > 0)
                assert worst > 1000 * REL, (wname, worst)
        if label == "2n":
            got = gc.always_scaled([g], float(c))[0]
            assert float(np.abs(got - g).max()) > 1000 * REL * float(np.abs(g).max())
    print(f"\n{name}: " + "; ".join(f"c={l}: n {nd!r} (float64 {n64!r}, rel {r:.1e}) scale {sd!r} (float64 {s64!r})" for l, nd, n64, r, sd, s64 in rows))


def _s8_rows(region, rows, width):
    """fp32 values of S8 rows (gemm_core.h: every 8 values are 8 bf16 hi halves, then 8 bf16 lo halves)"""
    halves = region[: rows * width].view(torch.bfloat16).reshape(-1, 2, 8).double()
    return (halves[:, 0] + halves[:, 1]).reshape(rows, width).cpu().numpy()


def test_dueling_structural_entries_are_outside_the_norm():
    """The raw weight gradient of the head kernel is not zero on the structural entries: it is dout_raw^T . act of the last hidden
    layer, rebuilt here in float64 from the run's own regions (grad_out never shows it: duel_mask_kernel zeroes it there too).  The
    norm that included those entries lies outside the tolerance of the norm the device reports."""
    on = Case("duel")
    g = on.grad()
    n_dev = float(on.clip()[0])
    info = on.eng.head_kernel_info()
    rows, in_p = int(info.dims[0]), int(info.dims[1])
    d = on.eng.region("dout_raw")[: on.B * rows].reshape(on.B, rows).double().cpu().numpy()
    x = _s8_rows(on.eng.region("act/Dense_1"), on.B, in_p)
    raw = (d.T @ x).reshape(-1)
    idx = on.structural - int(info.offset)
    live = np.ones(info.size, bool)
    live[idx] = False
    head = g[info.offset : info.offset + info.size].astype(np.float64)
    assert np.abs(raw[live] - head[live]).max() <= 1e-4 * np.abs(head).max()  # the rebuilt gradient is the device's where both exist
    s = raw[idx]
    # (head 0 is regressed on, never regressed: its rows carry no gradient -- a quarter of the entries)
    assert np.count_nonzero(s) > 0.5 * s.size and np.all(g[on.structural] == 0)
    n_masked = _norm64(g)
    n_with = float(np.sqrt(n_masked**2 + float((s * s).sum())))
    print(f"\nduel: norm {n_dev!r}, float64 masked {n_masked!r}, with the structural entries {n_with!r} ({(n_with - n_masked) / n_masked:.2e} above)")
    assert abs(n_dev - n_masked) <= REL * n_masked
    assert abs(n_dev - n_with) > 1000 * REL * n_with


# ------------------------------------------------------------------ 2. the update
@pytest.mark.parametrize("name", CASES)
def test_adam_consumes_the_scaled_gradient_and_the_mirror_follows(name):
    """tests/test_gpu_optimizer.py::test_adam_element_update_and_mirror_match_float64 with the option on at c = 0.5 n: planted moments
    (six classes) and step counts, p / m / v against float64 Adam on fl32(grad_out * fl32(scale read back)) within adam_bounds, the
    mirror against a fresh split bit for bit, adam_count + 1."""
    case = Case(name)
    eng = case.eng
    g_pre = case.grad()
    rng = np.random.default_rng(11)
    worst = {}
    for t0 in (0, 9):
        # (the planted moments move the parameters far -- class 0 steps by lr m / eps -- so each step halves the norm of ITS state)
        eng.set_max_grad_norm(float(np.float32(0.5) * _first_norm(case)))
        m0, v0 = _plant(g_pre, case.live, t0 + 1, case.eps, rng)
        eng.adam_m.copy_(torch.from_numpy(m0))
        eng.adam_v.copy_(torch.from_numpy(v0))
        eng.adam_count.fill_(t0)
        p0 = eng.params.cpu().numpy().copy()
        g = case.step()
        n_dev, s_dev = case.clip()[:2]
        assert np.isfinite(g).all() and int(eng.adam_count.item()) == t0 + 1
        assert abs(float(n_dev) - _norm64(g)) <= REL * _norm64(g) and np.float32(s_dev) < 1
        consumed = (g.astype(np.float32) * np.float32(s_dev)).astype(np.float32)  # one fp32 multiply
        (p, m, v, u), (ep, em, ev) = adam_bounds(p0, m0, v0, consumed, t0 + 1, LR, case.eps)
        got_p, got_m, got_v = (x.cpu().numpy().astype(np.float64) for x in (eng.params, eng.adam_m, eng.adam_v))
        for nm, got, want, bound in (("m", got_m, m, em), ("v", got_v, v, ev), ("p", got_p, p, ep)):
            assert np.isfinite(got).all()
            r = np.abs(got - want) / bound
            i = int(np.argmax(r))
            worst[(t0, nm)] = float(r[i])
            assert r[i] <= 1.0, (f"t0={t0} {nm}[{i}] (class {i % 6}, live {case.live[i]}): got {got[i]!r} want {want[i]!r} "
                                 f"err {abs(got[i] - want[i]):.3e} bound {bound[i]:.3e} g {g[i]!r} scale {s_dev!r}")
        # the unscaled gradient would not pass: the check sees the scale
        (_, m_raw, _, _), _ = adam_bounds(p0, m0, v0, g, t0 + 1, LR, case.eps)
        assert np.any(np.abs(got_m - m_raw) > em)
        assert np.count_nonzero(got_p[case.live] != p0[case.live]) > 0.5 * case.live.sum()
        mirror = _bits(eng.region("wsplit"))
        eng.rebuild_mirror()
        bad = np.flatnonzero(mirror != _bits(eng.region("wsplit")))
        assert bad.size == 0, f"t0={t0}: {bad.size} mirror words differ from a fresh split, first at float {bad[0]}"
    print(f"\n{name} worst |err| / bound:", {f"{k[0]}/{k[1]}": round(v, 3) for k, v in worst.items()})


# ------------------------------------------------------------------ 3. the gradient of the bypassed route
@pytest.mark.parametrize("name", ["fc", "headline-B32", "headline-B64"])
def test_grad_out_of_the_unfused_route_against_the_off_configuration(name):
    """grad_out with the option on against an engine without it, same parameters, same batch, one learn step each.  Every leaf both
    reduce in adam_kernel: bit for bit.  The Dense kernel the off configuration fuses into Adam (fc: Dense_1, headline: Dense_0) now
    goes through dense_wgrad's 128 x 128 tiles into one slab: the same bf16x3 products of the same S8 operands, accumulated in fp32 in
    another order.  Each order is within (depth of the chains) x 2^-24 of the magnitude sum S = sum_b |dz| |x| -- 3 passes x B <= 64 rows,
    under 2^-16 S (the model of tests/test_gpu_optimizer.py, test 3) -- so the two differ by at most 2^-15 S per element."""
    on, off = Case(name, c=INF), Case(name, c=0.0)
    assert torch.equal(on.eng.params, off.eng.params)
    g_on, g_off = on.step(), off.step()
    fused = "Dense_1/kernel" if name == "fc" else "Dense_0/kernel"
    seen = False
    for info in on.eng.infos:
        a, b = g_on[info.offset : info.offset + info.size], g_off[info.offset : info.offset + info.size]
        if info.name.decode() != fused:
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{info.name.decode()}: {np.count_nonzero(a != b)} elements differ"
            continue
        seen = True
        if name == "fc":
            dz = np.abs(_s8_rows(on.eng.region("dz/Dense_1"), on.B, 104))
            x = np.abs(_s8_rows(on.eng.region("act/Dense_0"), on.B, 104))
            S = (dz.T @ x).reshape(-1)  # internal layout [out][in]
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        else:
            z_hip = hip_preactivations(on.eng, on.B)
            _, scale = masked_reference_grads(on.params_tree, HEADLINE, on.K, on.A, on.ref, z_hip, layer_norm=True, gamma_n=0.99, with_scales=True)
            S = np.asarray(scale["Dense_0"]["kernel"], np.float64)
            fa, fb = (on.eng.internal_to_flax_grads(torch.from_numpy(x))["Dense_0"]["kernel"].astype(np.float64) for x in (g_on, g_off))
            d = np.abs(fa - fb)
        r = d / (2.0**-15 * S + 1e-300)
        print(f"\n{name} {fused}: bit-identical to the fused route: {bool(np.array_equal(a.view(np.int32), b.view(np.int32)))}; "
              f"{np.count_nonzero(a != b)} of {a.size} elements differ, max |d| / (2^-15 S) = {float(r.max()):.3e}")
        assert np.all(d <= 2.0**-15 * S), float(r.max())
    assert seen


# ------------------------------------------------------------------ 4. zero gradient
@pytest.mark.parametrize("name", ["fc", "headline-B32", "duel"])
def test_a_zero_gradient_has_norm_zero_scale_one_and_moves_by_the_moments_alone(name):
    probe = Case(name)
    g_pre = probe.grad()
    case = Case(name, c=1.0, weights=np.zeros(probe.B, np.float32))
    eng = case.eng
    m0, v0 = _plant(g_pre, case.live, 4, case.eps, np.random.default_rng(2))
    eng.adam_m.copy_(torch.from_numpy(m0))
    eng.adam_v.copy_(torch.from_numpy(v0))
    eng.adam_count.fill_(3)
    p0 = eng.params.cpu().numpy().copy()
    g = case.step()
    clip = case.clip()
    assert np.all(g == 0) and clip[0] == 0.0 and clip[1] == 1.0 and np.isfinite(clip).all()
    (p, m, v, u), (ep, em, ev) = adam_bounds(p0, m0, v0, np.zeros_like(g), 4, LR, case.eps)
    for nm, t, want, bound in (("m", eng.adam_m, m, em), ("v", eng.adam_v, v, ev), ("p", eng.params, p, ep)):
        got = t.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and np.all(np.abs(got - want) <= bound), nm
    assert torch.isfinite(eng.losses).all()


# ------------------------------------------------------------------ 5. accumulators
@pytest.mark.parametrize("name", ["fc", "dqn", "headline-B32"])
def test_accumulators_count_update_steps_only(name):
    case = Case(name, lr=1e-6)  # (steps of 1e-6 per element: the norm stays within a few percent of the first pass's, above 0.5 n)
    eng = case.eng
    n0 = _first_norm(case)
    assert np.all(case.clip()[2:] == 0)  # a fresh workspace, and the gradient-only pass above left them alone
    eng.set_max_grad_norm(float(np.float32(0.5) * n0))
    acc, norms = np.float32(0.0), []
    for _ in range(3):
        case.step()
        clip = case.clip()
        assert clip[1] < 1.0
        norms.append(np.float32(clip[0]))
        acc = np.float32(acc + np.float32(clip[0]))
    clip = case.clip()
    assert np.float32(clip[2]).view(np.int32) == acc.view(np.int32) and clip[3] == 3.0, (clip, norms)
    before = case.state()
    g = case.grad()  # gradient only: [0], [1] of this pass, nothing else
    after, clip2 = case.state(), case.clip()
    for nm, a, b in zip(("params", "adam_m", "adam_v", "adam_count", "mirror"), before, after):
        assert np.array_equal(a, b), nm
    assert np.array_equal(clip2[2:], clip[2:]) and abs(float(clip2[0]) - _norm64(g)) <= REL * _norm64(g)
    eng.grad_clip[2:4].zero_()
    eng.set_max_grad_norm(INF)
    for _ in range(3):
        case.step()
    clip = case.clip()
    assert clip[3] == 0.0 and clip[1] == 1.0 and clip[2] > 0


# ------------------------------------------------------------------ 6. determinism, the captured step, the agent
@pytest.mark.parametrize("name", ["headline-B32", "duel"])
def test_two_runs_from_the_same_state_give_identical_bits(name):
    runs = []
    for _ in range(2):
        case = Case(name)
        n0 = _first_norm(case)
        case.eng.set_max_grad_norm(float(np.float32(0.5) * n0))
        gs = [case.step() for _ in range(2)]
        runs.append(case.state() + [_bits(case.eng.grad_clip)] + [g.view(np.int32) for g in gs])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


class _Replica:
    """bench.Replica's training state (synthetic prefilled replay, headline widths) with clipping at ``c``."""

    def __init__(self, c, seed=3, capacity=2048, B=32, K=3, A=9):
        from slimdqn._engine import QNetEngine
        from slimdqn.sample_collection.replay_buffer import ReplayBuffer
        from slimdqn.sample_collection.samplers import UniformSamplingDistribution

        self.rb = ReplayBuffer(UniformSamplingDistribution(seed, device="cuda:0"), B, capacity, stack_size=4, update_horizon=1, gamma=0.99, device="cuda:0")
        self.rb.prefill_synthetic(capacity, (84, 84), A, seed=seed, p_terminal=0.005)
        self.eng = QNetEngine((84, 84, 4), A, 1 + K, HEADLINE, "cnn", True, B, gamma_n=0.99, learning_rate=6.25e-5, adam_eps=1.5e-4, device="cuda:0",
                              max_grad_norm=c)
        self.eng.init_params(seed)
        torch.cuda.synchronize()

    def step(self):
        batch = self.rb.sample()
        self.eng.learn_on_batch(self.eng.make_batch(frames=batch.frames, frame_stride=batch.frame_stride, frame_ids=batch.frame_ids, action=batch.action,
                                                    reward=batch.reward, terminal=batch.is_terminal))


def test_graph_replay_equals_eager_steps_with_clipping_on():
    from slimdqn._graph import GraphedUpdate

    S = 3
    probe = _Replica(INF)
    probe.step()
    torch.cuda.synchronize()
    c = 0.5 * float(probe.eng.grad_clip[0].item())  # half the first step's norm: the captured steps clip
    del probe
    eager, graphed = _Replica(c), _Replica(c)
    assert torch.equal(eager.eng.params, graphed.eng.params)
    g = GraphedUpdate(graphed.rb, graphed.eng, False, S)
    for _ in range(S):
        eager.step()
    g.run()
    torch.cuda.synchronize()
    for name in ("params", "adam_m", "adam_v", "adam_count", "losses_accum", "grad_clip"):
        a, b = getattr(eager.eng, name), getattr(graphed.eng, name)
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} elements differ between eager and graph replay"
    clip = eager.eng.grad_clip.cpu().numpy()
    assert clip[3] >= 1 and clip[2] > 0 and np.isfinite(clip).all()
    g.destroy()


@pytest.mark.parametrize("c", [1e-3, INF])
def test_isdqn_agent_logs_grad_norm_and_clipped_fraction(c):
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    K, A, B, tuf = 2, 5, 8, 4
    agent = iSDQN(0, (84, 84, 4), A, K, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 1, 1, tuf, adam_eps=1.5e-4, batch_size=B, max_grad_norm=c)
    rb = ReplayBuffer(UniformSamplingDistribution(5, device="cuda:0"), B, 256, stack_size=4, update_horizon=1, gamma=0.99, device="cuda:0")
    rb.prefill_synthetic(256, (84, 84), A, seed=1, p_terminal=0.01)
    seen = []
    for step in range(1, 2 * tuf + 1):
        agent.update_online_params(step, rb)
        updated, logs = agent.update_target_params(step)
        if updated:
            seen.append(logs)
    assert len(seen) == 2
    for logs in seen:
        assert np.isfinite(logs["grad_norm"]) and logs["grad_norm"] > 0
        assert logs["grad_clipped_fraction"] == (1.0 if c < INF else 0.0)  # (a norm below 1e-3 would be a dead network)
    assert np.all(agent._engine.grad_clip[2:4].cpu().numpy() == 0)  # read and zeroed
    plain = iSDQN(0, (84, 84, 4), A, K, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 1, 1, tuf, adam_eps=1.5e-4, batch_size=B)
    plain.update_online_params(tuf, rb)
    assert not any("grad" in k for k in plain.update_target_params(tuf)[1])  # nothing is added when the option is off


ARGV = ["-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "200", "-bs", "8", "-n", "1", "-horizon", "50", "-at", "cnn", "-ne", "1",
        "-ntspe", "48", "-utd", "4", "-nis", "20", "-ed", "100", "-ln", "-tuf", "16", "-env", "synthetic"]


@pytest.mark.parametrize("algo,extra", [("isdqn", ["-nbi", "2", "-duel", "-qr", "-nq", "8", "-hd", "1", "-gc", "10"]), ("dqn", ["-gc", "inf"]),
                                        ("tfdqn", ["-gc", "1e-3"]), ("analysisdqn", ["-nbi", "2", "-gc", "10"]), ("analysistfdqn", ["-gc", "10"])])
def test_entry_point_with_gc_logs_grad_norm(tmp_path, monkeypatch, algo, extra):
    import importlib
    import json

    from experiments.base import utils

    logged = []
    plain = utils._NullLogger.log
    monkeypatch.setattr(utils._NullLogger, "log", lambda self, d: (logged.append(dict(d)), plain(self, d))[1])
    importlib.import_module(f"experiments.atari.{algo}").run(["-en", "gc_Synthetic"] + ARGV + extra, root=str(tmp_path))
    stored = json.load(open(tmp_path / "atari" / "exp_output" / "gc_Synthetic" / "parameters.json"))
    assert not any("grad" in k for k in list(stored[algo]) + list(stored["shared_parameters"]))
    rows = [d for d in logged if "grad_norm" in d]
    assert rows and all(np.isfinite(d["grad_norm"]) and d["grad_norm"] > 0 and 0.0 <= d["grad_clipped_fraction"] <= 1.0 for d in rows), logged
    if extra[-1] == "inf":
        assert all(d["grad_clipped_fraction"] == 0.0 for d in rows)
    if extra[-1] == "1e-3":
        assert all(d["grad_clipped_fraction"] == 1.0 for d in rows)


# ------------------------------------------------------------------ 7. off is off
def test_off_has_no_region_and_the_refusals_return_their_codes():
    from slimdqn import _engine, _hip
    from slimdqn._engine import QNetEngine

    mk = lambda **kw: QNetEngine((8,), 4, 2, FC, kw.pop("arch", "fc"), True, 32, **kw)
    never, off, on = mk(), mk(max_grad_norm=0.0), mk(max_grad_norm=10.0)
    assert never.workspace_bytes == off.workspace_bytes < on.workspace_bytes
    with pytest.raises(Exception):
        off.region("grad_clip")
    with pytest.raises(Exception):
        off.grad_clip
    assert on.grad_clip.numel() == 4 and on.region("grad_clip_partials").numel() > 0
    lib, b = on.lib, ctypes.c_int64()
    for field, value, code in (("max_grad_norm", -1.0, _hip.ERR_ARG), ("max_grad_norm", float("nan"), _hip.ERR_ARG),
                               ("batch_norm", 1, _hip.ERR_UNSUPPORTED), ("arch", _hip.ARCH_IMPALA, _hip.ERR_UNSUPPORTED)):
        cfg = _hip.NetConfig.from_buffer_copy(on.cfg)
        if field == "arch":
            cfg.obs_h, cfg.obs_w, cfg.obs_c, cfg.n_features = 84, 84, 4, 4
            for i, f in enumerate((8, 8, 8, 16)):
                cfg.features[i] = f
        setattr(cfg, field, value)
        assert lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b)) == code, field
    for kw, msg in ((dict(max_grad_norm=-1.0), _engine.GRAD_CLIP_NEGATIVE_REFUSED), (dict(max_grad_norm=1.0, batch_norm=True), _engine.GRAD_CLIP_BATCH_NORM_REFUSED)):
        with pytest.raises(ValueError) as e:
            mk(**kw)
        assert str(e.value) == msg
    # the off engine's step is the step of an engine built without the keyword, bit for bit
    a, c = Case("fc", c=0.0), Case("fc", c=0.0)
    c.eng.cfg.max_grad_norm = -0.0
    ga, gc_ = a.step(), c.step()
    assert np.array_equal(ga.view(np.int32), gc_.view(np.int32)) and all(np.array_equal(x, y) for x, y in zip(a.state(), c.state()))
