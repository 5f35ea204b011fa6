"""Noisy Dense layers on the device (include/isdqn_hip.h, isdqn_noisy_layout; csrc/noisy.h) against the numpy / float64 reference of
tests/helpers/noisy.py.

Cases -- the smallest networks that reach each route of the step:
  fc            obs 8 -> (100, 100), K = 3, A = 4, B = 32: every Dense is noisy, padding lanes in every width (100 -> 104, 8 -> 8, 16 rows)
  duel          the same with dueling = 1: structural zeros of the head kernel, the masked gradient
  hist          the same with n_bins = 11: the head at the logit width
  dqn           one head, the target form: a second composed buffer from a stream_id = 1 draw
  headline-B32  cnn (32, 64, 64, 512), K = 9, A = 9: conv tensors that must pass through untouched, the internal column order of the
                7744-wide ein behind the torso (11 x 11 pixels of 64 channels), 90 head rows padded to 96

Tolerances.  Sample: |sign(f) f^2 - z64| <= 16 * 2^-24 * max(1, r64) per element, derived in the header's terms -- about 4 ulp each for the
logarithm and cospif, a correctly rounded square root, two multiplies and two more roundings through f and back; the margin over that budget
is a factor of two.  Compose and the gradient: bit for bit.  The update: tests.gpu_helpers.adam_bounds, unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from tests.gpu_helpers import adam_bounds, make_frame_batch, perturbed_params
from tests.helpers import dueling as du
from tests.helpers import noisy as nz

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().clone().view(torch.int32).cpu().numpy()


def _real(eng):
    """True where an internal parameter element is a real Flax element (not channel / row padding)."""
    mask = np.zeros(eng.n_param_floats, bool)
    for info in eng.infos:
        shape = tuple(info.flax_shape[: info.ndim])
        mask[info.offset : info.offset + info.size] = eng._to_internal(info, np.ones(shape, np.float32)) != 0
    return mask


def _priorities_ref(q_values, targets):
    """The loss kernels' own arithmetic on the q_values / targets they stored (td_kernel, hl_loss_kernel: the squared-error case):
    d = q - t and d * d in fp32, the fp32 sum over k in ascending order, divided by (float)K, then sqrt((double)x + 1e-10)."""
    q, t = np.asarray(q_values, np.float32), np.asarray(targets, np.float32)
    d = q - t
    td = d * d
    s = np.zeros(q.shape[0], np.float32)
    for k in range(q.shape[1]):
        s = s + td[:, k]
    return np.sqrt((s / np.float32(q.shape[1])).astype(np.float64) + 1e-10)


LR = 1e-3
HEADLINE, FC = (32, 64, 64, 512), (100, 100)
CASES = ["fc", "duel", "hist", "dqn", "headline-B32"]
SEED = (0x1234 << 32) | 0x9E3779B9


class Case:
    """One engine (noisy or plain, same mu) and one batch."""

    def __init__(self, name, noisy=True, sigma0=0.5):
        from slimdqn._engine import QNetEngine

        self.name = name
        d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        nkw = dict(noisy=True, noisy_sigma0=sigma0, noisy_seed=SEED) if noisy else {}
        gkw = dict(gamma_n=0.99, learning_rate=LR, **nkw)
        self.target = None
        if name.startswith("headline"):
            self.B, self.K, self.A, self.eps = 32, 9, 9, 1.5e-4
            tree = perturbed_params(3, (84, 84, 4), HEADLINE, "cnn", (1 + self.K) * self.A, True)
            eng = QNetEngine((84, 84, 4), self.A, 1 + self.K, HEADLINE, "cnn", True, self.B, adam_eps=self.eps, **gkw)
            eng.import_flax(tree)
            frames, ids, action, reward, terminal, _ = make_frame_batch(self.B, self.A, seed=23, n_frames=self.B + 64)
            self.batch = eng.make_batch(frames=d(frames), frame_stride=frames.shape[1], frame_ids=d(ids), action=d(action), reward=d(reward),
                                        terminal=d(terminal))
        else:
            self.B, self.A = 32, 4
            self.K, self.eps, kw, dueling = {"fc": (3, 1e-8, {}, False), "duel": (3, 1.5e-4, {}, True),
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
                                        terminal=d((rng.random(self.B) < 0.2).astype(np.uint8)))
        if noisy:
            eng.init_sigma()
        self.eng = eng
        self.real = _real(eng)

    # ---- the Dense tensors of the flat buffer: (kernel offset, bias offset, out_p, in_p, offset of ein, offset of eout) per noisy layer
    def dense(self):
        eng = self.eng
        kernels = sorted((i for i in eng.infos if i.kind == 1), key=lambda i: i.layer)
        biases = {i.name.decode().split("/")[0]: i for i in eng.infos if i.kind == 2}
        out = []
        for info, (off, n_in, n_out) in zip(kernels, eng.noise_layout):
            assert (int(info.dims[0]), int(info.dims[1])) == (n_out, n_in)
            out.append((int(info.offset), int(biases[info.name.decode().split("/")[0]].offset), n_out, n_in, off, off + n_in))
        return out

    def dense_mask(self):
        m = np.zeros(self.eng.n_param_floats, bool)
        for k, b, o, i, _, _ in self.dense():
            m[k:k + o * i] = True
            m[b:b + o] = True
        return m

    def factors(self, noise):
        """n of every element of the flat buffer (fp32; 0 outside the Dense tensors)."""
        n = np.zeros(self.eng.n_param_floats, np.float32)
        for k, b, o, i, a_in, a_out in self.dense():
            n[k:k + o * i] = nz.factors(noise[a_in:a_in + i], noise[a_out:a_out + o]).reshape(-1)
            n[b:b + o] = noise[a_out:a_out + o]
        return n

    def compose_ref(self, mu, sigma, noise):
        eff = mu.copy()
        for k, b, o, i, a_in, a_out in self.dense():
            ein, eout = noise[a_in:a_in + i], noise[a_out:a_out + o]
            eff[k:k + o * i] = nz.compose_kernel(mu[k:k + o * i].reshape(o, i), sigma[k:k + o * i].reshape(o, i), ein, eout).reshape(-1)
            eff[b:b + o] = nz.compose_bias(mu[b:b + o], sigma[b:b + o], eout)
        return eff


def _np(t):
    return t.detach().cpu().numpy()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ 1. sample
@pytest.mark.parametrize("name", ["fc", "headline-B32"])
def test_sample_matches_the_float64_reference_and_the_counter_advances(name):
    case = Case(name)
    eng = case.eng
    count0 = 5
    eng.noise_count.fill_(count0)
    eng.resample_noise()
    torch.cuda.synchronize()
    first = _np(eng.noise).copy()
    assert int(eng.noise_count.item()) == count0 + 1
    ref, z64, r64 = nz.sample_all(eng.noise_layout, SEED, count0, 0)
    s = np.copysign(first.astype(np.float64) ** 2, first)
    err = np.abs(s - z64)
    bound = 16 * 2.0**-24 * np.maximum(1.0, r64)
    print(f"{name}: max |s - z64| / bound = {(err / bound).max():.3f} over {err.size} elements (max abs error {err.max():.3e})")
    assert np.isfinite(first).all() and np.all(err <= bound)
    assert np.all(np.abs(first - ref) <= 2.0**-20 * np.maximum(1.0, np.abs(ref)))  # f itself, loosely: sign and magnitude
    # the same (seed, count, stream_id) reproduces the bits; the next count and the other stream do not
    eng.resample_noise()
    torch.cuda.synchronize()
    second = _np(eng.noise).copy()
    assert int(eng.noise_count.item()) == count0 + 2 and not np.array_equal(_u32(first), _u32(second))
    eng.noise_count.fill_(count0)
    eng.resample_noise()
    assert np.array_equal(_u32(_np(eng.noise)), _u32(first))
    eng.noise_count.fill_(count0)
    eng.resample_noise(1, eng.noise_target)
    torch.cuda.synchronize()
    other = _np(eng.noise_target)
    assert int(eng.noise_count.item()) == count0 + 1 and not np.array_equal(_u32(other), _u32(first))
    ref1, z1, r1 = nz.sample_all(eng.noise_layout, SEED, count0, 1)
    assert np.all(np.abs(np.copysign(other.astype(np.float64) ** 2, other) - z1) <= 16 * 2.0**-24 * np.maximum(1.0, r1))
    # a 64-bit count reaches the counter's high word
    eng.noise_count.fill_((3 << 32) | 7)
    eng.resample_noise()
    hi = _np(eng.noise)
    _, zh, rh = nz.sample_all(eng.noise_layout, SEED, (3 << 32) | 7, 0)
    assert np.all(np.abs(np.copysign(hi.astype(np.float64) ** 2, hi) - zh) <= 16 * 2.0**-24 * np.maximum(1.0, rh))
    assert int(eng.noise_count.item()) == ((3 << 32) | 7) + 1


def test_a_value_does_not_depend_on_the_widths_of_other_layers():
    from slimdqn._engine import QNetEngine

    a = QNetEngine((8,), 4, 4, (100, 100), "fc", True, 32, noisy=True, noisy_seed=SEED)
    b = QNetEngine((8,), 4, 4, (100, 60), "fc", True, 32, noisy=True, noisy_seed=SEED)
    for e in (a, b):
        e.resample_noise()
    na, nb = _np(a.noise), _np(b.noise)
    (oa0, ia0, wa0), (oa1, ia1, wa1), (oa2, ia2, wa2) = a.noise_layout
    (ob0, ib0, wb0), (ob1, ib1, wb1), (ob2, ib2, wb2) = b.noise_layout
    assert (ia0, wa0, ia1) == (ib0, wb0, ib1) and wa1 != wb1 and oa2 != ob2
    assert np.array_equal(_u32(na[oa0:oa0 + ia0 + wa0]), _u32(nb[ob0:ob0 + ib0 + wb0]))  # layer 0
    assert np.array_equal(_u32(na[oa1:oa1 + ia1]), _u32(nb[ob1:ob1 + ib1]))  # ein of layer 1
    assert np.array_equal(_u32(na[oa1 + ia1:oa1 + ia1 + wb1]), _u32(nb[ob1 + ib1:ob1 + ib1 + wb1]))  # eout of layer 1: the common prefix
    assert np.array_equal(_u32(na[oa2:oa2 + ib2]), _u32(nb[ob2:ob2 + ib2]))  # ein of the head: the common prefix, at another offset
    assert np.array_equal(_u32(na[oa2 + ia2:oa2 + ia2 + wa2]), _u32(nb[ob2 + ib2:ob2 + ib2 + wb2]))  # eout of the head


# ------------------------------------------------------------------ 2. compose
@pytest.mark.parametrize("name", CASES)
def test_compose_equals_the_fp32_reference_bit_for_bit(name):
    case = Case(name)
    eng = case.eng
    eng.resample_noise()
    eff = _np(eng.compose()).copy()
    mu, sigma, noise = _np(eng.params), _np(eng.sigma), _np(eng.noise)
    dense = case.dense_mask()
    assert np.array_equal(_u32(eff), _u32(case.compose_ref(mu, sigma, noise)))
    assert np.array_equal(_u32(eff[~dense]), _u32(mu[~dense])) and not np.array_equal(eff[dense & case.real], mu[dense & case.real])
    assert np.all(_u32(eff[~case.real]) == 0) and np.all(_u32(sigma[~(dense & case.real)]) == 0)  # padding: +0.0f, no sigma outside the Dense tensors
    assert np.all(sigma[dense & case.real] > 0) or eng.dueling
    if eng.dueling:
        info = eng.head_kernel_info()
        structural = int(info.offset) + du.structural_indices(FC[-1], int(info.dims[1]), eng.n_heads, case.A, 1)
        assert np.all(_u32(eff[structural]) == 0) and np.all(_u32(sigma[structural]) == 0)
        live = dense & case.real
        live[structural] = False
        assert np.all(sigma[live] > 0)
    # the mirror compose wrote is the one refresh_mirror builds from eff
    from slimdqn import _hip

    mine = _bits(eng.region("wsplit"))
    off, size = ctypes.c_int64(), ctypes.c_int64()
    _hip.check(eng.lib.isdqn_net_workspace_region(ctypes.byref(eng.cfg), b"wsplit", ctypes.byref(off), ctypes.byref(size)))
    ws2 = torch.zeros_like(eng.workspace)
    _hip.check(eng.lib.isdqn_net_refresh_mirror(ctypes.byref(eng.cfg), _hip.ptr(eng.eff), _hip.ptr(ws2), _hip.stream_ptr(eng.device)))
    torch.cuda.synchronize()
    assert np.array_equal(mine, _bits(ws2[off.value // 4:(off.value + size.value) // 4]))
    # without a workspace nothing but eff is written
    before = _bits(eng.workspace)
    eng.compose(mirror=False)
    assert np.array_equal(before, _bits(eng.workspace))
    # zero noise: the mean network, bit for bit
    eng.zero_noise()
    assert np.array_equal(_bits(eng.compose()), _bits(eng.params))


# ------------------------------------------------------------------ 3. zero noise: the plain step's outputs
@pytest.mark.parametrize("name", CASES)
def test_with_zero_noise_the_step_reports_what_the_plain_network_reports(name):
    noisy, plain = Case(name), Case(name, noisy=False)
    assert torch.equal(noisy.eng.params, plain.eng.params)
    g = torch.zeros_like(plain.eng.params)
    plain.eng.grad_on_batch(plain.batch, g, target_params=plain.target)
    want = [_bits(t) for t in (plain.eng.losses, plain.eng.q_values, plain.eng.targets)]
    e = noisy.eng
    s0 = [_bits(t) for t in (e.sigma, e.sigma_m, e.sigma_v)]
    e.zero_noise()
    if noisy.target is not None:
        e.learn_on_batch_target(noisy.batch, noisy.target)
    else:
        e.learn_on_batch(noisy.batch)
    torch.cuda.synchronize()
    got = [_bits(t) for t in (e.losses, e.q_values, e.targets)]
    for a, b, what in zip(got, want, ("losses", "q_values", "targets")):
        assert np.array_equal(a, b), what
    assert np.array_equal(_bits(e.grad), _bits(g))
    # priorities, bit for bit on every case: the loss kernels' own arithmetic on those (bit-identical) q_values and targets -- the
    # gradient-only pass of the plain network takes no priorities pointer, so the kernel's arithmetic restated in numpy is the reference
    want_p = _priorities_ref(_np(e.q_values), _np(e.targets))
    assert np.array_equal(_np(e.priorities).view(np.uint64), want_p.view(np.uint64)), "priorities differ from the loss kernel's arithmetic"
    # ... and the plain update step's own priorities.  fc and headline-B32 take the head chain there (another kernel, the same
    # arithmetic on its own q_values): the comparison holds on them too wherever that kernel forms the same q_values and targets
    if plain.target is not None:
        plain.eng.learn_on_batch_target(plain.batch, plain.target)
    else:
        plain.eng.learn_on_batch(plain.batch)
    torch.cuda.synchronize()
    same_q = np.array_equal(_bits(plain.eng.q_values), got[1]) and np.array_equal(_bits(plain.eng.targets), got[2])
    print(f"{name}: the plain update step's q_values / targets are {'the same bits' if same_q else 'other bits (head chain)'}")
    if same_q or name in ("duel", "hist", "dqn"):  # (no head chain on these three: the same loss kernel, the same bits)
        assert np.array_equal(_bits(e.priorities), _bits(plain.eng.priorities))
    for a, b, what in zip([_bits(t) for t in (e.sigma, e.sigma_m, e.sigma_v)], s0, ("sigma", "sigma_m", "sigma_v")):
        assert np.array_equal(a, b), what
    assert int(e.adam_count.item()) == 1 and not np.array_equal(_bits(e.params), _bits(noisy.eng.eff))  # mu moved, eff is the step's input


# ------------------------------------------------------------------ 4. noise on
@pytest.mark.parametrize("name", CASES)
def test_noisy_step_trains_mu_and_sigma_from_one_gradient(name):
    case, plain = Case(name, sigma0=0.5), Case(name, noisy=False)
    e = case.eng
    dense, real = case.dense_mask(), case.real
    e.resample_noise()
    for t in (1, 2):  # the second step uses the moments of the first
        mu0, s0 = _np(e.params).astype(np.float64), _np(e.sigma).astype(np.float64)
        m0, v0, sm0, sv0 = (_np(x).astype(np.float64) for x in (e.adam_m, e.adam_v, e.sigma_m, e.sigma_v))
        if case.target is not None:
            e.learn_on_batch_target(case.batch, case.target)
        else:
            e.learn_on_batch(case.batch)
        torch.cuda.synchronize()
        assert int(e.adam_count.item()) == t
        noise = _np(e.noise)
        grad = _np(e.grad).copy()
        # the gradient is the plain network's on eff (and, the DQN form, on the composed target)
        g = torch.zeros_like(plain.eng.params)
        plain.eng.grad_on_batch(plain.batch, g, target_params=None if case.target is None else e.eff_target, params=e.eff)
        assert np.array_equal(_u32(grad), _bits(g).view(np.uint32)), f"step {t}: grad differs from grad_on_batch on eff"
        assert np.array_equal(_u32(_np(e.eff)), _u32(case.compose_ref(mu0.astype(np.float32), s0.astype(np.float32), noise)))
        assert np.isfinite(grad).all() and np.all(grad[~real] == 0) and np.abs(grad[dense]).max() > 0
        if case.target is not None:
            assert not np.array_equal(_u32(_np(e.noise_target)), _u32(noise))
            assert not np.array_equal(_bits(e.eff_target), _bits(case.target))
        # mu: float64 Adam on grad
        (p, m, v, _), (ep, em, ev) = adam_bounds(mu0, m0, v0, grad, t, LR, case.eps)
        assert np.all(np.abs(_np(e.params) - p) <= ep) and np.all(np.abs(_np(e.adam_m) - m) <= em) and np.all(np.abs(_np(e.adam_v) - v) <= ev)
        # sigma: float64 Adam on fl32(grad * n) at the Dense positions, untouched +0 elsewhere
        gs = grad * case.factors(noise)
        assert np.abs(gs[dense]).max() > 0
        (p, m, v, _), (ep, em, ev) = adam_bounds(s0[dense], sm0[dense], sv0[dense], gs[dense], t, LR, case.eps)
        assert np.all(np.abs(_np(e.sigma)[dense] - p) <= ep) and np.all(np.abs(_np(e.sigma_m)[dense] - m) <= em)
        assert np.all(np.abs(_np(e.sigma_v)[dense] - v) <= ev)
        assert np.abs(_np(e.sigma)[dense] - s0[dense]).max() > 0.5 * LR  # it really moved
        for buf in (e.sigma, e.sigma_m, e.sigma_v):
            assert np.all(_u32(_np(buf)[~(dense & real)]) == 0), "a position outside the real Dense elements of sigma left +0.0f"
        if e.dueling:
            info = e.head_kernel_info()
            structural = int(info.offset) + du.structural_indices(FC[-1], int(info.dims[1]), e.n_heads, case.A, 1)
            for buf in (e.sigma, e.sigma_m, e.sigma_v, e.params, e.grad):
                assert np.all(_u32(_np(buf)[structural]) == 0)


# ------------------------------------------------------------------ 5. shift_params
def test_shift_params_moves_the_head_blocks_of_sigma_as_those_of_mu():
    case = Case("fc")
    e = case.eng
    x = torch.from_numpy(np.random.default_rng(0).normal(size=e.n_param_floats).astype(np.float32)).cuda()
    e.params.copy_(x)
    e.sigma.copy_(x)
    e.shift_params()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(e.sigma), _bits(e.params)) and not np.array_equal(_bits(e.sigma), _bits(x))
    moved = _np(e.sigma) != _np(x)
    assert np.all(case.dense_mask()[moved])


# ------------------------------------------------------------------ 6. agents
def _isdqn(use_graph=True, noisy=True, **kw):
    from slimdqn.networks.isdqn import iSDQN

    return iSDQN(0, (84, 84, 4), 5, 3, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 3, 1, 6, adam_eps=1.5e-4, batch_size=8, use_graph=use_graph,
                 noisy=noisy, **kw)


def test_acting_draws_new_noise_and_noisy_eval_is_the_mean_network():
    agent = _isdqn()
    state = np.random.default_rng(0).integers(0, 256, (84, 84, 4), dtype=np.uint8)
    c0 = int(agent._engine.noise_count.item())
    q1, q2 = agent.q_values(agent.params, state), agent.q_values(agent.params, state)
    assert not np.array_equal(q1, q2) and int(agent._engine.noise_count.item()) == c0 + 2
    with agent.noisy_evaluation():
        e1, e2 = agent.q_values(agent.params, state), agent.q_values(agent.params, state)
        a1, a2 = agent.best_action(agent.params, state, key=1), agent.best_action(agent.params, state, key=1)
    assert np.array_equal(e1, e2) and a1 == a2 and int(agent._engine.noise_count.item()) == c0 + 2
    assert not agent.noisy_eval
    # the mean network is the plain network on mu
    plain = _isdqn(noisy=False)
    assert torch.equal(plain._engine.params, agent._engine.params)
    assert np.array_equal(plain.q_values(plain.params, state), e1)
    # batched acting: one draw for all rows
    states = np.stack([state, state])
    agent.best_actions(agent.params, states, key=np.array([0, 0]))
    assert int(agent._engine.noise_count.item()) == c0 + 3


def _fill(rbs, n=40, A=5):
    from slimdqn.sample_collection.replay_buffer import TransitionElement

    rng = np.random.default_rng(0)
    for _ in range(n):
        obs = rng.integers(0, 256, (84, 84), dtype=np.uint8)
        a, r, term = int(rng.integers(0, A)), float(rng.choice([-1.0, 0.0, 1.0])), bool(rng.random() < 0.08)
        for rb in rbs:
            rb.add(TransitionElement(obs, a, r, term, term))


def test_three_captured_learn_steps_equal_three_eager_steps():
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    eager, graphed = _isdqn(use_graph=False), _isdqn(use_graph=True)
    rbs = [ReplayBuffer(UniformSamplingDistribution(5), 8, 64, update_horizon=3, gamma=0.99) for _ in range(2)]
    _fill(rbs)
    for agent, rb in zip((eager, graphed), rbs):
        agent.learn_steps(3, rb)
    torch.cuda.synchronize()
    assert eager._graphed is None and graphed._graphed is not None and graphed._graphed.S == 3
    for name in ("params", "sigma", "adam_m", "adam_v", "sigma_m", "sigma_v", "noise_count", "adam_count", "losses_accum"):
        a, b = getattr(eager._engine, name), getattr(graphed._engine, name)
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} elements differ between eager and captured noisy steps"
    assert int(graphed._engine.noise_count.item()) == 3 and int(graphed._engine.adam_count.item()) == 3
    fresh = _isdqn(use_graph=False)
    assert not torch.equal(fresh._engine.sigma, graphed._engine.sigma) and not torch.equal(fresh._engine.params, graphed._engine.params)
    # a second replay advances the noise again (the counter lives on the device)
    graphed.learn_steps(3, rbs[1])
    eager.learn_steps(3, rbs[0])
    torch.cuda.synchronize()
    assert int(graphed._engine.noise_count.item()) == 6
    assert torch.equal(eager._engine.sigma, graphed._engine.sigma) and torch.equal(eager._engine.params, graphed._engine.params)


def test_the_dqn_agent_draws_the_target_on_its_own_stream_and_get_model_round_trips():
    from slimdqn.networks.dqn import DQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    agent = DQN(0, (84, 84, 4), 5, [8, 12, 16, 24], True, "cnn", 2e-4, 0.99, 1, 1, 6, adam_eps=1.5e-4, batch_size=8, use_graph=False, noisy=True)
    rb = ReplayBuffer(UniformSamplingDistribution(5), 8, 64, update_horizon=1, gamma=0.99)
    _fill([rb])
    eng = agent._engine
    agent.update_online_params(0, rb)
    torch.cuda.synchronize()
    assert int(eng.noise_count.item()) == 2 and int(eng.adam_count.item()) == 1  # the online draw, then the target's
    assert not torch.equal(eng.noise, eng.noise_target) and bool((eng.noise_target != 0).any())
    layout = eng.noise_layout
    ref0, z0, r0 = nz.sample_all(layout, agent._seed, 0, 0)
    ref1, z1, r1 = nz.sample_all(layout, agent._seed, 1, 1)
    for dev, z, r in ((eng.noise, z0, r0), (eng.noise_target, z1, r1)):
        f = _np(dev).astype(np.float64)
        assert np.all(np.abs(np.copysign(f * f, f) - z) <= 16 * 2.0**-24 * np.maximum(1.0, r))
    assert not torch.equal(agent.target_sigma, eng.sigma)  # the target keeps its sigma until the next target update
    agent.update_target_params(6)
    assert torch.equal(agent.target_sigma, eng.sigma) and torch.equal(agent.target_params.tensor, eng.params)
    # get_model carries the sigma leaves and _bind loads both buffers back
    model = agent.get_model()
    tree = model["params"]["params"]
    assert all({"kernel", "bias", "sigma_kernel", "sigma_bias"} <= set(tree[m]) for m in ("Dense_0", "Dense_1"))
    assert "sigma_kernel" not in tree["Conv_0"] and tree["Dense_0"]["sigma_kernel"].shape == tree["Dense_0"]["kernel"].shape
    t = agent._bind(model)
    assert torch.equal(t, eng.params) and torch.equal(agent._bound_sigma, eng.sigma)
    other = DQN(1, (84, 84, 4), 5, [8, 12, 16, 24], True, "cnn", 2e-4, 0.99, 1, 1, 6, adam_eps=1.5e-4, batch_size=8, use_graph=False, noisy=True)
    other._load_bound(other._engine, other._bind(model))
    assert torch.equal(other._engine.params, eng.params) and torch.equal(other._engine.sigma, eng.sigma)
    with pytest.raises(ValueError):
        agent.recycle_dormant(rb, 0.1)


def test_an_analysis_agent_takes_its_three_gradients_and_its_step_under_one_draw():
    """AnalysisDQN with noisy layers: one draw per update serves the two single-pair gradients, the iS-DQN step (whose gradient is the
    third) and the churn passes behind it; the noise counter advances once per update and sigma trains."""
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(5), 8, 64, update_horizon=1, gamma=0.99)
    _fill([rb])
    for agent in (AnalysisDQN(0, (84, 84, 4), 5, 3, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 1, 1, 6, adam_eps=1.5e-4, batch_size=8, noisy=True),
                  AnalysisTFDQN(0, (84, 84, 4), 5, [8, 12, 16, 24], True, False, "cnn", 2e-4, 0.99, 1, 1, 6, adam_eps=1.5e-4, batch_size=8, noisy=True)):
        eng = agent._engine
        sigma0 = eng.sigma.clone()
        for step in (1, 2):
            agent.update_online_params(0, rb)
            torch.cuda.synchronize()
            assert int(eng.noise_count.item()) == step and int(eng.adam_count.item()) == step
        assert eng.resample_on_learn and not torch.equal(eng.sigma, sigma0) and bool(torch.isfinite(eng.params).all())
        if isinstance(agent, AnalysisDQN):
            assert np.isfinite(agent.cumulated_cosine_sim_is_to_tb) and np.isfinite(agent.cumulated_cosine_sim_tf_to_tb)
            assert abs(agent.cumulated_cosine_sim_is_to_tb) <= 2.0 + 1e-6 and np.isfinite(agent.cumulated_target_churns_train).all()
            # the step's gradient is the gradient-only pass on the same composed network: the same draw served both
            g = torch.zeros_like(eng.params)
            batch = rb.sample()
            cb = agent._c_batch(eng, batch)
            eng.grad_on_batch(cb, g)  # (composes with the noise of the last update: no new draw)
            assert int(eng.noise_count.item()) == 2
        else:
            assert np.isfinite(agent.cumulated_target_churn_train) and np.isfinite(agent.cumulated_target_churn_eval)
