"""REM, the random ensemble mixture, on the GPU (include/isdqn_hip.h, isdqn_mixture_draw / isdqn_batch_mixture / ISDQN_ACT_MEAN_HEADS)
against the float64 restatement of tests/helpers/mixture.py, which is written from the header's definition:

1. the draw: alpha bit for bit, the carry of the count into its high word, the count's advance, the refused head counts;
2. the loss on the device's own rows (regions "q" / "q_target"): q_values, targets, losses, priorities, dL/dq and the head-bias gradient
   in the *_target form and the same-parameter form, with the max form, double_q, Huber, loss weights and a discount tensor;
3. off is off: an engine without set_mixture keeps today's bits, and at H = 1 the *_target learn call with the flag has the bits of the
   call without it after three steps;
4. the whole path against the float64 oracle forward: every leaf's gradient and one Adam step, fc and a tiny cnn;
5. acting on the head average, exact ties, idx_networks = NULL;
6. the DQN agent: run-to-run bit identity, captured against eager steps with the draw count, -rr 2, hard and EMA targets, dueling;
7. the refusals of the C ABI.

Tolerances (section 2): rtol 1e-5, the project's bound of a float32 kernel against float64 on the same inputs, plus absolute floors
derived in tests/helpers/mixture.py (q_floor, bounds): a mixture of mixed-sign Q values cancels, so no relative bound alone holds.
The argmax is discontinuous: a transition is left out only when, in the float64 reference alone, the gap between the two largest mixed
next-state values is below 10 x the q floor; at most 10 % of a case may be left out, and the committed seeds leave out none
(scripts/mixture_seeds.py checks them on the CPU with the oracle forward)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import network as onet
from tests.gpu_helpers import adam64, make_frame_batch, perturbed_params
from tests.helpers import mixture as hm

pytestmark = pytest.mark.gpu

TOL = {"bf16x3": dict(q=1e-3, loss=1e-3, grad=3e-3), "bf16": dict(q=8e-2, loss=5e-2, grad=2.5e-1)}  # tests/test_gpu_double_q.py
FC_OBS, FC_FEATS, TINY = (8,), (16, 24), (7, 9, 11, 13)
SEED, TARGET_SEED = 0x5EED0123456789, 31
DOMINANT = 2.0  # per-head biased actions (biased_params)


def _obs(arch):
    return FC_OBS if arch == "fc" else (84, 84, 4)


def biased_params(seed, feats, A, H, arch, mul=2, add=1, width=None):
    """perturbed_params with one preferred action per head: two heads of three prefer action ``add``, every third head one of its own.
    About two thirds of the mixture's mass then sits on one action, so the mixed next-state values keep their distance under any
    draw, while taking max_a per head before mixing (every head's own preference) stays far from mixing first."""
    p = perturbed_params(seed, _obs(arch), feats, arch, H * A if width is None else width, True, scale=0.3)
    head = f"Dense_{len(feats) - (0 if arch == 'fc' else 3)}"
    if width is None:
        for h in range(H):
            p[head]["bias"][h * A + (add % A if h % 3 else (mul * h + add + 1) % A)] += np.float32(DOMINANT)
    return p


def _engine(H, A, B, arch="fc", feats=FC_FEATS, seed=1, mixture=True, precision="bf16x3", lr=1e-3, **kw):
    from slimdqn._engine import QNetEngine

    eng = QNetEngine(_obs(arch), A, H, feats, arch, True, B, gamma_n=0.99, learning_rate=lr, adam_eps=1.5e-4, precision=precision, **kw)
    width = None if not kw.get("dueling") else H * (A + 1)
    eng.import_flax(biased_params(seed, feats, A, H, arch, width=width))
    tgt = torch.zeros_like(eng.params)
    eng.import_flax(biased_params(TARGET_SEED, feats, A, H, arch, 3, 2, width=width), target=tgt)
    if mixture:
        eng.set_mixture(SEED)
    return eng, tgt


class _Batch:
    def __init__(self, eng, arch, B, A, seed, weights=False, discount=False):
        rng = np.random.default_rng(seed + 100)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.weights = rng.uniform(0.2, 1.0, B).astype(np.float32) if weights else None
        self.discount = rng.uniform(0.5, 0.99, B).astype(np.float32) if discount else None
        self.reward = rng.normal(size=B).astype(np.float32)
        if arch == "fc":
            s, ns = (rng.normal(size=(B, FC_OBS[0])).astype(np.float32) for _ in range(2))
            self.action = rng.integers(0, A, B).astype(np.int32)
            self.terminal = (rng.random(B) < 0.3).astype(np.uint8)
            self.x_state, self.x_next = torch.from_numpy(s), torch.from_numpy(ns)
            kw = lambda: dict(state=d(s), next_state=d(ns))
        else:
            frames, ids, self.action, _, self.terminal, ref = make_frame_batch(B, A, seed=seed)
            self.x_state, self.x_next = torch.from_numpy(ref.state), torch.from_numpy(ref.next_state)
            kw = lambda: dict(frames=d(frames), frame_stride=frames.shape[1], frame_ids=d(ids))
        if eng is not None:
            self.cb = eng.make_batch(action=d(self.action), reward=d(self.reward), terminal=d(self.terminal),
                                     loss_weights=None if self.weights is None else d(self.weights),
                                     discount=None if self.discount is None else d(self.discount), **kw())


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _rows(eng, name, n):
    w, w_p = eng.n_heads * eng.n_actions, (eng.n_heads * eng.n_actions + 7) // 8 * 8
    return eng.region(name)[: n * w_p].reshape(n, w_p)[:, :w].double().cpu().numpy()


def _close(got, want, floor, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, bound = np.abs(got - want), hm.RTOL * np.abs(want) + floor
    print(f"  {what}: max error {err.max():.3e}, smallest margin {np.min(bound - err):.3e} (largest bound {np.max(bound):.3e})")
    assert (err <= bound).all(), what


# ------------------------------------------------------------------ 1. the draw
@pytest.mark.parametrize("H", [1, 2, 63, 64, 65, 200, 1024])
def test_draw_is_the_helper_bit_for_bit(H):
    from slimdqn import _hip

    lib = _hip.lib()
    alpha = torch.zeros(H, dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for c0 in (0, 1, 2**32 - 1, 2**32):  # (the carry into hi32: 2^32 - 1 -> 2^32)
        count.fill_(c0)
        _hip.check(lib.isdqn_mixture_draw(H, SEED, _hip.ptr(count), _hip.ptr(alpha), _hip.stream_ptr(alpha.device)))
        torch.cuda.synchronize()
        want = hm.draw(H, SEED, c0)
        assert np.array_equal(_cpu(alpha).view(np.uint32), want.view(np.uint32)), (H, c0)
        assert int(count.item()) == c0 + 1
    if H == 1:
        assert _cpu(alpha)[0] == np.float32(1.0)
    else:
        assert abs(float(_cpu(alpha).astype(np.float64).sum()) - 1.0) < H * 2.0**-23 and (_cpu(alpha) > 0).all()


def test_draw_refuses_head_counts_outside_its_range_and_null_pointers():
    from slimdqn import _hip

    lib = _hip.lib()
    alpha = torch.full((8,), 7.0, dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = _hip.stream_ptr(alpha.device)
    for H in (0, 1025, -3):
        assert lib.isdqn_mixture_draw(H, SEED, _hip.ptr(count), _hip.ptr(alpha), st) == _hip.ERR_ARG
    assert lib.isdqn_mixture_draw(4, SEED, None, _hip.ptr(alpha), st) == _hip.ERR_ARG
    assert lib.isdqn_mixture_draw(4, SEED, _hip.ptr(count), None, st) == _hip.ERR_ARG
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and (_cpu(alpha) == 7.0).all()  # nothing was launched


# ------------------------------------------------------------------ 2. the loss on the device's own rows
# (H, A, B); B = 70: two workgroups of td_kernel's 64-row partition, the last ragged; A = 70: the actions walked in two chunks of 64 lanes,
# the path of A > 64 (mix_at / mix_argmax: the argmax and, with double_q, the value's chunk across the chunks)
CASES = [(3, 5, 5), (2, 1, 64), (8, 4, 70), (200, 18, 8), (2, 70, 5)]
OPTIONS = ["max", "double_q", "huber", "weights", "discount"]


def _option_kw(option):
    return dict(double_q=True) if option == "double_q" else dict(huber_delta=0.4) if option == "huber" else {}


def own_rows_case(H, A, B, option, form):
    kw = _option_kw(option)
    eng, tgt = _engine(H, A, B, **kw)
    b = _Batch(eng, "fc", B, A, seed=3 + H, weights=option == "weights", discount=option == "discount")
    return eng, tgt, b, kw


def oracle_rows(H, A, arch, feats, b, form, dq):
    """What needs no GPU: the float64 oracle forward of a case's two networks -> (rows [2B], value rows [B] or None) as section 2
    reads them from the device (scripts/mixture_seeds.py checks the committed seeds with it)."""
    f = lambda params, x: onet.forward(onet.to_torch(params, torch.float64), x, feats, arch, True).detach().numpy()
    p, tp = biased_params(1, feats, A, H, arch), biased_params(TARGET_SEED, feats, A, H, arch, 3, 2)
    on_s, on_n = f(p, b.x_state), f(p, b.x_next)
    if form == "same":
        return np.concatenate([on_s, on_n]), None
    tg_n = f(tp, b.x_next)
    return (np.concatenate([on_s, on_n]), tg_n) if dq else (np.concatenate([on_s, tg_n]), None)


def oracle_case(H, A, B, option, form):
    """(reference, floors) of a section-2 case on the oracle's rows, at the draw the test uses (count 1)."""
    kw = _option_kw(option)
    b = _Batch(None, "fc", B, A, seed=3 + H, weights=option == "weights", discount=option == "discount")
    dq = option == "double_q" and form == "target"
    rows, vrows = oracle_rows(H, A, "fc", FC_FEATS, b, form, dq)
    ref = hm.mixture(rows, vrows, hm.draw(H, SEED, 1), b.action, b.reward, b.terminal, 0.99, A, double_q=dq, weights=b.weights,
                     discount=b.discount, huber_delta=kw.get("huber_delta", 0.0))
    return ref, hm.bounds(ref, H, B)


@pytest.mark.parametrize("form", ["target", "same"])
@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("case", CASES)
def test_loss_matches_float64_on_the_device_rows(case, option, form):
    H, A, B = case
    eng, tgt, b, kw = own_rows_case(H, A, B, option, form)
    eng.mixture_draw()
    eng.mixture_draw()  # (the second draw of the engine: count 1)
    if form == "target":
        losses = eng.learn_on_batch_target(b.cb, tgt)
    else:
        losses = eng.learn_on_batch(b.cb)
    torch.cuda.synchronize()
    alpha = _cpu(eng.mix_alpha)
    assert np.array_equal(alpha.view(np.uint32), hm.draw(H, SEED, 1).view(np.uint32)) and int(eng.mix_count.item()) == 2
    dq = option == "double_q"
    rows = _rows(eng, "q", 2 * B)
    # *_target with double_q: the target network's rows are region "q_target"; without it they are rows [B, 2B) of "q"; the
    # same-parameter form reads rows [B, 2B) of its one forward on both sides (selector = value network: the max form)
    vrows = _rows(eng, "q_target", B) if (form == "target" and dq) else None
    args = dict(double_q=dq and form == "target", weights=b.weights, discount=b.discount, huber_delta=kw.get("huber_delta", 0.0))
    ref = hm.mixture(rows, vrows, alpha, b.action, b.reward, b.terminal, 0.99, A, **args)
    fl = hm.bounds(ref, H, B)
    keep = ref["gap"] >= 10 * fl["q_values"]
    assert (~keep).mean() <= 0.10, f"{(~keep).sum()} of {B} transitions left out"
    assert keep.all(), f"{(~keep).sum()} of {B} transitions left out: the committed cases leave out none"
    # the batch bites: each wrong reading is further than 100 x the bound from the restatement on these very rows
    for variant, key in (("online_only", "targets"), ("max_first", "targets"), ("no_alpha", "dout")):
        if A == 1 and variant == "max_first" or H == 1:
            continue  # (one action: max_a commutes with the mixture)
        wrong = hm.mixture(rows, vrows, alpha, b.action, b.reward, b.terminal, 0.99, A, variant=variant, **args)
        bound = hm.RTOL * np.abs(ref[key]) + (fl[key] if key != "dout" else fl[key] * np.ones_like(ref[key]))
        assert (np.abs(wrong[key] - ref[key]) > 100 * bound).any(), variant
    print(f"H={H} A={A} B={B} {option} {form}: min gap {ref['gap'].min():.3g} (left out below {10 * fl['q_values'].max():.3g})")
    _close(_cpu(eng.q_values).reshape(-1)[:B], ref["q_values"], fl["q_values"], "q_values")
    _close(_cpu(eng.targets).reshape(-1)[:B], ref["targets"], fl["targets"], "targets")
    _close(_cpu(losses)[0], ref["losses"], fl["losses"], "losses")
    _close(_cpu(eng.priorities), ref["priorities"], fl["priorities"], "priorities")
    w_p = (H * A + 7) // 8 * 8
    dout = _cpu(eng.region("dout")[: B * w_p]).reshape(B, w_p)
    assert not dout[:, H * A:].any()
    _close(dout[:, : H * A], ref["dout"], fl["dout"], "dout")
    assert ((dout[:, : H * A] != 0).sum(axis=1) <= H).all()
    dbh = _cpu(eng.region("dbh")[:w_p])
    _close(dbh[: H * A], ref["dbh"], fl["dbh"], "head-bias gradient")


# ------------------------------------------------------------------ 3. off is off
def _one_step(eng, b, tgt):
    losses = eng.learn_on_batch_target(b.cb, tgt)
    torch.cuda.synchronize()
    return [_cpu(x) for x in (losses, eng.q_values, eng.targets, eng.priorities, eng.params, eng.adam_m, eng.adam_v)]


def test_an_engine_without_a_mixture_builds_todays_batches_and_nothing_behind_them_is_read():
    """Without set_mixture the batch is the struct it was, and a call whose batch does not carry the flag reads nothing behind it: the
    same learn steps from a plain isdqn_batch and from an isdqn_batch_mixture without the flag, whose alpha points nowhere and whose
    n_mix is no head count, leave the same bits."""
    from slimdqn import _hip

    H, A, B = 3, 5, 8
    runs = []
    for longer in (False, True):
        eng, tgt = _engine(H, A, B, mixture=False)
        b = _Batch(eng, "fc", B, A, seed=3, weights=True)
        assert type(b.cb) is _hip.Batch and not b.cb.flags & _hip.BATCH_MIXTURE and eng.mix_alpha is None
        if longer:
            cb = _hip.BatchMixture()
            for name, _ in _hip.Batch._fields_:
                setattr(cb, name, getattr(b.cb, name))
            cb.alpha, cb.n_mix, cb.cql_alpha, cb.weight_decay, cb.discount = 0xDEAD0000, -5, 3.0, 7.0, 0xDEAD0000
            b.plain, b.cb = b.cb, cb  # (the plain batch keeps the tensors alive)
        steps = [_one_step(eng, b, tgt) for _ in range(2)]
        g = torch.zeros_like(eng.params)
        eng.learn_on_batch(b.cb, grad_out=g)  # (the same-parameter form too: the head chain's step)
        torch.cuda.synchronize()
        runs.append(steps + [[_cpu(x) for x in (eng.losses, eng.q_values, eng.targets, eng.priorities, eng.params, eng.adam_m, g)]])
    for s_off, s_on in zip(*runs):
        for x, y in zip(s_off, s_on):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("option", ["max", "double_q", "huber"])
def test_one_head_with_the_flag_has_the_bits_of_the_call_without_it(option):
    A, B = 5, 70
    kw = _option_kw(option)  # (huber: both branches of td_loss / td_dloss -- delta 0.4 with TD errors on either side of it)
    runs = []
    for mixture in (False, True):
        eng, tgt = _engine(1, A, B, mixture=mixture, **kw)
        b = _Batch(eng, "fc", B, A, seed=3, weights=True)
        steps = []
        for _ in range(3):
            if mixture:
                eng.mixture_draw()
            steps.append(_one_step(eng, b, tgt))
        if mixture:
            assert _cpu(eng.mix_alpha)[0] == np.float32(1.0)
        runs.append(steps)
    for s_off, s_on in zip(*runs):
        for name, x, y in zip(("losses", "q_values", "targets", "priorities", "params", "adam_m", "adam_v"), s_off, s_on):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name


# ------------------------------------------------------------------ 4. the whole path
E2E = dict(fc=0, cnn=5)  # batch seed per torso (scripts/mixture_seeds.py: they leave out no transition)
E2E_SHAPE = (4, 6, 32)


def e2e_gaps(arch):
    """(gap of the two largest mixed next-state values per transition, the bound below which one is left out) on the oracle's rows."""
    H, A, B = E2E_SHAPE
    feats = FC_FEATS if arch == "fc" else TINY
    b = _Batch(None, arch, B, A, seed=E2E[arch])
    rows, _ = oracle_rows(H, A, arch, feats, b, "same", False)
    ref = hm.mixture(rows, None, hm.draw(H, SEED, 0), b.action, b.reward, b.terminal, 0.99, A)
    return ref["gap"], 10 * TOL["bf16x3"]["q"] * max(1.0, float(np.abs(rows).max()))


@pytest.mark.parametrize("arch", ["fc", "cnn"])
def test_whole_path_matches_the_float64_oracle(arch):
    (H, A, B), lr = E2E_SHAPE, 1e-3
    feats = FC_FEATS if arch == "fc" else TINY
    t = TOL["bf16x3"]
    eng, tgt = _engine(H, A, B, arch=arch, feats=feats, lr=lr)
    b = _Batch(eng, arch, B, A, seed=E2E[arch])
    eng.mixture_draw()
    alpha = hm.draw(H, SEED, 0)
    pt = onet.to_torch(biased_params(1, feats, A, H, arch), torch.float64, requires_grad=True)
    rows = torch.cat([onet.forward(pt, b.x_state, feats, arch, True), onet.forward(pt, b.x_next, feats, arch, True)])
    ref = hm.mixture(rows.detach().numpy(), None, alpha, b.action, b.reward, b.terminal, 0.99, A)
    scale = max(1.0, float(np.abs(rows.detach().numpy()).max()))
    keep = ref["gap"] >= 10 * t["q"] * scale
    assert keep.all(), f"{(~keep).sum()} of {B} transitions left out: the committed cases leave out none"
    # the helper's loss with a graph through the online parameters: the target is a constant
    q_t = (rows[:B].reshape(B, H, A)[torch.arange(B), :, torch.from_numpy(b.action.astype(np.int64))] * torch.from_numpy(alpha.astype(np.float64))).sum(1)
    loss_t = ((q_t - torch.from_numpy(ref["targets"])) ** 2).mean()
    loss_t.backward()
    rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - want).max() / max(1.0, float(np.abs(want).max())))
    p0 = eng.params.clone()
    g = torch.zeros_like(eng.params)
    losses = eng.learn_on_batch(b.cb, grad_out=g)
    torch.cuda.synchronize()
    assert rel(_cpu(eng.q_values).reshape(-1)[:B], ref["q_values"]) < t["q"]
    assert rel(_cpu(eng.targets).reshape(-1)[:B], ref["targets"]) < t["q"]
    assert rel(_cpu(losses)[0], float(loss_t.detach())) < t["loss"]
    hip_g = eng.internal_to_flax_grads(g)
    for mod in pt:
        for leaf, tt in pt[mod].items():
            e = rel(hip_g[mod][leaf], tt.grad.numpy())
            print(f"  grad {mod}/{leaf}: max-rel {e:.2e}")
            assert e < t["grad"], (mod, leaf, e)
    head = f"Dense_{len(feats) - (0 if arch == 'fc' else 3)}"
    gk = np.asarray(hip_g[head]["kernel"]).reshape(-1, H, A)
    assert all(np.abs(gk[:, h]).max() > 0 for h in range(H))  # every head block of the head kernel has a gradient
    for info in eng.infos:
        sl = slice(info.offset, info.offset + info.size)
        pn, m, v, _, _ = adam64(p0[sl].cpu().numpy(), 0.0, 0.0, g[sl].cpu().numpy(), 1, lr, 1.5e-4)
        np.testing.assert_allclose(_cpu(eng.params[sl]), pn, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(_cpu(eng.adam_m[sl]), m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(_cpu(eng.adam_v[sl]), v, rtol=1e-5, atol=1e-15)
    assert int(eng.adam_count.item()) == 1


# ------------------------------------------------------------------ 5. acting
@pytest.mark.parametrize("case", [(3, 5, 6), (200, 18, 16), (2, 70, 5)])
def test_mean_heads_actions_are_numpys_on_the_device_rows(case):
    H, A, n = case
    eng, _ = _engine(H, A, max(n, 4), mixture=False)
    eng.import_flax(perturbed_params(1, FC_OBS, FC_FEATS, "fc", H * A, True, scale=0.3))  # (no preferred action: the rows disagree)
    obs = torch.from_numpy(np.random.default_rng(7).normal(size=(n, FC_OBS[0])).astype(np.float32)).cuda()
    out = eng.best_actions(obs=obs, idx_networks=None, mean_heads=True, n_rows=n)  # (idx_networks may be NULL)
    torch.cuda.synchronize()
    w_p = (H * A + 7) // 8 * 8
    q = _cpu(eng.region("q")[: n * w_p]).reshape(n, w_p)[:, : H * A]
    want, sums = hm.mean_heads_actions(q, A)
    assert np.array_equal(_cpu(out), want)
    with_idx = eng.best_actions(obs=obs, idx_networks=torch.zeros(n, dtype=torch.int32, device="cuda"), mean_heads=True)
    assert np.array_equal(_cpu(with_idx), want)
    assert len(set(want.tolist())) > 1 or n < 4  # (the rows do not all agree: the argmax is exercised)


def test_mean_heads_exact_ties_take_the_lowest_index():
    H, A, n = 4, 70, 4
    eng, _ = _engine(H, A, 4, mixture=False)
    p = eng.export_flax()
    head = "Dense_2"
    p[head]["kernel"][:] = 0.0  # the rows are the head bias: exact, equal from row to row
    bias = np.zeros((H, A), np.float32)
    bias[:, 66] = 0.5   # sums to 2.0 in the second chunk of 64 actions ...
    bias[0, 3] = 2.0    # ... and so does action 3 in the first: the lower index wins across the chunks
    bias[1, 69] = 2.0   # ... and action 69 behind it
    p[head]["bias"][:] = bias.reshape(-1)
    eng.import_flax(p)
    obs = torch.zeros(n, FC_OBS[0], dtype=torch.float32, device="cuda")
    out = eng.best_actions(obs=obs, idx_networks=None, mean_heads=True, n_rows=n)
    torch.cuda.synchronize()
    assert (_cpu(out) == 3).all()


# ------------------------------------------------------------------ 6. the agent
def _feed(rbs, rng, A):
    from slimdqn.sample_collection.replay_buffer import TransitionElement

    obs = rng.integers(0, 256, (84, 84), dtype=np.uint8)
    a, r, term = int(rng.integers(0, A)), float(rng.choice([-1.0, 0.0, 1.0])), bool(rng.random() < 0.08)
    for rb in rbs:
        rb.add(TransitionElement(obs, a, r, term, term))


def _agent(use_graph, A=5, B=8, C=48, **kw):
    from slimdqn.networks.dqn import DQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    agent = DQN(0, (84, 84, 4), A, [8, 12, 16, 24], True, "cnn", 2e-4, 0.99, 3, 1, 6, adam_eps=1.5e-4, batch_size=B, use_graph=use_graph,
                rem_heads=4, **kw)
    assert agent._engine.n_heads == 4 and agent._engine.mix_alpha is not None
    return agent, ReplayBuffer(UniformSamplingDistribution(5), B, C, update_horizon=3, gamma=0.99)


def _state(agent):
    e = agent._engine
    return [t.clone() for t in (e.params, e.adam_m, e.adam_v, e.adam_count, e.losses_accum, e.mix_count, e.mix_alpha, agent.target_params.tensor)]


@pytest.mark.parametrize("kw", [{}, dict(ema_tau=0.05), dict(dueling=True), dict(double_q=True)], ids=["hard", "ema", "dueling", "double_q"])
def test_agent_captured_steps_equal_eager_steps_and_runs_repeat(kw):
    A = 5
    agents = [_agent(False, **kw), _agent(True, **kw), _agent(True, **kw)]
    rng = np.random.default_rng(0)
    for _ in range(20):
        _feed([rb for _, rb in agents], rng, A)
    for step in range(1, 7):  # six gradient steps, a target update behind the sixth
        _feed([rb for _, rb in agents], rng, A)
        for agent, rb in agents:
            agent.update_online_params(step, rb)
            agent.update_target_params(step)
        torch.cuda.synchronize()
        states = [_state(agent) for agent, _ in agents]
        for name, e, g, g2 in zip(("params", "adam_m", "adam_v", "adam_count", "losses_accum", "mix_count", "mix_alpha", "target"), *states):
            assert torch.equal(e, g), f"step {step}: {name} differs between the eager and the captured steps"
            assert torch.equal(g, g2), f"step {step}: {name} differs from run to run"
    eager, graphed = agents[0][0], agents[1][0]
    assert eager._graphed is None and graphed._graphed is not None
    assert int(graphed._engine.mix_count.item()) == 6 and int(graphed._engine.adam_count.item()) == 6
    assert np.array_equal(_cpu(graphed._engine.mix_alpha).view(np.uint32), hm.draw(4, graphed._engine.mix_seed, 5).view(np.uint32))
    if "ema_tau" not in kw:
        assert torch.equal(graphed.target_params.tensor, graphed.params.tensor)  # the hard copy behind step 6
    # acting is on the head average, q_values too
    s = rng.integers(0, 256, (84, 84, 4), dtype=np.uint8)
    q = graphed.q_values(graphed.params, s)
    assert q.shape == (A,) and graphed.best_action(graphed.params, s) == int(np.argmax(q))


def test_agent_replay_ratio_two_is_two_draws_per_update():
    A = 5
    (eager, rb_e), (graphed, rb_g) = _agent(False), _agent(True)
    rng = np.random.default_rng(1)
    for _ in range(24):
        _feed((rb_e, rb_g), rng, A)
    for _ in range(3):
        eager.learn_steps(2, rb_e)
        graphed.learn_steps(2, rb_g)
    torch.cuda.synchronize()
    for name, e, g in zip(("params", "adam_m", "adam_v", "adam_count", "losses_accum", "mix_count", "mix_alpha", "target"), _state(eager), _state(graphed)):
        assert torch.equal(e, g), name
    assert int(graphed._engine.mix_count.item()) == 6


# ------------------------------------------------------------------ 7. the refusals of the C ABI
def _rc_loss(eng, cb, tgt):
    from slimdqn import _hip

    return eng.lib.isdqn_net_loss_on_batch_target(ctypes.byref(eng.cfg), _hip.ptr(eng.params), _hip.ptr(tgt), ctypes.byref(cb), _hip.ptr(eng.losses),
                                                  _hip.ptr(eng.q_values), _hip.ptr(eng.targets), _hip.ptr(eng.workspace), _hip.stream_ptr(eng.device))


def test_refused_calls_return_their_codes_and_launch_nothing():
    from slimdqn import _hip
    from slimdqn._engine import QNetEngine

    H, A, B = 3, 5, 8
    eng, tgt = _engine(H, A, B)
    b = _Batch(eng, "fc", B, A, seed=3)
    eng.q_values.fill_(-7.0)
    assert _rc_loss(eng, b.cb, tgt) == _hip.OK
    torch.cuda.synchronize()
    assert (_cpu(eng.q_values).reshape(-1)[:B] != -7.0).all()
    eng.q_values.fill_(-7.0)
    keep = b.cb.alpha
    b.cb.alpha = None
    assert _rc_loss(eng, b.cb, tgt) == _hip.ERR_ARG
    b.cb.alpha, b.cb.n_mix = keep, H + 1
    assert _rc_loss(eng, b.cb, tgt) == _hip.ERR_ARG
    b.cb.n_mix = H
    g = torch.zeros_like(eng.params)
    rc = eng.lib.isdqn_net_grad_on_batch(ctypes.byref(eng.cfg), _hip.ptr(eng.params), _hip.ptr(tgt), ctypes.byref(b.cb), 1, 1, 1, _hip.ptr(g),
                                         _hip.ptr(eng.losses), _hip.ptr(eng.q_values), _hip.ptr(eng.targets), _hip.ptr(eng.workspace),
                                         _hip.stream_ptr(eng.device))
    assert rc == _hip.ERR_UNSUPPORTED
    b.cb.flags |= _hip.BATCH_CONSERVATIVE
    b.cb.cql_alpha = 0.5
    assert _rc_loss(eng, b.cb, tgt) == _hip.ERR_UNSUPPORTED
    b.cb.cql_alpha = 0.0  # (the flag with a zero weight is off)
    assert _rc_loss(eng, b.cb, tgt) == _hip.OK
    b.cb.flags &= ~_hip.BATCH_CONSERVATIVE
    torch.cuda.synchronize()
    eng.q_values.fill_(-7.0)
    # configurations: a batch with the flag on an engine of another head type
    for kw in (dict(n_bins=11, min_value=-2.0, max_value=2.0, sigma=0.3), dict(n_quantiles=8), dict(munchausen_tau=0.03), dict(batch_norm=True)):
        arch, feats = ("cnn", TINY) if "batch_norm" in kw else ("fc", FC_FEATS)
        other = QNetEngine(_obs(arch), A, H, feats, arch, True, B, **kw)
        other.init_params(0)
        ob = _Batch(other, arch, B, A, seed=3)
        cb = _hip.BatchMixture()
        for name, _ in _hip.Batch._fields_:
            setattr(cb, name, getattr(ob.cb, name))
        cb.flags |= _hip.BATCH_MIXTURE
        alpha = torch.full((H,), 1.0 / H, device="cuda")
        cb.alpha, cb.n_mix = _hip.ptr(alpha), H
        t2 = other.params.clone()
        rc = _rc_loss(other, cb, t2) if "batch_norm" not in kw else other.lib.isdqn_net_loss_on_batch(
            ctypes.byref(other.cfg), _hip.ptr(other.params), ctypes.byref(cb), _hip.ptr(other.losses), _hip.ptr(other.q_values),
            _hip.ptr(other.targets), _hip.ptr(other.workspace), _hip.stream_ptr(other.device))
        assert rc == _hip.ERR_UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert (_cpu(eng.q_values) == -7.0).all()  # no refused call on `eng` wrote anything


def test_noisy_learn_step_refuses_the_mixture():
    from slimdqn import _hip
    from slimdqn._engine import QNetEngine

    H, A, B = 3, 5, 8
    eng = QNetEngine(FC_OBS, A, H, FC_FEATS, "fc", True, B, noisy=True)
    eng.init_params(0)
    b = _Batch(eng, "fc", B, A, seed=3)
    cb = _hip.BatchMixture()
    for name, _ in _hip.Batch._fields_:
        setattr(cb, name, getattr(b.cb, name))
    cb.flags |= _hip.BATCH_MIXTURE
    alpha = torch.full((H,), 1.0 / H, device="cuda")
    cb.alpha, cb.n_mix = _hip.ptr(alpha), H
    with pytest.raises(NotImplementedError):
        eng._noisy_learn(cb, None)
    with pytest.raises(ValueError):
        eng.set_mixture(1)


def test_an_engine_with_a_mixture_refuses_a_conservative_weight():
    from slimdqn import _mixture

    eng, _ = _engine(3, 5, 8)
    with pytest.raises(ValueError) as e:
        eng.set_conservative(0.5)
    assert str(e.value) == _mixture.REM_CQL_REFUSED and eng.cql_alpha == 0.0
    eng.set_conservative(0.0)  # (off stays allowed)
