"""The dense tail stage by stage at the widths, batch sizes and depths that select other kernels than the headline networks do
(tests/helpers/dense_routes.py: the cases and the route each Dense layer takes, pinned on the host by tests/test_dense_routes_host.py).

Same method as tests/test_gpu_bf16_model.py and tests/test_gpu_conv_routes.py: one run per (case, precision) -- loss_on_batch,
forward-only calls on 1, 2, 2B - 1 and 2B rows, best_actions, learn_on_batch with grad_out -- then every stored tensor of every Dense
layer against the float64 model of the one stage that produced it, on the run's own operands (S8 hi / lo halves, the weights'
nearest-even split, the run's own ReLU decisions act > 0), within c 2^-24 S, c from bf16_model.chain_depth of the route taken
(dense_routes.routes: the slabs dense_post_kernel or the head chain sums, the slabs of a weight gradient).  Negative control wherever a
pass count enters: the same operands at the other pass count must be 4x further away in the 2-norm and, where c <= 64, break the
bound on at least half of the elements.  No element is left out of any comparison.  fc-ladder also runs grad_on_batch (no update, so
no head chain): the generic head path -- td_kernel, the head's MFMA data gradient, ln_bwd_small<32> at Dense_6 = 72 -- is held to the
same models, gradient leaves included.

New here: the LayerNorm scale / bias leaves of g, against sum over rows of dy xhat and of dy (bf16_model.ln_param_grads: dy = mask da
with da the model of the stage above, xhat from the layer's own z), within E_da carried through, the fp32 error of xhat, and a plain
fp32 chain of (rows summed into a partial row + partial rows) additions from the route.  No new constant.  In the cnn case the three
convolutions' LayerNorm leaves are held the same way (partial rows of the image data gradients and of DenseDgradLN, summed by
reduce_rows_kernel); their kernel leaves and forward tensors are tests/test_gpu_conv_routes.py's (the same 40x40x2 torso).

fc-headonly (feats = ()): the engine builds and runs a network that is the head alone on the caller's observations; it has no hidden
layer, so only the head's checks apply.

Measured on the MI355X over all runs (max |d| / bound; the table per run is in docs/NOTEBOOK.md, "Dense tail by stage"): z 0.13
(2.3 x 2^-24 S), q 0.10, online activations 0.61 with a LayerNorm and 0.98 without one (relu(z) is exact: the S8 storage against its
worst case 2^-17 |a| is all that is left), next-state activations 0.78, forward-only rows 0.78 (act) and 0.10 (q), q_values 0.05,
targets 0.06, the da region 0.14, dz 0.76 under the head chain, 0.65 behind ln_bwd_wide, 0.38 / 0.48 / 0.45 / 0.32 behind
ln_bwd_small<64 / 32 / 16 / 8>, 0.29 where a data gradient fused it; kernel leaves 0.20 (4.0 x 2^-24 S), bias leaves 0.85, LayerNorm
scale / bias leaves 0.017 / 0.073 (their bound carries the worst case of E_da of every row to the sum), Adam p / m / v 1.0 / 0.48 /
0.65.  Negative control, smallest share of elements the other pass count puts outside the bound: z 96 %, q 75 % (91 % where c <= 64),
q_values 89 %, targets 39 %, the da region 91 %, dz 83 % where it is asserted elementwise (26 % at C = 4096), next-state activations
31 %, kernel leaves 31 %, LayerNorm leaves 47 %; the 2-norm control holds everywhere.  The file takes 5 s on the device, the largest
run 0.6 s.

Mutations each of which fails these tests (a scratch copy, one GPU run each; arithmetic only, none moves an address):
ln_bwd_small_kernel<64> starting its shuffle reductions one level short (6 tests: test_backward_dz_against_the_model and
test_gradient_leaves_against_the_model of fc-ladder and fc-rows); ln_bwd_wide_kernel looping over 15 columns (2: the same two tests
of fc-4096); dense_post_kernel skipping the slab tail (35: test_forward_z_and_q_against_the_model,
test_hidden_activations_of_both_halves and test_forward_only_rows_at_every_row_count of every run, test_head_losses_and_priorities of
fc-ladder and fc-headonly); DenseDgradLN dropping its last (ragged) K step at K = 104 (4: dz and gradient leaves of cnn-2dense);
ln_bwd_small_kernel adding dgamma without the xhat factor (8: test_gradient_leaves_against_the_model of every run with a LayerNorm
behind a small kernel); Adam's LayerNorm entries taking the partial rows one row short (9: the same test of every run with a
LayerNorm).

Found by fc-headonly, and fixed: dense_wgrad ran the first-layer kernel, which reads dz as an S8 tensor, on a head that reads the
caller's observations, whose dz is the fp32 dL/dq -- Dense_0/kernel was 2.7e21 where the model has 0 (docs/NOTEBOOK.md)."""
import time

import numpy as np
import pytest
import torch

from tests.gpu_helpers import adam_bounds, make_frame_batch, perturbed_params
from tests.helpers import bf16_model as M
from tests.helpers import conv_routes as R
from tests.helpers import dense_routes as D

pytestmark = pytest.mark.gpu

RUNS = [pytest.param(c, p, id=f"{c}-{p}") for c, p in D.RUNS]
GAMMA = 0.99
BATCH_SEED = 29
TIGHT = 64  # c up to which the other pass count must break the bound elementwise (2^-18 S: far below the lo products it adds or drops)

_CACHE = {}  # one run per (case, precision), kept while this module runs: every test reads the same step


@pytest.fixture(scope="module", autouse=True)
def _release_runs():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _regions(eng, hidden, extra=()):
    out = {}
    for L in hidden:
        for r in ("act", "z", "dz", "part"):
            out[f"{r}/{L['name']}"] = eng.region(f"{r}/{L['name']}").clone()
    for name in ("dout", "q") + tuple(extra):
        out[name] = eng.region(name).clone()
    return out


def _run(case, precision):
    key = (case, precision)
    if key in _CACHE:
        return _CACHE[key]
    from slimdqn._engine import QNetEngine

    t0 = time.time()
    cfg = D.CASES[case]
    obs, feats, K, A, B, arch, ln = cfg["obs"], cfg["feats"], cfg["K"], cfg["A"], cfg["B"], cfg["arch"], cfg["ln"]
    params = perturbed_params(17, obs, list(feats), arch, (1 + K) * A, ln)
    eng = QNetEngine(obs, A, 1 + K, list(feats), arch, ln, B, gamma_n=GAMMA, learning_rate=1e-3, adam_eps=1.5e-4, precision=precision)
    eng.import_flax(params)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    hidden, dense = D.dense_layers(cfg)
    if arch == "cnn":
        h, w, stack = obs
        frames, ids, action, reward, terminal, ref = make_frame_batch(B, A, seed=BATCH_SEED, h=h, w=w, stack=stack, n_frames=B + 8)
        fr = d(frames)
        batch = eng.make_batch(frames=fr, frame_stride=h * w, frame_ids=d(ids), action=d(action), reward=d(reward), terminal=d(terminal))
        x = np.concatenate([ref.state, ref.next_state])  # [2B][h][w][stack] uint8
        both = d(np.concatenate([ids[:, :stack], ids[:, stack:]]))
        fwd = lambda n: eng.forward(frames=fr, frame_stride=h * w, frame_ids=both[:n].contiguous(), n_rows=n)
        best = lambda heads: eng.best_actions(frames=fr, frame_stride=h * w, frame_ids=both, idx_networks=heads)
    else:
        rng = np.random.default_rng(BATCH_SEED)
        st, nx = (rng.normal(size=(B, obs[0])).astype(np.float32) for _ in range(2))
        action, reward = rng.integers(0, A, B).astype(np.int32), rng.normal(size=B).astype(np.float32)
        terminal = (rng.random(B) < 0.3).astype(np.uint8)
        batch = eng.make_batch(state=d(st), next_state=d(nx), action=d(action), reward=d(reward), terminal=d(terminal))
        x = np.concatenate([st, nx])
        xd = d(x)
        fwd = lambda n: eng.forward(obs=xd[:n].contiguous(), n_rows=n)
        best = lambda heads: eng.best_actions(obs=xd, idx_networks=heads)
    run = dict(case=case, cfg=cfg, precision=precision, hidden=hidden, dense=dense, x=torch.from_numpy(x).cuda(), action=action, reward=reward,
               terminal=terminal, nha=(1 + K) * A, nha_p=dense[-1]["cp"], routes={r["name"]: r for r in D.routes(cfg, precision)})
    # loss_on_batch: every layer through dense_post_kernel, td_kernel on the q rows
    eng.loss_on_batch(batch)
    torch.cuda.synchronize()
    run["p0"] = eng.export_flax()
    run["p0_internal"] = eng.params.clone()
    run["loss"] = dict(_regions(eng, hidden), qv=eng.q_values.clone(), tg=eng.targets.clone(), losses=eng.losses.clone())
    # the forward-only path on the first n of the same 2B rows
    run["fwd"] = {}
    for n in sorted({1, 2, 2 * B - 1, 2 * B}):
        q = fwd(n).clone()
        run["fwd"][n] = dict({f"act/{L['name']}": eng.region(f"act/{L['name']}")[: n * L["npix"] * L["cp"]].clone() for L in hidden}, q=q)
    heads = (torch.arange(2 * B, dtype=torch.int32, device="cuda") % K).contiguous()
    run["heads"], run["best"] = heads, best(heads).clone()
    nan = lambda: [t.fill_(float("nan")) for t in (eng.q_values, eng.targets, eng.priorities)]  # whatever a call leaves unwritten shows
    if case == "fc-ladder":  # the gradient-only pass: the generic head path at the same widths
        nan()
        g2 = torch.zeros_like(eng.params)
        losses = eng.grad_on_batch(batch, g2)
        torch.cuda.synchronize()
        run["grad"] = dict(_regions(eng, hidden, ("da",)), qv=eng.q_values.clone(), tg=eng.targets.clone(), losses=losses.clone(),
                           g=eng.internal_to_flax_grads(g2), routes={r["name"]: r for r in D.routes(cfg, precision, update=False)})
        assert torch.equal(eng.params, run["p0_internal"]) and int(eng.adam_count.item()) == 0, "a gradient-only pass moved the parameters"
    nan()
    g = torch.zeros_like(eng.params)
    losses = eng.learn_on_batch(batch, grad_out=g)
    torch.cuda.synchronize()
    run["learn"] = dict(_regions(eng, hidden, ("da",) if hidden else ()), qv=eng.q_values.clone(), tg=eng.targets.clone(), losses=losses.clone(),
                        prio=eng.priorities.clone(), g=eng.internal_to_flax_grads(g), routes=run["routes"])
    run.update(g_internal=g.clone(), adam_m=eng.adam_m.clone(), adam_v=eng.adam_v.clone(), adam_count=int(eng.adam_count.item()),
               mirror=eng.region("wsplit").clone().view(torch.int32), params_after=eng.params.clone())
    del eng
    run["seconds"] = time.time() - t0
    _CACHE[key] = run
    return run


def _views(run):
    """(label, tensors) of the learn step and, where it ran, of the gradient-only pass; each holds the routes it took"""
    return [("learn", run["learn"])] + ([("grad_on_batch", run["grad"])] if "grad" in run else [])


def _passes(run):
    return (1, 3) if run["precision"] == "bf16" else (3, 1)


def _w(run, mod):
    return M.split(torch.from_numpy(np.asarray(run["p0"][mod]["kernel"])).cuda())


def _vec(run, mod, leaf):
    return torch.from_numpy(np.asarray(run["p0"][mod][leaf], np.float64)).cuda()


def _leaf(T, mod, leaf):
    return torch.from_numpy(np.asarray(T["g"][mod][leaf], np.float64)).cuda()


def _planes(T, key, L, rows):
    """own S8 tensor `key` of hidden layer L, rows [0, rows), true channels: planes [rows][npix][c]"""
    hi, lo = M.s8_planes(T[key], rows, L["npix"] * L["cp"])
    f = lambda t: t.reshape(rows, L["npix"], L["cp"])[:, :, : L["c"]]
    return f(hi), f(lo)


def _z(T, L, rows):
    return T[f"z/{L['name']}"][: rows * L["npix"] * L["cp"]].reshape(rows, L["npix"], L["cp"])[:, :, : L["c"]].double()


def _dense_of(run, i):
    """the dense_routes layer dict of plan index i (the head: i = len(hidden))"""
    return next(L for L in run["dense"] if L["i"] == i)


def _input_planes(run, T, i, rows):
    """planes [rows][in] of the input of Dense layer i (plan index; the head: len(hidden)) over rows [0, rows): the caller's fp32
    observations, split as the kernel splits them, or the own act of the layer below from `T`"""
    if i == 0:
        return M.split(run["x"][:rows])
    below = run["hidden"][i - 1]
    return tuple(p.reshape(rows, -1) for p in _planes(T, f"act/{below['name']}", below, rows))


def _forward_model(run, T, i, rows, passes):
    """(z, S, c) of Dense layer i over rows [0, rows) on its input in `T`: contraction at `passes` plus bias, c from the slabs its route sums"""
    L = _dense_of(run, i)
    b, w = _vec(run, L["name"], "bias"), _w(run, L["name"])
    v, S = M.dense(passes, _input_planes(run, T, i, rows), w)
    return v + b, S + b.abs(), M.chain_depth(L["in_p"], slabs=run["routes"][L["name"]]["fwd"]["slabs"])


def _ln(run, L):
    return (_vec(run, L["ln"], "scale"), _vec(run, L["ln"], "bias")) if L["ln"] else (None, None)


def _report(run, rows):
    print(f"\n  [{run['case']}-{run['precision']}: one run {run['seconds']:.2f} s]")
    for r in rows:
        print("  " + r)


def _dense_hidden(run):
    return [(i, L) for i, L in enumerate(run["hidden"]) if L["kind"] == 1]


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("case,precision", RUNS)
def test_the_run_and_its_routes(case, precision):
    """Every call of the run is finite, the counter advanced once, and (cnn) every convolution takes the image-resident data gradient,
    so that the `da` region still holds what the lowest Dense layer's data gradient left.  Prints the route of every Dense layer."""
    run = _run(case, precision)
    for label, T in [("loss_on_batch", run["loss"])] + _views(run):
        for k in ("losses", "qv", "tg"):
            assert bool(torch.isfinite(T[k]).all()), f"{label}: {k}"
    assert bool(torch.isfinite(run["learn"]["prio"]).all()) and run["adam_count"] == 1
    if run["cfg"]["arch"] == "cnn":
        assert all(r["dgrad"] is None or r["dgrad"]["kernel"] == "dgimg" for r in R.routes(run["cfg"], precision))
    _report(run, [f"{n}: " + " | ".join(D.fmt(r)) for n, r in run["routes"].items()])


def test_the_engine_refuses_a_width_no_kernel_runs():
    """A hidden Dense of 4104 columns or a head row of 5464 is refused when the engine is built, with the plan's message: no launch
    has been made, nothing has moved."""
    from slimdqn._engine import QNetEngine

    for kw in (dict(features=[8, 4104], n_actions=2, n_heads=2), dict(features=[8], n_actions=683, n_heads=8)):
        with pytest.raises(Exception, match="bad dense width"):
            QNetEngine((8,), kw["n_actions"], kw["n_heads"], kw["features"], "fc", True, 3)
    QNetEngine((8,), 2, 2, [8, 4096], "fc", True, 3)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case,precision", RUNS)
def test_forward_z_and_q_against_the_model(case, precision):
    """z/<layer> (pre-LayerNorm fp32, online rows) of every hidden Dense layer -- of the learn step, where the head chain finishes the
    last one, of loss_on_batch, where dense_post_kernel finishes every one, and of the gradient-only pass -- against its contraction on
    the layer below's own act and the weights' nearest-even split, plus bias; the 2B q rows of loss_on_batch against the head row on
    own act.  Control: the other pass count."""
    run = _run(case, precision)
    own, other = _passes(run)
    B = run["cfg"]["B"]
    out = []
    for label, T in [("loss_on_batch", run["loss"])] + _views(run):
        for i, L in _dense_hidden(run):
            want, S, c = _forward_model(run, T, i, B, own)
            alt, _, _ = _forward_model(run, T, i, B, other)
            got = _z(T, L, B).reshape(want.shape)
            used, ratio, frac = M.check(got, want, M.bound(S, c), S, alt, elementwise_control=c <= TIGHT, label=f"{label}: z/{L['name']}")
            out.append(f"{label}: z/{L['name']}: c = {c}, max |d| / bound = {used:.3f}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
    T = run["loss"]
    n = len(run["hidden"])
    want, S, c = _forward_model(run, T, n, 2 * B, own)
    alt, _, _ = _forward_model(run, T, n, 2 * B, other)
    got = T["q"][: 2 * B * run["nha_p"]].reshape(2 * B, run["nha_p"])
    assert not bool(got[:, run["nha"]:].any()), "padded q columns are not zero"
    used, ratio, frac = M.check(got[:, : run["nha"]].double(), want, M.bound(S, c), S, alt, elementwise_control=c <= TIGHT, label="loss_on_batch: q")
    out.append(f"loss_on_batch: q: c = {c}, max |d| / bound = {used:.3f}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
    _report(run, out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_hidden_activations_of_both_halves(case, precision):
    """act/<layer> of every hidden Dense layer, rows [0, 2B): the online half through the float64 LayerNorm / ReLU of the layer's own
    z, the next-state half -- whose pre-activations are not stored -- through the model of the contraction on the layer below's own
    next-state act, carried through the LayerNorm (bf16_model.ln_relu_fwd).  Control on the next-state half: the other pass count, in
    the 2-norm."""
    run = _run(case, precision)
    own, other = _passes(run)
    B = run["cfg"]["B"]
    out = []
    for label, T in [("loss_on_batch", run["loss"])] + _views(run):
        for i, L in _dense_hidden(run):
            gamma, beta = _ln(run, L)
            hi, lo = _planes(T, f"act/{L['name']}", L, 2 * B)
            got = (hi + lo).reshape(2 * B, L["c"])
            z = _z(T, L, B).reshape(B, L["c"])
            a, E = M.ln_relu_fwd(z, gamma, beta, torch.zeros_like(z), has_ln=L["ln"] is not None)
            used_on, _, _ = M.check(got[:B], a, E, label=f"{label}: act/{L['name']} online")
            zm = []
            for p in (own, other):
                v, S, c = _forward_model(run, T, i, 2 * B, p)
                zm.append((v[B:], M.bound(S, c)[B:]))
            a, E = M.ln_relu_fwd(zm[0][0], gamma, beta, zm[0][1], has_ln=L["ln"] is not None)
            alt, _ = M.ln_relu_fwd(zm[1][0], gamma, beta, zm[1][1], has_ln=L["ln"] is not None)
            used, _, frac = M.check(got[B:], a, E, None, alt, elementwise_control=False, label=f"{label}: act/{L['name']} next-state")
            out.append(f"{label}: act/{L['name']}: online max |d| / bound = {used_on:.3f}, next-state {used:.3f}, other passes outside: {frac:.0%}")
    _report(run, out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_forward_only_rows_at_every_row_count(case, precision):
    """eng.forward(n_rows = n), n in {1, 2, 2B - 1, 2B}: act of every hidden Dense layer and the q rows, each against the model of
    its contraction on the same call's own act of the layer below, through the LayerNorm.  The split-K factor of every Dense GEMM is
    the plan's, not a function of n_rows, every kernel of these networks works per row (cnn: one tile per image), and the slabs are
    summed in slab order: row r has the same bits at every n.  best_actions on the 2B rows is the argmax of head 1 + idx of those q
    rows, which hold no tie."""
    run = _run(case, precision)
    own, other = _passes(run)
    cfg = run["cfg"]
    K, A, B = cfg["K"], cfg["A"], cfg["B"]
    full = run["fwd"][2 * B]["q"]
    assert bool(torch.isfinite(full).all())
    out = []
    for n, T in run["fwd"].items():
        assert T["q"].shape == (n, run["nha"])
        worst = 0.0
        for i, L in _dense_hidden(run):
            gamma, beta = _ln(run, L)
            v, S, c = _forward_model(run, T, i, n, own)
            a, E = M.ln_relu_fwd(v, gamma, beta, M.bound(S, c), has_ln=L["ln"] is not None)
            alt = None
            if n == 2 * B:
                v2, S2, _ = _forward_model(run, T, i, n, other)
                alt, _ = M.ln_relu_fwd(v2, gamma, beta, M.bound(S2, c), has_ln=L["ln"] is not None)
            hi, lo = _planes(T, f"act/{L['name']}", L, n)
            used, _, _ = M.check((hi + lo).reshape(n, L["c"]), a, E, None, alt, elementwise_control=False, label=f"n_rows = {n}: act/{L['name']}")
            worst = max(worst, used)
        v, S, c = _forward_model(run, T, len(run["hidden"]), n, own)
        alt = _forward_model(run, T, len(run["hidden"]), n, other)[0] if n == 2 * B else None
        usedq, _, frac = M.check(T["q"].double(), v, M.bound(S, c), S, alt, elementwise_control=c <= TIGHT, label=f"n_rows = {n}: q")
        same = torch.equal(T["q"].view(torch.int32), full[:n].view(torch.int32))
        out.append(f"n_rows = {n}: act max |d| / bound = {worst:.3f}, q {usedq:.3f}" + (f", other passes outside: {frac:.0%}" if alt is not None else "")
                   + f", bits of the 2B-row forward: {same}")
        assert same, f"n_rows = {n}: rows differ from the 2B-row forward's"
    _report(run, out)
    rows = torch.arange(2 * B, device="cuda")
    qh = full.reshape(2 * B, 1 + K, A)[rows, 1 + run["heads"].long()]
    top = torch.sort(qh, descending=True).values
    assert bool((top[:, 0] > top[:, 1]).all()), "a tie between the two largest q values: pick another seed"
    assert torch.equal(run["best"].long(), qh.argmax(-1))


def _head(run, T, passes):
    """model q of all 2B rows at `passes` on the act in `T`, and the online q of the taken actions / the Bellman targets with bounds"""
    cfg = run["cfg"]
    K, A, B = cfg["K"], cfg["A"], cfg["B"]
    n = len(run["hidden"])
    q, S, c = _forward_model(run, T, n, 2 * B, passes)
    head = run["dense"][-1]
    if T["routes"][head["name"]]["head"]["kernel"] == "chain":
        c = M.chain_depth(head["in_p"], slabs=8)  # head chain: K steps dealt over 8 waves, then the 8 wave partials
    E = M.bound(S, c)
    a = torch.from_numpy(run["action"].astype(np.int64)).cuda()
    cols = (torch.arange(K, device=a.device)[None, :] + 1) * A + a[:, None]
    qv, Eqv = q[:B].gather(1, cols), E[:B].gather(1, cols)
    r = torch.from_numpy(run["reward"].astype(np.float64)).cuda()
    t = torch.from_numpy(run["terminal"].astype(np.float64)).cuda()
    tg = M.bellman_targets(q[B:], r, t, GAMMA, K, A)
    # max is 1-Lipschitz in the max norm: where the two largest are within the bound either is accepted
    Eq = E[B:, : K * A].reshape(B, K, A).max(-1).values
    Etg = GAMMA * Eq + M.ROUNDING * 3 * M.U * (r.abs()[:, None] + GAMMA * tg.abs()) + M.FLOOR
    return qv, Eqv, S[:B].gather(1, cols), tg, Etg, cols, r, t


@pytest.mark.parametrize("case,precision", RUNS)
def test_head_losses_and_priorities(case, precision):
    """q_values and targets of the learn step (head chain, or td_kernel on the q rows of the generic path) and of the gradient-only
    pass against the head model on own act, the Bellman target over the model's next-state q; dL/dq ("dout"), the per-head losses and
    the priorities in float64 from the call's own q_values / targets; loss_on_batch's q_values / targets from the q rows it wrote."""
    run = _run(case, precision)
    own, other = _passes(run)
    K, A, B = run["cfg"]["K"], run["cfg"]["A"], run["cfg"]["B"]
    out = []
    for label, T in _views(run):
        qv, Eqv, Sqv, tg, Etg, cols, r, t = _head(run, T, own)
        aqv, _, _, atg, _, _, _, _ = _head(run, T, other)
        used, ratio, frac = M.check(T["qv"].double(), qv, Eqv, Sqv, aqv, elementwise_control=False, label=f"{label}: q_values")
        out.append(f"{label}: q_values: max |d| / bound = {used:.3f}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside: {frac:.0%}")
        used, _, frac = M.check(T["tg"].double(), tg, Etg, None, atg, elementwise_control=False, label=f"{label}: targets")
        out.append(f"{label}: targets: max |d| / bound = {used:.3f}, other passes outside: {frac:.0%}")
        # float64 from the call's own q_values / targets (no pass count enters: no control)
        td = T["qv"].double() - T["tg"].double()
        want = torch.zeros(B, run["nha_p"], dtype=torch.float64, device=td.device)
        want.scatter_(1, cols, 2.0 * td / B)
        got = T["dout"][: B * run["nha_p"]].reshape(B, -1).double()
        M.check(got, want, M.ROUNDING * 3 * M.U * want.abs() + M.FLOOR, label=f"{label}: dout")
        lw = (td * td).mean(0)
        M.check(T["losses"].double()[:K], lw, M.bound(lw, M.chain_depth(0, slabs=B, epilogue=3)), label=f"{label}: losses")
        if "prio" in T:
            arg = (td * td).sum(1) / K + 1e-10
            pw = arg.sqrt()
            M.check(T["prio"].double(), pw, M.ROUNDING * (K + 4) * M.U * arg / (2 * pw) + 1e-300, label=f"{label}: priorities")
        if T["routes"][run["dense"][-1]["name"]]["head"]["kernel"] == "generic":  # td_kernel reads the q rows the forward wrote
            q = T["q"][: 2 * B * run["nha_p"]].reshape(2 * B, -1)
            assert torch.equal(T["qv"], q[:B].gather(1, cols)), f"{label}: q_values are not the q rows"
    # loss_on_batch reads its q_values off the q rows it wrote (checked in test_forward_z_and_q_against_the_model)
    T = run["loss"]
    q = T["q"][: 2 * B * run["nha_p"]].reshape(2 * B, -1)
    assert torch.equal(T["qv"], q[:B].gather(1, cols))
    ltg = M.bellman_targets(q[B:].double(), r, t, GAMMA, K, A)
    M.check(T["tg"].double(), ltg, M.ROUNDING * 3 * M.U * (r.abs()[:, None] + ltg.abs()) + M.FLOOR, label="loss_on_batch targets")
    _report(run, out)


def _da_model(run, T, i, passes):
    """(da, E_da, pass count enters) of hidden layer i, [B][npix][c]: the model of the data gradient the layer above ran.
    Under the head chain: da = dL/dq W_head, an fp32 AXPY on the fp32 master weights (head_chain.h), a plain fp32 sum with no pass
    count.  Under the generic head path: the head's MFMA data gradient of the fp32 dL/dq rows, split by the kernel.  Under a Dense
    layer: bf16_model.dense on its own dz planes and transposed weight split (dense_dgrad, or DenseDgradLN under the first Dense of a
    cnn).  Under a convolution: the transposed SAME convolution of its own dz."""
    cfg, hidden = run["cfg"], run["hidden"]
    B = cfg["B"]
    L, up = hidden[i], i + 1
    shape = (B, L["npix"], L["c"])
    if up == len(hidden):
        head = run["dense"][-1]
        dq = T["dout"][: B * run["nha_p"]].reshape(B, -1)[:, : run["nha"]]
        if T["routes"][head["name"]]["head"]["kernel"] == "chain":
            W = _vec(run, head["name"], "kernel")
            da, S = dq.double() @ W.T, dq.double().abs() @ W.abs().T
            return da.reshape(shape), M.bound(S, M.chain_depth(0, slabs=cfg["K"] + 1)).reshape(shape), False
        da, S = M.dense(passes, M.split(dq), tuple(p.T for p in _w(run, head["name"])))
        return da.reshape(shape), M.bound(S, M.chain_depth(head["cp"], epilogue=3)).reshape(shape), True
    U_ = hidden[up]
    dz = _planes(T, f"dz/{U_['name']}", U_, B)
    if U_["kind"] == 0:
        da, S = M.conv_dgrad(passes, dz, _w(run, U_["name"]), (L["h"], L["w"]), U_["s"])
        # every tap of every output channel at most (a class-split kernel sums ceil(k / s)^2 of them), then the epilogue
        return da.reshape(shape), M.bound(S, M.chain_depth(U_["k"] ** 2 * U_["cp"], epilogue=4)).reshape(shape), True
    da, S = M.dense(passes, tuple(p.reshape(B, -1) for p in dz), tuple(p.T for p in _w(run, U_["name"])))
    return da.reshape(shape), M.bound(S, M.chain_depth(U_["cp"], epilogue=3)).reshape(shape), True


def _mask(T, L, B):
    hi, lo = _planes(T, f"act/{L['name']}", L, B)
    return ((hi + lo) > 0).double()


def _checked_layers(run):
    """hidden layers whose backward this file holds: every Dense, and in a cnn the convolutions below them (DenseDgradLN writes
    Conv_2's dz; the LayerNorm leaves of all three pass through partial rows)"""
    return list(range(len(run["hidden"]) - 1, -1, -1))


@pytest.mark.parametrize("case,precision", RUNS)
def test_backward_dz_against_the_model(case, precision):
    """dz/<layer> of every hidden layer: da modelled from the layer above (_da_model), through the float64 LayerNorm / ReLU backward
    on the layer's own z and ReLU decisions (bf16_model.ln_relu_bwd).  The `da` region survives for the lowest Dense layer -- nothing
    below it writes da -- and is held against that same model directly.  Control: the other pass count, where one enters."""
    run = _run(case, precision)
    own, other = _passes(run)
    hidden, B = run["hidden"], run["cfg"]["B"]
    out = []
    for label, T in _views(run):
        for i in _checked_layers(run):
            L = hidden[i]
            da, E_da, has_passes = _da_model(run, T, i, own)
            gamma = _vec(run, L["ln"], "scale") if L["ln"] else None
            z, mask = _z(T, L, B), _mask(T, L, B)
            want, E = M.ln_relu_bwd(z, gamma, mask, da, E_da, has_ln=L["ln"] is not None)
            alt = None
            if has_passes:
                da2, E2, _ = _da_model(run, T, i, other)
                alt = M.ln_relu_bwd(z, gamma, mask, da2, E2, has_ln=L["ln"] is not None)[0]
            hi, lo = _planes(T, f"dz/{L['name']}", L, B)
            # the LayerNorm backward's own arithmetic enters the bound with c_ln = ROUNDING (C + 8) on terms of dz's size: above
            # 8 TIGHT (C > 248) that is no longer far below what the pass count changes, and the control holds in the 2-norm only
            tight = L["ln"] is None or M.ROUNDING * (L["c"] + 8) <= 8 * TIGHT
            used, _, frac = M.check(hi + lo, want, E, None, alt, elementwise_control=tight, label=f"{label}: dz/{L['name']}")
            out.append(f"{label}: dz/{L['name']} [{_ln_route_text(run, T, i)}]: max |d| / bound = {used:.3f}"
                       + (f", other passes outside: {frac:.0%}" if alt is not None else " (head chain AXPY: no pass count)"))
        lowest = [i for i, L in enumerate(hidden) if L["kind"] == 1][:1]
        if lowest and lowest[0] + 1 <= len(hidden) and _da_model(run, T, lowest[0], own)[2]:
            i = lowest[0]
            L = hidden[i]
            da, E_da, _ = _da_model(run, T, i, own)
            alt, _, _ = _da_model(run, T, i, other)
            got = T["da"][: B * L["cp"]].reshape(B, 1, L["cp"])
            assert not bool(got[:, :, L["c"]:].any()), f"{label}: padded da columns are not zero"
            used, _, frac = M.check(got[:, :, : L["c"]].double(), da, E_da, None, alt, label=f"{label}: da under {L['name']}")
            out.append(f"{label}: da region (for {L['name']}): max |d| / bound = {used:.3f}, other passes outside: {frac:.0%}")
    _report(run, out)


def _ln_route(run, T, i):
    """dict(kernel, rows, parts, by) of the LayerNorm backward of hidden layer i: dense_routes for a Dense; a convolution's partial rows
    come from the kernel above it -- DenseDgradLN (dense_routes.conv2_ln), or the image data gradient of the next convolution, one row
    per 128-pixel tile (conv_routes.plan_fields dgi_tiles), both summed by reduce_rows_kernel"""
    L = run["hidden"][i]
    if L["kind"] == 1:
        return T["routes"][L["name"]]["ln"]
    if run["hidden"][i + 1]["kind"] == 1:
        return D.conv2_ln(run["cfg"])
    B = run["cfg"]["B"]
    return dict(kernel="fused", rows=128, parts=B * R.plan_fields(run["cfg"], B)[i + 1]["dgi_tiles"], by="reduce_rows")


def _ln_route_text(run, T, i):
    n = _ln_route(run, T, i)
    return (f"small<{n['tpr']}>" if n["kernel"] == "small" else n["kernel"]) + f" rows={n['rows']} parts={n['parts']}"


@pytest.mark.parametrize("case,precision", RUNS)
def test_gradient_leaves_against_the_model(case, precision):
    """Every Dense kernel leaf of g against the sum over the online rows of own input x own dz at the pass count, within the chain of
    its route (fused into Adam: one accumulator over B; slabs: their K steps and their sum); every bias against the sum of own dz;
    every LayerNorm scale / bias leaf against sum dy xhat / sum dy (bf16_model.ln_param_grads), the chain from the route that wrote
    and summed its partial rows.  Control (2-norm): the other pass count, where one enters."""
    run = _run(case, precision)
    own, other = _passes(run)
    hidden, B = run["hidden"], run["cfg"]["B"]
    out = []
    for label, T in _views(run):
        for L in run["dense"]:
            mod, route = L["name"], T["routes"][L["name"]]["wgrad"]
            if L["head"]:
                dz = M.split(T["dout"][: B * run["nha_p"]].reshape(B, -1)[:, : run["nha"]])  # fp32 dL/dq, split by the kernel
            else:
                dz = tuple(p.reshape(B, -1) for p in _planes(T, f"dz/{mod}", hidden[L["i"]], B))
            xin = _input_planes(run, T, L["i"], B)
            c = M.chain_depth(B, slabs=route["slabs"])
            want, S = M.wgrad(own, xin, dz)
            alt, _ = M.wgrad(other, xin, dz)
            used, ratio, frac = M.check(_leaf(T, mod, "kernel"), want, M.bound(S, c), S, alt, elementwise_control=False, label=f"{label}: {mod}/kernel")
            out.append(f"{label}: {mod}/kernel [{D.fmt(T['routes'][mod])[3]}]: c = {c}, max |d| / bound = {used:.3f}, max |d| / 2^-24 S = {ratio:.2f}, "
                       f"other passes outside: {frac:.0%}")
            # bias: a plain fp32 sum of dz (hi + lo of the S8 value: within S8_STORE of the fp32 one); no pass count, no control
            dzv = dz[0] + dz[1]
            bw, bS = dzv.sum(0), dzv.abs().sum(0)
            usedb, _, _ = M.check(_leaf(T, mod, "bias"), bw, M.bound(bS, M.chain_depth(0, slabs=B, epilogue=4)) + M.S8_STORE * bS, label=f"{label}: {mod}/bias")
            out.append(f"{label}: {mod}/bias: max |d| / bound = {usedb:.3f}")
        for i in _checked_layers(run):
            L = hidden[i]
            if not L["ln"]:
                continue
            n = _ln_route(run, T, i)
            z, mask = _z(T, L, B), _mask(T, L, B)
            da, E_da, has_passes = _da_model(run, T, i, own)
            dg, Eg, db, Eb = M.ln_param_grads(z, mask, da, E_da, n["rows"] + n["parts"])
            ag = ab = None
            if has_passes:
                da2, E2, _ = _da_model(run, T, i, other)
                ag, _, ab, _ = M.ln_param_grads(z, mask, da2, E2, n["rows"] + n["parts"])
            ug, _, fg = M.check(_leaf(T, L["ln"], "scale"), dg, Eg, None, ag, elementwise_control=False, label=f"{label}: {L['ln']}/scale ({L['name']})")
            ub, _, fb = M.check(_leaf(T, L["ln"], "bias"), db, Eb, None, ab, elementwise_control=False, label=f"{label}: {L['ln']}/bias ({L['name']})")
            out.append(f"{label}: {L['ln']} of {L['name']} [{_ln_route_text(run, T, i)} by {n['by']}]: scale max |d| / bound = {ug:.3f}, bias {ub:.3f}"
                       + (f", other passes outside: {fg:.0%} / {fb:.0%}" if has_passes else " (head chain AXPY: no pass count)"))
    _report(run, out)


@pytest.mark.parametrize("case,precision", RUNS)
def test_splits_padding_and_mirror(case, precision):
    """Every stored act / dz element of every Dense layer is a nearest-even split (|lo| <= half an ulp of hi); columns [C, Cp) of act,
    z and dz are exactly 0, and so are those of the partial rows its route wrote -- the optimizer never sees padding move; after
    the step the weight mirror equals a fresh nearest-even split of the fp32 parameters, bit for bit."""
    run = _run(case, precision)
    B = run["cfg"]["B"]
    for label, T in [("loss_on_batch", run["loss"])] + _views(run):
        for i, L in _dense_hidden(run):
            for r, rows in (("act", 2 * B), ("dz", B)):
                if r == "dz" and label == "loss_on_batch":
                    continue
                hi, lo = M.s8_planes(T[f"{r}/{L['name']}"], rows, L["cp"])
                n = int(M.s8_malformed(hi, lo).sum())
                assert n == 0, f"{label}: {r}/{L['name']}: {n} elements are not a nearest-even split"
                assert not bool(torch.stack([hi, lo])[..., L["c"]:].any()), f"{label}: {r}/{L['name']}: padded columns are not zero"
            z = T[f"z/{L['name']}"][: B * L["cp"]].reshape(B, L["cp"])[:, L["c"]:]
            assert not bool(z.any()), f"{label}: z/{L['name']}: padded columns are not zero"
            if label != "loss_on_batch":
                n = T["routes"][L["name"]]["ln"]
                part = T[f"part/{L['name']}"][: n["parts"] * 3 * L["cp"]].reshape(n["parts"], 3, L["cp"])
                assert bool(torch.isfinite(part).all())
                assert not bool(part[:, :, L["c"]:].any()), f"{label}: part/{L['name']}: padded columns of the {n['parts']} partial rows are not zero"
                if L["c"] < L["cp"]:
                    assert bool(part[:, :, : L["c"]].any()), f"{label}: part/{L['name']}: the partial rows are empty"
    want = M.split_words(run["params_after"])
    bad = (run["mirror"][: want.numel()] != want).nonzero()
    assert bad.numel() == 0, f"{bad.numel()} mirror words differ from a nearest-even split, first at {int(bad[0])}"
    moved = run["params_after"] != run["p0_internal"]  # (padding has a zero gradient: Adam from zero moments leaves it where it was)
    assert not bool((moved & (run["g_internal"] == 0)).any()), "an element with a zero gradient moved"


@pytest.mark.parametrize("case,precision", RUNS)
def test_adam_step_against_float64(case, precision):
    """The learn step's Adam update (first step from zero moments: adam_kernel over slabs and partial rows, and the fused-Adam GEMM
    epilogue, whichever each tensor takes at this size) against float64 Adam applied to the gradient it reported, element by element
    within the float32 rounding that gpu_helpers.adam_bounds derives; the count advances to 1."""
    run = _run(case, precision)
    assert run["adam_count"] == 1
    p0, g = (run[k].cpu().numpy() for k in ("p0_internal", "g_internal"))
    zero = np.zeros_like(p0)
    (p, m, v, _), (ep, em, ev) = adam_bounds(p0, zero, zero, g, 1, 1e-3, 1.5e-4)
    out = []
    for name, got, want, bound in (("m", run["adam_m"], m, em), ("v", run["adam_v"], v, ev), ("p", run["params_after"], p, ep)):
        r = np.abs(got.cpu().numpy().astype(np.float64) - want) / bound
        i = int(np.argmax(r))
        assert r[i] <= 1.0, f"{name}[{i}]: got {float(got[i])!r} want {want[i]!r} bound {bound[i]:.3e} g {g[i]!r}"
        out.append(f"{name}: max |d| / bound = {r[i]:.3f}")
    assert np.count_nonzero(run["params_after"].cpu().numpy() != p0) > 0.5 * np.count_nonzero(g)
    _report(run, out)
