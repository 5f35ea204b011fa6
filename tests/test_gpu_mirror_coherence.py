"""The trusted weight mirror against the parameters behind every writer (slimdqn/_engine.py, "weight-mirror bookkeeping").

Engine level: two engines of one variant and one seed -- T with ``trust_mirror = True``, D the default, which rebuilds in every call --
run the same seeded walk over the op table of tests/helpers/mirror_walk.py (every writer directly followed by every reader:
tests/test_mirror_walk_host.py).  Behind every op: (a) parameters, moments and count are bit-equal between T and D, (b) so is every
output of a reader, (c) whenever T says its mirror is current the mirror's words equal what isdqn_net_refresh_mirror makes of T's
parameters in a scratch workspace, (d) T's flag is what the table predicts from the op history.  The kernels are deterministic: no
tolerance anywhere in this file.

Agent level: iSDQN (plain, soft_shift_tau = 0.25) and DQN (plain, ema_tau = 0.005) with a trusted twin each, on device replays fed by
SyntheticAtariEnv from one seed, through the act graph, the captured update, learn_steps, target updates, recycle_dormant,
reset_parameters, a torch-side write, a learn call on foreign parameters and a change of batch size."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import mirror_walk as mw

pytestmark = pytest.mark.gpu


def _words(t):
    return t.contiguous().view(torch.int32) if t.dtype != torch.int32 else t


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_words(a), _words(b))


# ---------------------------------------------------------------------------------------------------------------- invariant (c)
class MirrorCheck:
    """The words of an engine's weight mirror (workspace region "wsplit", same offsets as the master) against a rebuild from
    ``source`` in a scratch workspace: over the conv and Dense kernel tensors -- the operands the MFMA stages read --, and on engines
    without BatchNorm over the whole region."""

    def __init__(self, eng):
        from slimdqn import _hip

        self._hip = _hip
        self.eng = eng
        off, size = ctypes.c_int64(), ctypes.c_int64()
        _hip.check(eng.lib.isdqn_net_workspace_region(ctypes.byref(eng.cfg), b"wsplit", ctypes.byref(off), ctypes.byref(size)))
        assert off.value % 32 == 0 and size.value >= 4 * eng.n_param_floats
        self.lo, self.n = off.value // 4, eng.n_param_floats
        self.scratch = torch.zeros_like(eng.workspace)
        self.kernels = [(i.name.decode(), int(i.offset), int(i.size)) for i in eng.infos if i.kind in (0, 1)]
        assert self.kernels and all(o + s <= self.n for _, o, s in self.kernels)
        self.whole = not eng.batch_norm

    def words(self, workspace):
        return workspace[self.lo : self.lo + self.n].view(torch.int32)

    def assert_holds(self, source, what):
        eng, _hip = self.eng, self._hip
        _hip.check(eng.lib.isdqn_net_refresh_mirror(ctypes.byref(eng.cfg), _hip.ptr(source), _hip.ptr(self.scratch), _hip.stream_ptr(eng.device)))
        got, want = self.words(eng.workspace), self.words(self.scratch)
        for name, o, s in self.kernels:
            bad = int((got[o : o + s] != want[o : o + s]).sum())
            assert bad == 0, f"{what}: {bad} mirror words of {name} differ from a rebuild"
        if self.whole:
            bad = int((got != want).sum())
            assert bad == 0, f"{what}: {bad} mirror words outside the kernels differ from a rebuild"


# ---------------------------------------------------------------------------------------------------------------- engine level
STATE = ("params", "adam_m", "adam_v", "adam_count", "losses_accum")
NOISY_STATE = ("sigma", "sigma_m", "sigma_v", "noise_count")
N_ROWS = 3


def _engine(variant, trusted):
    from slimdqn._engine import QNetEngine

    v = mw.VARIANTS[variant]
    kw = dict(v["options"])
    if kw.get("noisy"):
        kw["noisy_seed"] = 11
    eng = QNetEngine(v["obs"], mw.N_ACTIONS, 1 + mw.K, v["features"], v["arch"], v["layer_norm"], mw.BATCH, gamma_n=0.99, learning_rate=1e-3,
                     adam_eps=1.5e-4, batch_norm=v["batch_norm"], **kw)
    eng.init_params(5)
    eng.trust_mirror = trusted
    return eng


class Rig:
    """One engine with the buffers its ops take: the engine's own copies, the same bits in T and in D."""

    def __init__(self, variant, trusted):
        self.variant = variant
        self.eng = eng = _engine(variant, trusted)
        v = mw.VARIANTS[variant]
        rng = np.random.default_rng(17)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
        A, B = mw.N_ACTIONS, mw.BATCH
        self.fields = dict(action=dev(rng.integers(0, A, B).astype(np.int32)), reward=dev(rng.normal(size=B).astype(np.float32)),
                           terminal=dev((rng.random(B) < 0.3).astype(np.uint8)))
        if v["arch"] == "fc":
            d = int(np.prod(v["obs"]))
            self.fields.update(state=dev(rng.normal(size=(B, d)).astype(np.float32)), next_state=dev(rng.normal(size=(B, d)).astype(np.float32)))
            obs = dev(rng.normal(size=(N_ROWS, d)).astype(np.float32))
            self.rows, self.row = dict(obs=obs), dict(obs=obs[:1])
        else:
            h, w, stack = v["obs"]
            n_frames = 3 * B + 8
            frames = dev(rng.integers(0, 256, (n_frames, h * w), dtype=np.uint8))
            ids = rng.integers(0, n_frames, (B, 2 * stack)).astype(np.int32)
            ids[rng.random(ids.shape) < 0.1] = -1
            self.fields.update(frames=frames, frame_stride=h * w, frame_ids=dev(ids))
            row_ids = dev(rng.integers(0, n_frames, N_ROWS * stack).astype(np.int32))
            self.rows = dict(frames=frames, frame_stride=h * w, frame_ids=row_ids)
            self.row = dict(frames=frames, frame_stride=h * w, frame_ids=row_ids[:stack])
        self.heads = dev(np.arange(N_ROWS, dtype=np.int32) % mw.K)
        self.foreign, self.target, self.fresh = eng.fresh_params(101), eng.fresh_params(202), eng.fresh_params(303)
        self.tree = eng.export_flax(eng.fresh_params(404))  # (host side: what import_flax loads)
        self.grad = torch.zeros_like(eng.params)
        if eng.noisy:
            eng.resample_noise()  # (under zero noise sigma has no gradient)
        self.check = MirrorCheck(eng)

    def batch(self, mirror_current=False):
        return self.eng.make_batch(mirror_current=mirror_current, **self.fields)

    def state(self):
        names = STATE + (NOISY_STATE if self.eng.noisy else ())
        return {**{n: getattr(self.eng, n) for n in names}, "foreign": self.foreign, "target": self.target}

    def _buffer(self, op):
        return {"own": None, "foreign": self.foreign, "alias": self.eng.params}[op.args.get("target", "own")]

    def _learnt(self):
        eng = self.eng
        return [eng.losses.clone(), eng.q_values.clone(), eng.targets.clone(), eng.priorities.clone()]

    def _loss(self):
        eng = self.eng
        return [eng.losses.clone(), eng.q_values.clone(), eng.targets.clone()]

    def apply(self, name):
        """Run op ``name``; returns the device tensors a reader produced (copies)."""
        eng, op = self.eng, mw.BY_NAME[name]
        if name == "forward":
            return [eng.forward(n_rows=N_ROWS, **self.rows)]
        if name == "forward_foreign":
            return [eng.forward(n_rows=N_ROWS, params=self.foreign, **self.rows)]
        if name == "best_action":
            return [eng.best_action(idx_network=1, **self.row).clone()]
        if name == "best_actions":
            return [eng.best_actions(idx_networks=self.heads, **self.rows)]
        if name == "loss_on_batch":
            eng.loss_on_batch(self.batch())
            return self._loss()
        if name == "loss_on_batch_foreign":
            eng.loss_on_batch(self.batch(), params=self.foreign)
            return self._loss()
        if name == "loss_on_batch_target":
            eng.loss_on_batch_target(self.batch(), self.target)
            return self._loss()
        if name == "grad_on_batch":
            eng.grad_on_batch(self.batch(), self.grad)
            return self._loss() + [self.grad.clone()]
        if name == "grad_on_batch_target":
            eng.grad_on_batch(self.batch(), self.grad, target_params=self.target)
            return self._loss() + [self.grad.clone()]
        if name == "analysis":
            feats, scores = eng.analysis(n_rows=N_ROWS, **self.rows)
            return [feats, *scores]
        if name == "analysis_foreign":
            feats, scores = eng.analysis(n_rows=N_ROWS, params=self.foreign, **self.rows)
            return [feats, *scores]
        if name == "learn_promised":
            eng.learn_on_batch(self.batch(mirror_current=eng._mirror_is_current(None)))
            return self._learnt()
        if name == "learn_on_batch":
            eng.learn_on_batch(self.batch())
            return self._learnt()
        if name == "learn_on_batch_grad_out":
            eng.learn_on_batch(self.batch(), grad_out=self.grad)
            return self._learnt() + [self.grad.clone()]
        if name == "learn_on_batch_target":
            eng.learn_on_batch_target(self.batch(), self.target)
            return self._learnt()
        if name in ("shift_params", "shift_params_foreign"):
            eng.shift_params(params=self._buffer(op))
        elif name.startswith("soft_shift_"):
            eng.soft_shift(op.args["tau"], params=self._buffer(op))
        elif name == "redo":
            scores, mask, n = eng.redo(n_rows=N_ROWS, tau=0.1, fresh=self.fresh, **self.rows)
            return [*scores, *mask, n]
        elif name in ("reset", "reset_foreign", "reset_alias"):
            eng.reset(self.fresh, params=self._buffer(op))
        elif name == "ema_foreign":
            eng.ema(self.target, 0.25)
        elif name == "ema_alias":
            eng.ema(eng.params, 0.25, online=self.foreign)
        elif name == "import_flax":
            eng.import_flax(self.tree)
        elif name == "params_mul_":
            eng.params.mul_(0.999)
        elif name == "data_write_invalidate":
            version = eng.params._version
            eng.params.data.mul_(1.001)
            assert eng.params._version == version  # (the write torch's counter cannot see)
            eng.invalidate_mirror()
        elif name == "rebuild_mirror":
            eng.rebuild_mirror()
        elif name == "commit_batch_stats":
            eng.commit_batch_stats()
        elif name == "compose":
            return [eng.compose().clone()]
        else:
            raise KeyError(name)
        return []


def run_walk(variant, names):
    """The walk on T and D with the four assertions behind every op; returns how often a reader that takes the flag found it set."""
    T, D = Rig(variant, True), Rig(variant, False)
    expected = mw.predict(variant, names)
    skipped = 0
    for i, name in enumerate(names):
        what = f"{variant} op {i} {name} (after {names[max(0, i - 3):i]})"
        skipped += name in ("best_actions", "learn_promised") and T.eng._mirror_is_current(None)
        out_t, out_d = T.apply(name), D.apply(name)
        # (b)
        assert len(out_t) == len(out_d)
        for k, (a, b) in enumerate(zip(out_t, out_d)):
            assert _same_bits(a, b), f"{what}, (b): output {k} differs between the trusted and the default engine"
        # (a)
        other = D.state()
        for n, a in T.state().items():
            assert _same_bits(a, other[n]), f"{what}, (a): {n} differs between the trusted and the default engine"
        # (c)
        flag = T.eng._mirror_is_current(None)
        if flag:
            T.check.assert_holds(T.eng.params, what + ", (c)")
        if name == "compose":  # (noisy: right behind compose(mirror=True) the mirror is the split of eff)
            T.check.assert_holds(T.eng.eff, what + ", (c) on eff")
        # (d)
        assert flag == expected[i], (f"{what}, (d): _mirror_is_current is {flag}, the table says {expected[i]} -- "
                                     + ("a stale mirror is trusted" if flag else "a current mirror is rebuilt"))
        assert not D.eng._mirror_is_current(None)
    # (the walk stayed on numbers: equal bits of NaN would compare equal and show nothing)
    assert bool(torch.isfinite(T.eng.params).all()) and float(T.eng.params.abs().max()) > 0
    return skipped


@pytest.mark.parametrize("seed", mw.SEEDS)
@pytest.mark.parametrize("variant", list(mw.VARIANTS))
def test_trusted_engine_equals_the_default_one_along_a_walk(variant, seed):
    names = mw.walk(variant, seed)
    skipped = run_walk(variant, names)
    if not mw.is_noisy(variant):  # (a noisy engine composes in front of every call: nothing of its own is ever skipped)
        assert skipped >= mw.N_TRUSTED_RUNS, "the trusted engine hardly ever skipped a rebuild: the walk exercised nothing"


# ---------------------------------------------------------------------------------------------------------------- agent level
A_, K_, B_ = mw.N_ACTIONS, mw.K, mw.BATCH
FEATS = [8, 8, 8, 16]
N_STEPS, FILL, T_FREQ = 120, 16, 25
AGENTS = {
    "isdqn": ("iSDQN", {}),
    "isdqn-soft": ("iSDQN", dict(soft_shift_tau=0.25)),
    "dqn": ("DQN", {}),
    "dqn-ema": ("DQN", dict(ema_tau=0.005)),
}


class Twin:
    def __init__(self, which, trusted):
        from slimdqn.environments.synthetic import SyntheticAtariEnv
        from slimdqn.networks.dqn import DQN
        from slimdqn.networks.isdqn import iSDQN
        from slimdqn.sample_collection.replay_buffer import ReplayBuffer
        from slimdqn.sample_collection.samplers import UniformSamplingDistribution

        cls, kw = AGENTS[which]
        self.isdqn = cls == "iSDQN"
        tail = ("cnn", 1e-3, 0.99, 1, 1, T_FREQ)
        if self.isdqn:
            self.agent = iSDQN(3, (84, 84, 4), A_, K_, FEATS, True, False, *tail, adam_eps=1.5e-4, batch_size=B_, **kw)
        else:
            self.agent = DQN(3, (84, 84, 4), A_, FEATS, True, *tail, adam_eps=1.5e-4, batch_size=B_, **kw)
        if trusted:
            self.agent.trust_mirror = True
        self.env = SyntheticAtariEnv("Synthetic", n_actions=A_, seed=9, episode_length=23)
        self.env.reset()
        self.rb = ReplayBuffer(UniformSamplingDistribution(4), B_, 200, update_horizon=1, gamma=0.99)

    def act(self, t):
        agent, env = self.agent, self.env
        action = agent.best_action(agent.params, env.state, key=t % K_) if self.isdqn else agent.best_action(agent.params, env.state)
        return int(action)

    def store(self, action):
        from slimdqn.sample_collection.replay_buffer import TransitionElement

        env = self.env
        obs = env.observation
        reward, terminal = env.step(action)
        self.rb.add(TransitionElement(obs, action, reward, terminal, terminal))
        if terminal:
            env.reset()

    def learn_eager(self, params, samples):
        agent = self.agent
        if self.isdqn:
            agent.learn_on_batch(params, agent.optimizer_state, samples)
        else:
            agent.learn_on_batch(params, agent.target_params, agent.optimizer_state, samples)

    def state(self):
        eng = self.agent._engine
        out = {n: getattr(eng, n) for n in STATE}
        if not self.isdqn:
            out["target"] = self.agent.target_params.tensor
        return out


def _script(t):
    """The writers of step ``t`` behind its acting call, as (label, what to do with a Twin)."""
    if t < FILL:
        return []
    steps = []
    if t in (35, 80):
        steps.append(("mul_", lambda w: w.agent._engine.params.mul_(1.001)))
    if t in (45, 95):
        def foreign(w):
            handle = w.agent.params.clone()
            handle.tensor.mul_(0.5)
            w.learn_eager(handle, w.rb.sample())  # (_load_bound: the foreign parameters become the engine's)
        steps.append(("foreign", foreign))
    if t == 60:  # a batch of another size: _engine_for -> copy_state_from (and back again at the next update on the replay)
        steps.append(("batch_size", lambda w: w.learn_eager(w.agent.params, w.rb.sample(size=2 * B_))))
    if t in (50, 90):
        steps.append(("recycle", lambda w: w.agent.recycle_dormant(w.rb, 0.1)))
    if t in (70, 100):
        steps.append(("reset", lambda w: w.agent.reset_parameters()))
    if t >= 64 and t % 4 == 0:
        steps.append(("learn_steps", lambda w: w.agent.learn_steps(3, w.rb)))
    elif t % 2 == 0 or t < 64:
        steps.append(("update", lambda w: w.agent.update_online_params(t, w.rb)))
    steps.append(("target", lambda w: w.agent.update_target_params(t)))
    return steps


def _labels_behind(label, which, t, agent):
    """What the writer ``label`` of step ``t`` was to the weight mirror, or None when it wrote no online parameter."""
    if label == "target":  # (only iS-DQN's hard head shift writes the online parameters here)
        return ("shift",) if which == "isdqn" and t % T_FREQ == 0 else None
    if label in ("update", "learn_steps"):
        g = agent._graphed
        replayed = g is not None and (label == "learn_steps" or g.S == 1)  # (iSDQN steps eagerly while learn_steps' capture is live)
        return ("captured_replay" if replayed else "eager_step",) + (("soft_shift",) if which == "isdqn-soft" else ())
    return (label,)


@pytest.mark.parametrize("which", list(AGENTS))
def test_trusted_agent_equals_its_default_twin(which):
    trusted, default = Twin(which, True), Twin(which, False)
    assert trusted.agent.trust_mirror and not default.agent.trust_mirror
    skips = {}    # what the last writer was -> calls behind it that found the mirror current, sampled in front of the call
    labels = ()
    checks = []   # one MirrorCheck per engine the trusted agent has had

    def sample():
        if trusted.agent._engine._mirror_is_current(None):
            for label in labels:
                skips[label] = skips.get(label, 0) + 1

    def compare(what):
        eng = trusted.agent._engine
        if not checks or checks[-1].eng is not eng:
            checks.append(MirrorCheck(eng))
        other = default.state()
        for n, a in trusted.state().items():
            assert _same_bits(a, other[n]), f"{what}: {n} differs between the trusted agent and its default twin"
        if eng._mirror_is_current(None):
            checks[-1].assert_holds(eng.params, what)

    for t in range(N_STEPS):
        sample()
        a_t, a_d = trusted.act(t), default.act(t)
        assert a_t == a_d, f"step {t}: the trusted agent acts {a_t}, its default twin {a_d} (after {labels})"
        compare(f"step {t}, acting (after {labels})")
        trusted.store(a_t)
        default.store(a_d)
        for label, do in _script(t):
            if label in ("update", "learn_steps"):  # (a captured replay rebuilds in front only when the flag is down: _graph.py run)
                sample()
            do(trusted)
            do(default)
            behind = _labels_behind(label, which, t, trusted.agent)
            labels = labels if behind is None else behind
            compare(f"step {t}, {label} (after {labels})")
    assert len(checks) >= 3  # (the change of batch size built a new engine, the next update on the replay another)
    for w in (trusted, default):
        agent = w.agent
        assert agent._graphed is not None and agent._graphed.S == (3 if w.isdqn else 1)  # (learn_steps' capture where the agent has one)
        assert agent._ring is not None and agent._ring.get("graph") and agent._ring["graph"]["graphs"]  # the one-frame act graph ran
    assert any(current for _, current in trusted.agent._ring["graph"]["graphs"])  # (an act graph captured without the rebuild)
    assert not any(current for _, current in default.agent._ring["graph"]["graphs"])
    wanted = ["captured_replay", "recycle", "reset"] + (["soft_shift"] if which == "isdqn-soft" else [])
    for label in wanted:
        assert skips.get(label, 0) >= 1, f"the trusted twin never skipped a rebuild behind {label}: {skips}"
