"""The grid and the recorder of the step-order snapshot (tests/golden/step_order_snapshot.txt) and everything its two users share:
oracle/make_golden_step_order.py records the snapshot, tests/test_step_order_host.py holds the tree to it.

What is recorded, without a GPU: which engine calls a gradient step of every agent makes, in which order and on which buffer -- the
eager step, and what the captured step (hipGraph) is handed as its learn call, its state tensors and its step count.  The recorder
hooks at two seams and nowhere inside the agents:

  slimdqn.networks._agent.QNetEngine   -> Engine: CPU tensors where the agents read buffers, and a log of every method called on it
  slimdqn._graph.GraphedUpdate         -> Graph: keeps its constructor's arguments and calls ``learn`` once on a dummy batch

and feeds the agents two stub replays: one that passes the guards of ``_graphed_update`` like this GPU's device replay, one that does
not.  Both hand out batches of BATCH + 1 rows, one more than the agent was built with: every recorded step therefore also shows
where the engine of the new batch size is built, and that the calls behind it go to that engine (e1) and not to the first (e0).

A row is one class x torso x setting of the six axes below; a constructor that refuses the combination is a row too (type and
message).  An accepted row records

  (a) eager     update_online_params(0, eager replay): every engine call, then ``_prune_t``;
  (b) captured  update_online_params(0, device-like replay), iSDQN / DQN / TFDQN: steps, the state tensors by name, every engine
                call with the ones inside the learn call between ``[`` and ``]``, then ``_prune_t`` after the one replay;
  (c) steps3    learn_steps(3, device-like replay), iSDQN: as (b).

``soft_shift``, ``ema``, ``prune_apply``, ``project_weights`` and ``learn_on_batch_target`` are logged with the buffers they were
given, named by identity (params, sigma, target, target_sigma), and the first two with their tau."""
import itertools
import types
from unittest import mock

import torch

from tests.helpers import options_grid as og

GOLDEN = og.GOLDEN.replace("options_snapshot", "step_order_snapshot")
TORSOS = ("cnn", "fc")
BATCH = og.BATCH + 1  # of the stub replays: not the agents' own
PRUNE_KW = dict(prune_sparsity=0.5, prune_start=0, prune_end=10, prune_period=10)  # (og.build_agent: target_update_frequency 10)

# axis -> (value's name in a row's name, the keywords it adds); the first value of every axis is "off": no keyword at all
AXES = {
    "shift": (("0", {}), ("0.25", dict(soft_shift_tau=0.25)), ("0.5", dict(soft_shift_tau=0.5))),
    "ema": (("0", {}), ("0.005", dict(ema_tau=0.005))),
    "rem": (("0", {}), ("3", dict(rem_heads=3))),
    "noisy": (("0", {}), ("1", dict(noisy=True))),
    "prune": (("off", {}), ("idle", PRUNE_KW), ("active", PRUNE_KW)),  # idle: on, nothing pruned yet; active: a mask update pruned
    "nap": (("0", {}), ("1", dict(weight_projection=True))),
}
CAPTURED = ("iSDQN", "DQN", "TFDQN")  # the classes whose update replays a captured step


def rows():
    """Every combination of the axes' values, as tuples of value names in the order of AXES."""
    return list(itertools.product(*[[name for name, _ in values] for values in AXES.values()]))


def row_name(row):
    return " ".join(f"{axis}={v}" for axis, v in zip(AXES, row))


def keywords(row):
    kw = {}
    for values, v in zip(AXES.values(), row):
        kw.update(dict(values)[v])
    return kw


def cells():
    return [(c, t) for c in og.CLASSES for t in TORSOS]


# ------------------------------------------------------------------ the stand-ins
class Engine:
    """Stands where QNetEngine stands.  Every engine of one recording appends to ``Engine.log``: (engine, method name, tensors)."""

    log = []
    built = []
    mix_alpha = mix_count = prune_mask = project_scales = None
    project_infos = ()
    trust_mirror = False
    resample_on_learn = False

    def __init__(self, observation_dim, n_actions, n_heads, features, architecture_type, layer_norm, batch_size, **kw):
        self.batch_size, self.n_heads, self.architecture_type = batch_size, n_heads, architecture_type
        self.noisy, self.dueling, self.batch_norm = bool(kw.get("noisy", False)), bool(kw.get("dueling", False)), bool(kw.get("batch_norm", False))
        self.device = "cpu"
        self.params, self.sigma, self.adam_m, self.adam_v = (torch.zeros(8) for _ in range(4))
        self.adam_count = torch.zeros(1, dtype=torch.int32)
        self.losses, self.losses_accum = torch.zeros(n_heads), torch.zeros(n_heads)
        self.targets = torch.zeros(batch_size, max(n_heads - 1, 1))
        self.priorities = torch.zeros(batch_size)
        self.n_param_floats = 8
        self.infos = [types.SimpleNamespace(layer=0, kind=0, offset=0, size=8, dims=(1, 8))]
        Engine.built.append(self)
        self._say("QNetEngine")

    def _say(self, name, **tensors):
        Engine.log.append((self, name, tensors))

    def __getattr__(self, name):  # every method the agents call and nobody spelled out below: logged, returns None
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: self._say(name)

    def set_mixture(self, seed):
        self._say("set_mixture")
        self.mix_alpha, self.mix_count = torch.zeros(self.n_heads), torch.zeros(1, dtype=torch.int64)

    def set_pruning(self):
        self._say("set_pruning")
        self.prune_mask = torch.zeros(1, dtype=torch.int32)
        return [100, 50]

    def set_weight_projection(self, target_norms=None):
        self._say("set_weight_projection")
        self.project_scales = torch.ones(2)
        return [1.0, 2.0] if target_norms is None else list(target_norms)

    def learn_on_batch(self, batch, grad_out=None):
        self._say("learn_on_batch")
        return self.losses

    def learn_on_batch_target(self, batch, target_params, target_sigma=None):
        self._say("learn_on_batch_target", target=target_params, **({} if target_sigma is None else dict(sigma=target_sigma)))
        return self.losses

    def loss_on_batch(self, batch, params=None):
        self._say("loss_on_batch")
        return self.losses

    def soft_shift(self, tau, params=None):
        self._say(f"soft_shift:{tau!r}", on=self.params if params is None else params)

    def ema(self, target, tau, online=None):
        self._say(f"ema:{tau!r}", on=target, online=self.params if online is None else online)

    def prune_apply(self, params=None):
        self._say("prune_apply", on=self.params if params is None else params)

    def project_weights(self, params=None):
        self._say("project_weights", on=self.params if params is None else params)


class Graph:
    """Stands where GraphedUpdate stands: the capture is one call of ``learn`` on a dummy batch, logged between "[" and "]"."""

    made = []

    def __init__(self, rb, eng, prioritized, steps_per_graph=8, writeback=None, learn=None, weighted=False, augment=None, state=(),
                 horizon=False):
        self.rb, self.eng, self.prioritized, self.S = rb, eng, prioritized, steps_per_graph
        self.writeback = prioritized if writeback is None else (writeback and prioritized)
        self.weighted, self.horizon, self.augment_pad = bool(weighted), bool(horizon), int(augment[0]) if augment else 0
        self.learn_given, self.state, self.key = learn, list(state), None
        Graph.made.append(self)
        Engine.log.append((eng, "[", {}))
        (eng.learn_on_batch if learn is None else learn)(object())
        Engine.log.append((eng, "]", {}))

    def run(self, betas=None, horizons=None, gammas=None):
        Engine.log.append((self.eng, "replay", {}))

    def destroy(self):
        pass


def _batch():
    z = torch.zeros(BATCH)
    return types.SimpleNamespace(frame_ids=z, frames=z, frame_stride=1, state=z, next_state=z, action=z, reward=z, is_terminal=z)


class EagerReplay:
    """A replay that is not this GPU's device replay: ``_graphed_update`` answers None and the agent takes the eager path."""

    _batch_size = BATCH

    def sample(self, **kw):
        return _batch()


class DeviceReplay(EagerReplay):
    """Enough of the device replay to pass the guards at the head of ``_graphed_update``."""

    _d_elem_frames, _lib, add_count, _obs_float, _stack_size = 0, object(), 1, True, 1
    _sampling_distribution = object()  # (no ``_tree``: uniform)


# ------------------------------------------------------------------ the recorder
def _names(agent):
    """{id(tensor): name} of the buffers a call can be given; an engine's own are qualified where another engine is handed them."""
    out = {}
    target = getattr(agent, "target_params", None)
    for name, t in (("target", None if target is None else target.tensor), ("target_sigma", getattr(agent, "target_sigma", None))):
        if t is not None:
            out[id(t)] = (None, name)
    for eng in Engine.built:
        for name in ("params", "sigma", "mix_alpha", "mix_count"):
            if getattr(eng, name) is not None:
                out.setdefault(id(getattr(eng, name)), (eng, name))
    return out


def _name(names, eng, t):
    owner, name = names.get(id(t), (None, "?"))
    return name if owner is None or owner is eng else f"e{Engine.built.index(owner)}.{name}"


def _calls(agent):
    """The log as text: e<engine>.<method>[(<buffer>, ...)], the capture's learn call between "[" and "]"."""
    names, out = _names(agent), []
    for eng, name, tensors in Engine.log:
        if name in "[]":
            out.append(name)
            continue
        args = ",".join(f"{k}={_name(names, eng, t)}" for k, t in tensors.items())
        out.append(f"e{Engine.built.index(eng)}.{name}" + (f"({args})" if args else ""))
    return out


def _key(agent, key):
    """The captured step's key with every buffer pointer in it replaced by the buffer's name: comparable between two agents."""
    ptrs = {t.data_ptr(): name for name, t in (("target", getattr(getattr(agent, "target_params", None), "tensor", None)),
                                               ("params", agent._engine.params)) if t is not None}
    if isinstance(key, tuple):
        return tuple(_key(agent, k) for k in key)
    return ptrs.get(key, key) if isinstance(key, int) and not isinstance(key, bool) else key


def _agent(cls_name, torso, row):
    """A fresh agent of the row with nothing logged yet; ``active`` rows have had the mask update past ``prune_end`` that prunes."""
    Engine.log, Engine.built, Graph.made = [], [], []
    agent = og.build_agent(cls_name, torso, keywords(row))
    if dict(zip(AXES, row))["prune"] == "active":
        agent._prune_t = 20
        agent.prune_target_update(10)
        assert agent.prune_active
        agent._prune_t = 0
    del Engine.log[:]
    return agent


def _captured(agent, call):
    """One phase on the device-like replay: (lines of the record, the key with names for pointers, what the key must tell apart)."""
    call(DeviceReplay())
    (g,) = Graph.made
    assert agent._graphed is g
    names = _names(agent)
    state = sorted({_name(names, g.eng, t) for t in g.state})
    calls = _calls(agent)
    learn = calls[calls.index("[") + 1 : calls.index("]")]
    lines = [f"steps: {g.S}", f"state: {' '.join(state) or '-'}", f"calls: {' '.join(calls)}", f"prune_t: {agent._prune_t}"]
    return lines, _key(agent, g.key), (tuple(state), tuple(learn), g.learn_given is None)


def record_row(cls_name, torso, row):
    """dict(kind="err", text="Type: message") of the constructor's refusal, or dict(kind="ok", text=the record, key=, told=, key3=):
    the key of (b) with names for pointers, what it must tell apart -- (state, calls inside learn, whether ``learn`` was None) --, and
    the key of (c).  The keys are not part of the text: their spelling is private."""
    try:
        agent = _agent(cls_name, torso, row)
    except Exception as e:  # noqa: BLE001 (whatever the constructor raises is the row)
        return dict(kind="err", text=f"{type(e).__name__}: {e}")
    agent.update_online_params(0, EagerReplay())
    assert not Graph.made
    out = dict(kind="ok", key=None, told=None, key3=None)
    text = [f"(a) calls: {' '.join(_calls(agent))}", f"(a) prune_t: {agent._prune_t}"]
    if cls_name in CAPTURED:
        agent = _agent(cls_name, torso, row)  # (a fresh one per phase: each shows the engine of the new batch size being built)
        lines, out["key"], out["told"] = _captured(agent, lambda rb: agent.update_online_params(0, rb))
        text += [f"(b) {l}" for l in lines]
    if cls_name == "iSDQN":
        agent = _agent(cls_name, torso, row)
        lines, out["key3"], _ = _captured(agent, lambda rb: agent.learn_steps(3, rb))
        text += [f"(c) {l}" for l in lines]
    out["text"] = "".join(l + "\n" for l in text)
    return out


def record():
    """{(class, torso, row name): record_row(...)} over cells() x rows()."""
    from slimdqn import _graph
    from slimdqn.networks import _agent as agent_module

    out = {}
    with mock.patch.object(agent_module, "QNetEngine", Engine), mock.patch.object(_graph, "GraphedUpdate", Graph):
        for cls_name, torso in cells():
            for row in rows():
                out[(cls_name, torso, row_name(row))] = record_row(cls_name, torso, row)
    return out


# ------------------------------------------------------------------ the snapshot file
def snapshot(recorded):
    """The text of the snapshot.  [messages]: the distinct refusals in order of first appearance.  [records]: the distinct records of
    accepted rows, in full.  [rows]: one line per row, ``m<i>`` a refusal, ``r<i>`` a record."""
    messages, records, lines = {}, {}, []
    for key, r in recorded.items():
        table, prefix = (messages, "m") if r["kind"] == "err" else (records, "r")
        lines.append(f"{' '.join(key)}\t{prefix}{table.setdefault(r['text'], len(table) + 1)}")
    out = ["[messages]"] + [f"{i}\t{m}" for m, i in messages.items()] + ["[records]"]
    for text, i in records.items():
        out.append(f"== r{i}\n{text}".rstrip("\n"))
    return "\n".join(out + ["[rows]"] + lines) + "\n"


def read(text):
    """{(class, torso, row name): ("err", message) or ("ok", record text)} of a snapshot."""
    head, row_lines = text.split("[rows]\n")
    messages, records = head.split("[messages]\n")[1].split("[records]\n")
    table = {"m" + i: ("err", m) for i, m in (l.split("\t", 1) for l in messages.splitlines())}
    for block in records.split("== ")[1:]:
        name, body = block.split("\n", 1)
        table[name] = ("ok", body)
    out = {}
    for l in row_lines.splitlines():
        key, token = l.split("\t")
        cls_name, torso, name = key.split(" ", 2)
        out[(cls_name, torso, name)] = table[token]
    return out
