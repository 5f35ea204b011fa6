"""The option grid of the options snapshot (tests/golden/options_snapshot.txt) and everything its two users share:
oracle/make_golden_options.py records the snapshot, tests/test_options_snapshot_host.py holds the tree to it.

Two recordings, both without a GPU:

  [agents]  every agent class x torso x row of option settings -> the arguments its constructor hands to QNetEngine (bound to the real
            signature, defaults applied, ``noisy_seed`` included), or the type and message of the exception that came out of it.  The
            name ``QNetEngine`` in slimdqn.networks._agent is replaced by a recorder: nothing is allocated.
  [engine]  QNetEngine called directly x torso x row -> every field of the isdqn_net_config it filled, read at its first C-ABI call
            (isdqn_net_param_layout) through a stand-in library, or the exception.

A row is all options off, one setting, or a pair of settings: the pairs pin which refusal answers first when two rules are violated.
Floats are written as float.hex(), every value with its type."""
import ctypes
import hashlib
import inspect
import itertools
import os
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "options_snapshot.txt")

N_ACTIONS, K, BATCH = 4, 2, 4
SEED = 7

# name -> the keywords it switches on.  "c51" (histogram heads with the categorical loss) stands beside its two halves: paired with
# Munchausen targets it is the only row of two settings that reaches CATEGORICAL_MUNCHAUSEN_REFUSED
SETTINGS = {
    "n_bins": dict(n_bins=51),
    "categorical": dict(categorical=True),
    "c51": dict(n_bins=51, categorical=True),
    "n_quantiles": dict(n_quantiles=5),
    "munchausen": dict(munchausen_tau=0.03),
    "double_q": dict(double_q=True),
    "dueling": dict(dueling=True),
    "huber": dict(huber_delta=1.0),
    "clip10": dict(max_grad_norm=10),
    "clip_inf": dict(max_grad_norm=float("inf")),
    "clip_neg": dict(max_grad_norm=-1),
    "clip_nan": dict(max_grad_norm=float("nan")),
    "noisy": dict(noisy=True),
    "sigma0": dict(noisy_sigma0=0.25),
    "pad4": dict(augment_pad=4),
    "pad128": dict(augment_pad=128),
    "pad_true": dict(augment_pad=True),
    "ema": dict(ema_tau=0.005),
    "ema1.5": dict(ema_tau=1.5),
}
AGENT_ONLY = ("pad4", "pad128", "pad_true", "ema", "ema1.5")
ENGINE_SETTINGS = {**{k: v for k, v in SETTINGS.items() if k not in AGENT_ONLY}, "bf16": dict(precision="bf16")}

TORSOS = {
    "cnn": dict(arch="cnn", obs=(84, 84, 4), features=[8, 8, 8, 16], layer_norm=True, batch_norm=False),
    "cnn_bn": dict(arch="cnn", obs=(84, 84, 4), features=[8, 8, 8, 16], layer_norm=False, batch_norm=True),
    "cnn_odd": dict(arch="cnn", obs=(84, 84, 4), features=[8, 8, 8, 15], layer_norm=True, batch_norm=False),
    "cnn_no_hidden": dict(arch="cnn", obs=(84, 84, 4), features=[8, 8, 8], layer_norm=True, batch_norm=False),
    "impala": dict(arch="impala", obs=(84, 84, 4), features=[8, 8, 8, 16], layer_norm=False, batch_norm=False),
    "fc": dict(arch="fc", obs=(8,), features=[20, 14], layer_norm=True, batch_norm=False),
    "fc_empty": dict(arch="fc", obs=(8,), features=[], layer_norm=False, batch_norm=False),
}
CLASSES = ("iSDQN", "DQN", "TFDQN", "AnalysisDQN", "AnalysisTFDQN")
TAKES_BATCH_NORM = ("iSDQN", "TFDQN", "AnalysisDQN", "AnalysisTFDQN")


class Recorded(Exception):
    """Raised by the two recorders with what they saw: the constructor under observation ends here."""


def rows(settings):
    """[()] + every single setting + every pair that does not set one keyword twice, as tuples of names in the order of `settings`."""
    names = list(settings)
    pairs = [(a, b) for a, b in itertools.combinations(names, 2) if not set(settings[a]) & set(settings[b])]
    return [()] + [(a,) for a in names] + pairs


def row_name(row):
    return "+".join(row) or "-"


def keywords(settings, row):
    kw = {}
    for name in row:
        kw.update(settings[name])
    return kw


def agent_cells():
    return [(c, t) for c in CLASSES for t in TORSOS if c in TAKES_BATCH_NORM or not TORSOS[t]["batch_norm"]]


def canon(v):
    """A value with its type; floats in hex (inf and nan included), sequences element by element."""
    if isinstance(v, (list, tuple)):
        return f"{type(v).__name__}[{', '.join(canon(x) for x in v)}]"
    if isinstance(v, float):
        return f"float:{v.hex()}"
    return f"{type(v).__name__}:{v}"


def record_text(mapping):
    return "".join(f"{k}={canon(v)}\n" for k, v in mapping.items())


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def _outcome(call):
    """("ok", record text) of what the recorder saw, or ("err", "Type: message") of the exception that came out first."""
    try:
        call()
    except Recorded as r:
        return "ok", record_text(r.args[0])
    except Exception as e:  # noqa: BLE001 (whatever the constructor raises is the row)
        return "err", f"{type(e).__name__}: {e}"
    raise AssertionError("the constructor returned: the recorder was not reached")


# ------------------------------------------------------------------ [agents]
def _agent_classes():
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    return dict(iSDQN=iSDQN, DQN=DQN, TFDQN=TFDQN, AnalysisDQN=AnalysisDQN, AnalysisTFDQN=AnalysisTFDQN)


def build_agent(cls_name, torso, kw):
    """The constructor call of one row: the leading arguments positionally, as the entry points pass them."""
    t, cls = TORSOS[torso], _agent_classes()[cls_name]
    tail = (t["arch"], 1e-3, 0.99, 1, 1, 10)  # architecture_type, learning_rate, gamma, update_horizon, data_to_update, target_update_frequency
    if cls_name in ("iSDQN", "AnalysisDQN"):
        return cls(SEED, t["obs"], N_ACTIONS, K, t["features"], t["layer_norm"], t["batch_norm"], *tail, batch_size=BATCH, **kw)
    if cls_name == "DQN":
        return cls(SEED, t["obs"], N_ACTIONS, t["features"], t["layer_norm"], *tail, batch_size=BATCH, **kw)
    return cls(SEED, t["obs"], N_ACTIONS, t["features"], t["layer_norm"], t["batch_norm"], *tail, batch_size=BATCH, **kw)


def record_agents():
    """{(class, torso, row name): outcome} over agent_cells() x rows(SETTINGS)."""
    from slimdqn._engine import QNetEngine
    from slimdqn.networks import _agent

    sig = inspect.signature(QNetEngine.__init__)

    def recorder(*args, **kwargs):
        bound = sig.bind(None, *args, **kwargs)
        bound.apply_defaults()
        raise Recorded({k: v for k, v in bound.arguments.items() if k != "self"})

    out = {}
    with mock.patch.object(_agent, "QNetEngine", recorder):
        for cls_name, torso in agent_cells():
            for row in rows(SETTINGS):
                out[(cls_name, torso, row_name(row))] = _outcome(lambda: build_agent(cls_name, torso, keywords(SETTINGS, row)))
    return out


# ------------------------------------------------------------------ [engine]
class _ConfigReader:
    """Stands where the loaded library stands: the first call an engine makes dumps the isdqn_net_config it was handed."""

    def isdqn_net_param_layout(self, ref, *rest):
        cfg = ref._obj
        fields = {}
        for name, _ in cfg._fields_:
            v = getattr(cfg, name)
            fields[name] = list(v) if isinstance(v, ctypes.Array) else v
        raise Recorded(fields)


def build_engine(torso, kw):
    from slimdqn._engine import QNetEngine

    t = TORSOS[torso]
    return QNetEngine(t["obs"], N_ACTIONS, 1 + K, t["features"], t["arch"], t["layer_norm"], BATCH, batch_norm=t["batch_norm"], **kw)


def record_engine():
    """{(torso, row name): outcome} over TORSOS x rows(ENGINE_SETTINGS)."""
    from slimdqn import _hip

    out = {}
    nothing = lambda *a, **k: None  # noqa: E731
    with mock.patch.object(_hip, "require_gpu", nothing), mock.patch.object(_hip, "resolve_device", nothing), \
            mock.patch.object(_hip, "bind_device", nothing), mock.patch.object(_hip, "lib", _ConfigReader):
        for torso in TORSOS:
            for row in rows(ENGINE_SETTINGS):
                out[(torso, row_name(row))] = _outcome(lambda: build_engine(torso, keywords(ENGINE_SETTINGS, row)))
    return out


# ------------------------------------------------------------------ the snapshot file
def _is_full(row):
    return "+" not in row  # all-off and single-setting rows keep their record as text


def changed_lines(text, base):
    """The lines of a record that the all-off record of its cell does not have (same keys, same order: the fields that moved)."""
    have = set(base.splitlines())
    return "".join(l + "\n" for l in text.splitlines() if l not in have)


def full_text(outcomes, key):
    """What the [full] section keeps of an accepted row: the whole record of an all-off row, else its changed_lines."""
    text = outcomes[key][1]
    base = outcomes[key[:-1] + ("-",)]
    return text if key[-1] == "-" or base[0] != "ok" else changed_lines(text, base[1])


def snapshot(agents, engine):
    """The text of the snapshot.  [messages]: the distinct "Type: message" in order of first appearance.  [records]: the distinct
    SHA-256 of accepted records.  [agents] / [engine]: one line per cell, one token per row of rows(): m<i> a refusal, r<i> a record.
    [full]: full_text of every accepted all-off and single-setting row."""
    messages, records = {}, {}

    def token(outcome):
        kind, text = outcome
        return f"m{messages.setdefault(text, len(messages) + 1)}" if kind == "err" else f"r{records.setdefault(sha(text), len(records) + 1)}"

    sections = []
    for title, outcomes in (("agents", agents), ("engine", engine)):
        cells = {}
        for key, outcome in outcomes.items():
            cells.setdefault(" ".join(key[:-1]), []).append(token(outcome))
        sections += [f"[{title}]"] + [f"{cell}\t{' '.join(t)}" for cell, t in cells.items()]
    out = ["[messages]"] + [f"{i}\t{m}" for m, i in messages.items()] + ["[records]"] + [f"{i}\t{h}" for h, i in records.items()] + sections
    out.append("[full]")
    for title, outcomes in (("agents", agents), ("engine", engine)):
        for key, (kind, _) in outcomes.items():
            if kind == "ok" and _is_full(key[-1]):
                out.append(f"== {title} {' '.join(key)}\n{full_text(outcomes, key)}".rstrip("\n"))
    return "\n".join(out) + "\n"


def read(text):
    """(agents, engine, full) of a snapshot: {key: ("err", message) or ("ok", SHA-256)} twice, and {(section, *key): text}."""
    head, full = text.split("[full]\n")
    messages, rest = head.split("[messages]\n")[1].split("[records]\n")
    records, rest = rest.split("[agents]\n")
    agent_lines, engine_lines = rest.split("[engine]\n")
    table = {"m" + i: ("err", m) for i, m in (l.split("\t", 1) for l in messages.splitlines())}
    table.update({"r" + i: ("ok", h) for i, h in (l.split("\t") for l in records.splitlines())})

    def section(lines, settings):
        out = {}
        for l in lines.splitlines():
            cell, tokens = l.split("\t")
            tokens = tokens.split(" ")
            assert len(tokens) == len(rows(settings)), "the grid is not the one the snapshot was recorded from"
            for row, t in zip(rows(settings), tokens):
                out[tuple(cell.split(" ")) + (row_name(row),)] = table[t]
        return out

    blocks = {}
    for block in full.split("== ")[1:]:
        name, body = (block.rstrip("\n") + "\n").split("\n", 1)
        blocks[tuple(name.split(" "))] = body
    return section(agent_lines, SETTINGS), section(engine_lines, ENGINE_SETTINGS), blocks
