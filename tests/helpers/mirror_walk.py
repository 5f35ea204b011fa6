"""The engine's operations as the weight-mirror bookkeeping sees them, as one table, and seeded walks over it (pure Python: no torch
device, no library).

The MFMA stages read the split-bf16 mirror of the weights in the workspace (region "wsplit"), not the float32 master.  An engine with
``trust_mirror = True`` skips the rebuild while its bookkeeping (slimdqn/_engine.py, "weight-mirror bookkeeping") says the mirror still
equals the master.  Every operation below is a READER (its result depends on the mirror), a WRITER (it writes the master, the mirror or
the bookkeeping) or both, and has one documented effect on "mirror == master and the bookkeeping knows it":

  makes_current  the call ends with the mirror rebuilt from -- or written together with -- the engine's own parameters
  keeps          the call touches neither side, or both sides alike: current stays current, stale stays stale
  invalidates    the master moved alone, or the mirror now holds something else (a foreign buffer, a noisy engine's ``eff``)

The effects are read off the docstrings and comments of slimdqn/_engine.py and include/isdqn_hip.h (``source`` says where), not off a
run.  Where the documents say nothing the entry says ``invalidates`` -- the safe answer -- and its source says so.

tests/test_mirror_walk_host.py holds the walks to the conditions that keep tests/test_gpu_mirror_coherence.py from hiding a path;
DESIGN.md (section 3) carries ``table_markdown()``: a new writer of the engine is registered here and there.
"""
import dataclasses
import random

MAKES_CURRENT, KEEPS, INVALIDATES = "makes_current", "keeps", "invalidates"
READER, WRITER = "reader", "writer"

# ---------------------------------------------------------------------------------------------------------------- variants
# The smallest shapes on which every route exists (tests/helpers/options_grid.py: N_ACTIONS = 4, K = 2, BATCH = 4 are its values; the
# host side of this file imports nothing, so they are restated and tests/test_mirror_walk_host.py compares them).
N_ACTIONS, K, BATCH = 4, 2, 4
CNN = dict(arch="cnn", obs=(84, 84, 4), features=(8, 8, 8, 16))
FC = dict(arch="fc", obs=(8,), features=(20, 14))
VARIANTS = {
    "cnn-ln": dict(CNN, layer_norm=True, batch_norm=False, options={}),
    "fc": dict(FC, layer_norm=True, batch_norm=False, options={}),
    "cnn-hl51": dict(CNN, layer_norm=True, batch_norm=False, options=dict(n_bins=51, min_value=-10.0, max_value=10.0, sigma=0.3)),
    "cnn-bn": dict(CNN, layer_norm=False, batch_norm=True, options={}),
    "fc-noisy": dict(FC, layer_norm=True, batch_norm=False, options=dict(noisy=True)),
}
ALL = tuple(VARIANTS)
NOT_BN = tuple(v for v in ALL if not VARIANTS[v]["batch_norm"])  # check_*: BatchNorm networks take separate target parameters in gradient-only passes alone
REDO = tuple(v for v in NOT_BN if not VARIANTS[v]["options"].get("noisy"))  # check_redo (batch_norm), NOISY_REDO_REFUSED
BN = tuple(v for v in ALL if VARIANTS[v]["batch_norm"])
NOISY = tuple(v for v in ALL if VARIANTS[v]["options"].get("noisy"))


def is_noisy(variant) -> bool:
    return variant in NOISY


# ---------------------------------------------------------------------------------------------------------------- the table
@dataclasses.dataclass(frozen=True)
class Op:
    name: str
    kind: tuple        # (READER,), (WRITER,) or both
    variants: tuple    # the engine variants it applies to
    effect: str        # on an engine without noisy layers
    noisy_effect: str  # on a noisy engine: every call on its own parameters composes first, and the mirror then holds eff
    source: str        # where the effect is documented
    args: dict = dataclasses.field(default_factory=dict)  # the small fixed arguments the GPU test calls it with

    def effect_on(self, variant) -> str:
        return self.noisy_effect if is_noisy(variant) else self.effect

    @property
    def reads(self) -> bool:
        return READER in self.kind

    @property
    def writes(self) -> bool:
        return WRITER in self.kind


def _op(name, kind, variants, effect, source, noisy_effect=None, **args):
    return Op(name, kind if isinstance(kind, tuple) else (kind,), variants, effect, effect if noisy_effect is None else noisy_effect, source, args)


_REBUILDS = "_engine.py bookkeeping: every entry point rebuilds; _mirror_holds"
_FOREIGN_READ = "_engine.py _mirror_holds(params): rebuilt from the caller's buffer"
_ADAM = "isdqn_hip.h ISDQN_BATCH_MIRROR_CURRENT: Adam writes both forms; _engine.py _noisy_learn"
_SOFT = "_engine.py soft_shift; isdqn_hip.h isdqn_net_soft_shift"
_ALONE = "that buffer alone"
_ALIAS = "_engine.py _wrote_without_mirror"

OPS = (
    # ---- readers
    _op("forward", READER, ALL, MAKES_CURRENT, _REBUILDS, INVALIDATES),
    _op("forward_foreign", READER, ALL, INVALIDATES, _FOREIGN_READ),
    _op("best_action", READER, ALL, MAKES_CURRENT, _REBUILDS, INVALIDATES),
    _op("best_actions", READER, ALL, MAKES_CURRENT, _REBUILDS + "; the flag is _mirror_is_current's", INVALIDATES),
    _op("loss_on_batch", READER, ALL, MAKES_CURRENT, _REBUILDS, INVALIDATES),
    _op("loss_on_batch_foreign", READER, ALL, INVALIDATES, _FOREIGN_READ),
    _op("loss_on_batch_target", READER, NOT_BN, MAKES_CURRENT, _REBUILDS + " (the target's first, then the online one)", INVALIDATES),
    _op("grad_on_batch", READER, ALL, MAKES_CURRENT, _REBUILDS, INVALIDATES),
    _op("grad_on_batch_target", READER, ALL, MAKES_CURRENT, _REBUILDS + " (the target's first, then the online one)", INVALIDATES),
    _op("analysis", READER, ALL, MAKES_CURRENT, _REBUILDS, INVALIDATES),
    _op("analysis_foreign", READER, ALL, INVALIDATES, _FOREIGN_READ),
    _op("learn_promised", (READER, WRITER), ALL, MAKES_CURRENT,
        "_engine.py make_batch(mirror_current=_mirror_is_current(None)), then as learn_on_batch", INVALIDATES),
    # ---- writers
    _op("learn_on_batch", WRITER, ALL, MAKES_CURRENT, _ADAM, INVALIDATES),
    _op("learn_on_batch_grad_out", WRITER, ALL, MAKES_CURRENT, _ADAM, INVALIDATES),
    _op("learn_on_batch_target", WRITER, NOT_BN, MAKES_CURRENT, _ADAM, INVALIDATES),
    _op("shift_params", WRITER, ALL, INVALIDATES, "_engine.py shift_params: the head rows moved in the master only"),
    _op("shift_params_foreign", WRITER, ALL, INVALIDATES, "the documents are silent on a foreign buffer: invalidates", target="foreign"),
    *[_op(f"soft_shift_{label}_{target}", WRITER, ALL, effect, source, noisy, tau=tau, target=target)
      for tau, label in ((0.0, "0"), (0.25, "025"), (1.0, "1"))
      for target, effect, noisy, source in (
          ("own", MAKES_CURRENT if tau == 1.0 else KEEPS, INVALIDATES if tau > 0 else KEEPS,
           _SOFT + (": the hard shift's route ends by rebuilding" if tau == 1.0 else "")),
          ("foreign", KEEPS, KEEPS, "_engine.py soft_shift: " + _ALONE),
          ("alias", INVALIDATES, INVALIDATES, _ALIAS))],
    _op("redo", WRITER, REDO, MAKES_CURRENT, "isdqn_hip.h isdqn_net_redo: ends by rebuilding the mirror"),
    _op("reset", WRITER, ALL, MAKES_CURRENT, "isdqn_hip.h isdqn_net_reset: ends by rebuilding the mirror; _engine.py reset", INVALIDATES),
    _op("reset_foreign", WRITER, ALL, KEEPS, "_engine.py reset: " + _ALONE, target="foreign"),
    _op("reset_alias", WRITER, ALL, INVALIDATES, _ALIAS, target="alias"),
    _op("ema_foreign", WRITER, ALL, KEEPS, "_engine.py ema: the mirror is not written", target="foreign"),
    _op("ema_alias", WRITER, ALL, INVALIDATES, _ALIAS, target="alias"),
    _op("import_flax", WRITER, ALL, INVALIDATES, "_engine.py bookkeeping (c): params.copy_ moves the version counter"),
    _op("params_mul_", WRITER, ALL, INVALIDATES, "_engine.py bookkeeping (c): a torch operation wrote the tensor"),
    _op("data_write_invalidate", WRITER, ALL, INVALIDATES, "_engine.py invalidate_mirror"),
    _op("rebuild_mirror", WRITER, ALL, MAKES_CURRENT, "_engine.py rebuild_mirror"),
    _op("commit_batch_stats", WRITER, BN, INVALIDATES, "the documents were silent: invalidates (now _engine.py commit_batch_stats)"),
    _op("compose", WRITER, NOISY, INVALIDATES, "_engine.py compose: the mirror now holds eff"),
)
BY_NAME = {op.name: op for op in OPS}
assert len(BY_NAME) == len(OPS)


def ops_of(variant):
    return [op for op in OPS if variant in op.variants]


def readers(variant):
    return [op for op in ops_of(variant) if op.reads]


def writers(variant):
    return [op for op in ops_of(variant) if op.writes]


def predict(variant, names, current=False):
    """The value of ``_mirror_is_current(None)`` on a trusted engine behind every op of ``names``, from the table alone (a new engine
    starts stale: nothing has built its mirror)."""
    out = []
    for name in names:
        effect = BY_NAME[name].effect_on(variant)
        current = True if effect == MAKES_CURRENT else False if effect == INVALIDATES else current
        out.append(current)
    return out


def table_markdown() -> str:
    """The table as DESIGN.md carries it."""
    lines = ["| op | kind | variants | effect | noisy engine | documented in |", "| --- | --- | --- | --- | --- | --- |"]
    for op in OPS:
        variants = "all" if op.variants == ALL else ", ".join(op.variants)
        lines.append(f"| `{op.name}` | {' + '.join(op.kind)} | {variants} | {op.effect} | {op.noisy_effect} | {op.source} |")
    return "\n".join(lines) + "\n"


# ---------------------------------------------------------------------------------------------------------------- walks
SEEDS = (0, 1)
# Every writer directly followed by every reader is (writers x readers) adjacent pairs, and a pair costs two ops: 25 x 12 = 300 pairs, 600
# ops on the plain variants.  The walks are that cover, a few trusted runs, every invalidating op once behind a raised flag (two ops
# each, 30 of them on the noisy variant) and random filler up to one common length.
N_OPS = 700
N_TRUSTED_RUNS = 6
MAX_REPEAT = 3


def _longest_repeat(names) -> int:
    best = run = 0
    for i, n in enumerate(names):
        run = run + 1 if i and names[i - 1] == n else 1
        best = max(best, run)
    return best


def walk(variant, seed, n_ops=N_OPS):
    """A seeded sequence of ``n_ops`` op names of ``variant``: every (writer, reader) pair once as neighbours, in shuffled order;
    ``N_TRUSTED_RUNS`` runs of three ops that leave the mirror current or as it is, each ending in a reader that takes the flag
    (``best_actions`` / ``learn_promised``) so that a trusted engine really skips a rebuild; every invalidating op once directly
    behind an op that makes the mirror current; and single random ops between them."""
    rng = random.Random(f"mirror-walk/{variant}/{seed}")
    pool = ops_of(variant)
    segments = [[w.name, r.name] for w in writers(variant) for r in readers(variant)]
    calm = [op.name for op in pool if op.effect_on(variant) in (MAKES_CURRENT, KEEPS)]
    starts = [op.name for op in pool if op.effect_on(variant) == MAKES_CURRENT]
    for _ in range(N_TRUSTED_RUNS):
        segments.append([rng.choice(starts), rng.choice(calm), rng.choice(calm), rng.choice(("best_actions", "learn_promised"))])
    # every op that invalidates, once directly behind an op that raised the flag: an op that forgets to lower it shows only then (on a
    # noisy engine hardly anything but rebuild_mirror raises it, so chance alone would never get there)
    segments += [[rng.choice(starts), op.name] for op in pool if op.effect_on(variant) == INVALIDATES]
    n_cover = sum(len(s) for s in segments)
    if n_cover > n_ops:
        raise ValueError(f"{variant}: the cover alone takes {n_cover} ops, n_ops = {n_ops}")
    segments += [[rng.choice(pool).name] for _ in range(n_ops - n_cover)]
    for _ in range(1000):
        rng.shuffle(segments)
        names = [n for s in segments for n in s]
        if _longest_repeat(names) <= MAX_REPEAT:
            return names
    raise ValueError(f"{variant}, seed {seed}: no order without a fourfold repeat")
