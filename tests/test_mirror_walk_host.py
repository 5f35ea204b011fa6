"""The walks of tests/helpers/mirror_walk.py against the conditions that keep tests/test_gpu_mirror_coherence.py from hiding a path, from
the op table alone (no GPU): for every (variant, seed) the GPU test runs, every applicable writer is directly followed by every
applicable reader at least once, the walk holds a run of three ops that leave the mirror current or alone -- so a trusted reader
behind it really skips a rebuild --, no op stands more than three times in a row, and every op that invalidates runs at least once
where the table calls the mirror current.

A (writer, reader) pair as neighbours costs two ops and there are 25 x 12 of them on the plain variants, so a walk that holds them all
is about 700 ops long (mirror_walk.N_OPS), not 150; on the GPU a walk of that length takes well under a second."""
import os

import pytest

from tests.helpers import mirror_walk as mw
from tests.helpers import options_grid

CASES = [(v, s) for v in mw.VARIANTS for s in mw.SEEDS]


def test_the_table_is_well_formed():
    assert (mw.N_ACTIONS, mw.K, mw.BATCH) == (options_grid.N_ACTIONS, options_grid.K, options_grid.BATCH)
    for name in ("cnn-ln", "cnn-hl51", "cnn-bn"):
        t = options_grid.TORSOS["cnn_bn" if name == "cnn-bn" else "cnn"]
        assert (mw.VARIANTS[name]["obs"], list(mw.VARIANTS[name]["features"])) == (t["obs"], t["features"])
    for name in ("fc", "fc-noisy"):
        t = options_grid.TORSOS["fc"]
        assert (mw.VARIANTS[name]["obs"], list(mw.VARIANTS[name]["features"])) == (t["obs"], t["features"])
    for op in mw.OPS:
        assert op.kind and set(op.kind) <= {mw.READER, mw.WRITER}, op.name
        assert op.variants and set(op.variants) <= set(mw.VARIANTS), op.name
        assert {op.effect, op.noisy_effect} <= {mw.MAKES_CURRENT, mw.KEEPS, mw.INVALIDATES}, op.name
        assert op.source, op.name
    # what the library refuses is not in a variant's column
    assert "redo" not in {op.name for op in mw.ops_of("fc-noisy")} and "redo" not in {op.name for op in mw.ops_of("cnn-bn")}
    assert not {"learn_on_batch_target", "loss_on_batch_target"} & {op.name for op in mw.ops_of("cnn-bn")}
    assert "commit_batch_stats" in {op.name for op in mw.ops_of("cnn-bn")} and "compose" in {op.name for op in mw.ops_of("fc-noisy")}
    # the issue's lists: 12 readers; 9 soft shifts, 3 resets, 2 EMAs, 2 shifts among the writers; the three aliasing paths invalidate
    assert len(mw.readers("cnn-ln")) == 12 and len(mw.writers("cnn-ln")) == 25
    assert sum(op.name.startswith("soft_shift_") for op in mw.OPS) == 9
    for name in ("soft_shift_0_alias", "soft_shift_025_alias", "soft_shift_1_alias", "reset_alias", "ema_alias"):
        assert mw.BY_NAME[name].effect == mw.BY_NAME[name].noisy_effect == mw.INVALIDATES


def test_predict_follows_the_effects():
    assert mw.predict("fc", ["forward", "soft_shift_025_own", "ema_foreign", "shift_params", "reset_foreign", "redo"]) == [True, True, True, False, False, True]
    assert mw.predict("fc-noisy", ["forward", "rebuild_mirror", "soft_shift_0_own", "soft_shift_025_own"]) == [False, True, True, False]


@pytest.mark.parametrize("variant,seed", CASES)
def test_walk_covers_every_writer_reader_pair(variant, seed):
    names = mw.walk(variant, seed)
    assert len(names) == mw.N_OPS and names == mw.walk(variant, seed)  # (seeded: the GPU test walks these very ops)
    applicable = {op.name for op in mw.ops_of(variant)}
    assert set(names) == applicable
    neighbours = set(zip(names, names[1:]))
    missing = [(w.name, r.name) for w in mw.writers(variant) for r in mw.readers(variant) if (w.name, r.name) not in neighbours]
    assert not missing, f"{len(missing)} (writer, reader) pairs never stand next to each other, e.g. {missing[:5]}"


@pytest.mark.parametrize("variant,seed", CASES)
def test_walk_holds_a_trusted_run_and_no_long_repeat(variant, seed):
    names = mw.walk(variant, seed)
    calm = [mw.BY_NAME[n].effect_on(variant) in (mw.MAKES_CURRENT, mw.KEEPS) for n in names]
    current = mw.predict(variant, names)
    # three calm ops in a row that end with a current mirror, and directly behind them a reader whose rebuild the flag decides
    runs = [i for i in range(3, len(names)) if all(calm[i - 3:i]) and current[i - 1] and names[i] in ("best_actions", "learn_promised")]
    assert runs, "no run of three makes_current / keeps ops in front of a reader that takes the flag"
    assert mw._longest_repeat(names) <= mw.MAX_REPEAT
    assert mw._longest_repeat(["a", "b", "b", "b", "b", "c"]) == 4


@pytest.mark.parametrize("variant,seed", CASES)
def test_every_invalidating_op_meets_a_raised_flag(variant, seed):
    """An op that forgets to lower the flag shows only where the flag was up in front of it."""
    names = mw.walk(variant, seed)
    current = [False] + mw.predict(variant, names)
    met = {n for i, n in enumerate(names) if current[i]}
    missing = [op.name for op in mw.ops_of(variant) if op.effect_on(variant) == mw.INVALIDATES and op.name not in met]
    assert not missing, f"never run on a mirror the table calls current: {missing}"


def test_walks_of_two_seeds_differ():
    for variant in mw.VARIANTS:
        assert mw.walk(variant, mw.SEEDS[0]) != mw.walk(variant, mw.SEEDS[1])


def test_design_document_carries_the_table():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md")) as f:
        text = f.read()
    assert mw.table_markdown() in text, "DESIGN.md section 3 does not hold tests/helpers/mirror_walk.py's table_markdown()"
