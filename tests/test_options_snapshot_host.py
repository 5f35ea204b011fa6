"""The option plumbing of the agents and the engine against tests/golden/options_snapshot.txt, without a GPU.  Between a constructor's
keywords and isdqn_net_config nothing computes: a swapped pair of arguments or a refusal that answers in another order fails no other
CPU test.  The snapshot was recorded (oracle/make_golden_options.py) from commit bcb845e3b057 -- the hand-threaded plumbing, before the
options became one value (slimdqn/_engine.py, NetOptions); it is never regenerated from the code it is compared with -- where the two
disagree, the code is wrong.

(a) [agents]: the five agent classes over the grid of tests/helpers/options_grid.py (torso x all-off, every setting, every pair): the
    arguments handed to QNetEngine, bound to its real signature, or the type and message of the exception;
(b) [engine]: QNetEngine called directly over the same grid: every field of the isdqn_net_config it fills, or the exception;
(c) the snapshot itself: every refusal a constructor can raise wins somewhere, every class x torso has an accepted row."""
import pytest

from tests.helpers import options_grid as og

HASH_ONLY = "the snapshot holds its SHA-256 only: record this row from the recorded commit to see the field"


@pytest.fixture(scope="module")
def golden():
    agents, engine, full = og.read(open(og.GOLDEN).read())
    return dict(agents=agents, engine=engine, full=full)


def differences(section, outcomes, golden):
    """One paragraph per row that is not the snapshot's: the row key and both sides, in full wherever the text exists."""
    want_rows, full = golden[section], golden["full"]
    assert list(outcomes) == list(want_rows), "the grid is not the one the snapshot was recorded from"
    out = []
    for key, (kind, text) in outcomes.items():
        want_kind, want = want_rows[key]
        name = f"[{section}] {' '.join(key)}"
        if kind == "err":
            if (kind, text) != (want_kind, want):
                kept = full.get((section,) + key, HASH_ONLY)
                out.append(f"{name}: refused with\n  {text}\nthe snapshot holds " + (f"the refusal\n  {want}" if want_kind == "err" else f"the record\n{kept}"))
        elif want_kind == "err":
            out.append(f"{name}: accepted with the record\n{text}the snapshot holds the refusal\n  {want}")
        elif og.sha(text) != want:
            kept = full.get((section,) + key)
            out.append(f"{name}: the record\n{text}is not the snapshot's" + (f" ({HASH_ONLY})" if kept is None else f", which holds (an all-off row in full, else the "
                       f"fields that differ from it)\n{kept}and of this row those are\n{og.full_text(outcomes, key)}"))
        elif (section,) + key in full:
            assert og.full_text(outcomes, key) == full[(section,) + key], name  # (same SHA-256: the text section is damaged)
    return out


def test_what_every_agent_hands_to_the_engine_is_the_snapshot(golden):
    bad = differences("agents", og.record_agents(), golden)
    assert not bad, f"{len(bad)} rows differ; the first:\n" + "\n".join(bad[:3])


def test_the_net_config_the_engine_fills_is_the_snapshot(golden):
    bad = differences("engine", og.record_engine(), golden)
    assert not bad, f"{len(bad)} rows differ; the first:\n" + "\n".join(bad[:3])


def test_every_accepted_all_off_and_single_setting_row_is_kept_as_text(golden):
    for section in ("agents", "engine"):
        for key, (kind, _) in golden[section].items():
            assert ((section,) + key in golden["full"]) == (kind == "ok" and "+" not in key[-1]), (section, key)


def test_every_refusal_a_constructor_can_raise_wins_somewhere(golden):
    from slimdqn import _engine
    from slimdqn.networks import _agent, tfdqn

    # recycle_dormant / redo raise these three, no constructor does
    not_constructors = {"NOISY_REDO_REFUSED", "REDO_IMPALA_REFUSED", "REDO_BATCH_NORM_REFUSED"}
    constants = {k: v for k, v in vars(_engine).items() if k.isupper() and isinstance(v, str) and ("REFUSED" in k or "NEEDS" in k)}
    assert len(constants) == 22 and not_constructors < set(constants)
    for name in not_constructors:
        del constants[name]
    constants.update(EMA_REFUSED=_agent.EMA_REFUSED, DOUBLE_Q_REFUSED=tfdqn.DOUBLE_Q_REFUSED,
                     ema_range="ema_tau must be in [0, 1] (0 = off: hard target updates)",
                     analysis_double_q="AnalysisDQN: double_q with batch_norm is not built (ISDQN_ERR_UNSUPPORTED with target parameters)")
    for section, must in (("agents", constants), ("engine", {k: v for k, v in constants.items() if v in vars(_engine).values() and not k.startswith("AUGMENT")})):
        won = {m.split(": ", 1)[1] for kind, m in golden[section].values() if kind == "err"}
        assert {k for k, v in must.items() if v not in won} == set(), section
    assert _engine.AUGMENT_PAD_REFUSED in constants.values()  # (check_augment's range error is one of the constants)


def test_every_class_and_torso_has_an_accepted_row(golden):
    accepted = {key[:-1] for key, (kind, _) in golden["agents"].items() if kind == "ok"}
    assert accepted == set(og.agent_cells()) and len(accepted) == 5 * 7 - 1  # (DQN takes no batch_norm)
    assert {key[:-1] for key, (kind, _) in golden["engine"].items() if kind == "ok"} == {(t,) for t in og.TORSOS}
