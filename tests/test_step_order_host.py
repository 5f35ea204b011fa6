"""What stands behind the learn call of every agent's gradient step, eager and captured, against tests/golden/step_order_snapshot.txt,
without a GPU.  The order of the soft head shift, the prune apply, the projection, the mixture draw and the EMA is stated once per
agent (slimdqn/networks/_agent.py, ``_after_learn``) and read by the eager and by the captured step; a stage on
the wrong side of another, a key that does not say a node is there or a state tensor that is not announced fails no other CPU test.
The snapshot was recorded (oracle/make_golden_step_order.py) from commit 74ec7ce -- the order woven by hand into every agent, twice --
and is never regenerated from the code it is compared with: where the two disagree, the code is wrong.

(1) the tree reproduces every row of the grid of tests/helpers/step_order.py: the engine calls of the eager step, of the captured step
    and of iSDQN's learn_steps, the captured step's state and step count, the schedule clock ``_prune_t`` behind each;
(2) within a class two accepted rows have equal keys exactly when their captured steps have the same state and the same calls inside
    the learn call (the calls carry their taus and buffers).  ``_prune_t`` is left out of that comparison: it is the host's clock,
    not part of what is captured -- an agent whose schedule has pruned nothing yet replays the step of the agent without the option
    while its clock runs (tests/test_gpu_prune.py).  Rows are compared with rows of the same ``noisy``: a noisy agent's engine is
    another engine (``_graphed_update`` compares the engine beside the key), and the snapshot's own keys, the recorded commit's, do
    not say whether ``target_sigma`` follows the target;
(3) in every row the calls behind the learn call are the same sequence in the eager and in the captured step, and learn_steps is
    handed the key of update_online_params;
(4) every stage of the table in DESIGN.md section 6 appears in an accepted row of every class that has it."""
import itertools
import re

import pytest

from tests.helpers import step_order as so


@pytest.fixture(scope="module")
def golden():
    return so.read(open(so.GOLDEN).read())


@pytest.fixture(scope="module")
def recorded():
    return so.record()


def test_every_row_is_the_snapshot(golden, recorded):
    assert list(recorded) == list(golden), "the grid is not the one the snapshot was recorded from"
    bad = []
    for key, r in recorded.items():
        kind, text = golden[key]
        if (r["kind"], r["text"]) != (kind, text):
            bad.append(f"{' '.join(key)}: {r['kind']}\n{r['text']}\nthe snapshot holds: {kind}\n{text}")
    assert not bad, f"{len(bad)} rows differ; the first:\n" + "\n".join(bad[:3])


def test_two_keys_are_equal_exactly_when_the_captured_steps_are(recorded):
    n = 0
    for cls_name in so.CAPTURED:
        rows = [(key, r) for key, r in recorded.items() if key[0] == cls_name and r["kind"] == "ok"]
        for (ka, a), (kb, b) in itertools.combinations(rows, 2):
            if ("noisy=1" in ka[2]) != ("noisy=1" in kb[2]):
                continue  # (another engine, which _graphed_update compares beside the key: see (2) above)
            assert (a["key"] == b["key"]) == (a["told"] == b["told"]), (ka, a["key"], kb, b["key"])
            n += a["key"] != b["key"]
    assert n > 100  # (the grid does tell keys apart: both taus of the soft shift among them)
    shifts = {r["key"] for key, r in recorded.items() if key[0] == "iSDQN" and r["kind"] == "ok" and "shift=0 " not in key[2]}
    assert len(shifts) >= 2 * 4  # (two taus x nap x prune active or not)


def _behind_learn(calls):
    last = max(i for i, c in enumerate(calls) if ".learn_on_batch" in c)
    return [c for c in calls[last + 1:] if not c.endswith(".replay")]


def _lines(text):
    return dict(l.split(": ", 1) for l in text.splitlines())


def test_the_eager_and_the_captured_step_run_the_same_calls_behind_the_learn_call(golden, recorded):
    n = 0
    for key, (kind, text) in golden.items():
        if kind != "ok" or key[0] not in so.CAPTURED:
            continue
        lines = _lines(text)
        eager = _behind_learn(lines["(a) calls"].split(" "))
        for phase in ("(b)", "(c)") if key[0] == "iSDQN" else ("(b)",):
            calls = lines[f"{phase} calls"].split(" ")
            inside = calls[calls.index("[") + 1 : calls.index("]")]
            assert _behind_learn(inside) == eager, (key, phase)
            assert calls[calls.index("]") + 1 :] == [calls[-1]] and calls[-1].endswith(".replay"), (key, phase)  # nothing behind the capture but its replay
        assert recorded[key]["key3"] == recorded[key]["key"] or key[0] != "iSDQN", key
        n += 1
    assert n > 50


STAGES = {  # stage of the table -> a pattern over the calls of a row's eager step
    "projection in front of the soft shift": r"(learn|loss)_on_batch e1\.project_weights\(on=params\) e1\.soft_shift:0\.\d+\(on=params\)$",
    "soft shift": r"(learn|loss)_on_batch e1\.soft_shift:0\.25\(on=params\)$",
    "prune apply behind the soft shift": r"soft_shift:0\.5\(on=params\) e1\.prune_apply\(on=params\)$",
    "projection behind the prune apply": r"soft_shift:0\.5\(on=params\) e1\.prune_apply\(on=params\) e1\.project_weights\(on=params\)$",
    "prune apply": r"(learn|loss)_on_batch\S* e1\.prune_apply\(on=params\)",
    "projection": r"(learn|loss)_on_batch\S* (e1\.prune_apply\(on=params\) )?e1\.project_weights\(on=params\)",
    "prune apply, then projection": r"(learn|loss)_on_batch\S* e1\.prune_apply\(on=params\) e1\.project_weights\(on=params\)",
    "mixture draw": r"e1\.mixture_draw e1\.make_batch e1\.learn_on_batch_target\(target=target\)",
    "EMA behind everything": r"prune_apply\(on=params\) e1\.project_weights\(on=params\) e1\.ema:0\.005\(on=target,online=params\)$",
    "EMA of the noisy target": r"e1\.ema:0\.005\(on=target,online=params\) e1\.ema:0\.005\(on=target_sigma,online=sigma\)$",
}
SHIFT = ("projection in front of the soft shift", "soft shift", "prune apply behind the soft shift", "projection behind the prune apply")
COMMON = ("prune apply", "projection", "prune apply, then projection")
HAS = {"iSDQN": SHIFT + COMMON, "AnalysisDQN": SHIFT + COMMON, "TFDQN": COMMON, "AnalysisTFDQN": COMMON,
       "DQN": COMMON + ("mixture draw", "EMA behind everything", "EMA of the noisy target")}


@pytest.mark.parametrize("cls_name", list(HAS))
def test_every_stage_appears_in_an_accepted_row(golden, cls_name):
    eager = [_lines(text)["(a) calls"] for key, (kind, text) in golden.items() if key[0] == cls_name and kind == "ok"]
    assert eager
    for stage in HAS[cls_name]:
        assert any(re.search(STAGES[stage], calls) for calls in eager), stage
    for stage in set(STAGES) - set(HAS[cls_name]):  # (and the others' stages in none of its rows)
        if stage not in COMMON:
            assert not any(re.search(STAGES[stage], calls) for calls in eager), stage
