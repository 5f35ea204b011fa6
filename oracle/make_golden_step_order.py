"""Record tests/golden/step_order_snapshot.txt: which engine calls a gradient step of every agent makes, eager and captured, in which
order and on which buffer, over the grid of tests/helpers/step_order.py.

The snapshot pins the refactor that states what follows an agent's learn call once (slimdqn/networks/_agent.py, ``_after_learn``), so
it is recorded from the code BEFORE that refactor and never from the tree that is held to it: pass the `is-dqn_amd` directory of a
checkout of that commit.  The grid and the stand-ins are this tree's; nothing is built and nothing needs a GPU.

Usage:  python oracle/make_golden_step_order.py <checkout>/is-dqn_amd        (CPU, seconds)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.abspath(sys.argv[1])]
from tests.helpers import step_order as so  # noqa: E402

recorded = so.record()
text = so.snapshot(recorded)
with open(so.GOLDEN, "w") as f:
    f.write(text)
print(f"{so.GOLDEN}: {len(text)} bytes, {len(recorded)} rows, {sum(r['kind'] == 'ok' for r in recorded.values())} accepted, "
      f"{len(set(r['text'] for r in recorded.values() if r['kind'] == 'ok'))} distinct records")
