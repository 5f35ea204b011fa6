"""Record tests/golden/options_snapshot.txt: what every agent constructor hands to QNetEngine and what QNetEngine writes into
isdqn_net_config, or which refusal answers first, over the grid of tests/helpers/options_grid.py.

The snapshot pins a refactor of the option plumbing (slimdqn/_engine.py, slimdqn/networks/), so it is recorded from the code BEFORE
the refactor and never from the tree that is held to it: pass the `is-dqn_amd` directory of a checkout of that commit.  The grid and
the two recorders are this tree's; nothing is built and nothing needs a GPU.

Usage:  python oracle/make_golden_options.py <checkout>/is-dqn_amd        (CPU, seconds)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.abspath(sys.argv[1])]
from tests.helpers import options_grid as og  # noqa: E402

agents, engine = og.record_agents(), og.record_engine()
text = og.snapshot(agents, engine)
with open(og.GOLDEN, "w") as f:
    f.write(text)
print(f"{og.GOLDEN}: {len(text)} bytes, {len(agents)} + {len(engine)} rows, "
      f"{sum(k == 'ok' for k, _ in list(agents.values()) + list(engine.values()))} accepted")
