"""Record tests/golden/plan_snapshot.txt: the host-side plan (csrc/net_plan.h) of every configuration of tests/helpers/plan_grid.py
and what the C ABI's three layout entry points say about the accepted ones.

The snapshot pins a refactor of the plan builder, so it is recorded from the code BEFORE the refactor and never from the tree that
is held to it: pass the `csrc` directory of a checkout of that commit, with its library built next to it
(python is-dqn_amd/build.py in that checkout).  The dumper and the grid are this tree's.

Usage:  python oracle/make_golden_plan.py <checkout>/is-dqn_amd/csrc        (CPU, seconds)
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = os.path.abspath(sys.argv[1])
os.environ["ISDQN_HIP_LIB"] = os.path.join(os.path.dirname(csrc), "lib", "libisdqn_hip.so")
sys.path[:0] = [ROOT, os.path.join(ROOT, "is-dqn_amd")]
from slimdqn import _hip  # noqa: E402
from tests.helpers import plan_grid as pg  # noqa: E402

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "plan_dump")
    assert pg.compile_dumper(csrc, exe).wait() == 0
    text = pg.snapshot(lambda lines: pg.run_dumper(exe, lines), _hip.lib())
with open(pg.GOLDEN, "w") as f:
    f.write(text)
print(f"{pg.GOLDEN}: {len(text)} bytes, {len(pg.valid_grid())} + {len(pg.refusal_grid())} configurations, {len(pg.full_text_grid())} in full")
