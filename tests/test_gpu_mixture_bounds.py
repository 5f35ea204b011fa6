"""Memory safety of the mixture's kernels (tests/test_gpu_prune_bounds.py's child-process pattern): the bounds-checked build of the library
(-DISDQN_BOUNDS) runs the draw, the loss and learn calls of both forms and the mean-heads acting call through
scripts/mixture_bounds_check.py on fc H = 3, A = 5, B = 5 on fc H = 200, A = 18, B = 8 with double_q and on fc H = 2, A = 70, B = 5 with double_q (A > 64: the chunked path), with the exact extents of
every tensor registered: the count (site 53), alpha (54), the head-output rows (55), the discounts (56) and the "q" rows of the acting
call (57) must stay inside them, like every operand load of the steps around them.  The control, whose registration leaves out alpha's
last element, must record site 54: the check is live."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_load_of_a_mixture_call_leaves_the_tensors_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "mixture_bounds_check.py")], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [r["case"] for r in rows] == ["fc-H3-A5-B5", "fc-H200-A18-B8-double_q", "fc-H2-A70-B5-double_q", "control-fc-H3-A5-B5"], out.stdout
    control = rows.pop()
    assert control["bad"] == 1 and control["site"] == 54, control
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent access in {r['case']}: site {r['site']} at {r['addr']}"
