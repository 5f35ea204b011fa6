"""Memory safety of the soft head shift (tests/test_gpu_reset_bounds.py's child-process pattern): the bounds-checked build of the library
(-DISDQN_BOUNDS) runs isdqn_net_soft_shift through scripts/soft_shift_bounds_check.py on every configuration of
tests/helpers/soft_shift.py -- with and without a workspace, and on a noisy engine's sigma -- with the exact extents of heads 0 .. K of
the last Dense registered, in the master and in the weight mirror: every load and store of soft_shift_kernel (site 51) must stay inside
them.  The control, whose registration leaves out head K of the master, must record that site: the check is live."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import soft_shift as hs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_access_of_a_soft_shift_leaves_the_head_rows_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "soft_shift_bounds_check.py")], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [r["case"] for r in rows] == list(hs.CONFIGS) + ["noisy-f20-K3-scalar", "control-f20-K3-scalar"], out.stdout
    control = rows.pop()
    assert control["bad"] == 1 and control["site"] == 51, control
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent access in {r['case']}: site {r['site']} at {r['addr']}"
