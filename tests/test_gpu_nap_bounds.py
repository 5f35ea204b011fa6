"""Memory safety of the projection kernels (tests/test_gpu_prune_bounds.py's child-process pattern): the bounds-checked build of the
library (-DISDQN_BOUNDS) runs isdqn_net_project_norms and isdqn_net_project_apply through scripts/nap_bounds_check.py on the fc [20, 14]
and the cnn configuration of tests/helpers/prune.py -- with and without a workspace -- with the exact extents of the projected kernels
registered in the master and in the weight mirror, beside the target norms, the norms, the scales and the scratch: every load and store of
the three kernels (site 58) must stay inside them.  The control, whose registration leaves out the master's last projected kernel, must
record that site: the check is live."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_access_of_a_projection_call_leaves_the_kernels_and_vectors_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "nap_bounds_check.py")], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [r["case"] for r in rows] == ["fc-20-14", "cnn", "control-fc-20-14"], out.stdout
    control = rows.pop()
    assert control["bad"] == 1 and control["site"] == 58, control
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent access in {r['case']}: site {r['site']} at {r['addr']}"
