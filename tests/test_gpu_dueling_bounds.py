"""Memory safety of the dueling heads (tests/test_gpu_bounds.py's child-process pattern): the bounds-checked build of the library
(-DISDQN_BOUNDS) runs forward / loss / learn / acting / gradient-only steps with dueling = 1 through scripts/bounds_check.py, one case
per head kind -- scalar (iS-DQN and the Double DQN form), histogram with Munchausen targets, categorical in the Double DQN form, quantile
-- with the new regions ("head_raw", "head_raw_target", "dout_raw", "dbh_raw") inside the registered workspace: duel_combine_kernel's
loads of the raw rows (site 36), duel_backward_kernel's loads of dout / dbh (site 37) and every load of the generic head backward at the
raw width must stay inside the tensors the caller registered."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_load_of_a_dueling_step_leaves_the_tensors_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bounds_check.py"), "duel-"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 5 and all(r["case"].startswith("duel-") for r in rows), out.stdout
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent load in {r['case']}: site {r['site']} at {r['addr']}"
