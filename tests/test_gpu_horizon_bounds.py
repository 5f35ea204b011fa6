"""Memory safety of the horizon windows (tests/test_gpu_augment_bounds.py's child-process pattern): the bounds-checked build of the
library (-DISDQN_BOUNDS) runs isdqn_replay_gather_horizon and isdqn_replay_apply_staged_horizon through
scripts/horizon_bounds_check.py with the exact extents of their buffers registered -- first and last slot, ragged B, m = n_max and a
clamped horizon, with and without the index table -- and one learn, loss and gradient step with a registered discount tensor on the
headline head chain, a tiny td_kernel case and a C51 case: the gather's loads (site 48), the scatter's (site 49) and the discount loads of
the loss kernels (site 50) must stay inside them."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_load_of_the_horizon_kernels_leaves_the_buffers_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "horizon_bounds_check.py"), "horizon-"], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 9 and all(r["case"].startswith("horizon-") for r in rows), out.stdout
    control = [r for r in rows if "control" in r["case"]]
    assert len(control) == 1 and control[0]["bad"] == 1 and control[0]["site"] == 48, f"the check does not see an unregistered load: {control}"
    for r in rows:
        if r not in control:
            assert r["bad"] == 0, f"out-of-extent load in {r['case']}: site {r['site']} at {r['addr']}"
