"""Memory safety of the reset and EMA kernels (tests/test_gpu_noisy_bounds.py's child-process pattern): the bounds-checked build of the
library (-DISDQN_BOUNDS) runs resets of the engine's own parameters at three split layers, a reset of a target copy and two EMA calls
through scripts/reset_bounds_check.py -- the cnn case and the impala + BatchNorm case, whose tensor table is the longest the plan
builds -- with the exact extents of the buffers registered: every load and store of reset_kernel and the count store (site 46) and every
load and store of ema_kernel (site 47) must stay inside them."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_access_of_a_reset_or_an_ema_call_leaves_the_tensors_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "reset_bounds_check.py"), "reset-"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 2 and all(r["case"].startswith("reset-") for r in rows), out.stdout
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent access in {r['case']}: site {r['site']} at {r['addr']}"
