"""Memory safety of the noisy Dense layers (tests/test_gpu_bounds.py's child-process pattern): the bounds-checked build of the library
(-DISDQN_BOUNDS) runs sample, compose, two noisy learn steps, a loss pass and acting on the composed parameters through
scripts/noisy_bounds_check.py -- the fc step, its DQN form (a second draw and a second composed buffer) and the headline step -- with the
exact extents of the new caller-owned buffers registered (sigma and its moments, noise, eff, grad, noise_count): the counter load of
noisy_sample_kernel (site 40), the parameter / sigma / noise-vector loads of noisy_compose_kernel (site 41) and every load of
noisy_adam_kernel (site 42) must stay inside them, and so must every load of the existing gradient pass on the composed parameters."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_load_of_a_noisy_step_leaves_the_tensors_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "noisy_bounds_check.py"), "noisy-"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 3 and all(r["case"].startswith("noisy-") for r in rows), out.stdout
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent load in {r['case']}: site {r['site']} at {r['addr']}"
