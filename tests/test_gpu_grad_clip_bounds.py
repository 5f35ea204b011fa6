"""Memory safety of gradient clipping (tests/test_gpu_bounds.py's child-process pattern): the bounds-checked build of the library
(-DISDQN_BOUNDS) runs forward / loss / learn / acting / gradient-only steps with max_grad_norm > 0 through scripts/bounds_check.py --
the headline plan and a dueling network -- with the new regions ("grad_clip_partials", "grad_clip") inside the registered workspace:
the loads of the first and the last slab of every position in grad_reduce_sq_kernel and grad_flat_sq_kernel (site 38), grad_clip_finalize_kernel's loads of the
partial sums (site 39) and every load of the Dense weight gradient that now goes through its slab must stay inside the tensors the
caller registered."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_load_of_a_clipped_step_leaves_the_tensors_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bounds_check.py"), "gc-"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 2 and all(r["case"].startswith("gc-") for r in rows), out.stdout
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent load in {r['case']}: site {r['site']} at {r['addr']}"
