"""Memory safety of the distributional loss kernels off R = 4 (tests/test_gpu_bounds.py's child-process pattern): the bounds-checked
build of the library (-DISDQN_BOUNDS) runs learn / loss / forward / acting / gradient-only steps through scripts/bounds_check.py on four
rows of tests/helpers/head_geometry.py's table -- HL-Gauss on workgroups of 3 + 2 transitions (with the conservative term on the same
partition), C51 on 2 + 2 + 1 at A = 1, the quantile loss on one transition per workgroup at A = 1, and the widest head row the plan takes
(5456 outputs) -- and every checked load must stay inside the tensors the caller registered."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"geo-hl-r3-ragged", "geo-c51-r2", "geo-qr-r1", "geo-hl-widest"}


def test_no_load_of_a_step_off_four_rows_per_workgroup_leaves_the_tensors_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bounds_check.py"), "geo-"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 4 and {r["case"] for r in rows} == CASES, out.stdout
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent load in {r['case']}: site {r['site']} at {r['addr']}"
