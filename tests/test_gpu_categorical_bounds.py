"""Memory safety of the categorical loss (tests/test_gpu_bounds.py's child-process pattern): the bounds-checked build of the library
(-DISDQN_BOUNDS) runs learn / loss / forward / acting / gradient-only steps with categorical = 1 on histogram heads of n_bins = 65 --
two atoms per lane, a ragged last group -- through scripts/bounds_check.py, with and without Double Q-learning and in the DQN form;
c51_loss_kernel's loads of the selector and value rows (sites 34 and 35) and every load of the generic head backward must stay inside
the tensors the caller registered."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_load_of_a_categorical_step_leaves_the_tensors_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bounds_check.py"), "c51-"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 3 and all(r["case"].startswith("c51-") and "nb65" in r["case"] for r in rows), out.stdout
    for r in rows:
        assert r["bad"] == 0, f"out-of-extent load in {r['case']}: site {r['site']} at {r['addr']}"
