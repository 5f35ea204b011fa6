"""Memory safety of the random-shift augmentation (tests/test_gpu_bounds.py's child-process pattern): the bounds-checked build of the
library (-DISDQN_BOUNDS) runs the kernel shapes of tests/test_gpu_augment.py -- the 16-byte path, the byte path with odd frame bases, a
pad larger than the frame on both paths -- and one learn step on an augmented batch through scripts/augment_bounds_check.py, with the
exact extents of the frame store, the id table, the counter, the scratch pool and the out table registered (the store ends with its last
frame's last pixel): the id loads of augment_shift_kernel (site 43), the counter loads of both kernels (site 44) and the source-frame
loads of both paths (site 45) must stay inside them, and so must every load of the learn step that reads the pool through the table."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_load_of_the_augmentation_leaves_the_buffers_it_was_given():
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = build.build(verbose=False, variant="bounds", defines=("ISDQN_BOUNDS",))  # (no-op when the build is current)
    env = dict(os.environ, ISDQN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "augment_bounds_check.py"), "augment-"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 6 and all(r["case"].startswith("augment-") for r in rows), out.stdout
    control = [r for r in rows if "control" in r["case"]]
    assert len(control) == 1 and control[0]["bad"] == 1 and control[0]["site"] == 44, f"the check does not see an unregistered load: {control}"
    for r in rows:
        if r not in control:
            assert r["bad"] == 0, f"out-of-extent load in {r['case']}: site {r['site']} at {r['addr']}"
