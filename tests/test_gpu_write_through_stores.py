"""Write-through activation stores of the forward convolutions (WriteThroughDst in csrc/gemm_core.h: a buffer per image, a byte
offset per lane) against the plain stores they replace (the -DISDQN_PLAIN_STORES build of the same sources): bit for bit.

Method of tests/test_gpu_conv0_image_kernel.py: one child process per library (ISDQN_HIP_LIB), one after the other, fingerprints of
scripts/conv0_bits.py's CASES (SHA-256 of params, Adam moments, losses, q-values, targets and priorities after three learn steps, of
the loss-only pass and of a one-row forward; the two children run once for the whole module).  A store that lands in another row,
is dropped by the buffer's bound or is skipped by a lane changes the next layer's input and with it every fingerprint.

CASES holds the shapes where such a store can go wrong: 48 / 52 / 64 pixel observations with a nearly empty last tile (lanes without
a pixel), 104 pixels (three halves per image), B = 1 and 3 (an unpaired image in the two-image kernel's place), first-layer widths 7
and 16 (a channel group that is not full, lanes of a pair that skip), LayerNorm on and off, both precisions; the 68 pixel case runs
the one-tile kernel's store.  The second and third layers (widths 8) store through conv_fwd_img_kernel in every case."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from conv0_bits import CASES  # noqa: E402


def _variant(name, define):
    sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
    import build

    lib = os.path.join(build.LIBDIR, "libisdqn_hip_%s.so" % name)
    return lib if os.path.exists(lib) else build.build(verbose=False, variant=name, defines=(define,))


def _child(lib):
    import build

    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "conv0_bits.py")], env=dict(os.environ, ISDQN_HIP_LIB=lib or build.LIB),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def fingerprints():
    out = []
    for lib in (_variant("plain", "ISDQN_PLAIN_STORES"), None):
        lines = _child(lib).stdout.splitlines()
        out.append({l.split(":")[0]: l for l in lines if ": params " in l})
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_write_through_stores_are_bit_identical_to_plain_stores(fingerprints, case):
    plain, product = fingerprints
    assert case in plain and case in product
    assert product[case] == plain[case]
