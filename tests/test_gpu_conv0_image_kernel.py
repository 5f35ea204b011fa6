"""First convolution, one workgroup per image with resident weights (csrc/conv_u8_pair.h), against the one-tile kernel it replaces
(conv_fwd_img_kernel<2, PASSES, true>, the -DISDQN_NO_U8_PAIR build of the same sources) at the small shapes where its index
arithmetic takes another path: bit for bit.

Method of tests/test_gpu_network.py::test_first_layer_pair_kernel_is_bit_identical_to_the_one_tile_kernel: one child process per
library (ISDQN_HIP_LIB), one after the other, SHA-256 of params, Adam moments, losses, q-values, targets and priorities after three
learn steps, of the loss-only pass and of a one-row forward (scripts/conv0_bits.py; the two children run once for the whole module).

Observation sizes.  The torso pads SAME: an S x S observation gives ceil(S / 4)^2 output pixels, so 84 x 84 is 21 x 21 = 441 pixels
(four tiles, the last with 57), 68 x 68 is 17 x 17 = 289 (THREE tiles: the shape the route must refuse; it runs on the one-tile kernel
and matches trivially) and 52 x 52 is 13 x 13 = 169 (two tiles, the second with 41).  The layouts a VALID convolution would give those
three sizes -- exactly two full tiles with no dead wave, two tiles with 16 pixels in the second -- are 64 x 64 (256 pixels) and 48 x 48
(144 pixels) here; 104 x 104 (676 pixels, six tiles) runs the loop over more than two halves.  Every case carries frame-id rows with
negative ids (zero frames) in both halves of the id table and the last frame of the store."""
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


def _child(lib, cases=(), env=None):
    import build

    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "conv0_bits.py"), *cases],
                       env=dict(os.environ, ISDQN_HIP_LIB=lib or build.LIB, **(env or {})), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def fingerprints():
    out = []
    for lib in (_variant("nopair", "ISDQN_NO_U8_PAIR"), None):
        lines = _child(lib).stdout.splitlines()
        out.append({l.split(":")[0]: l for l in lines if ": params " in l})
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_image_kernel_is_bit_identical_to_the_one_tile_kernel(fingerprints, case):
    one_tile, image = fingerprints
    assert case in one_tile and case in image
    assert image[case] == one_tile[case]


@pytest.mark.parametrize("case,taken", [("84-four-tiles-last-57px", True), ("68-three-tiles-refused", False)])
def test_route(case, taken):
    """The development build names the kernels it launches (ISDQN_DEBUG_OCCUPANCY): the 84 x 84 network takes the image kernel at two
    workgroups per CU, the three-tile shape the one-tile kernel."""
    err = _child(_variant("dev", "ISDQN_DEV"), [case], {"ISDQN_DEBUG_OCCUPANCY": "1"}).stderr
    pair = [l for l in err.splitlines() if "launch_conv_fwd_u8_pair" in l]
    assert bool(pair) == taken, err[-2000:]
    if taken:
        assert all("x 512 threads" in l and l.rstrip().endswith("-> 2 workgroups per CU") for l in pair), pair
    else:
        assert any("launch_conv_fwd_img" in l and "U8 = true" in l for l in err.splitlines()), err[-2000:]
