"""Store flavours in the emitted gfx950 assembly (no GPU): the forward convolution kernels store their activations write-through
(WriteThroughDst in csrc/gemm_core.h), 16 bytes per lane, and nothing else in the library does; the -DISDQN_PLAIN_STORES build, which
tests/test_gpu_write_through_stores.py holds to the same bits, has no such store at all.

One activation store in the code per channel tile of 16 and pixel tile of 16: MT x 2 per image (the two-group kernels hold the stores
of both pixel tiles as well: which one a group finalizes is decided at run time), twice that in the two-image kernel."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))


def _expected(name):
    """Write-through 16-byte stores of the kernel with this demangled name."""
    m = re.match(r"conv_fwd_u8_pair_kernel<(\d+), \d+>", name)
    if m:
        return 2 * 2  # MT = 2, two pixel tiles
    if name.startswith("conv_fwd_s8_pair_kernel<"):
        return 2 * 4 * 2  # two images, MT = 4, two pixel tiles
    m = re.match(r"conv_fwd_img_kernel<(\d+), \d+, (true|false), \d+>", name)
    if m:
        return int(m.group(1)) * 2
    return 0


def _stores(path):
    """{demangled kernel name: [write-through 16-byte stores, other stores that carry sc1]} of every kernel in the file."""
    text = open(path).read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m:
            cur = m.group(1) if m.group(1) in kernels else None
            if cur:
                out[cur] = [0, 0]
            continue
        if cur is None or not line.startswith("\t"):
            continue
        code = line.split(";")[0]
        if "_store_" not in code or not re.search(r"\bsc1\b", code):
            continue
        out[cur][0 if re.search(r"\b(buffer|global)_store_dwordx4\b", code) else 1] += 1
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    short = lambda d: re.sub(r"\(.*", "", d).replace("isdqn::", "").replace("void ", "")
    return {short(d): v for d, v in zip(names, out.values())}


@pytest.fixture(scope="module")
def build():
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import build

    return build


def test_forward_convolutions_store_activations_write_through_and_nothing_else_does(build):
    seen = {}
    for path in (build.emit_asm() + build.emit_side_asm() + build.emit_prune_asm() + build.emit_mixture_asm() + build.emit_project_asm()):
        seen.update(_stores(path))
    assert sum(k.startswith("conv_fwd_") for k in seen) >= 13, sorted(seen)
    wrong = {k: v for k, v in seen.items() if v != [_expected(k), 0]}
    assert not wrong, wrong
    assert seen["conv_fwd_u8_pair_kernel<2, 8>"] == [4, 0] and seen["conv_fwd_s8_pair_kernel<8>"] == [16, 0]
    assert seen["conv_fwd_img_kernel<4, 3, false, 1>"] == [8, 0] and seen["conv_fwd_img_kernel<4, 3, false, 2>"] == [8, 0]


def test_plain_stores_build_has_no_write_through_store(build):
    (path,) = build.emit_asm(sources=["net_kernels.hip"], variant="plain", defines=("ISDQN_PLAIN_STORES",))
    seen = _stores(path)
    assert sum(k.startswith("conv_fwd_") for k in seen) >= 13, sorted(seen)
    assert all(v == [0, 0] for v in seen.values()), {k: v for k, v in seen.items() if v != [0, 0]}
