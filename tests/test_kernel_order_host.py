"""The order of the kernels in each source's code object against tests/golden/kernel_order.txt, without a GPU.  The kernels of the
plain learn step keep their places (docs/NOTEBOOK.md, NoisyNet and augmentation entries): a new kernel goes behind every kernel its
code object had, and a templated kernel sits where host code first names its instantiation -- so a host-only edit can move one.
The snapshot was recorded (oracle/make_golden_kernel_order.py) from the single-file net_kernels.hip before it was split by concern;
it is never regenerated from a tree that claims to have moved nothing.  Names and order only: no instruction is inspected."""
import os

import pytest

from oracle.make_golden_kernel_order import GOLDEN, kernel_order_text

REGENERATE = ("a change that must move no kernel is wrong here; one that adds kernels on purpose appends them and records the file again: "
              "python oracle/make_golden_kernel_order.py")


def sections(text):
    out = {}
    for line in text.splitlines():
        if line.startswith("["):
            out[line] = cur = []
        else:
            cur.append(line)
    return out


def test_every_kernel_is_where_the_snapshot_has_it():
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    got, want = sections(kernel_order_text()), sections(open(GOLDEN).read())
    assert list(got) == list(want), "the sources are not the ones the snapshot was recorded from"
    assert sum(len(v) for v in want.values()) >= 180 and len(want["[net_kernels.hip]"]) >= 150
    for src in want:
        g, w = got[src], want[src]
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, (f"{src}: kernel {i + 1} of {len(g)} is {a}, the snapshot holds {b} there"
                            f"{' (now kernel %d)' % (g.index(b) + 1) if b in g else ' (gone)'}; {REGENERATE}")
        assert len(g) == len(w), f"{src}: {len(g)} kernels, the snapshot holds {len(w)}; the first one without a partner: {max(g, w, key=len)[min(len(g), len(w)):][:1]}; {REGENERATE}"
