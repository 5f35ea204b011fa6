"""Record tests/golden/kernel_order.txt: the kernel symbols of each of the four sources, in the order the device assembly of the
product flags defines them (build.emit_asm(), cached by mtime).

The plain learn step's kernels keep their places in the code object (docs/NOTEBOOK.md, NoisyNet and augmentation entries): new
kernels go behind every kernel the code object had, and the templated ones follow the order in which host code first names each
instantiation.  The snapshot pins that order, so it is recorded from the commit BEFORE a change that must not move a kernel and never
from the tree that is held to it: pass the `is-dqn_amd` directory of a checkout of that commit.  A change that adds kernels on purpose
records it from its own tree and shows in the diff of the fixture that the new names are the last of their source.

Usage:  python oracle/make_golden_kernel_order.py [<checkout>/is-dqn_amd]        (CPU, about 75 s when nothing is cached)
"""
import importlib.util
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_order.txt")


def kernel_order_text(pkg_dir=os.path.join(ROOT, "is-dqn_amd")):
    """`[source]` and then one kernel symbol per line, for every source of build.SOURCES in its order.  Names and order only."""
    spec = importlib.util.spec_from_file_location("isdqn_build_order", os.path.join(pkg_dir, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    out = []
    for src, asm in zip(build.SOURCES, build.emit_asm()):
        out.append(f"[{src}]")
        out += re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(asm).read(), re.M)
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    text = kernel_order_text(*[os.path.abspath(a) for a in sys.argv[1:2]])
    with open(GOLDEN, "w") as f:
        f.write(text)
    print(f"{GOLDEN}: {text.count(chr(10)) - text.count('[')} kernels")
