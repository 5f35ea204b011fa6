"""Build libisdqn_hip.so (the C-ABI HIP library) in-tree for gfx950.

    python is-dqn_amd/build.py [--force]

hipcc cross-compiles without a GPU; the .so is git-ignored but travels with gpurun snapshots.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libisdqn_hip.so")
SOURCES = ["api.hip", "tree_kernels.hip", "replay_kernels.hip", "net_kernels.hip"]
# Translation units beside the four whose kernels and kernel order tests/golden/kernel_order.txt pins: compiled and linked into every
# variant, and behind the four in emit_asm()'s list (scripts/isa_lint.py reads them all).
EXTRA_SOURCES = ["conservative_kernels.hip"]
# Further translation units of their own (tests/test_conservative_host.py holds the two lists above to what they are): compiled and linked
# into every variant like the others; their assembly comes from emit_side_asm(), which tests/test_soft_shift_host.py lints.
SIDE_SOURCES = ["soft_shift_kernels.hip"]
# Gradual magnitude pruning, a translation unit of its own as well (tests/test_soft_shift_host.py holds the three lists above to what
# they are): compiled and linked into every variant in the same loop; its assembly comes from emit_prune_asm(), which
# tests/test_prune_host.py lints.
PRUNE_SOURCES = ["prune_kernels.hip"]
# The random ensemble mixture, a translation unit of its own as well (tests/test_prune_host.py holds the four lists above to what they
# are): compiled and linked into every variant in the same loop; its assembly comes from emit_mixture_asm(), which
# tests/test_mixture_host.py lints.
MIXTURE_SOURCES = ["mixture_kernels.hip"]
# Normalize-and-Project, a translation unit of its own as well (tests/test_mixture_host.py holds the five lists above apart): compiled and
# linked into every variant in the same loop; its assembly comes from emit_project_asm(), which tests/test_nap_host.py lints.
PROJECT_SOURCES = ["project_kernels.hip"]
HEADERS = sorted(f for f in os.listdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")) if f.endswith(".h")) + [
    os.path.join("..", "..", "include", "isdqn_hip.h")]
# -fno-slp-vectorize: hipcc's SLP vectoriser turns scalar fp32 epilogue math into packed v_pk_*_f32 sequences, and one of
# them (LayerNorm backward of the 64-row DenseDgradLN tile) returned run-to-run different partial sums on gfx950 --
# the one reproducible instability behind round 1's "unstable tiles" (scripts/isa_lint.py rule R3).
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-fno-gpu-rdc", "-ffp-contract=off", "-fno-slp-vectorize"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True, variant=None, defines=(), extra_flags=()):
    """`variant` / `defines`: development builds (A/B timing, hazard experiments) go to lib/libisdqn_hip_<variant>.so
    with their own object directory; the product build is the one without arguments."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(HERE, "build" if not variant else "build_" + variant)
    lib = LIB if not variant else os.path.join(LIBDIR, "libisdqn_hip_%s.so" % variant)
    flags = FLAGS + ["-D" + d for d in defines] + list(extra_flags)
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    procs = []
    for src in SOURCES + EXTRA_SOURCES + SIDE_SOURCES + PRUNE_SOURCES + MIXTURE_SOURCES + PROJECT_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [hipcc] + flags + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    failed = [src for src, p in procs if p.wait() != 0]
    if failed:
        raise RuntimeError(f"hipcc failed for {failed}")
    if force or procs or _stale(lib, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return lib


def emit_asm(force=False, verbose=False, sources=None, variant=None, defines=()):
    """Device-side assembly of every source of SOURCES + EXTRA_SOURCES (or of ``sources``) under the product flags (build/<name>.s), for
    scripts/isa_lint.py.  `variant` / `defines`: of a development build, to build_<variant>/<name>.s (tests/test_store_policy_host.py)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build" if not variant else "build_" + variant)
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, h) for h in HEADERS]
    outs, procs = [], []
    for src in (SOURCES + EXTRA_SOURCES if sources is None else sources):
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".s"))
        outs.append(o)
        if force or _stale(o, [s] + headers + [os.path.abspath(__file__)]):
            cmd = [hipcc] + [f for f in FLAGS if f != "-fPIC"] + ["-D" + d for d in defines] + ["-S", "--cuda-device-only", "-w", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    failed = [src for src, p in procs if p.wait() != 0]
    if failed:
        raise RuntimeError(f"hipcc -S failed for {failed}")
    return outs


def emit_side_asm(force=False, verbose=False):
    """emit_asm for SIDE_SOURCES."""
    return emit_asm(force=force, verbose=verbose, sources=SIDE_SOURCES)


def emit_prune_asm(force=False, verbose=False):
    """emit_asm for PRUNE_SOURCES."""
    return emit_asm(force=force, verbose=verbose, sources=PRUNE_SOURCES)


def emit_mixture_asm(force=False, verbose=False):
    """emit_asm for MIXTURE_SOURCES."""
    return emit_asm(force=force, verbose=verbose, sources=MIXTURE_SOURCES)


def emit_project_asm(force=False, verbose=False):
    """emit_asm for PROJECT_SOURCES."""
    return emit_asm(force=force, verbose=verbose, sources=PROJECT_SOURCES)


if __name__ == "__main__":
    _variant = None
    _defs = []
    for _i, _a in enumerate(sys.argv):
        if _a == "--variant":
            _variant = sys.argv[_i + 1]
        if _a.startswith("-D"):
            _defs.append(_a[2:])
    _extra = [_a for _a in sys.argv[1:] if _a.startswith("-f") or _a.startswith("-m")]
    print(build(force="--force" in sys.argv, variant=_variant, defines=_defs, extra_flags=_extra))
    if "--emit-asm" in sys.argv:
        print("\n".join(emit_asm(force="--force" in sys.argv, verbose=True) + emit_side_asm(force="--force" in sys.argv, verbose=True)
                        + emit_prune_asm(force="--force" in sys.argv, verbose=True) + emit_mixture_asm(force="--force" in sys.argv, verbose=True)
                        + emit_project_asm(force="--force" in sys.argv, verbose=True)))
