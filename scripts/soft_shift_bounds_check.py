"""Run the soft head shift (include/isdqn_hip.h, isdqn_net_soft_shift) of a bounds-checked build (-DISDQN_BOUNDS) with the EXACT extents
of what the call may touch registered -- not the whole parameter buffer and workspace, but the rows of heads 0 .. K of the last Dense's
kernel and bias, and the same ranges of the workspace's weight mirror (in whole groups of 8 floats) -- and print one JSON line per case:
{"case", "bad", "site", "addr"}.  Site 51 is every load and store of soft_shift_kernel, the mirror's included; the kernel lives in a
translation unit of its own, whose table isdqn_debug_soft_shift_bounds_set / _get reach (as scripts/augment_bounds_check.py reaches the
replay object's).  Cases: the configurations of tests/helpers/soft_shift.py (tau 0.005 and 0.5, with and without a workspace), and a
noisy engine's sigma; the control registers the master's kernel rows without head K, which every call reads, and must record site 51.
tau = 1 is not this kernel's: it is routed to isdqn_net_shift_params and a rebuild of the whole mirror.  Started by
tests/test_gpu_soft_shift_bounds.py with ISDQN_HIP_LIB pointing at that build."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
import torch

from slimdqn import _hip
from tests.helpers import soft_shift as hs

lib = _hip.lib()
lib.isdqn_debug_soft_shift_bounds_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
lib.isdqn_debug_soft_shift_bounds_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def register(tensors):
    """The byte extents of ``tensors`` become the only ones the kernel may touch; the record of the last case is cleared."""
    lo = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() for t in tensors])
    hi = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() + t.numel() * t.element_size() for t in tensors])
    _hip.check(lib.isdqn_debug_soft_shift_bounds_set(lo, hi, len(tensors)))


def report(case):
    bad, site, addr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    _hip.check(lib.isdqn_debug_soft_shift_bounds_get(ctypes.byref(bad), ctypes.byref(site), ctypes.byref(addr)))
    print(json.dumps({"case": case, "bad": int(bad.value), "site": int(site.value), "addr": hex(addr.value)}), flush=True)


def extents(eng, buffers):
    """The views of heads 0 .. K of the last Dense in every buffer of the parameter layout, and in the engine's weight mirror."""
    off, size = ctypes.c_int64(), ctypes.c_int64()
    assert eng.lib.isdqn_net_workspace_region(ctypes.byref(eng.cfg), b"wsplit", ctypes.byref(off), ctypes.byref(size)) == 0
    mirror = eng.workspace[off.value // 4 : (off.value + size.value) // 4]
    return [t[o : o + s] for t in buffers for o, s in hs.written_extents(eng)] + [mirror[o : o + s] for o, s in hs.written_extents(eng, mirror=True)]


def run_case(name, noisy=False, control=False):
    eng = hs.make_engine(name, **(dict(noisy=True, noisy_seed=7) if noisy else {}))
    eng.params.normal_()
    copy = eng.params.clone()
    if noisy:
        eng.sigma.uniform_(0.01, 0.5)
    torch.cuda.synchronize()
    views = extents(eng, [eng.params, copy] + ([eng.sigma] if noisy else []))
    if control:  # (the accesses are the same, inside the engine's own buffers: only the registration is short)
        in_p, R = hs.head_geometry(eng)[2], hs.head_geometry(eng)[4]
        views[0] = views[0][: views[0].numel() - R * in_p]
    register(views)
    for tau in hs.TAUS:
        eng.soft_shift(tau)               # the engine's own parameters: master and mirror (noisy: mu and sigma, masters alone)
        eng.soft_shift(tau, params=copy)  # another buffer of the layout: the master alone
    report(("noisy-" if noisy else "control-" if control else "") + name)
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else ""
    for name in hs.CONFIGS:
        if which in name:
            run_case(name)
    if which in "noisy-f20-K3-scalar":
        run_case("f20-K3-scalar", noisy=True)
    if which in "control-f20-K3-scalar":
        run_case("f20-K3-scalar", control=True)
