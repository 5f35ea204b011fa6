"""Run the pruning calls (include/isdqn_hip.h, isdqn_net_prune_update / _apply) of a bounds-checked build (-DISDQN_BOUNDS) with the EXACT
extents of what they may touch registered -- the prunable kernels in the parameter buffer (not the biases and LayerNorm vectors between
them, not the last Dense), the same ranges of the workspace's weight mirror, the mask and the scratch -- and print one JSON line per case:
{"case", "bad", "site", "addr"}.  Site 52 is every load, store and atomic of prune_select_kernel and prune_apply_kernel; the kernels live
in a translation unit of their own, whose table isdqn_debug_prune_bounds_set / _get reach.  Cases: fc [20, 14] and the cnn torso of
tests/helpers/prune.py (an update at 50 %, one at 75 % on top, an apply, and the same on a copy without a workspace); the control registers
the master without its last prunable kernel, which every call reads, and must record site 52.  Started by tests/test_gpu_prune_bounds.py
with ISDQN_HIP_LIB pointing at that build."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
import torch

from slimdqn import _hip
from tests.helpers import prune as hp

lib = _hip.lib()
lib.isdqn_debug_prune_bounds_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
lib.isdqn_debug_prune_bounds_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

CASES = {"fc-20-14": hp.FC_SMALL, "cnn": hp.CNN}


def register(tensors):
    """The byte extents of ``tensors`` become the only ones the kernels may touch; the record of the last case is cleared."""
    lo = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() for t in tensors])
    hi = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() + t.numel() * t.element_size() for t in tensors])
    _hip.check(lib.isdqn_debug_prune_bounds_set(lo, hi, len(tensors)))


def report(case):
    bad, site, addr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    _hip.check(lib.isdqn_debug_prune_bounds_get(ctypes.byref(bad), ctypes.byref(site), ctypes.byref(addr)))
    print(json.dumps({"case": case, "bad": int(bad.value), "site": int(site.value), "addr": hex(addr.value)}), flush=True)


def run_case(name, control=False):
    eng = hp.make_engine(CASES[name])
    n = eng.set_pruning()
    eng.params.copy_(torch.from_numpy(hp.case_params(eng, "normal")))
    copy = eng.params.clone()
    off, size = ctypes.c_int64(), ctypes.c_int64()
    assert eng.lib.isdqn_net_workspace_region(ctypes.byref(eng.cfg), b"wsplit", ctypes.byref(off), ctypes.byref(size)) == 0
    mirror = eng.workspace[off.value // 4 : (off.value + size.value) // 4]
    torch.cuda.synchronize()
    kernels = [(int(i.offset), int(i.size)) for i in hp.prunable(eng)]
    views = [t[o : o + s] for t in (copy, mirror, eng.params) for o, s in kernels]
    if control:  # (the accesses are the same, inside the engine's own buffers: only the registration is short)
        views.pop()
    register(views + [eng.prune_mask, eng.prune_scratch])
    for share in (0.5, 0.75):
        eng.prune_update([int(share * x) for x in n])  # the engine's own parameters: master and mirror
        eng.prune_apply()
    eng.prune_mask.fill_(-1)
    eng.prune_update([int(0.5 * x) for x in n], params=copy)  # another buffer of the layout: the master alone
    eng.prune_apply(params=copy)
    report(("control-" if control else "") + name)
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in CASES:
        run_case(name)
    run_case("fc-20-14", control=True)
