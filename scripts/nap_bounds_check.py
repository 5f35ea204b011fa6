"""Run the projection calls (include/isdqn_hip.h, isdqn_net_project_norms / _apply) of a bounds-checked build (-DISDQN_BOUNDS) with the EXACT
extents of what they may touch registered -- the projected kernels in the parameter buffer (not the biases and LayerNorm vectors between
them, not the last Dense), the same ranges of the workspace's weight mirror, the target norms, the norms, the scales and the scratch -- and
print one JSON line per case: {"case", "bad", "site", "addr"}.  Site 58 is every load and store of project_sumsq_kernel,
project_scale_kernel and project_norms_kernel; the kernels live in a translation unit of their own, whose table
isdqn_debug_project_bounds_set / _get reach.  Cases: fc [20, 14] and the cnn torso of tests/helpers/prune.py (a measurement, two applies,
and the same on a copy without a workspace); the control registers the master without its last projected kernel, which every call reads,
and must record site 58.  Started by tests/test_gpu_nap_bounds.py with ISDQN_HIP_LIB pointing at that build."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
import torch

from slimdqn import _hip
from tests.helpers import nap
from tests.helpers import prune as hp

lib = _hip.lib()
lib.isdqn_debug_project_bounds_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
lib.isdqn_debug_project_bounds_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

CASES = {"fc-20-14": hp.FC_SMALL, "cnn": hp.CNN}


def register(tensors):
    """The byte extents of ``tensors`` become the only ones the kernels may touch; the record of the last case is cleared."""
    lo = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() for t in tensors])
    hi = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() + t.numel() * t.element_size() for t in tensors])
    _hip.check(lib.isdqn_debug_project_bounds_set(lo, hi, len(tensors)))


def report(case):
    bad, site, addr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    _hip.check(lib.isdqn_debug_project_bounds_get(ctypes.byref(bad), ctypes.byref(site), ctypes.byref(addr)))
    print(json.dumps({"case": case, "bad": int(bad.value), "site": int(site.value), "addr": hex(addr.value)}), flush=True)


def run_case(name, control=False):
    eng = hp.make_engine(CASES[name])
    eng.params.copy_(torch.from_numpy(nap.case_params(eng, "normal")))
    eng.set_weight_projection(nap.case_targets(eng))
    k = len(eng.project_infos)
    copy = eng.params.clone()
    off, size = ctypes.c_int64(), ctypes.c_int64()
    assert eng.lib.isdqn_net_workspace_region(ctypes.byref(eng.cfg), b"wsplit", ctypes.byref(off), ctypes.byref(size)) == 0
    mirror = eng.workspace[off.value // 4 : (off.value + size.value) // 4]
    torch.cuda.synchronize()
    kernels = [(int(i.offset), int(i.size)) for i in nap.projected(eng)]
    views = [t[o : o + s] for t in (copy, mirror, eng.params) for o, s in kernels]
    if control:  # (the accesses are the same, inside the engine's own buffers: only the registration is short)
        views.pop()
    register(views + [eng.project_target[:k], eng.project_norms_out[:k], eng.project_scales[:k], eng.project_scratch])
    eng.project_norms()
    eng.project_weights()  # the engine's own parameters: master and mirror
    eng.project_weights()
    eng.project_norms(params=copy)
    eng.project_weights(params=copy)  # another buffer of the layout: the master alone
    report(("control-" if control else "") + name)
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in CASES:
        run_case(name)
    run_case("fc-20-14", control=True)
