"""Run the mixture's calls (include/isdqn_hip.h, isdqn_mixture_draw / isdqn_batch_mixture / ISDQN_ACT_MEAN_HEADS) of a bounds-checked
build (-DISDQN_BOUNDS) with the EXACT extents of every tensor handed to the library registered, and print one JSON line per case:
{"case", "bad", "site", "addr"}.  The new sites: 53 (the draw's count), 54 (alpha in mix_td_kernel), 55 (the head-output rows a mixture
reads), 56 (the discount of a row), 57 (the "q" rows of the mean-heads argmax) -- the kernels live in a translation unit of their own,
whose table isdqn_debug_mixture_bounds_set / _get reach; the same extents go into the table of the steps around them
(isdqn_debug_bounds_set), and a case reports the first violation of either.  Cases: fc H = 3, A = 5, B = 5 and fc H = 200, A = 18,
B = 8 with double_q and fc H = 2, A = 70, B = 5 with double_q (the actions in two chunks of 64 lanes), each a draw, a loss and a learn call in the *_target form with loss weights and discounts, a same-parameter learn
call and the mean-heads acting call; the control registers alpha without its last element and must record site 54.  Started by
tests/test_gpu_mixture_bounds.py with ISDQN_HIP_LIB pointing at that build."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
import numpy as np
import torch

from slimdqn import _hip
from slimdqn._engine import QNetEngine

lib = _hip.lib()
lib.isdqn_debug_bounds_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
lib.isdqn_debug_bounds_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
lib.isdqn_debug_mixture_bounds_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
lib.isdqn_debug_mixture_bounds_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

CASES = {"fc-H3-A5-B5": (3, 5, 5, False), "fc-H200-A18-B8-double_q": (200, 18, 8, True), "fc-H2-A70-B5-double_q": (2, 70, 5, True)}


def register(tensors):
    lo = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() for t in tensors])
    hi = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() + t.numel() * t.element_size() for t in tensors])
    _hip.check(lib.isdqn_debug_bounds_set(lo, hi, len(tensors)))
    _hip.check(lib.isdqn_debug_mixture_bounds_set(lo, hi, len(tensors)))


def report(case):
    bad, site, addr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    _hip.check(lib.isdqn_debug_mixture_bounds_get(ctypes.byref(bad), ctypes.byref(site), ctypes.byref(addr)))
    if not bad.value:  # (the mixture's own table first; else what the kernels of the steps around it recorded)
        _hip.check(lib.isdqn_debug_bounds_get(ctypes.byref(bad), ctypes.byref(site), ctypes.byref(addr)))
    print(json.dumps({"case": case, "bad": int(bad.value), "site": int(site.value), "addr": hex(addr.value)}), flush=True)


def run_case(name, control=False):
    H, A, B, double_q = CASES[name]
    eng = QNetEngine((8,), A, H, [16, 24], "fc", True, B, double_q=double_q)
    eng.init_params(0)
    eng.set_mixture(7)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st, nx = dev(rng.normal(size=(B, 8)).astype(np.float32)), dev(rng.normal(size=(B, 8)).astype(np.float32))
    action, reward = dev(rng.integers(0, A, B).astype(np.int32)), dev(rng.normal(size=B).astype(np.float32))
    terminal = dev((rng.random(B) < 0.3).astype(np.uint8))
    weights, discount = dev(rng.uniform(0.2, 1.0, B).astype(np.float32)), dev(rng.uniform(0.5, 0.99, B).astype(np.float32))
    batch = eng.make_batch(state=st, next_state=nx, action=action, reward=reward, terminal=terminal, loss_weights=weights, discount=discount)
    target = eng.params.clone()
    out = torch.zeros(B, dtype=torch.int32, device="cuda")
    # (the control: the accesses are the same, inside the engine's own buffer -- only the registration is short by alpha's last element)
    alpha = eng.mix_alpha[: H - 1] if control else eng.mix_alpha
    torch.cuda.synchronize()
    register([eng.params, eng.adam_m, eng.adam_v, eng.workspace, eng.losses, eng.losses_accum, eng.q_values, eng.targets, eng.priorities,
              eng.adam_count, st, nx, action, reward, terminal, weights, discount, target, out, alpha, eng.mix_count])
    eng.mixture_draw()
    eng.loss_on_batch_target(batch, target)
    eng.learn_on_batch_target(batch, target)
    eng.mixture_draw()
    eng.learn_on_batch(batch)
    eng.best_actions(obs=st, idx_networks=None, mean_heads=True, out=out)
    report(("control-" if control else "") + name)
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in CASES:
        run_case(name)
    run_case("fc-H3-A5-B5", control=True)
