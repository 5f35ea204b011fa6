"""Run the two horizon-window kernels (include/isdqn_hip.h: isdqn_replay_apply_staged_horizon, isdqn_replay_gather_horizon) of a
bounds-checked build (-DISDQN_BOUNDS) with the EXACT extents of their buffers registered -- the staged block, the three tables, the
action and terminal tables, the index table, the slots, the two scalars -- first and last slot, ragged B, m = n_max; then one learn, loss
and gradient step with a registered discount tensor (isdqn_batch_discount::discount) on the headline head chain, a tiny td_kernel case and a C51
case (scripts/bounds_check.py holds the helpers of the learn step's table).  One JSON line per case: {"case", "bad", "site", "addr"}.
Sites 48 (the gather's loads) and 49 (the scatter's) are checked against the replay code object's own table
(isdqn_debug_replay_bounds_set / _get), site 50 (the discount loads of the loss kernels) against the learn step's.  Started by
tests/test_gpu_horizon_bounds.py with ISDQN_HIP_LIB pointing at that build."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch

from bounds_check import engine_tensors, register, result
from slimdqn import _hip
from slimdqn._engine import QNetEngine

lib = _hip.lib()
lib.isdqn_debug_replay_bounds_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
lib.isdqn_debug_replay_bounds_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def register_replay(tensors):
    lo = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() for t in tensors])
    hi = (ctypes.c_uint64 * len(tensors))(*[t.data_ptr() + t.numel() * t.element_size() for t in tensors])
    _hip.check(lib.isdqn_debug_replay_bounds_set(lo, hi, len(tensors)))


def replay_result():
    bad, site, addr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    _hip.check(lib.isdqn_debug_replay_bounds_get(ctypes.byref(bad), ctypes.byref(site), ctypes.byref(addr)))
    return int(bad.value), int(site.value), int(addr.value)


def report(case, *results):
    bad, site, addr = next((r for r in results if r[0]), results[0])
    print(json.dumps({"case": case, "bad": bad, "site": site, "addr": hex(addr)}), flush=True)


def tables(C, stack, n_max, rng):
    window = dev(rng.integers(-1, 1000, (C, stack + n_max)).astype(np.int32))
    steps = dev(rng.normal(size=(C, n_max)).astype(np.float32))
    length = dev(rng.integers(1, n_max + 1, C).astype(np.int32))
    action = dev(rng.integers(0, 5, C).astype(np.int32))
    terminal = dev((rng.random(C) < 0.3).astype(np.uint8))
    return window, steps, length, action, terminal


def run_gather_case(name, C, stack, n_max, B, horizon, with_index, omit_gamma=False):
    rng = np.random.default_rng(0)
    window, steps, length, action, terminal = tables(C, stack, n_max, rng)
    slots_np = rng.integers(0, C, B).astype(np.int32)
    slots_np[0], slots_np[-1] = C - 1, 0  # the last and the first slot
    slots = dev(slots_np)
    index = dev(rng.permutation(C).astype(np.int32)) if with_index else None
    h, g = dev(np.array([horizon], np.int32)), dev(np.array([0.97], np.float32))
    out = [torch.zeros(B, 2 * stack, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
           torch.zeros(B, dtype=torch.float32, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda"),
           torch.zeros(B, dtype=torch.float32, device="cuda")]
    torch.cuda.synchronize()
    register_replay([window, steps, length, action, terminal, slots, h] + ([] if omit_gamma else [g]) + ([index] if with_index else []))
    _hip.check(lib.isdqn_replay_gather_horizon(_hip.ptr(window), _hip.ptr(steps), _hip.ptr(length), _hip.ptr(action), _hip.ptr(terminal), stack,
                                               n_max, _hip.ptr(index), _hip.ptr(slots), B, _hip.ptr(h), _hip.ptr(g), *[_hip.ptr(t) for t in out],
                                               _hip.stream_ptr(window.device)), name)
    report(name, replay_result())


def run_scatter_case(name, C, stack, n_max, n_rows):
    rng = np.random.default_rng(1)
    window, steps, length, _a, _t = tables(C, stack, n_max, rng)
    rows = rng.permutation(C)[:n_rows].astype(np.int32)
    rows[0], rows[-1] = C - 1, 0
    sections = [rows, rng.integers(-1, 1000, (n_rows, stack + n_max)).astype(np.int32), rng.normal(size=(n_rows, n_max)).astype(np.float32),
                rng.integers(1, n_max + 1, n_rows).astype(np.int32)]
    offs, blob = [], b""
    for a in sections:  # the staged block ends with its last section's last byte
        offs.append(len(blob))
        blob += a.tobytes()
        if a is not sections[-1]:
            blob += b"\0" * (-len(blob) % 16)
    staged = dev(np.frombuffer(blob, np.uint8).copy())
    torch.cuda.synchronize()
    register_replay([staged, window, steps, length])
    _hip.check(lib.isdqn_replay_apply_staged_horizon(_hip.ptr(staged), n_rows, *offs, stack, n_max, _hip.ptr(window), _hip.ptr(steps),
                                                     _hip.ptr(length), _hip.stream_ptr(staged.device)), name)
    report(name, replay_result())


def run_learn_case(name, feats, K, A, B, ln=True, **kw):
    eng = QNetEngine((84, 84, 4), A, 1 + K, feats, "cnn", ln, B, **kw)
    eng.init_params(0)
    rng = np.random.default_rng(2)
    n_frames = 8 * B + 3
    frames = dev(rng.integers(0, 256, (n_frames, 84 * 84), dtype=np.uint8))
    ids = dev(rng.integers(-1, n_frames, (B, 8)).astype(np.int32))
    action, reward = dev(rng.integers(0, A, B).astype(np.int32)), dev(rng.normal(size=B).astype(np.float32))
    terminal = dev((rng.random(B) < 0.3).astype(np.uint8))
    discount = dev(rng.choice(np.array([0.0, 0.9, 0.97], np.float32), B))
    grad_out = torch.zeros_like(eng.params)
    torch.cuda.synchronize()
    register(engine_tensors(eng) + [frames, ids, action, reward, terminal, discount, grad_out])
    batch = eng.make_batch(frames=frames, frame_stride=84 * 84, frame_ids=ids, action=action, reward=reward, terminal=terminal, discount=discount)
    eng.learn_on_batch(batch)
    eng.loss_on_batch(batch)
    eng.grad_on_batch(batch, grad_out)
    report(name, result())
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    HL = (32, 64, 64, 512)
    cases = [
        (run_gather_case, dict(name="horizon-gather-stack4-n10-B5-m-nmax", C=97, stack=4, n_max=10, B=5, horizon=10, with_index=True)),
        (run_gather_case, dict(name="horizon-gather-stack1-n1-B1", C=3, stack=1, n_max=1, B=1, horizon=1, with_index=False)),
        (run_gather_case, dict(name="horizon-gather-stack4-n3-B257-clamped", C=97, stack=4, n_max=3, B=257, horizon=99, with_index=True)),
        (run_scatter_case, dict(name="horizon-scatter-stack4-n10-rows37", C=97, stack=4, n_max=10, n_rows=37)),
        (run_scatter_case, dict(name="horizon-scatter-stack1-n1-rows2", C=3, stack=1, n_max=1, n_rows=2)),
        (run_learn_case, dict(name="horizon-learn-headline-B7", feats=HL, K=9, A=9, B=7)),
        (run_learn_case, dict(name="horizon-learn-td-kernel-B5", feats=(7, 9, 11, 13), K=2, A=3, B=5, ln=False)),
        (run_learn_case, dict(name="horizon-learn-c51-B6", feats=(7, 9, 11, 13), K=3, A=5, B=6, n_bins=51, min_value=-10.0, max_value=10.0,
                              categorical=True)),
        # the check does see a load outside the table: the gather with its discount scalar left unregistered must record site 48
        (run_gather_case, dict(name="horizon-control-gamma-unregistered", C=97, stack=4, n_max=10, B=5, horizon=10, with_index=True,
                               omit_gamma=True)),
    ]
    for fn, c in cases:
        if which == "all" or which in c["name"]:
            fn(**c)
