"""Run the random-shift augmentation (include/isdqn_hip.h, isdqn_replay_augment_shift) of a bounds-checked build (-DISDQN_BOUNDS) with
the EXACT extents of its buffers registered -- the frame store, the id table, the counter, the scratch pool and the out table -- over
the kernel shapes of tests/test_gpu_augment.py (the 16-byte path, the byte path with odd bases, a pad larger than the frame on both
paths), then one learn step on an augmented batch with the pool and its table registered in place of the store (scripts/bounds_check.py
holds the helpers of the learn step's table).  One JSON line per case: {"case", "bad", "site", "addr"}.  Sites 43 (the id table), 44 (the
counter) and 45 (the source frames) are the new kernels' loads; they are checked against a table of the replay code object's own
(isdqn_debug_replay_bounds_set / _get).  Started by tests/test_gpu_augment_bounds.py with ISDQN_HIP_LIB pointing at that build."""
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
SEED = 0x5EED0123456789AB


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


def buffers(h, w, stack, n_rows, stride, rng):
    """A store that ends with its last frame's h*w bytes (no slack behind it), ids that name its first and last frame, some -1."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n_frames = 2 * n_rows * stack + 3
    store = dev(rng.integers(0, 256, (n_frames - 1) * stride + h * w, dtype=np.uint8))
    ids_np = rng.integers(0, n_frames, (n_rows, 2 * stack)).astype(np.int32)
    ids_np[rng.random(ids_np.shape) < 0.2] = -1
    ids_np[0, 0], ids_np[-1, -1] = n_frames - 1, 0
    ids = dev(ids_np)
    pool = torch.zeros((n_rows * 2 * stack - 1) * stride + h * w, dtype=torch.uint8, device="cuda")
    out_ids = torch.zeros(n_rows, 2 * stack, dtype=torch.int32, device="cuda")
    count = torch.tensor([5], dtype=torch.int64, device="cuda")
    return store, ids, count, pool, out_ids


def run_kernel_case(name, h, w, stack, n_rows, rps, pad, stride):
    store, ids, count, pool, out_ids = buffers(h, w, stack, n_rows, stride, np.random.default_rng(0))
    torch.cuda.synchronize()
    register_replay([store, ids, count, pool, out_ids])
    for _ in range(2):
        _hip.check(lib.isdqn_replay_augment_shift(_hip.ptr(store), stride, h, w, stack, _hip.ptr(ids), n_rows, rps, pad, SEED, _hip.ptr(count),
                                                  _hip.ptr(pool), _hip.ptr(out_ids), _hip.stream_ptr(store.device)), name)
    report(name, replay_result())


def run_control(name):
    """The check does see a load outside the table: the same call with the counter left unregistered must record site 44 (a load the
    kernel is entitled to -- nothing is read out of bounds here)."""
    h, w, stack, n_rows = 21, 19, 2, 5
    store, ids, count, pool, out_ids = buffers(h, w, stack, n_rows, 401, np.random.default_rng(0))
    torch.cuda.synchronize()
    register_replay([store, ids, pool, out_ids])
    _hip.check(lib.isdqn_replay_augment_shift(_hip.ptr(store), 401, h, w, stack, _hip.ptr(ids), n_rows, 1, 3, SEED, _hip.ptr(count), _hip.ptr(pool),
                                              _hip.ptr(out_ids), _hip.stream_ptr(store.device)), name)
    report(name, replay_result())


def run_learn_case(name):
    h, w, stack, B, A, K = 84, 84, 4, 6, 5, 3
    eng = QNetEngine((h, w, stack), A, 1 + K, (7, 9, 11, 13), "cnn", True, B)
    eng.init_params(0)
    rng = np.random.default_rng(1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    store, ids, count, pool, out_ids = buffers(h, w, stack, B, h * w, rng)
    action, reward = dev(rng.integers(0, A, B).astype(np.int32)), dev(rng.normal(size=B).astype(np.float32))
    terminal = dev((rng.random(B) < 0.3).astype(np.uint8))
    torch.cuda.synchronize()
    register_replay([store, ids, count, pool, out_ids])
    # the learn step sees the pool and its table, never the store
    register(engine_tensors(eng) + [pool, out_ids, action, reward, terminal])
    _hip.check(lib.isdqn_replay_augment_shift(_hip.ptr(store), h * w, h, w, stack, _hip.ptr(ids), B, B, 4, SEED, _hip.ptr(count), _hip.ptr(pool),
                                              _hip.ptr(out_ids), _hip.stream_ptr(store.device)), name)
    eng.learn_on_batch(eng.make_batch(frames=pool, frame_stride=h * w, frame_ids=out_ids, action=action, reward=reward, terminal=terminal))
    report(name, replay_result(), result())


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    cases = [
        dict(name="augment-84x84-stack4-wide", h=84, w=84, stack=4, n_rows=3, rps=3, pad=4, stride=7056),
        dict(name="augment-21x19-stack2-bytes", h=21, w=19, stack=2, n_rows=5, rps=1, pad=3, stride=401),
        dict(name="augment-4x4-pad6-wide", h=4, w=4, stack=1, n_rows=2, rps=2, pad=6, stride=16),
        dict(name="augment-4x4-pad6-bytes", h=4, w=4, stack=1, n_rows=2, rps=1, pad=6, stride=19),
    ]
    for c in cases:
        if which == "all" or which in c["name"]:
            run_kernel_case(**c)
    if which == "all" or which in "augment-learn-step-B6":
        run_learn_case("augment-learn-step-B6")
    if which == "all" or which in "augment-control-counter-unregistered":
        run_control("augment-control-counter-unregistered")
