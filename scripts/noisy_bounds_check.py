"""Run the noisy entry points (sample, compose, the noisy learn step, acting on the composed parameters) of a bounds-checked build
(-DISDQN_BOUNDS; scripts/bounds_check.py holds the registration helpers) with the EXACT extents of the new caller-owned buffers
registered -- sigma, its moments, noise, eff, grad, noise_count, the DQN form's second draw and composed target -- and print one JSON
line per case: {"case", "bad", "site", "addr"}.  Sites 40 (the counter), 41 (compose and the noise factors), 42 (the two-buffer Adam)
are the new kernels' loads.  Started by tests/test_gpu_noisy_bounds.py with ISDQN_HIP_LIB pointing at that build."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch

from bounds_check import engine_tensors, register, report
from slimdqn._engine import QNetEngine


def noisy_tensors(eng):
    return [eng.sigma, eng.sigma_m, eng.sigma_v, eng.noise, eng.eff, eng.grad, eng.noise_count, eng.noise_target, eng.eff_target]


def run_case(name, arch, obs, feats, K, A, B, target=False):
    n_heads = 1 + K if K > 0 else 1
    eng = QNetEngine(obs, A, n_heads, feats, arch, True, B, noisy=True, noisy_seed=7)
    eng.init_params(0)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    action = dev(rng.integers(0, A, B).astype(np.int32))
    reward = dev(rng.normal(size=B).astype(np.float32))
    terminal = dev((rng.random(B) < 0.3).astype(np.uint8))
    if arch == "fc":
        d = int(np.prod(obs))
        st, nx = dev(rng.normal(size=(B, d)).astype(np.float32)), dev(rng.normal(size=(B, d)).astype(np.float32))
        batch = eng.make_batch(state=st, next_state=nx, action=action, reward=reward, terminal=terminal)
        act = dict(obs=torch.cat((st, nx)).contiguous())
        extra = [st, nx, act["obs"]]
    else:
        h, w, stack = obs
        n_frames = 3 * B + 8
        frames = dev(rng.integers(0, 256, (n_frames, h * w), dtype=np.uint8))
        ids_np = rng.integers(0, n_frames, (B, 2 * stack)).astype(np.int32)
        ids_np[rng.random(ids_np.shape) < 0.1] = -1
        ids = dev(ids_np)
        flat = dev(np.concatenate([ids_np[:, :stack], ids_np[:, stack:]], 0))
        batch = eng.make_batch(frames=frames, frame_stride=h * w, frame_ids=ids, action=action, reward=reward, terminal=terminal)
        act = dict(frames=frames, frame_stride=h * w, frame_ids=flat)
        extra = [frames, ids, flat]
    heads = torch.arange(min(5, 2 * B), dtype=torch.int32, device="cuda") % max(K, 1)
    tparams = eng.params.clone()
    tensors = engine_tensors(eng) + noisy_tensors(eng) + extra + [heads, tparams, action, reward, terminal]
    torch.cuda.synchronize()
    register(tensors)
    eng.resample_noise()
    eng.compose()
    eng.compose(mirror=False)
    for _ in range(2):
        if target:
            eng.learn_on_batch_target(batch, tparams)
        else:
            eng.learn_on_batch(batch)
    eng.resample_noise()
    eng.loss_on_batch(batch) if not target else eng.loss_on_batch_target(batch, tparams)
    if arch == "fc":
        eng.best_actions(obs=act["obs"], idx_networks=heads)
    else:
        eng.best_actions(frames=act["frames"], frame_stride=act["frame_stride"], frame_ids=act["frame_ids"], idx_networks=heads)
    report(name)
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    cases = [
        dict(name="noisy-fc-B32", arch="fc", obs=(8,), feats=(100, 100), K=3, A=4, B=32),
        dict(name="noisy-fc-one-head-dqn-B32", arch="fc", obs=(8,), feats=(100, 100), K=0, A=4, B=32, target=True),
        dict(name="noisy-headline-B32", arch="cnn", obs=(84, 84, 4), feats=(32, 64, 64, 512), K=9, A=9, B=32),
    ]
    for c in cases:
        if which != "all" and which not in c["name"]:
            continue
        run_case(**c)
