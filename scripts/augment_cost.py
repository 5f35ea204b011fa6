"""What the random-shift augmentation costs (include/isdqn_hip.h, isdqn_replay_augment_shift), measured on the GPU from ONE build:

  * the kernel alone at B = 32, stack 4, 84 x 84, pad 4 -- one call is the shift launch plus the one-thread counter launch -- beside
    isdqn_replay_materialize on the same rows: the yardstick, a kernel the parent commit already has that reads and writes the same
    number of bytes with an aligned, unshifted access pattern.  HIP events around every single call, alternating between the two,
    medians over --launches calls each after --warmup untimed ones.
  * the step at the headline shape (cnn 32 64 64 512 + LN, K = 9, A = 9, B = 32), with augment_pad = 4 and without: eager
    update_online_params, and learn_steps as one captured graph of S = 8, on a uniform and on a prioritized replay.  A host clock around
    --steps steps that end in a device synchronise, the two agents alternating over --rounds rounds, medians.

    python scripts/augment_cost.py [--launches 200] [--warmup 50] [--steps 200] [--rounds 5] [--capacity 20000]

Prints one JSON line.  It compares this build with ITSELF: the cost of the option, nothing a test may depend on.  bench.py stays the
measure of the default step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))


def kernel_alone(args):
    import torch

    from slimdqn import _hip
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    B, stack, h, w, pad = 32, 4, 84, 84, 4
    rb = ReplayBuffer(UniformSamplingDistribution(0), B, args.capacity, stack_size=stack, update_horizon=1, gamma=0.99)
    rb.prefill_synthetic(args.capacity, (h, w), 9, seed=0)
    lib, stream = _hip.lib(), _hip.stream_ptr(rb.device)
    count = torch.zeros(1, dtype=torch.int64, device=rb.device)
    pool, table = rb._augment_pool(B)
    st = torch.empty(B, h, w, stack, dtype=torch.uint8, device=rb.device)
    nx = torch.empty_like(st)
    batches = [rb.sample() for _ in range(8)]  # other rows every call: no call re-reads what the previous one left in the caches

    def shift(b):
        _hip.check(lib.isdqn_replay_augment_shift(_hip.ptr(rb._frames), rb._hw, h, w, stack, _hip.ptr(b.frame_ids), B, B, pad, 12345, _hip.ptr(count),
                                                  _hip.ptr(pool), _hip.ptr(table), stream))

    def materialize(b):
        _hip.check(lib.isdqn_replay_materialize(_hip.ptr(rb._frames), rb._hw, h, w, stack, _hip.ptr(b.frame_ids), B, _hip.ptr(st), _hip.ptr(nx), stream))

    us = {"augment_shift": [], "materialize": []}
    for i in range(args.warmup + args.launches):
        for name, call in (("augment_shift", shift), ("materialize", materialize)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            call(batches[i % len(batches)])
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(v) for k, v in us.items()}
    q = lambda v, p: sorted(v)[int(p * (len(v) - 1))]
    return dict(shape=dict(B=B, stack=stack, h=h, w=w, pad=pad, frames=B * 2 * stack, bytes_read=B * 2 * stack * h * w, bytes_written=B * 2 * stack * h * w),
                launches=args.launches, median_us=med, p10_us={k: q(v, 0.1) for k, v in us.items()}, p90_us={k: q(v, 0.9) for k, v in us.items()},
                ratio_shift_over_materialize=med["augment_shift"] / med["materialize"],
                note="augment_shift = the shift launch + the one-thread counter launch; materialize = one launch")


def step_cost(args, prioritized, captured):
    import numpy as np
    import torch

    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

    B, S = 32, 8

    def make(pad):
        agent = iSDQN(0, (84, 84, 4), 9, 9, [32, 64, 64, 512], True, False, "cnn", 6.25e-5, 0.99, 1, 1, 8000, adam_eps=1.5e-4, batch_size=B,
                      use_graph=captured, augment_pad=pad)
        sampler = PrioritizedSamplingDistribution(0, args.capacity) if prioritized else UniformSamplingDistribution(0)
        rb = ReplayBuffer(sampler, B, args.capacity, stack_size=4, update_horizon=1, gamma=0.99)
        pri = np.random.default_rng(0).uniform(0.1, 2.0, args.capacity) if prioritized else None
        rb.prefill_synthetic(args.capacity, (84, 84), 9, seed=0, priorities=pri)
        agent.priority_writeback = prioritized
        return agent, rb

    legs = {"plain": make(0), "augment_pad=4": make(4)}

    def run(agent, rb, n):
        if captured:
            agent._captures = 0  # (learn_steps captures what its first call asks for: S steps; the calls behind it replay that graph)
            for _ in range(n // S):
                agent.learn_steps(S, rb)
        else:
            for _ in range(n):
                agent.update_online_params(0, rb)

    n = args.steps // S * S
    ms = {k: [] for k in legs}
    for r in range(args.rounds + 1):  # (round 0 is untimed: clocks, caches, the sampler's first prefetch block)
        for k, (agent, rb) in legs.items():
            run(agent, rb, 4 * S)  # the leg's warm-up; captured: its capture too (one live executable graph at a time: DESIGN.md 6)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(agent, rb, n)
            torch.cuda.synchronize()
            if r > 0:
                ms[k].append((time.perf_counter() - t0) / n * 1e3)
            agent._drop_graph()
    med = {k: statistics.median(v) for k, v in ms.items()}
    finite = {k: bool(torch.isfinite(a._engine.losses_accum).all()) for k, (a, _rb) in legs.items()}
    return dict(ms_per_step=ms, median_ms=med, cost_us_per_step=(med["augment_pad=4"] - med["plain"]) * 1e3, losses_finite=finite,
                aug_count=int(legs["augment_pad=4"][0].aug_count.item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="timed calls of each kernel (at least 100)")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed leg of the step measurement")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=20_000)
    ap.add_argument("--only", default="kernel,step", help="kernel, step or both")
    args = ap.parse_args()
    assert args.launches >= 100
    import torch

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is nothing to fall back to"
    out = dict(device=torch.cuda.get_device_name(0))
    if "kernel" in args.only:
        out["kernel_alone"] = kernel_alone(args)
    if "step" in args.only:
        out["step_headline_B32"] = {f"{'captured_S8' if cap else 'eager'}_{'prioritized' if pri else 'uniform'}": step_cost(args, pri, cap)
                                    for cap in (False, True) for pri in (False, True)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
