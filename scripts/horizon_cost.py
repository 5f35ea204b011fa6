"""What the annealed update horizon and discount cost (include/isdqn_hip.h, isdqn_replay_gather_horizon and isdqn_batch_discount::discount),
measured on the GPU from ONE build (scripts/augment_cost.py's pattern):

  * the kernel alone at B = 32, stack 4, n_max 10 beside isdqn_replay_gather_rows on the same rows: the yardstick, a kernel the parent
    commit already has.  HIP events around every single call, alternating between the two, medians over --launches calls each after
    --warmup untimed ones.
  * the step at the headline shape (cnn 32 64 64 512 + LN, K = 9, A = 9, B = 32), with the schedule (n 10 -> 3, gamma 0.97 -> 0.997) and
    without: eager update_online_params, and learn_steps as one captured graph of S = 8, on a uniform and on a prioritized replay.  Both
    legs sample a replay with horizon windows at n_max = 10 -- the plain leg through the existing row gather -- so the difference is
    the option's: the gather at a horizon (uniform and captured: S gathers of B rows in place of one of S * B), the two staged scalars
    per step and the discount loads of the loss.  A host clock around --steps steps that end in a device synchronise, the two agents
    alternating over --rounds rounds, medians.

    python scripts/horizon_cost.py [--launches 200] [--warmup 50] [--steps 200] [--rounds 5] [--capacity 20000]

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

N_MAX = 10
SCHEDULE = (10, 3, 0.97, 0.997)


def _replay(args, B, prioritized=False):
    import numpy as np

    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

    sampler = PrioritizedSamplingDistribution(0, args.capacity) if prioritized else UniformSamplingDistribution(0)
    rb = ReplayBuffer(sampler, B, args.capacity, stack_size=4, update_horizon=N_MAX, gamma=0.97, horizon_window=True)
    pri = np.random.default_rng(0).uniform(0.1, 2.0, args.capacity) if prioritized else None
    rb.prefill_synthetic(args.capacity, (84, 84), 9, seed=0, priorities=pri)
    return rb


def kernel_alone(args):
    import torch

    B = 32
    rb = _replay(args, B)
    indices = [rb._sampling_distribution.sample_device(B) for _ in range(8)]  # other rows every call
    horizon = torch.tensor([5], dtype=torch.int32, device=rb.device)
    gamma = torch.tensor([0.97], dtype=torch.float32, device=rb.device)
    calls = {"gather_horizon": lambda idx: rb.gather(idx, horizon=horizon, gamma=gamma), "gather_rows": lambda idx: rb.gather(idx)}
    us = {k: [] for k in calls}
    for i in range(args.warmup + args.launches):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            call(indices[i % len(indices)])
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(v) for k, v in us.items()}
    q = lambda v, p: sorted(v)[int(p * (len(v) - 1))]
    return dict(shape=dict(B=B, stack=4, n_max=N_MAX, horizon=5), launches=args.launches, median_us=med,
                p10_us={k: q(v, 0.1) for k, v in us.items()}, p90_us={k: q(v, 0.9) for k, v in us.items()},
                ratio_horizon_over_rows=med["gather_horizon"] / med["gather_rows"],
                note="each call allocates its output tensors (four, five with the discounts) and launches one kernel")


def step_cost(args, prioritized, captured):
    import torch

    from slimdqn.networks.isdqn import iSDQN

    B, S = 32, 8

    def make(schedule):
        agent = iSDQN(0, (84, 84, 4), 9, 9, [32, 64, 64, 512], True, False, "cnn", 6.25e-5, 0.97, N_MAX, 1, 8000, adam_eps=1.5e-4, batch_size=B,
                      use_graph=captured)
        rb = _replay(args, B, prioritized)
        agent.priority_writeback = prioritized
        if schedule:
            agent.set_horizon_schedule(*SCHEDULE, period=args.steps * (args.rounds + 1), replay_buffer=rb)
        return agent, rb

    legs = {"plain": make(False), "schedule": make(True)}

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
    return dict(ms_per_step=ms, median_ms=med, cost_us_per_step=(med["schedule"] - med["plain"]) * 1e3, losses_finite=finite,
                last_pair=legs["schedule"][0]._horizon_logs())


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
