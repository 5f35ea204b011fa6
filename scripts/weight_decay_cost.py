"""What AdamW's decoupled weight decay costs (include/isdqn_hip.h, isdqn_batch_decay), measured on the GPU from ONE build
(scripts/horizon_cost.py's pattern):

  the step at the headline shape (cnn 32 64 64 512 + LN, K = 9, A = 9, B = 32) with weight_decay = 0.1 on the conv and dense kernels and
  without: eager update_online_params, and learn_steps as one captured graph of S = 8, on a uniform replay.  The two legs differ in the
  struct behind the batch and in the `wd` every optimizer entry carries: the decayed leg runs three more VALU operations per decayed
  element in adam_kernel and in the fused epilogue of Dense_0's weight-gradient GEMM and moves no more memory.  A host clock around
  --steps steps that end in a device synchronise, the two agents alternating over --rounds rounds, medians.

    python scripts/weight_decay_cost.py [--steps 200] [--rounds 5] [--capacity 20000] [--all-kinds]

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

WEIGHT_DECAY = 0.1


def _replay(args, B):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(0), B, args.capacity, stack_size=4, update_horizon=3, gamma=0.99)
    rb.prefill_synthetic(args.capacity, (84, 84), 9, seed=0)
    return rb


def step_cost(args, captured):
    import torch

    from slimdqn.networks.isdqn import iSDQN

    B, S = 32, 8

    def make(weight_decay):
        agent = iSDQN(0, (84, 84, 4), 9, 9, [32, 64, 64, 512], True, False, "cnn", 6.25e-5, 0.99, 3, 1, 8000, adam_eps=1.5e-4, batch_size=B,
                      use_graph=captured, weight_decay=weight_decay, weight_decay_all=args.all_kinds)
        return agent, _replay(args, B)

    legs = {"plain": make(0.0), "decay": make(WEIGHT_DECAY)}

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
    moved = not torch.equal(legs["plain"][0]._engine.params, legs["decay"][0]._engine.params)
    return dict(ms_per_step=ms, median_ms=med, cost_us_per_step=(med["decay"] - med["plain"]) * 1e3, losses_finite=finite,
                legs_differ=moved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=20_000)
    ap.add_argument("--all-kinds", action="store_true", help="decay the biases and the normalisation parameters too")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is nothing to fall back to"
    out = dict(device=torch.cuda.get_device_name(0), weight_decay=WEIGHT_DECAY, all_kinds=bool(args.all_kinds))
    out["step_headline_B32"] = {"captured_S8" if cap else "eager": step_cost(args, cap) for cap in (False, True)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
