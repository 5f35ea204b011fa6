"""What the importance-sampling weights of prioritized replay cost: the c3-shaped captured step (bench.py's replica: capacity
1e6, B = 256, K = 9, n = 3, prioritized sampling with write-back) with weights off and on, alternating, device synchronise at
both ends of every timed leg.

    python scripts/per_weights_cost.py [--capacity 1000000] [--graph 20] [--replays 50] [--rounds 5]
    rocprofv3 --kernel-trace --stats ... -- python scripts/per_weights_cost.py --rounds 1 --replays 10   # the two query kernels

Prints one JSON line: ms per step of every leg, the medians and the difference.  It compares this build with ITSELF (weights
off): the cost of the feature, nothing a test may depend on.  bench.py stays the measure of the default step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--graph", type=int, default=20, help="steps per captured graph")
    ap.add_argument("--replays", type=int, default=50, help="graph replays per timed leg")
    ap.add_argument("--rounds", type=int, default=5, help="alternations off / on")
    ap.add_argument("--beta", type=float, default=0.5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import Replica
    from slimdqn._graph import GraphedUpdate

    S = args.graph
    r = Replica("c3", args.capacity, "bf16x3", 0, "cuda:0", trust_mirror=True)
    betas = np.full(S, args.beta, dtype=np.float32)
    last_weights = None

    def leg(weighted, replays, warm):
        """One leg on the one replica: its captured update replaces the previous leg's (one live executable graph at a time:
        DESIGN.md 6), a short warm-up, then `replays` timed replays between two device synchronisations."""
        nonlocal last_weights
        if r.graphed is not None:
            r.graphed.destroy()
        g = r.graphed = GraphedUpdate(r.rb, r.eng, True, S, weighted=weighted)
        for _ in range(warm):
            g.run(betas if weighted else None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(replays):
            g.run(betas if weighted else None)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / (replays * S) * 1e3
        if weighted:
            last_weights = g.weights.cpu().numpy()
        return dt

    leg(False, 1, max(4, 4000 // S))  # clocks, caches, the sampler's first prefetch block
    ms = {"off": [], "on": []}
    for _ in range(args.rounds):
        ms["off"].append(leg(False, args.replays, 8))
        ms["on"].append(leg(True, args.replays, 8))
    r.rb._sampling_distribution._sum_tree.check_status()
    w = last_weights
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps(dict(workload="c3-shaped captured step", capacity=args.capacity, steps_per_graph=S, replays_per_leg=args.replays,
                          ms_per_step=ms, median_ms=med, cost_ms=med["on"] - med["off"], cost_percent=100.0 * (med["on"] / med["off"] - 1.0),
                          spread_off_ms=max(ms["off"]) - min(ms["off"]), last_weights_min=float(w.min()), last_weights_max=float(w.max()))))


if __name__ == "__main__":
    main()
