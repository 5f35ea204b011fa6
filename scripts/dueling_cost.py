"""What dueling heads cost at the c2 shape (bench.py's replica: B = 256, K = 9, A = 9, features 32 64 64 512, uniform device replay): the
learn step with and without dueling=True, as the captured multi-step graph and as eager launches, the legs alternating in one process on
ONE replay, untraced, device synchronise at both ends of every timed leg.  Scalar heads with dueling take the generic loss and head
backward instead of the head chain (net_kernels.hip: head_chain_plan) and add three small launches (combine, backward map, mask): that
difference is what this measures.  --heads adds the same pair of legs on histogram or quantile heads, where both sides take the generic
path and only the three launches and the wider head GEMMs differ.

    python scripts/dueling_cost.py [--capacity 100000] [--graph 20] [--replays 50] [--eager-steps 400] [--rounds 5] [--heads scalar,n_quantiles=51]
    rocprofv3 --kernel-trace --stats ... -- python scripts/dueling_cost.py --rounds 1 --replays 10   # duel_*_kernel, td_kernel, the head GEMMs

Prints one JSON line: ms per step of every leg, the medians, the spread of every leg and the cost of the option per head kind and mode.
It compares this build with ITSELF: the cost of the option, nothing a test may depend on.  bench.py stays the measure of the default step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))

HEADS = {
    "scalar": dict(),
    "n_bins=51": dict(n_bins=51, min_value=-10.0, max_value=10.0, sigma=0.75 * 20.0 / 51),
    "n_quantiles=51": dict(n_quantiles=51, huber_delta=1.0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=100_000)
    ap.add_argument("--graph", type=int, default=20, help="steps per captured graph")
    ap.add_argument("--replays", type=int, default=50, help="graph replays per timed graph leg")
    ap.add_argument("--eager-steps", type=int, default=400, help="steps per timed eager leg")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the legs")
    ap.add_argument("--heads", default="scalar", help="comma-separated head kinds: " + ", ".join(HEADS))
    args = ap.parse_args()

    import torch

    from bench import FEATURES, WORKLOADS, Replica
    from slimdqn._engine import QNetEngine
    from slimdqn._graph import GraphedUpdate

    S, w = args.graph, WORKLOADS["c2"]
    r = Replica("c2", args.capacity, "bf16x3", 0, "cuda:0", trust_mirror=True)
    engines = {}
    for head in args.heads.split(","):
        for duel in (False, True):
            eng = QNetEngine((84, 84, 4), w["n_actions"], 1 + w["K"], FEATURES, "cnn", True, w["B"], gamma_n=0.99 ** w["n"], learning_rate=6.25e-5,
                             adam_eps=1.5e-4, precision="bf16x3", device="cuda:0", dueling=duel, **HEADS[head])
            eng.init_params(0)
            eng.trust_mirror = True
            engines[f"{head}{'+dueling' if duel else ''}"] = eng
    torch.cuda.synchronize()
    live = [None]

    def graph_leg(name, replays, warm):
        """One captured leg: its update replaces the previous leg's (one live executable graph at a time: DESIGN.md 6), a short warm-up,
        then `replays` timed replays between two device synchronisations."""
        if live[0] is not None:
            live[0].destroy()
        g = live[0] = GraphedUpdate(r.rb, engines[name], False, S)
        for _ in range(warm):
            g.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(replays):
            g.run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (replays * S) * 1e3

    def eager_leg(name, steps, warm):
        eng = engines[name]

        def step():
            batch = r.rb.sample()
            eng.learn_on_batch(eng.make_batch(frames=batch.frames, frame_stride=batch.frame_stride, frame_ids=batch.frame_ids, action=batch.action,
                                              reward=batch.reward, terminal=batch.is_terminal))

        for _ in range(warm):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    first = next(iter(engines))
    graph_leg(first, 1, max(4, 2000 // S))  # clocks, caches, the sampler's first prefetch block
    ms = {f"{name} {mode}": [] for name in engines for mode in ("graph", "eager")}
    for _ in range(args.rounds):
        for name in engines:
            ms[f"{name} graph"].append(graph_leg(name, args.replays, 8))
        if live[0] is not None:
            live[0].destroy()
            live[0] = None
        for name in engines:
            ms[f"{name} eager"].append(eager_leg(name, args.eager_steps, 20))
    med = {k: statistics.median(v) for k, v in ms.items()}
    cost = {f"{head} {mode}": med[f"{head}+dueling {mode}"] - med[f"{head} {mode}"] for head in args.heads.split(",") for mode in ("graph", "eager")}
    finite = {k: bool(torch.isfinite(e.losses_accum).all()) for k, e in engines.items()}
    print(json.dumps(dict(workload="c2-shaped learn step", capacity=args.capacity, steps_per_graph=S, replays_per_leg=args.replays,
                          eager_steps_per_leg=args.eager_steps, ms_per_step=ms, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in ms.items()},
                          dueling_cost_ms=cost, losses_finite=finite)))


if __name__ == "__main__":
    main()
