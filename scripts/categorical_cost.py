"""What the distributional losses cost at the c2 shape (bench.py's replica: B = 256, K = 9, A = 9, uniform device replay): the captured step
with scalar heads, with HL-Gauss histogram heads (n_bins = 51), with the C51 categorical loss on the same heads (categorical) and with
QR-DQN quantile heads (n_quantiles = 51, kappa = 1), the four legs alternating in one process on ONE replay, untraced, device synchronise
at both ends of every timed leg.

    python scripts/categorical_cost.py [--capacity 100000] [--graph 20] [--replays 50] [--rounds 5] [--legs scalar,n_bins=51]
    rocprofv3 --kernel-trace --stats ... -- python scripts/categorical_cost.py --rounds 1 --replays 10   # c51_loss_kernel / hl_loss_kernel / qr_loss_kernel

Prints one JSON line: ms per step of every leg, the medians, the spread of the scalar legs.  It compares this build with ITSELF: the cost
of the options, nothing a test may depend on.  bench.py stays the measure of the default step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))

LEGS = {
    "scalar": dict(),
    "n_bins=51": dict(n_bins=51, min_value=-10.0, max_value=10.0, sigma=0.75 * 20.0 / 51),
    "categorical": dict(n_bins=51, min_value=-10.0, max_value=10.0, categorical=True),
    "n_quantiles=51": dict(n_quantiles=51, huber_delta=1.0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=100_000)
    ap.add_argument("--graph", type=int, default=20, help="steps per captured graph")
    ap.add_argument("--replays", type=int, default=50, help="graph replays per timed leg")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the legs")
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of the legs (a tree without the categorical keyword runs the other three)")
    args = ap.parse_args()
    legs = {name: LEGS[name] for name in args.legs.split(",")}

    import torch

    from bench import FEATURES, WORKLOADS, Replica
    from slimdqn._engine import QNetEngine
    from slimdqn._graph import GraphedUpdate

    S, w = args.graph, WORKLOADS["c2"]
    r = Replica("c2", args.capacity, "bf16x3", 0, "cuda:0", trust_mirror=True)
    engines = {"scalar": r.eng}
    for name, kw in legs.items():
        if name not in engines:
            eng = QNetEngine((84, 84, 4), w["n_actions"], 1 + w["K"], FEATURES, "cnn", True, w["B"], gamma_n=0.99 ** w["n"], learning_rate=6.25e-5,
                             adam_eps=1.5e-4, precision="bf16x3", device="cuda:0", **kw)
            eng.init_params(0)
            eng.trust_mirror = True
            engines[name] = eng
    torch.cuda.synchronize()
    live = [None]

    def leg(name, replays, warm):
        """One leg: its captured update replaces the previous leg's (one live executable graph at a time: DESIGN.md 6), a short
        warm-up, then `replays` timed replays between two device synchronisations."""
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

    leg("scalar", 1, max(4, 2000 // S))  # clocks, caches, the sampler's first prefetch block
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name in legs:
            ms[name].append(leg(name, args.replays, 8))
    med = {k: statistics.median(v) for k, v in ms.items()}
    finite = {k: bool(torch.isfinite(engines[k].losses_accum).all()) for k in legs}
    print(json.dumps(dict(workload="c2-shaped captured step", capacity=args.capacity, steps_per_graph=S, replays_per_leg=args.replays,
                          ms_per_step=ms, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in ms.items()},
                          cost_ms={k: med[k] - med["scalar"] for k in med if "scalar" in med}, losses_finite=finite)))


if __name__ == "__main__":
    main()
