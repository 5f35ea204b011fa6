"""What global-norm gradient clipping costs at the c2 shape (bench.py's replica: B = 256, K = 9, A = 9, features 32 64 64 512, uniform
device replay): the captured learn step with max_grad_norm off, at inf (the norm is measured, nothing is ever clipped) and at half the
measured norm (every step is clipped), the legs alternating in one process on ONE replay, untraced, device synchronise at both ends of
every timed leg, medians over the rounds.  With the option the step gives up the Dense weight gradient fused into Adam (Dense_0 goes
through one slab in "gw/Dense_0" and back) and the optimizer launches on two streams (both streams join in front of the norm, one
adam_flat_kernel follows it), and adds the launches of the norm (grad_reduce_sq_kernel, grad_flat_sq_kernel, grad_clip_finalize_kernel:
csrc/grad_clip.h): the difference between the legs is all of that.  The share of the added launches alone comes from a kernel trace of
the same script:

    python scripts/grad_clip_cost.py [--capacity 100000] [--graph 20] [--replays 50] [--rounds 5] [--heads scalar,n_quantiles=51]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o gc -- python scripts/grad_clip_cost.py --rounds 1 --replays 5 --legs inf --heads scalar
    python scripts/grad_clip_cost.py --stats-csv DIR/.../gc_kernel_stats.csv      # the added launches' share of the traced kernel time

Prints one JSON line: ms per step of every leg, the medians, the spread of every leg and the cost of the option per head kind.  It
compares this build with ITSELF: the cost of the option, nothing a test may depend on.  bench.py stays the measure of the default step."""
import argparse
import csv
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
ADDED = ("grad_reduce_sq_kernel", "grad_flat_sq_kernel", "grad_clip_finalize_kernel")  # the norm
OTHER = ("adam_flat_kernel", "adam_kernel")  # the optimizer launches, for comparison


def share_from_stats(path):
    """The launches of the norm in a `rocprofv3 --kernel-trace --stats` kernel_stats.csv: their time, calls and share of all kernel time
    (and the optimizer launches beside them)."""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    for r in rows:
        for k in ADDED + OTHER:
            if k in r["Name"]:
                out[k] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, share=float(r["TotalDurationNs"]) / total)
    out["norm_share"] = sum(v["share"] for k, v in out.items() if k in ADDED)
    out["norm_us_per_step"] = sum(v["average_us"] for k, v in out.items() if k in ADDED)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=100_000)
    ap.add_argument("--graph", type=int, default=20, help="steps per captured graph")
    ap.add_argument("--replays", type=int, default=50, help="graph replays per timed leg")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the legs")
    ap.add_argument("--heads", default="scalar,n_quantiles=51", help="comma-separated head kinds: " + ", ".join(HEADS))
    ap.add_argument("--legs", default="off,inf,half", help="comma-separated legs: off, inf, half")
    ap.add_argument("--stats-csv", default=None, help="only read a rocprofv3 kernel_stats.csv and print the added launches' share")
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps(dict(stats_csv=args.stats_csv, added_launches=share_from_stats(args.stats_csv))))
        return

    import torch

    from bench import FEATURES, WORKLOADS, Replica
    from slimdqn._engine import QNetEngine
    from slimdqn._graph import GraphedUpdate

    S, w = args.graph, WORKLOADS["c2"]
    r = Replica("c2", args.capacity, "bf16x3", 0, "cuda:0", trust_mirror=True)
    legs = args.legs.split(",")
    engines, norms = {}, {}

    def make(head, c):
        eng = QNetEngine((84, 84, 4), w["n_actions"], 1 + w["K"], FEATURES, "cnn", True, w["B"], gamma_n=0.99 ** w["n"], learning_rate=6.25e-5,
                         adam_eps=1.5e-4, precision="bf16x3", device="cuda:0", max_grad_norm=c, **HEADS[head])
        eng.init_params(0)
        eng.trust_mirror = True
        return eng

    def eager_step(eng):
        batch = r.rb.sample()
        eng.learn_on_batch(eng.make_batch(frames=batch.frames, frame_stride=batch.frame_stride, frame_ids=batch.frame_ids, action=batch.action,
                                          reward=batch.reward, terminal=batch.is_terminal))

    for head in args.heads.split(","):
        # the threshold of the `half` leg: half the mean norm of eager steps 300 .. 400 of a probe engine.  (The norm of the first steps
        # is 20 x that of a network a few hundred steps in -- 59 against 2.4 on scalar heads -- and the legs, which restart from
        # init_params and then train through all their rounds, spend their time at the settled one.)
        probe = make(head, float("inf"))
        for k in range(400):
            if k == 300:
                probe.grad_clip[2:4].zero_()
            eager_step(probe)
        torch.cuda.synchronize()
        norms[head] = float(probe.grad_clip[2].item()) / 100.0
        del probe
        for leg in legs:
            engines[f"{head} {leg}"] = make(head, {"off": 0.0, "inf": float("inf"), "half": 0.5 * norms[head]}[leg])
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

    graph_leg(next(iter(engines)), 1, max(4, 2000 // S))  # clocks, caches, the sampler's first prefetch block
    ms = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name in engines:
            ms[name].append(graph_leg(name, args.replays, 8))
    if live[0] is not None:
        live[0].destroy()
    med = {k: statistics.median(v) for k, v in ms.items()}
    heads = args.heads.split(",")
    cost = {f"{head} {leg}": (med[f"{head} {leg}"] - med[f"{head} off"]) * 1e3 for head in heads for leg in legs if leg != "off" and "off" in legs}
    clipped = {}
    for name, eng in engines.items():
        if eng.max_grad_norm > 0:
            n_sum, n_clip = (float(x) for x in eng.grad_clip[2:4].cpu().numpy())
            steps = int(eng.adam_count.item())
            clipped[name] = dict(steps=steps, mean_norm=n_sum / max(steps, 1), clipped_fraction=n_clip / max(steps, 1))
    finite = {k: bool(torch.isfinite(e.losses_accum).all()) for k, e in engines.items()}
    print(json.dumps(dict(workload="c2-shaped captured learn step", capacity=args.capacity, steps_per_graph=S, replays_per_leg=args.replays,
                          probe_mean_norm=norms, ms_per_step=ms, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in ms.items()},
                          cost_us_per_step=cost, clipping=clipped, losses_finite=finite)))


if __name__ == "__main__":
    main()
