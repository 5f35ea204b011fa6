"""What one ReDo recycle costs at the c2 shape (bench.py's replica: B = 256, K = 9, A = 9, LayerNorm cnn) on n_rows = 512 observations:
the isdqn_net_redo call next to isdqn_net_analysis on the same rows, one isdqn_net_refresh_mirror and one full forward, every leg
alternating in one process, untraced, device synchronise at both ends of every timed leg; and the host cost of fresh_params (numpy
initialisation + import into the internal layout + upload).

    python scripts/redo_cost.py [--calls 50] [--rounds 5]
    rocprofv3 --kernel-trace --stats ... -- python scripts/redo_cost.py --rounds 1 --calls 10   # the three redo_* kernels by name

Legs: mirror, forward (mirror + the whole network), analysis (mirror + torso + the four sum launches), redo_none (tau = 0 on a fresh
LayerNorm network: nothing is dormant, the recycle launches find nothing to write), redo_all (tau = 1e30: every neuron is dormant, every
weight, bias, LayerNorm parameter and moment of the hidden layers and every weight of the last Dense is written: the worst case).
Derived, in ms: forward_only = forward - mirror; score = redo_none - forward_only - 2 mirror (the score kernels plus the near-empty
recycle launches); recycle = redo_all - redo_none; analysis_sums = analysis - forward_only - mirror.  A tree without the redo entry
points (the parent commit) runs the other legs.

Prints one JSON line.  It compares this build with ITSELF; nothing a test may depend on.  bench.py stays the measure of the learn step."""
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
    ap.add_argument("--calls", type=int, default=50, help="calls per timed leg")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the legs")
    ap.add_argument("--rows", type=int, default=512)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import FEATURES, WORKLOADS
    from slimdqn._engine import QNetEngine

    w = WORKLOADS["c2"]
    n = args.rows
    eng = QNetEngine((84, 84, 4), w["n_actions"], 1 + w["K"], FEATURES, "cnn", True, w["B"], gamma_n=0.99 ** w["n"], learning_rate=6.25e-5,
                     adam_eps=1.5e-4, precision="bf16x3", device="cuda:0")
    eng.init_params(0)
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (n * 4, 84 * 84), dtype=np.uint8)).cuda()
    ids = torch.arange(n * 4, dtype=torch.int32, device="cuda")
    inp = dict(frames=frames, frame_stride=84 * 84, frame_ids=ids, n_rows=n)
    legs = {"mirror": eng.rebuild_mirror, "forward": lambda: eng.forward(**inp), "analysis": lambda: eng.analysis(**inp)}
    counts = {}
    if hasattr(eng, "redo"):
        fresh = eng.fresh_params(1)
        start = eng.params.clone()

        def redo(tau, key):
            _, _, c = eng.redo(tau=tau, fresh=fresh, **inp)
            counts[key] = c

        legs["redo_none"] = lambda: redo(0.0, "redo_none")
        legs["redo_all"] = lambda: redo(1e30, "redo_all")
    torch.cuda.synchronize()

    def leg(name, calls):
        if name.startswith("redo"):
            eng.params.copy_(start)  # (redo_all leaves a network whose weights into every layer but the first are 0)
            eng.adam_m.fill_(1.0)
            eng.adam_v.fill_(1.0)
        fn = legs[name]
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    for name in legs:
        leg(name, 20)  # clocks, caches
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name in legs:
            ms[name].append(leg(name, args.calls))
    med = {k: statistics.median(v) for k, v in ms.items()}
    derived = {"forward_only": med["forward"] - med["mirror"]}
    derived["analysis_sums"] = med["analysis"] - derived["forward_only"] - med["mirror"]
    out = dict(shape="c2", rows=n, calls_per_leg=args.calls, ms_per_call=ms, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in ms.items()})
    if "redo_none" in med:
        derived["score"] = med["redo_none"] - derived["forward_only"] - 2 * med["mirror"]
        derived["recycle"] = med["redo_all"] - med["redo_none"]
        derived["bound_analysis_sums_plus_mirror"] = derived["analysis_sums"] + med["mirror"]
        out["recycled"] = {k: v.cpu().tolist() for k, v in counts.items()}
        torch.cuda.synchronize()
        host = []
        for k in range(5):
            t0 = time.perf_counter()
            eng.fresh_params(100 + k)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        out["fresh_params_host_ms"] = host
    out["derived_ms"] = derived
    print(json.dumps(out))


if __name__ == "__main__":
    main()
