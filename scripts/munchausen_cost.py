"""What Munchausen targets (isdqn_net_config::munchausen_tau) cost: the c2-shaped captured step (bench.py's replica: B = 256, A = 9,
uniform sampling, n = 1) with the option off and on (tau 0.03, alpha 0.9, clip -1), alternating, device synchronise at both ends of
every timed leg --
  * the iS-DQN form (K = 9): the value head's state row lies in the LDS rows the head chain already holds, 2 A expf and two logf per
    (transition, head) where the max loop runs;
  * the DQN form (one head, separate target parameters): the target forward covers concat(state, next_state) instead of the B next
    states (one more B-row forward) into "q_target"; the mirror is rebuilt twice per step either way.

    python scripts/munchausen_cost.py [--capacity 200000] [--graph 20] [--replays 50] [--rounds 5]

Prints one JSON line: ms per step of every leg, the medians, each form's difference against its OWN munchausen_tau = 0 legs of the
same run and the spread of those legs.  It compares this build with itself: the cost of the feature, nothing a test may depend on.  bench.py
stays the measure of the default step."""
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
    ap.add_argument("--capacity", type=int, default=200_000)
    ap.add_argument("--graph", type=int, default=20, help="steps per captured graph")
    ap.add_argument("--replays", type=int, default=50, help="graph replays per timed leg")
    ap.add_argument("--rounds", type=int, default=5, help="alternations off / on")
    args = ap.parse_args()

    import torch

    from bench import FEATURES, WORKLOADS, Replica
    from slimdqn._engine import QNetEngine
    from slimdqn._graph import GraphedUpdate

    S, w = args.graph, WORKLOADS["c2"]
    r = Replica("c2", args.capacity, "bf16x3", 0, "cuda:0", trust_mirror=True)  # the replay and the iS-DQN engine without the option

    def engine(n_heads, on):
        eng = QNetEngine((84, 84, 4), w["n_actions"], n_heads, FEATURES, "cnn", True, w["B"], gamma_n=0.99 ** w["n"], learning_rate=6.25e-5,
                         adam_eps=1.5e-4, precision="bf16x3", device="cuda:0", munchausen_tau=0.03 if on else 0.0)
        eng.init_params(0)
        eng.trust_mirror = True
        return eng

    engines = {("isdqn", False): r.eng, ("isdqn", True): engine(1 + w["K"], True), ("dqn", False): engine(1, False), ("dqn", True): engine(1, True)}
    targets = {k: e.params.clone() for k, e in engines.items() if k[0] == "dqn"}
    live = [None]

    def leg(form, on, replays, warm):
        """One leg: its captured update replaces the previous leg's (one live executable graph at a time: DESIGN.md 6), a short
        warm-up, then `replays` timed replays between two device synchronisations."""
        if live[0] is not None:
            live[0].destroy()
        eng = engines[(form, on)]
        learn = None if form == "isdqn" else (lambda cb, e=eng, t=targets[(form, on)]: e.learn_on_batch_target(cb, t))
        g = live[0] = GraphedUpdate(r.rb, eng, False, S, learn=learn)
        for _ in range(warm):
            g.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(replays):
            g.run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (replays * S) * 1e3

    leg("isdqn", False, 1, max(4, 4000 // S))  # clocks, caches, the sampler's first prefetch block
    ms = {f"{form}-{'on' if on else 'off'}": [] for form in ("isdqn", "dqn") for on in (False, True)}
    for _ in range(args.rounds):
        for form in ("isdqn", "dqn"):
            for on in (False, True):
                ms[f"{form}-{'on' if on else 'off'}"].append(leg(form, on, args.replays, 8))
    live[0].destroy()
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(workload="c2-shaped captured step", capacity=args.capacity, steps_per_graph=S, replays_per_leg=args.replays, ms_per_step=ms,
               median_ms=med)
    for form in ("isdqn", "dqn"):
        off, on = med[f"{form}-off"], med[f"{form}-on"]
        out[form] = dict(cost_ms=on - off, cost_percent=100.0 * (on / off - 1.0), spread_off_ms=max(ms[f"{form}-off"]) - min(ms[f"{form}-off"]))
    for k, e in engines.items():
        assert torch.isfinite(e.losses_accum).all(), k
    print(json.dumps(out))


if __name__ == "__main__":
    main()
