"""What the soft head shift costs (include/isdqn_hip.h, isdqn_net_soft_shift), measured on the GPU from ONE build
(scripts/conservative_cost.py's pattern):

  the step at the headline shape (cnn 32 64 64 512 + LN, K = 9, A = 9, B = 32) with soft_shift_tau = 0.005 and with tau = 0 (the hard
  shift, which no step of the timed region runs), on scalar heads (100 rows of 512 columns) and on histogram heads (-hl -nb 51: 4590
  rows): learn_steps as one captured graph of S = 8 -- where the shift is one more node per step -- and eager update_online_params, on
  a uniform replay.  A host clock around --steps steps that end in a device synchronise, the two agents alternating over --rounds
  rounds, medians and spread;
  the kernel alone: engine.soft_shift with the workspace (master + mirror) and on a copy (master alone), device events around --calls
  calls, with the bytes it moves: heads 0 .. K read, heads 0 .. K-1 written, and their mirror rows written.

    python scripts/soft_shift_cost.py [--steps 200] [--rounds 5] [--capacity 20000]

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

TAU = 0.005
HEADS = {"scalar": {}, "histogram_51": dict(n_bins=51, min_value=-10.0, max_value=10.0, sigma=0.3)}
K, A = 9, 9


def _replay(args, B):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(0), B, args.capacity, stack_size=4, update_horizon=3, gamma=0.99)
    rb.prefill_synthetic(args.capacity, (84, 84), A, seed=0)
    return rb


def _agent(args, heads, captured, tau):
    from slimdqn.networks.isdqn import iSDQN

    return iSDQN(0, (84, 84, 4), A, K, [32, 64, 64, 512], True, False, "cnn", 6.25e-5, 0.99, 3, 1, 8000, adam_eps=1.5e-4, batch_size=32,
                 use_graph=captured, soft_shift_tau=tau, **HEADS[heads]), _replay(args, 32)


def step_cost(args, heads, captured):
    import torch

    S = 8
    legs = {"hard": _agent(args, heads, captured, 0.0), "soft": _agent(args, heads, captured, TAU)}

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
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    finite = {k: bool(torch.isfinite(a._engine.losses_accum).all()) for k, (a, _rb) in legs.items()}
    moved = not torch.equal(legs["hard"][0]._engine.params, legs["soft"][0]._engine.params)
    return dict(ms_per_step=ms, median_ms=med, spread_ms=spread, cost_us_per_step=(med["soft"] - med["hard"]) * 1e3, losses_finite=finite,
                legs_differ=moved)


def kernel_cost(args, heads):
    """engine.soft_shift alone, back to back on one stream: with the workspace (master and mirror) and on a copy (master alone)."""
    import torch

    agent, _rb = _agent(args, heads, False, 0.0)
    eng = agent._engine
    copy = eng.params.clone()
    last = max(i.layer for i in eng.infos)
    kernel = next(i for i in eng.infos if i.layer == last and i.kind == 1)
    in_p = int(kernel.dims[1])
    R = A * max(int(eng.cfg.n_bins), 1)
    head_bytes = R * (in_p + 1) * 4
    moved = dict(master_and_mirror=((1 + K) + 2 * K) * head_bytes, master=((1 + K) + K) * head_bytes)
    us = {}
    for name, kw in (("master_and_mirror", {}), ("master", dict(params=copy))):
        for _ in range(20):
            eng.soft_shift(TAU, **kw)
        times = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                eng.soft_shift(TAU, **kw)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.calls * 1e3)
        us[name] = statistics.median(times)
    return dict(call_us=us, bytes_moved=moved, rows_per_head=R, columns=in_p,
                gb_per_s={k: moved[k] / us[k] * 1e-3 for k in us})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="soft_shift calls per timed sample of the kernel alone")
    ap.add_argument("--capacity", type=int, default=20_000)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is nothing to fall back to"
    out = dict(device=torch.cuda.get_device_name(0), soft_shift_tau=TAU)
    for heads in HEADS:
        out[heads] = {"captured_S8" if cap else "eager": step_cost(args, heads, cap) for cap in (True, False)}
        out[heads]["kernel"] = kernel_cost(args, heads)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
