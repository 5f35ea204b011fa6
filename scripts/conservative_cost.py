"""What the conservative (CQL) term costs (include/isdqn_hip.h, isdqn_batch_conservative), measured on the GPU from ONE build
(scripts/weight_decay_cost.py's pattern):

  the step at the headline shape (cnn 32 64 64 512 + LN, K = 9, A = 9, B = 32) with cql_alpha = 1 and without, on scalar heads -- where
  the term also takes the learn step off the head chain, as dueling heads do -- and on quantile heads (-qr -nq 51), which run the generic
  loss either way: eager update_online_params, and learn_steps as one captured graph of S = 8, on a uniform replay.  A host clock around
  --steps steps that end in a device synchronise, the two agents alternating over --rounds rounds, medians and spread;
  the term's own kernel: the loss-only call with and without the flag behind the same batch, device events around --calls calls.

    python scripts/conservative_cost.py [--steps 200] [--rounds 5] [--capacity 20000]

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

CQL_ALPHA = 1.0
HEADS = {"scalar": {}, "quantile_51": dict(n_quantiles=51, huber_delta=1.0)}


def _replay(args, B):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(0), B, args.capacity, stack_size=4, update_horizon=3, gamma=0.99)
    rb.prefill_synthetic(args.capacity, (84, 84), 9, seed=0)
    return rb


def _agent(args, heads, captured, cql_alpha):
    from slimdqn.networks.isdqn import iSDQN

    return iSDQN(0, (84, 84, 4), 9, 9, [32, 64, 64, 512], True, False, "cnn", 6.25e-5, 0.99, 3, 1, 8000, adam_eps=1.5e-4, batch_size=32,
                 use_graph=captured, cql_alpha=cql_alpha, **HEADS[heads]), _replay(args, 32)


def step_cost(args, heads, captured):
    import torch

    S = 8
    legs = {"plain": _agent(args, heads, captured, 0.0), "cql": _agent(args, heads, captured, CQL_ALPHA)}

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
    moved = not torch.equal(legs["plain"][0]._engine.params, legs["cql"][0]._engine.params)
    return dict(ms_per_step=ms, median_ms=med, spread_ms=spread, cost_us_per_step=(med["cql"] - med["plain"]) * 1e3, losses_finite=finite,
                legs_differ=moved)


def kernel_cost(args, heads):
    """The loss-only call (forward, loss kernel, [the term's kernel], loss_finalize) with and without the flag: the difference of the two
    medians is the term's own launch and run time at this shape."""
    import torch

    agent, rb = _agent(args, heads, False, 0.0)
    eng = agent._engine
    samples = agent._sample(rb)  # (the batch an eager gradient step would train on)
    us = {}
    for name, alpha in (("plain", 0.0), ("cql", CQL_ALPHA), ("plain_again", 0.0)):
        eng.set_conservative(alpha)
        b = agent._c_batch(eng, samples)
        for _ in range(20):
            eng.loss_on_batch(b)
        times = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                eng.loss_on_batch(b)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.calls * 1e3)
        us[name] = statistics.median(times)
    return dict(loss_call_us=us, term_us=us["cql"] - 0.5 * (us["plain"] + us["plain_again"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="loss-only calls per timed sample of the term's own kernel")
    ap.add_argument("--capacity", type=int, default=20_000)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is nothing to fall back to"
    out = dict(device=torch.cuda.get_device_name(0), cql_alpha=CQL_ALPHA)
    for heads in HEADS:
        out[heads] = {"captured_S8" if cap else "eager": step_cost(args, heads, cap) for cap in (False, True)}
        out[heads]["term_kernel"] = kernel_cost(args, heads)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
