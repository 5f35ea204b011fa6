"""What gradual magnitude pruning costs (include/isdqn_hip.h, isdqn_net_prune_*), measured on the GPU from ONE build in ONE process:

  the captured step at the headline shape (cnn 32 64 64 512 + LN, K = 9, A = 9, B = 32, learn_steps of 8) without the option -- the
    step of a build that never heard of it: no node, no buffer -- and with the apply node behind every learn call at sparsity ~0 (one
    element pruned, so that the node is there), 0.5 and 0.95; legs interleaved, one untimed round, the median of --rounds rounds;
  the apply launch alone at the three sparsities (device events around --calls back-to-back calls), beside its byte model: the mask
    words read plus 8 bytes per pruned element (4 in the master, 4 in the mirror) over a measured device-to-device copy rate, plus one
    launch;
  one isdqn_net_prune_update from a full mask to sparsity 0.5 at -f 32 64 64 512 and -f 32 64 64 2048 (device events, the median).

    python scripts/prune_cost.py [--steps 200] [--rounds 5] [--capacity 20000]

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

K, A, S = 9, 9, 8
SPARSITIES = (0.0, 0.5, 0.95)


def _replay(args, B):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(0), B, args.capacity, stack_size=4, update_horizon=3, gamma=0.99)
    rb.prefill_synthetic(args.capacity, (84, 84), A, seed=0)
    return rb


def _agent(width, pruned, captured=True):
    from slimdqn.networks.isdqn import iSDQN

    kw = dict(prune_sparsity=0.95, prune_start=0, prune_end=1, prune_period=8000) if pruned else {}
    return iSDQN(0, (84, 84, 4), A, K, [32, 64, 64, width], True, False, "cnn", 6.25e-5, 0.99, 3, 1, 8000, adam_eps=1.5e-4, batch_size=32,
                 use_graph=captured, **kw)


def _counts(eng, sparsity):
    n = [i[3] for i in eng.prune_infos]
    return [1] + [0] * (len(n) - 1) if sparsity == 0.0 else [int(sparsity * x) for x in n]


def _set_sparsity(agent, sparsity):
    """The mask of ``sparsity`` on the agent's engine, and the schedule told so: the node is behind every step from here on."""
    eng = agent._engine
    eng.prune_mask.fill_(-1)
    counts = _counts(eng, sparsity)
    eng.prune_update(counts)
    agent._prune.counts = counts


def step_cost(args):
    import torch

    legs = {"off": (_agent(512, False), _replay(args, 32))}
    for s in SPARSITIES:
        legs[f"s{s}"] = (_agent(512, True), _replay(args, 32))
        _set_sparsity(legs[f"s{s}"][0], s)

    def run(agent, rb, n):
        agent._captures = 0  # (learn_steps captures what its first call asks for: S steps; the calls behind it replay that graph)
        for _ in range(n // S):
            agent.learn_steps(S, rb)

    n = args.steps // S * S
    ms = {k: [] for k in legs}
    for r in range(args.rounds + 1):  # (round 0 is untimed: clocks, caches, the sampler's first prefetch block)
        for k, (agent, rb) in legs.items():
            run(agent, rb, 4 * S)  # the leg's warm-up and its capture (one live executable graph at a time)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(agent, rb, n)
            torch.cuda.synchronize()
            if r > 0:
                ms[k].append((time.perf_counter() - t0) / n * 1e3)
            agent._drop_graph()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(ms_per_step=ms, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in ms.items()},
                cost_us_per_step={k: (med[k] - med["off"]) * 1e3 for k in med if k != "off"},
                losses_finite={k: bool(torch.isfinite(a._engine.losses_accum).all()) for k, (a, _rb) in legs.items()})


def _timed(fn, rounds, calls=1, before=None):
    import torch

    times = []
    for _ in range(rounds):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / calls * 1e3)
    return statistics.median(times)


def kernel_cost(args):
    """engine.prune_apply alone (master and mirror), the copy rate of a buffer of the parameters' size and of 256 MiB, an empty-ish launch
    (the apply pass on a full mask: the mask is read, nothing is written), and one prune_update per torso width."""
    import torch

    out = {}
    for width in (512, 2048):
        agent = _agent(width, True, captured=False)
        eng = agent._engine
        start = eng.params.clone()
        n_real = [i[3] for i in eng.prune_infos]

        def fresh():
            eng.params.copy_(start)
            eng.prune_mask.fill_(-1)

        half = [x // 2 for x in n_real]
        row = dict(n_param_floats=int(eng.n_param_floats), n_real=n_real,
                   update_to_half_us=_timed(lambda: eng.prune_update(half), args.rounds, before=fresh))
        if width == 512:
            other = torch.empty_like(start)
            big_a, big_b = torch.empty(64 << 20, device=eng.device), torch.empty(64 << 20, device=eng.device)
            for _ in range(3):
                other.copy_(start)
                big_b.copy_(big_a)
            copy_us = _timed(lambda: other.copy_(start), args.rounds, calls=50)
            big_us = _timed(lambda: big_b.copy_(big_a), args.rounds, calls=10)
            row["copy_gb_per_s"] = dict(params_sized=2 * start.numel() * 4 / copy_us * 1e-3, mib_256=2 * (256 << 20) / big_us * 1e-3)
            fresh()
            row["apply_full_mask_us"] = _timed(eng.prune_apply, args.rounds, calls=args.calls)
            row["apply"] = {}
            for s in SPARSITIES:
                fresh()
                counts = _counts(eng, s)
                eng.prune_update(counts)
                us = _timed(eng.prune_apply, args.rounds, calls=args.calls)
                written = 8 * sum(counts)
                read = 4 * int(eng.prune_mask.numel())
                rate = row["copy_gb_per_s"]["params_sized"] * 1e3  # bytes per us
                row["apply"][f"s{s}"] = dict(call_us=us, bytes_written=written, mask_bytes_read=read,
                                             model_us=row["apply_full_mask_us"] + written / rate)
        out[f"f{width}"] = row
        del agent, eng
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="prune_apply calls per timed sample of the kernel alone")
    ap.add_argument("--capacity", type=int, default=20_000)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is nothing to fall back to"
    out = dict(device=torch.cuda.get_device_name(0), steps_per_graph=S)
    out["kernel"] = kernel_cost(args)
    out["captured_step"] = step_cost(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
