"""What Normalize-and-Project costs (include/isdqn_hip.h, isdqn_net_project_*), measured on the GPU from ONE build in ONE process, in the
protocol of scripts/prune_cost.py:

  the captured step at the headline shape (cnn 32 64 64 512 + LN, K = 9, A = 9, B = 32, learn_steps of 8) without the option -- the
    step of a build that never heard of it: no node, no buffer -- and with the projection behind every learn call; legs interleaved, one
    untimed round, the median of --rounds rounds;
  the two launches alone (device events around --calls back-to-back calls): isdqn_net_project_norms is the first launch (the chunk sums)
    plus a launch of one workgroup per tensor, isdqn_net_project_apply is both launches -- the target norms alternate between rho and
    1.25 rho from call to call, so that every call has a scale away from 1 and stores every element --, the second launch is the
    difference; beside them the byte model: 4 bytes read per real element in each of the two passes and 8 written (master and mirror)
    over the device-to-device copy rate of a buffer of the parameters' size, measured in the same process;
  the same two entry points on fc [20, 14] (440 real elements): the fixed cost of two dependent launches.

    python scripts/nap_cost.py [--steps 200] [--rounds 5] [--capacity 20000]

Prints one JSON line.  It compares this build with ITSELF: the cost of the option, nothing a test may depend on.  bench.py stays the
measure of the default step."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))

K, A, S = 9, 9, 8


def _replay(args, B):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(0), B, args.capacity, stack_size=4, update_horizon=3, gamma=0.99)
    rb.prefill_synthetic(args.capacity, (84, 84), A, seed=0)
    return rb


def _agent(projected, captured=True):
    from slimdqn.networks.isdqn import iSDQN

    kw = dict(weight_projection=True) if projected else {}
    return iSDQN(0, (84, 84, 4), A, K, [32, 64, 64, 512], True, False, "cnn", 6.25e-5, 0.99, 3, 1, 8000, adam_eps=1.5e-4, batch_size=32,
                 use_graph=captured, **kw)


def step_cost(args):
    import torch

    legs = {"off": (_agent(False), _replay(args, 32)), "nap": (_agent(True), _replay(args, 32))}

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
    nap = legs["nap"][0]
    return dict(ms_per_step=ms, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in ms.items()},
                cost_us_per_step=(med["nap"] - med["off"]) * 1e3, last_scales=nap.nap_target_update(0),
                losses_finite={k: bool(torch.isfinite(a._engine.losses_accum).all()) for k, (a, _rb) in legs.items()})


def _timed(fn, rounds, calls=1):
    import torch

    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / calls * 1e3)
    return statistics.median(times)


def _calls(eng):
    """(apply, norms): the two entry points on the engine's own parameters and mirror, straight through the C ABI (no host read); the
    target norms of successive apply calls alternate between rho and 1.25 rho."""
    from slimdqn import _hip

    targets = [eng.project_target.clone(), eng.project_target * 1.25]
    cfg, stream = ctypes.byref(eng.cfg), _hip.stream_ptr(eng.device)
    fixed = (_hip.ptr(eng.project_norms_out), _hip.ptr(eng.project_scales), _hip.ptr(eng.project_scratch), _hip.ptr(eng.workspace), stream)
    turn = [0]

    def apply():
        turn[0] ^= 1
        _hip.check(eng.lib.isdqn_net_project_apply(cfg, _hip.ptr(eng.params), _hip.ptr(targets[turn[0]]), *fixed), "isdqn_net_project_apply")

    def norms():
        _hip.check(eng.lib.isdqn_net_project_norms(cfg, _hip.ptr(eng.params), fixed[0], fixed[2], stream), "isdqn_net_project_norms")

    return apply, norms


def fixed_cost(args):
    """The same two entry points on fc [20, 14] -- 440 real elements in two workgroups: what two dependent launches cost with next to
    nothing to move."""
    from slimdqn._engine import QNetEngine

    eng = QNetEngine((8,), 4, 3, (20, 14), "fc", False, 4)
    eng.init_params(0)
    eng.set_weight_projection()
    apply, norms = _calls(eng)
    for _ in range(4):
        apply()
        norms()
    return dict(norms_call_us=_timed(norms, args.rounds, calls=args.calls), apply_call_us=_timed(apply, args.rounds, calls=args.calls))


def kernel_cost(args):
    """The two entry points alone on the engine's own parameters (master and mirror), and the copy rate of a buffer of their size."""
    import torch

    agent = _agent(True, captured=False)
    eng = agent._engine
    start = eng.params.clone()
    n_real = [i[3] for i in eng.project_infos]
    k = len(n_real)
    other = torch.empty_like(start)
    for _ in range(3):
        other.copy_(start)
    copy_us = _timed(lambda: other.copy_(start), args.rounds, calls=50)
    rate = 2 * start.numel() * 4 / copy_us  # bytes per us, reads and writes counted
    apply, norms = _calls(eng)
    for _ in range(4):
        apply()
        norms()
    norms_us = _timed(norms, args.rounds, calls=args.calls)
    apply_us = _timed(apply, args.rounds, calls=args.calls)
    scales = [float(x) for x in eng.project_scales[:k].cpu()]
    total = sum(n_real)
    model = dict(sumsq_us=4 * total / rate, scale_us=12 * total / rate, apply_us=16 * total / rate)
    return dict(n_param_floats=int(eng.n_param_floats), n_real=n_real, copy_gb_per_s=rate * 1e-3, norms_call_us=norms_us, apply_call_us=apply_us,
                second_launch_us=apply_us - norms_us, model_us=model, apply_over_model=apply_us / model["apply_us"], last_scales=scales)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed sample of an entry point alone")
    ap.add_argument("--capacity", type=int, default=20_000)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is nothing to fall back to"
    out = dict(device=torch.cuda.get_device_name(0), steps_per_graph=S)
    out["kernel"] = kernel_cost(args)
    out["two_launches_on_440_elements"] = fixed_cost(args)
    out["captured_step"] = step_cost(args)
    out["step_cost_over_model"] = out["captured_step"]["cost_us_per_step"] / out["kernel"]["model_us"]["apply_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
