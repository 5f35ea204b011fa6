"""What REM, the random ensemble mixture, costs (include/isdqn_hip.h, isdqn_batch_mixture), measured on the GPU from ONE build in ONE
process:

  the captured DQN step at the headline torso (cnn 32 64 64 512 + LN, A = 18, B = 32 and B = 256) as a plain DQN -- the step of a build
    that never heard of the option: no node, no buffer --, with -rem 1 and with -rem 200; legs interleaved, one untimed round, the
    median of --rounds rounds;
  the draw alone (isdqn_mixture_draw: two launches; device events around --calls back-to-back calls);
  the byte model of mix_td_kernel beside them: 2B rows of H * A floats read (3B with double_q) plus the B dout rows of the padded
    width written once, over a measured device-to-device copy rate.

    python scripts/mixture_cost.py [--steps 200] [--rounds 5] [--capacity 20000]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/mixture_cost.py --kernels     # kernel times, in a run of their own

``--kernels`` runs eager learn steps of the -rem 1 and -rem 200 engines at both batch sizes and times nothing: the trace of that run
holds mixture_draw_kernel and mix_td_kernel by name.  Prints one JSON line.  It compares this build with ITSELF: the cost of the
option, nothing a test may depend on.  bench.py stays the measure of the default step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))

A = 18
LEGS = {"dqn": 0, "rem1": 1, "rem200": 200}
BATCHES = (32, 256)


def _replay(args, B):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(0), B, args.capacity, stack_size=4, update_horizon=3, gamma=0.99)
    rb.prefill_synthetic(args.capacity, (84, 84), A, seed=0)
    return rb


def _agent(H, B, captured=True):
    from slimdqn.networks.dqn import DQN

    kw = dict(rem_heads=H) if H else {}
    return DQN(0, (84, 84, 4), A, [32, 64, 64, 512], True, "cnn", 6.25e-5, 0.99, 3, 1, 8000, adam_eps=1.5e-4, batch_size=B, use_graph=captured, **kw)


def byte_model(H, B, double_q=False):
    pitch = (H * A + 7) // 8 * 8
    return dict(bytes_read=(3 if double_q else 2) * B * H * A * 4, bytes_written=B * pitch * 4)


def step_cost(args, B):
    import torch

    legs = {k: (_agent(H, B), _replay(args, B)) for k, H in LEGS.items()}

    def run(agent, rb, n):
        for _ in range(n):
            agent.update_online_params(0, rb)

    ms = {k: [] for k in legs}
    for r in range(args.rounds + 1):  # (round 0 is untimed: clocks, caches, the sampler's first prefetch block)
        for k, (agent, rb) in legs.items():
            run(agent, rb, 16)  # the leg's warm-up and its capture (one live executable graph at a time)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(agent, rb, args.steps)
            torch.cuda.synchronize()
            if r > 0:
                ms[k].append((time.perf_counter() - t0) / args.steps * 1e3)
            agent._drop_graph()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(ms_per_step=ms, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in ms.items()},
                cost_us_per_step={k: (med[k] - med["dqn"]) * 1e3 for k in med if k != "dqn"},
                draw_count={k: int(a._engine.mix_count.item()) for k, (a, _rb) in legs.items() if a.rem_heads},
                losses_finite={k: bool(torch.isfinite(a._engine.losses_accum).all()) for k, (a, _rb) in legs.items()})


def _timed(fn, rounds, calls):
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


def draw_cost(args):
    import torch

    out = {}
    a, b = torch.empty(64 << 20, device="cuda"), torch.empty(64 << 20, device="cuda")
    for _ in range(3):
        b.copy_(a)
    out["copy_gb_per_s_256_mib"] = 2 * (256 << 20) / _timed(lambda: b.copy_(a), args.rounds, 10) * 1e-3
    for k, H in LEGS.items():
        if H:
            eng = _agent(H, 32, captured=False)._engine
            for _ in range(10):
                eng.mixture_draw()
            out[k] = dict(draw_call_us=_timed(eng.mixture_draw, args.rounds, args.calls), bytes_written=4 * H + 8)
    return out


def kernels(args):
    """Eager learn steps for a kernel trace: nothing is timed here."""
    import torch

    for B in BATCHES:
        for k, H in LEGS.items():
            if H:
                agent, rb = _agent(H, B, captured=False), _replay(args, B)
                for _ in range(args.steps):
                    agent.update_online_params(0, rb)
                torch.cuda.synchronize()
    return dict(eager_steps_per_leg=args.steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="draw calls per timed sample")
    ap.add_argument("--capacity", type=int, default=20_000)
    ap.add_argument("--kernels", action="store_true", help="eager steps of the mixture legs for a kernel trace; times nothing")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is nothing to fall back to"
    out = dict(device=torch.cuda.get_device_name(0), n_actions=A)
    if args.kernels:
        out["kernels"] = kernels(args)
    else:
        out["byte_model"] = {f"{k}_B{B}": byte_model(H, B) for k, H in LEGS.items() if H for B in BATCHES}
        out["draw"] = draw_cost(args)
        out["captured_step"] = {f"B{B}": step_cost(args, B) for B in BATCHES}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
