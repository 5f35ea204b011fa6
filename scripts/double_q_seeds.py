"""CPU check of the seeds of tests/test_gpu_double_q.py, section 5 (no GPU): for every case the float64 oracle forward and the float64
helper give the share of (b, k) pairs whose a* differs from the value head's own argmax, the largest move of a target against the max
form, and the pairs the argmax rule would leave out at the case's precision bound (selector gap below 10 x the q bound x max(1, |q|max)).

    python scripts/double_q_seeds.py            # the committed seeds
    python scripts/double_q_seeds.py --scan 40  # batch seeds 0..39 per case: the first that leaves out none
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "is-dqn_amd")]

from tests import test_gpu_double_q as T  # noqa: E402


def report(name):
    c = T.oracle_case(name)
    ref = c["ref"]
    bound = 10 * T.TOL[T.E2E_PRECISION.get(name, "bf16x3")]["q"] * c["scale"]
    out = int((c["gap"] < bound).sum())
    share = float((ref["a_star"] != ref["greedy"]).mean())
    moved = float(np.abs(ref["targets"] - ref["max_targets"]).max())
    return out, share, moved, float(c["gap"].min()), bound


if __name__ == "__main__":
    scan = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--scan" else 0
    for name in T.E2E:
        if scan:
            case = list(T.E2E[name])
            for s in range(scan):
                T.E2E[name] = tuple(case[:-1] + [s])
                out, share, moved, gap, bound = report(name)
                if out == 0 and share >= 0.3 and moved > 0.1:
                    break
            print(f"{name:12s} batch seed {s}: left out {out}, a* != greedy {share:.2f}, max move {moved:.3g}, min gap {gap:.3g} (bound {bound:.3g})", flush=True)
        else:
            out, share, moved, gap, bound = report(name)
            print(f"{name:12s} left out {out} of {T.oracle_case(name)['gap'].size}, a* != greedy {share:.2f}, max move {moved:.3g}, min gap {gap:.3g} "
                  f"(bound {bound:.3g})", flush=True)
