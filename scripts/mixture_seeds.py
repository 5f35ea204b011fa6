"""CPU check of the seeds of tests/test_gpu_mixture.py (no GPU): for every case of section 2 and both torsos of section 4 the float64
oracle forward and the float64 helper give the transitions the argmax rule would leave out -- those whose two largest mixed next-state
values are closer than 10 x the q bound -- and the smallest gap beside that bound.  The committed seeds leave out none.

    python scripts/mixture_seeds.py            # the committed seeds
    python scripts/mixture_seeds.py --scan 40  # section 4: batch seeds 0..39 per torso, the first that leaves out none
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "is-dqn_amd")]

from tests import test_gpu_mixture as T  # noqa: E402

if __name__ == "__main__":
    scan = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--scan" else 0
    total = 0
    for H, A, B in T.CASES:
        for option in T.OPTIONS:
            for form in ("target", "same"):
                ref, fl = T.oracle_case(H, A, B, option, form)
                out = int((ref["gap"] < 10 * fl["q_values"]).sum())
                total += out
                print(f"H={H:<4d} A={A:<3d} B={B:<3d} {option:9s} {form:6s}: left out {out} of {B}, min gap {ref['gap'].min():.3g} "
                      f"(bound {10 * fl['q_values'].max():.3g})", flush=True)
    for arch in T.E2E:
        seeds = range(scan) if scan else [T.E2E[arch]]
        for s in seeds:
            T.E2E[arch] = s
            gap, bound = T.e2e_gaps(arch)
            out = int((gap < bound).sum())
            if out == 0 or not scan:
                break
        total += out
        print(f"whole path {arch:4s} batch seed {s}: left out {out} of {gap.size}, min gap {gap.min():.3g} (bound {bound:.3g})", flush=True)
    print(f"left out in all: {total}")
    sys.exit(1 if total else 0)
