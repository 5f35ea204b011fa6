"""CPU check of the seeds of tests/test_gpu_dueling.py (no GPU).  Section 3: for every committed case and both precisions the float64
model -- oracle.network's forward with the masked raw head, the helper's combine, the float64 loss helper -- gives the pairs the argmax
rule would leave out at the case's precision bound (top-two gap of the deciding head's action values below 10 x the q bound x
max(1, |Q|max)) and the smallest gap: the committed cases leave out none.

    python scripts/dueling_seeds.py
"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "is-dqn_amd")]

from tests import test_gpu_dueling as T  # noqa: E402

if __name__ == "__main__":
    bad = 0
    for name in T.E2E:
        for prec in T.PRECISIONS:
            c = T.oracle_case(name, prec)
            bound = 10 * T.TOL[prec]["q"] * c["scale"]
            out = int((c["gap"] < bound).sum())
            bad += out
            losses = c["ref"]["losses"].detach().numpy()
            print(f"{name:20s} {prec:7s} left out {out} of {c['gap'].size}, min gap {c['gap'].min():.3g} (bound {bound:.3g}), |Q|max {c['scale']:.3g}, "
                  f"losses {losses.min():.3g} .. {losses.max():.3g}", flush=True)
    sys.exit(1 if bad else 0)
