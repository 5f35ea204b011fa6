"""CPU check of the seeds of tests/test_gpu_quantile.py (no GPU).  Section 3: for every case the float64 oracle forward and the float64
helper give the pairs the argmax rule would leave out at the case's precision bound (top-two gap of the deciding head's means below
10 x the q bound x max(1, |Q|max)), the smallest gap and the share of u_ij < 0.  With --own-rows also the preconditions that sections 2
and 5 assert on the device's rows -- share of u_ij < 0 in [0.2, 0.8], terminal rows present, every gap above 1e-5 x max(1, |Q|max), a*
off the value head's own argmax on a quarter of the pairs -- evaluated on the oracle forward of the same parameters and batch.

    python scripts/quantile_seeds.py             # the committed cases of section 3
    python scripts/quantile_seeds.py --own-rows  # sections 2 and 5 as well
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "is-dqn_amd")]

from oracle import network as onet  # noqa: E402
from tests import test_gpu_quantile as T  # noqa: E402
from tests.helpers import quantile as qr  # noqa: E402


def own_rows(tag, feats, K, A, B, arch, N, kappa, pseed, bseed, double_q=False, single=False):
    n_heads = 1 if single else 1 + K
    p = onet.to_torch(T._params(pseed, feats, A, n_heads, arch, N), torch.float64)
    b = T._Batch(None, arch, B, A, seed=bseed)
    rows = torch.cat([onet.forward(p, b.x_state, feats, arch, True), onet.forward(p, b.x_next, feats, arch, True)])
    vrows = None
    if single:
        tp = onet.to_torch(T._params(T.TARGET_SEED, feats, A, 1, arch, N), torch.float64)
        vrows = onet.forward(tp, b.x_next, feats, arch, True)
    on0 = 0 if single else 1
    ref = qr.qr_loss(rows, b.action, b.reward, b.terminal, float(np.float32(0.99)), K, on0, 0, A, N, kappa, value_rows=vrows,
                     selector_rows=rows[B:] if double_q else None)
    val = qr.means(rows[B:] if vrows is None else vrows, N).reshape(B, -1, A)[:, :K]
    off = float((ref["a_star"] != qr.first_argmax(val)).double().mean())
    print(f"{tag:34s} u<0 {ref['neg_share']:.2f}  terminal {int(b.terminal.sum())}/{B}  min gap {float(ref['gap'].min()):.3g} "
          f"(needs > {1e-5 * max(1.0, ref['qmax']):.2g})  a* off the value argmax {off:.2f}", flush=True)


if __name__ == "__main__":
    for name in T.E2E:
        c = T.oracle_case(name)
        bound = 10 * T.TOL[T.E2E[name][6]]["q"] * c["scale"]
        out = int((c["gap"] < bound).sum())
        print(f"{name:16s} left out {out} of {c['gap'].size}, min gap {c['gap'].min():.3g} (bound {bound:.3g}), u<0 {c['ref']['neg_share']:.2f}", flush=True)
    if "--own-rows" in sys.argv:
        for param in T.OWN_ROWS:
            N, kappa, K, A, B, arch, feats = param.values[0]
            own_rows("2 " + param.id, feats, K, A, B, arch, N, kappa, 0, 5)
        own_rows("4 cnn-tiny", T.TINY, 3, 5, 6, "cnn", 32, 1.0, 4, 13)
        own_rows("4 fc", (32, 32), 2, 4, 9, "fc", 32, 1.0, 4, 13)
        own_rows("5 isdqn tiny-N33", T.TINY, 3, 5, 6, "cnn", 33, 1.0, 2, 5, double_q=True)
        own_rows("5 isdqn fc-B11-ragged", (16, 16), 2, 3, 11, "fc", 32, 1.0, 2, 5, double_q=True)
        own_rows("5 dqn tiny-N33", T.TINY, 1, 5, 6, "cnn", 33, 1.0, 2, 5, double_q=True, single=True)
        own_rows("5 dqn fc-B11-ragged", (16, 16), 1, 3, 11, "fc", 32, 1.0, 2, 5, double_q=True, single=True)
