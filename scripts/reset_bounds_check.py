"""Run the reset and EMA entry points (include/isdqn_hip.h, isdqn_net_reset / isdqn_net_ema) of a bounds-checked build (-DISDQN_BOUNDS;
scripts/bounds_check.py holds the registration helpers) with the EXACT extents of the buffers they are given registered -- parameters,
both moments, the step count, the fresh parameters, a target copy, the workspace -- and print one JSON line per case: {"case", "bad",
"site", "addr"}.  Sites 46 (every load and store of reset_kernel, the count store) and 47 (every load and store of ema_kernel) are the
new kernels' accesses.  Started by tests/test_gpu_reset_bounds.py with ISDQN_HIP_LIB pointing at that build."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

from bounds_check import engine_tensors, register, report
from slimdqn._engine import QNetEngine


def run_case(name, arch, obs, feats, K, A, B, ln=True, bn=False):
    eng = QNetEngine(obs, A, 1 + K, feats, arch, ln, B, batch_norm=bn)
    eng.init_params(0)
    eng.adam_m.fill_(0.25)
    eng.adam_v.fill_(0.5)
    fresh = eng.fresh_params(1)
    target = eng.params.clone()
    torch.cuda.synchronize()
    register(engine_tensors(eng) + [fresh, target])
    n_layers, first = eng.reset_layout()
    eng.reset(fresh, first)                          # the agents' call: blend below the first Dense, replace from there on
    eng.reset(fresh, 0, 0.8, 0.2, 0.3, 0.7)          # every tensor in the upper class, a general blend
    eng.reset(fresh, n_layers, 0.8, 0.2, 0.0, 1.0)   # every tensor in the lower class
    eng.reset(fresh, first, params=target)           # a target copy: no moments, no count, no mirror
    eng.ema(target, 0.005)
    eng.ema(target, 1.0)
    report(name)
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    cases = [
        dict(name="reset-cnn-B4", arch="cnn", obs=(84, 84, 4), feats=(8, 12, 16, 24), K=2, A=5, B=4),
        dict(name="reset-impala-bn-B4", arch="impala", obs=(36, 36, 2), feats=(16, 8, 16, 24), K=2, A=5, B=4, ln=False, bn=True),
    ]
    for c in cases:
        if which != "all" and which not in c["name"]:
            continue
        run_case(**c)
