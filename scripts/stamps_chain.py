"""scripts/stamps.py's set-up; prints the workgroup chain of one layer's forward kernel: last (start + stamped duration) after the first start."""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
import numpy as np, torch
from slimdqn._engine import QNetEngine
from slimdqn import _hip
B, K, A = 256, 9, 9
eng = QNetEngine((84, 84, 4), A, 1 + K, (32, 64, 64, 512), "cnn", True, B, gamma_n=0.99, learning_rate=6.25e-5, adam_eps=1.5e-4)
eng.init_params(0)
nf = 100_000
g = torch.Generator(device="cuda").manual_seed(0)
frames = torch.randint(0, 256, (nf, 84 * 84), dtype=torch.uint8, device="cuda", generator=g)
base = torch.randint(0, nf - 8, (B, 1), device="cuda", generator=g)
ids = (base + torch.arange(4, device="cuda")[None, :]).int()
ids = torch.cat([ids, ids + 1], 1).contiguous()
batch = eng.make_batch(frames=frames, frame_stride=84 * 84, frame_ids=ids, action=torch.randint(0, A, (B,), device="cuda", generator=g).int(),
                       reward=torch.randn(B, device="cuda", generator=g), terminal=torch.zeros(B, dtype=torch.uint8, device="cuda"))
for _ in range(20):
    eng.learn_on_batch(batch)
lib = _hip.lib()
lib.isdqn_debug_set_stamps.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
GHZ = 2.38
for layer in sys.argv[1:]:
    last = 6 if layer == "Conv_0" else 5
    res = []
    for rep in range(9):
        st = torch.zeros(4096 * 8, dtype=torch.int64, device="cuda")
        lib.isdqn_debug_set_stamps(ctypes.c_void_p(st.data_ptr()), layer.encode())
        eng.learn_on_batch(batch)
        torch.cuda.synchronize()
        lib.isdqn_debug_set_stamps(None, b"")
        s = st.cpu().numpy().reshape(4096, 8)
        s = s[s[:, 7] != 0]
        rt = (s[:, 7] - s[:, 7].min()) / 100.0
        tot = (s[:, last] - s[:, 0]) / GHZ / 1e3
        ok = s[:, last] != 0
        res.append((len(s), float(np.median(tot[ok])), float(rt.max()), float((rt + tot)[ok].max())))
    r = np.array(res)
    print(f"{layer}: workgroups {int(r[0,0])}  per-WG stamped total median {np.median(r[:,1]):.2f} us  last start {np.median(r[:,2]):.2f} us  "
          f"chain (last start+total) median {np.median(r[:,3]):.2f} min {r[:,3].min():.2f} max {r[:,3].max():.2f} us  [@{GHZ} GHz, 9 steps]")
