"""Bit fingerprint of the first convolution's routes (csrc/conv_u8_pair.h against the one-tile kernel): small cnn networks at the
observation sizes, batch sizes, first-layer widths, LayerNorm and precision settings where the image kernel's index arithmetic takes
another path.  One line per case: SHA-256 of params, Adam moments, losses, q-values, targets and priorities after three learn steps,
of the loss-only pass and of a one-row forward.  Two builds of the library (ISDQN_HIP_LIB) must print identical lines.

usage: conv0_bits.py [case ...]      (default: every case; tests/test_gpu_conv0_image_kernel.py)"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))

# name: (observation side, B, first-layer width, LayerNorm, precision).  Output side = ceil(side / 4) (SAME padding, stride 4).
CASES = {
    "84-four-tiles-last-57px": (84, 3, 32, True, "bf16x3"),     # 21 x 21 = 441: two halves, waves 6-7 of half 1 dead
    "68-three-tiles-refused": (68, 3, 32, True, "bf16x3"),      # 17 x 17 = 289: odd tile count, one-tile kernel
    "52-two-tiles-second-41px": (52, 3, 32, True, "bf16x3"),    # 13 x 13 = 169: one half, waves 6-7 dead
    "64-two-full-tiles": (64, 3, 32, True, "bf16x3"),           # 16 x 16 = 256: one half, no dead wave
    "48-two-tiles-second-16px": (48, 3, 32, True, "bf16x3"),    # 12 x 12 = 144: one half, waves 5-7 dead
    "104-six-tiles": (104, 3, 32, True, "bf16x3"),              # 26 x 26 = 676: three halves (the third is requested under the second)
    "84-B1": (84, 1, 32, True, "bf16x3"),                       # n_img = 2: tail group only
    "84-B9": (84, 9, 32, True, "bf16x3"),                       # n_img = 18: two groups of eight and a tail
    "84-width16": (84, 3, 16, True, "bf16x3"),
    "84-width7": (84, 3, 7, True, "bf16x3"),                    # padded channels in channel tile 0
    "84-no-layernorm": (84, 3, 32, False, "bf16x3"),
    "84-bf16": (84, 3, 32, True, "bf16"),                       # <1, 8>: hi plane only
    "48-bf16-width7-no-layernorm": (48, 1, 7, False, "bf16"),
}


def main(names):
    import numpy as np, torch
    from tests.gpu_helpers import make_frame_batch, device_batch
    from slimdqn._engine import QNetEngine

    def h(t):
        return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]

    for name in names:
        side, B, width, ln, prec = CASES[name]
        K, A, stack = 2, 3, 4
        frames, ids, action, reward, terminal, _ = make_frame_batch(B, A, seed=7, h=side, w=side, stack=stack)
        # zero frames of an episode start in both halves of the table, and the last frame of the store
        ids[0, 0] = -1
        ids[0, stack + 1] = -1
        ids[-1, stack - 1] = len(frames) - 1
        ids[-1, 2 * stack - 1] = len(frames) - 1
        eng = QNetEngine((side, side, stack), A, 1 + K, (width, 8, 8, 16), "cnn", ln, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4,
                         precision=prec)
        eng.init_params(1)
        b = device_batch(eng, frames, ids, action, reward, terminal)
        for _ in range(3):
            eng.learn_on_batch(b)
        pre = eng.loss_on_batch(b).clone()
        fr = torch.from_numpy(frames).cuda()
        one = torch.from_numpy(ids[:1, :stack].copy()).cuda()
        q1 = eng.forward(frames=fr, frame_stride=frames.shape[1], frame_ids=one, n_rows=1)
        torch.cuda.synchronize()
        n = eng.n_param_floats
        print(f"{name}: params {h(eng.params[:n])} m {h(eng.adam_m[:n])} v {h(eng.adam_v[:n])} losses {h(eng.losses)} q {h(eng.q_values)} "
              f"t {h(eng.targets)} pri {h(eng.priorities)} loss_only {h(pre)} fwd1 {h(q1)}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
