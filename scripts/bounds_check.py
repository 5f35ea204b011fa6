"""Run the learn / loss / forward / acting / gradient-only entry points of a bounds-checked build (-DISDQN_BOUNDS: every operand load
of the tile engine, the image kernels, the frame-id table and the head chain is checked on the device against the byte extents
registered here -- the EXACT extents of every tensor handed to the library) over the shapes the GPU suite uses, and print one JSON
line per case: {"case", "bad", "site", "addr"}.  Started by tests/test_gpu_bounds.py with ISDQN_HIP_LIB pointing at that build."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "is-dqn_amd"))
import numpy as np
import torch

from slimdqn import _hip
from slimdqn._engine import QNetEngine

lib = _hip.lib()
lib.isdqn_debug_bounds_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
lib.isdqn_debug_bounds_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


_first = [None]  # first violation of the running case (a re-registration clears the device record)


def register(tensors, fresh=True):
    if fresh:
        _first[0] = None
    else:
        r = result()
        if r[0] and _first[0] is None:
            _first[0] = r
    ts = [t for t in tensors if t is not None]
    lo = (ctypes.c_uint64 * len(ts))(*[t.data_ptr() for t in ts])
    hi = (ctypes.c_uint64 * len(ts))(*[t.data_ptr() + t.numel() * t.element_size() for t in ts])
    _hip.check(lib.isdqn_debug_bounds_set(lo, hi, len(ts)))


def result():
    bad, site, addr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    _hip.check(lib.isdqn_debug_bounds_get(ctypes.byref(bad), ctypes.byref(site), ctypes.byref(addr)))
    return int(bad.value), int(site.value), int(addr.value)


def engine_tensors(eng):
    return [eng.params, eng.adam_m, eng.adam_v, eng.workspace, eng.losses, eng.losses_accum, eng.q_values, eng.targets, eng.priorities,
            eng.adam_count, eng.action_out]


def report(case, omit=None):
    bad, site, addr = _first[0] if _first[0] is not None else result()
    print(json.dumps({"case": case, "bad": bad, "site": site, "addr": hex(addr), "omitted": omit}), flush=True)


def run_case(name, arch, obs, feats, K, A, B, ln=True, bn=False, target=False, grad=True, omit=None, double_q=False, n_bins=0, munchausen=False, n_quantiles=0, categorical=False, dueling=False, max_grad_norm=0.0, cql=False):
    n_heads = 1 + K if K > 0 else 1
    eng = QNetEngine(obs, A, n_heads, feats, arch, ln, B, batch_norm=bn, double_q=double_q, n_bins=n_bins, min_value=-10.0, max_value=10.0, sigma=0.3,
                     munchausen_tau=0.03 if munchausen else 0.0, n_quantiles=n_quantiles, huber_delta=1.0 if n_quantiles else 0.0, categorical=categorical, dueling=dueling,
                     max_grad_norm=max_grad_norm)
    eng.init_params(0)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    action = dev(rng.integers(0, A, B).astype(np.int32))
    reward = dev(rng.normal(size=B).astype(np.float32))
    terminal = dev((rng.random(B) < 0.3).astype(np.uint8))
    extra = []
    if arch == "fc":
        d = int(np.prod(obs))
        st, nx = dev(rng.normal(size=(B, d)).astype(np.float32)), dev(rng.normal(size=(B, d)).astype(np.float32))
        inputs = dict(state=st, next_state=nx)
        batch = eng.make_batch(**inputs, action=action, reward=reward, terminal=terminal)
        fwd = dict(obs=torch.cat((st, nx)).contiguous(), n_rows=2 * B)
        one = dict(obs=st[:1].contiguous())
        extra += [st, nx, fwd["obs"], one["obs"]]
    else:
        h, w, stack = obs
        n_frames = 3 * B + 8
        frames = dev(rng.integers(0, 256, (n_frames, h * w), dtype=np.uint8))
        ids_np = rng.integers(0, n_frames, (B, 2 * stack)).astype(np.int32)
        ids_np[rng.random(ids_np.shape) < 0.1] = -1
        ids = dev(ids_np)
        flat = dev(np.concatenate([ids_np[:, :stack], ids_np[:, stack:]], 0))
        inputs = dict(frames=frames, frame_stride=h * w, frame_ids=ids)
        batch = eng.make_batch(**inputs, action=action, reward=reward, terminal=terminal)
        fwd = dict(frames=frames, frame_stride=h * w, frame_ids=flat, n_rows=2 * B)
        one = dict(frames=frames, frame_stride=h * w, frame_ids=flat[:1].contiguous())
        extra += [frames, ids, flat, one["frame_ids"]]
    heads = torch.arange(min(5, 2 * B), dtype=torch.int32, device="cuda") % max(K, 1)
    grad_out = torch.zeros_like(eng.params)
    tparams = eng.params.clone()
    small = [action, reward, terminal]
    tensors = engine_tensors(eng) + extra + [heads, grad_out, tparams] + [t for t in small if omit is None or t is not {"action": action, "reward": reward, "terminal": terminal}[omit]]
    torch.cuda.synchronize()
    register(tensors)
    q = eng.forward(**fwd)
    eng.loss_on_batch(batch)
    eng.learn_on_batch(batch)
    eng.learn_on_batch(batch, grad_out=grad_out)
    register(tensors + [q], fresh=False)  # (outputs allocated meanwhile are written, not read; the table is re-read by every kernel)
    eng.best_action(idx_network=0, **one)
    nrow = int(heads.numel())
    if arch == "fc":
        eng.best_actions(obs=fwd["obs"][:nrow].contiguous() if False else fwd["obs"], idx_networks=heads)
    else:
        eng.best_actions(frames=fwd["frames"], frame_stride=fwd["frame_stride"], frame_ids=fwd["frame_ids"], idx_networks=heads)
    if grad:  # (BatchNorm networks too: the analysis agents' gradient-only passes, with and without separate target parameters)
        eng.grad_on_batch(batch, grad_out)
        if K >= 1 and n_heads >= 2 and not (bn and (double_q or munchausen)):  # (BatchNorm + either option + target parameters: refused)
            eng.grad_on_batch(batch, grad_out, target_params=tparams, online_head=1, target_head=1, n_pairs=1)
    if target and not bn:
        eng.learn_on_batch_target(batch, tparams)
        eng.loss_on_batch_target(batch, tparams)
    # importance-sampling weights (isdqn_batch.loss_weights: site 29 in the head chain), last so that a case's first violation stays
    # what it was: the same batch with a registered weights tensor through learn / loss / gradient-only
    weights = dev(np.random.default_rng(1).uniform(0.1, 1.0, B).astype(np.float32))
    wbatch = eng.make_batch(**inputs, action=action, reward=reward, terminal=terminal, loss_weights=weights)
    register(tensors + [q, weights], fresh=False)
    eng.learn_on_batch(wbatch)
    eng.loss_on_batch(wbatch)
    if grad:
        eng.grad_on_batch(wbatch, grad_out)
    if cql:  # the conservative term on the loss kernel's row partition (conservative_kernels.hip), after everything else, as the weights are
        eng.set_conservative(0.7)
        cbatch = eng.make_batch(**inputs, action=action, reward=reward, terminal=terminal, loss_weights=weights)
        eng.learn_on_batch(cbatch)
        eng.loss_on_batch(cbatch)
        if grad:
            eng.grad_on_batch(cbatch, grad_out)
    report(name, omit)
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    HL = (32, 64, 64, 512)
    cases = [
        dict(name="cnn-headline-B8", arch="cnn", obs=(84, 84, 4), feats=HL, K=9, A=9, B=8),
        dict(name="cnn-headline-B7-ragged", arch="cnn", obs=(84, 84, 4), feats=HL, K=9, A=9, B=7),
        dict(name="cnn-tiny-noln-B5", arch="cnn", obs=(84, 84, 4), feats=(16, 20, 5, 24), K=2, A=3, B=5, ln=False),
        dict(name="cnn-a18-B33", arch="cnn", obs=(84, 84, 4), feats=HL, K=4, A=18, B=33),
        dict(name="cnn-44x44x6-generic-first-layer", arch="cnn", obs=(44, 44, 6), feats=(7, 9, 11, 13), K=2, A=3, B=5),
        dict(name="cnn-52x60x2", arch="cnn", obs=(52, 60, 2), feats=(16, 20, 12, 24), K=3, A=4, B=6),
        dict(name="cnn-one-head-dqn-B8", arch="cnn", obs=(84, 84, 4), feats=HL, K=0, A=6, B=8, target=True),
        dict(name="cnn-tiny-B515-ragged", arch="cnn", obs=(84, 84, 4), feats=(8, 8, 8, 16), K=9, A=9, B=515, grad=False),
        dict(name="cnn-c2-full-B256", arch="cnn", obs=(84, 84, 4), feats=HL, K=9, A=9, B=256, grad=False),
        dict(name="cnn-c5-full-B1024", arch="cnn", obs=(84, 84, 4), feats=HL, K=32, A=4, B=1024, grad=False),
        dict(name="fc-lunar-lander-100x100-B32", arch="fc", obs=(8,), feats=(100, 100), K=1, A=4, B=32, target=False),
        dict(name="fc-three-hidden-B10", arch="fc", obs=(6,), feats=(24, 40, 16), K=3, A=3, B=10, ln=False),
        dict(name="fc-one-head-dqn-B32", arch="fc", obs=(8,), feats=(100, 100), K=0, A=4, B=32, target=True),
        dict(name="impala-tiny-B3", arch="impala", obs=(84, 84, 4), feats=(8, 16, 16, 24), K=2, A=5, B=3),
        dict(name="impala-44x44x3-B2", arch="impala", obs=(44, 44, 3), feats=(12, 20, 9, 16), K=3, A=4, B=2),
        dict(name="bn-cnn-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, bn=True),
        dict(name="bn-cnn-headline-B8", arch="cnn", obs=(84, 84, 4), feats=HL, K=9, A=9, B=8, bn=True),
        dict(name="bn-fc-B10", arch="fc", obs=(6,), feats=(24, 40, 16), K=3, A=3, B=10, ln=False, bn=True),
        dict(name="bn-impala-B4", arch="impala", obs=(36, 36, 2), feats=(16, 8, 16, 24), K=3, A=4, B=4, bn=True),
        # Double Q-learning targets (site 30: the selector / value rows of td_kernel; the DQN form reads them from region "q_target")
        dict(name="dq-cnn-tiny-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, double_q=True),
        dict(name="dq-cnn-one-head-dqn-B8", arch="cnn", obs=(84, 84, 4), feats=HL, K=0, A=6, B=8, target=True, double_q=True),
        dict(name="dq-fc-one-head-dqn-B32", arch="fc", obs=(8,), feats=(100, 100), K=0, A=4, B=32, target=True, double_q=True),
        # histogram heads: the selector / value logit rows of hl_loss_kernel (site 30), the DQN form's from region "logits_target"
        dict(name="dq-hist-cnn-tiny-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, double_q=True, n_bins=51),
        dict(name="dq-hist-cnn-one-head-dqn-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=0, A=5, B=6, target=True, double_q=True, n_bins=51),
        dict(name="dq-bn-cnn-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, bn=True, double_q=True),
        # Munchausen targets (site 31: the value head's state / next-state rows of td_kernel; the DQN form reads both halves from the
        # [2B] region "q_target"); the head chain reads them from LDS
        dict(name="mq-cnn-tiny-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, munchausen=True),
        dict(name="mq-cnn-headline-B7-ragged", arch="cnn", obs=(84, 84, 4), feats=HL, K=9, A=9, B=7, munchausen=True),
        dict(name="mq-cnn-one-head-dqn-B8", arch="cnn", obs=(84, 84, 4), feats=HL, K=0, A=6, B=8, target=True, munchausen=True),
        dict(name="mq-fc-one-head-dqn-B32", arch="fc", obs=(8,), feats=(100, 100), K=0, A=4, B=32, target=True, munchausen=True),
        # histogram heads: the value head's logit rows of hl_loss_kernel (site 31), the DQN form's from the [2B] region "logits_target"
        dict(name="mq-hist-cnn-tiny-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, munchausen=True, n_bins=51),
        dict(name="mq-hist-cnn-one-head-dqn-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=0, A=5, B=6, target=True, munchausen=True, n_bins=51),
        dict(name="mq-bn-cnn-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, bn=True, munchausen=True),
        # quantile heads (sites 32 / 33: the selector / value quantile rows of qr_loss_kernel; N = 65: two values per lane, a ragged last
        # group), the DQN form's value rows from region "logits_target"
        dict(name="qr-cnn-tiny-N65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, n_quantiles=65),
        dict(name="qr-dq-cnn-tiny-N65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, double_q=True, n_quantiles=65),
        dict(name="qr-dq-cnn-one-head-dqn-N65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=0, A=5, B=6, target=True, double_q=True, n_quantiles=65),
        # categorical loss on the histogram heads (sites 34 / 35: the selector / value logit rows of c51_loss_kernel; nb = 65: two atoms per
        # lane, a ragged last group), the DQN form's value rows from region "logits_target"
        dict(name="c51-cnn-tiny-nb65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, n_bins=65, categorical=True),
        dict(name="c51-dq-cnn-tiny-nb65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, double_q=True, n_bins=65, categorical=True),
        dict(name="c51-dq-cnn-one-head-dqn-nb65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=0, A=5, B=6, target=True, double_q=True, n_bins=65,
             categorical=True),
        # dueling heads (sites 36 / 37: the raw rows duel_combine_kernel reads and the dout / dbh rows duel_backward_kernel reads; F = 14:
        # a group of 8 hidden units straddles the two streams), one case per head kind, the DQN forms' rows from region "head_raw_target"
        dict(name="duel-scalar-cnn-tiny-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 14), K=3, A=5, B=6, dueling=True),
        dict(name="duel-scalar-fc-one-head-dqn-B5", arch="fc", obs=(8,), feats=(20, 14), K=0, A=3, B=5, target=True, double_q=True, dueling=True),
        dict(name="duel-hist-cnn-tiny-nb65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 14), K=3, A=5, B=6, n_bins=65, munchausen=True, dueling=True),
        dict(name="duel-cat-cnn-one-head-dqn-nb65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 14), K=0, A=5, B=6, target=True, double_q=True, n_bins=65,
             categorical=True, dueling=True),
        dict(name="duel-quant-cnn-tiny-N65-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 14), K=3, A=5, B=6, n_quantiles=65, dueling=True),
        # gradient clipping (sites 38 / 39: the slab loads of grad_reduce_sq_kernel / grad_flat_sq_kernel -- first and last slab of every position -- and the
        # partial sums grad_clip_finalize_kernel reads; the regions "grad_clip_partials" and "grad_clip" lie inside the registered
        # workspace): the headline plan (Dense_0 through its one slab, per-image conv slabs) and dueling heads (the live mask)
        dict(name="gc-cnn-headline-B8", arch="cnn", obs=(84, 84, 4), feats=HL, K=9, A=9, B=8, max_grad_norm=10.0),
        dict(name="gc-dueling-cnn-tiny-B6", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 14), K=3, A=5, B=6, dueling=True, max_grad_norm=1e-3),
        # the distributional loss kernels off R = 4 transitions per workgroup (head_loss.h, rows_per_wg; tests/helpers/head_geometry.py's
        # table): 3 + 2 rows with the conservative term on the same partition, 2 + 2 + 1 rows and one row per workgroup at A = 1, and the
        # widest head row the plan takes (11 * 2 * 248 = 5456 outputs: dense_post_kernel's three staged rows fill its 64 KB of LDS)
        dict(name="geo-hl-r3-ragged", arch="fc", obs=(8,), feats=(16, 16), K=9, A=2, B=5, n_bins=256, cql=True),
        dict(name="geo-c51-r2", arch="fc", obs=(8,), feats=(16, 16), K=12, A=1, B=5, n_bins=256, categorical=True),
        dict(name="geo-qr-r1", arch="fc", obs=(8,), feats=(16, 16), K=20, A=1, B=3, n_quantiles=256),
        dict(name="geo-hl-widest", arch="fc", obs=(8,), feats=(16, 16), K=10, A=2, B=4, n_bins=248),
        # the geometries of tests/helpers/conv_routes.py: several 128-pixel tiles per image and per stride class (a ragged last one), the
        # u8 pair kernel's loop over halves, the one-tile u8 kernel at 64 channels and at three stacked frames, the generic forward at 64
        # input channels and the generic weight gradients behind the image kernels' LDS checks, the smallest observation
        dict(name="routes-100x100", arch="cnn", obs=(100, 100, 4), feats=(32, 64, 64, 32), K=3, A=5, B=6),
        dict(name="routes-160x120", arch="cnn", obs=(160, 120, 4), feats=(32, 64, 64, 32), K=2, A=3, B=3),
        dict(name="routes-128x128-w64", arch="cnn", obs=(128, 128, 4), feats=(64, 64, 64, 32), K=2, A=3, B=4),
        dict(name="routes-64x64x3", arch="cnn", obs=(64, 64, 3), feats=(32, 64, 64, 32), K=3, A=4, B=6),
        dict(name="routes-84-w64-48-24", arch="cnn", obs=(84, 84, 4), feats=(64, 48, 24, 32), K=2, A=5, B=5),
        dict(name="routes-40x40x2", arch="cnn", obs=(40, 40, 2), feats=(16, 32, 64, 32), K=3, A=3, B=7),
        dict(name="routes-8x8x1", arch="cnn", obs=(8, 8, 1), feats=(8, 8, 8, 32), K=2, A=3, B=3),
        # negative control: the checker must notice a tensor that was not registered
        dict(name="control-action-not-registered", arch="cnn", obs=(84, 84, 4), feats=(7, 9, 11, 13), K=3, A=5, B=6, omit="action"),
    ]
    for c in cases:
        if which != "all" and not c["name"].startswith(which):  # (a prefix: "qr-" must not take "geo-qr-r1" along)
            continue
        run_case(**c)
