"""ctypes binding of libisdqn_hip.so (C ABI: include/isdqn_hip.h).

The product path has no CPU fallback: if the library is missing this module raises at first
use.  Device memory and streams come from PyTorch-ROCm (plumbing only); every hot-path
computation goes through the entry points bound here.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char, c_char_p, c_double, c_float, c_int32, c_int64, c_uint8, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# ISDQN_HIP_LIB: development override (A/B timing of two builds inside one gpurun call); still a HIP build, never a fallback
LIB_PATH = os.environ.get("ISDQN_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libisdqn_hip.so")

OK = 0
ERR_CAPACITY, ERR_NEGATIVE, ERR_SHAPE, ERR_EMPTY, ERR_RANGE, ERR_UNSUPPORTED, ERR_HIP, ERR_ARG = range(-1, -9, -1)
STATUS_NEGATIVE_VALUE, STATUS_TARGET_RANGE, STATUS_EMPTY_TREE = 1, 2, 4
BATCH_MIRROR_CURRENT = 1  # include/isdqn_hip.h: ISDQN_BATCH_MIRROR_CURRENT
BATCH_DISCOUNT = 2  # include/isdqn_hip.h: ISDQN_BATCH_DISCOUNT
BATCH_WEIGHT_DECAY = 4  # include/isdqn_hip.h: ISDQN_BATCH_WEIGHT_DECAY
BATCH_CONSERVATIVE = 8  # include/isdqn_hip.h: ISDQN_BATCH_CONSERVATIVE
BATCH_MIXTURE = 16  # include/isdqn_hip.h: ISDQN_BATCH_MIXTURE
ACT_MEAN_HEADS = 32  # include/isdqn_hip.h: ISDQN_ACT_MEAN_HEADS (isdqn_net_best_actions' flags)
DECAY_KINDS_KERNELS, DECAY_KINDS_ALL = 0x03, 0x7F  # include/isdqn_hip.h: ISDQN_DECAY_KINDS_* (bit k: TensorInfo.kind k decays)
TREE_MAX_BATCH = 4096
ARCH_CNN, ARCH_FC, ARCH_IMPALA = 0, 1, 2
PRECISION_BF16X3, PRECISION_BF16 = 0, 1
MAX_FEATURES = 8


class NetConfig(ctypes.Structure):
    _fields_ = [
        ("arch", c_int32),
        ("obs_h", c_int32),
        ("obs_w", c_int32),
        ("obs_c", c_int32),
        ("n_features", c_int32),
        ("features", c_int32 * MAX_FEATURES),
        ("n_actions", c_int32),
        ("n_heads", c_int32),
        ("dueling", c_int32),  # 0: off; 1: dueling value / advantage heads, combined on the device (include/isdqn_hip.h)
        ("layer_norm", c_int32),
        ("batch_size", c_int32),
        ("precision", c_int32),
        ("gamma_n", c_float),
        ("learning_rate", c_float),
        ("adam_b1", c_float),
        ("adam_b2", c_float),
        ("adam_eps", c_float),
        ("max_grad_norm", c_float),  # 0: off; > 0 (inf allowed): clip the gradient by its global norm in front of Adam (include/isdqn_hip.h)
        ("huber_delta", c_float),
        ("munchausen_tau", c_float),  # 0: off; > 0: Munchausen targets at this temperature (include/isdqn_hip.h)
        ("munchausen_alpha", c_float),
        ("munchausen_clip", c_float),
        ("batch_norm", c_int32),
        ("categorical", c_int32),  # 0: off; 1: the C51 categorical projection loss on the histogram heads of n_bins (include/isdqn_hip.h)
        ("n_bins", c_int32),  # 0: scalar heads; > 0: HL-Gauss histogram loss over [hl_min, hl_max] (include/isdqn_hip.h)
        ("n_quantiles", c_int32),  # 0: off; 2..256: QR-DQN quantile-regression heads, kappa = huber_delta (include/isdqn_hip.h)
        ("hl_min", c_float),
        ("hl_max", c_float),
        ("hl_sigma", c_float),
        ("double_q", c_int32),  # 0: max_a' Q(s', a'); 1: Double Q-learning targets (include/isdqn_hip.h)
    ]


class TensorInfo(ctypes.Structure):
    _fields_ = [
        ("name", c_char * 48),
        ("offset", c_int64),
        ("size", c_int64),
        ("kind", c_int32),
        ("layer", c_int32),
        ("ndim", c_int32),
        ("flax_shape", c_int32 * 4),
        ("dims", c_int32 * 4),
    ]


class StagedUpdates(ctypes.Structure):  # isdqn_staged_updates
    _fields_ = [
        ("n_frames", c_int32), ("frame_bytes", c_int32), ("off_frame_slots", c_int64), ("off_frame_data", c_int64),
        ("n_rows", c_int32), ("stack2", c_int32), ("off_rows", c_int64), ("off_row_frames", c_int64), ("off_row_action", c_int64),
        ("off_row_reward", c_int64), ("off_row_terminal", c_int64),
        ("n_index", c_int32), ("reserved", c_int32), ("off_index_rows", c_int64), ("off_index_vals", c_int64),
    ]


class Batch(ctypes.Structure):
    _fields_ = [
        ("B", c_int32),
        ("frames", c_void_p),
        ("frame_stride", c_int64),
        ("frame_ids", c_void_p),
        ("state", c_void_p),
        ("next_state", c_void_p),
        ("action", c_void_p),
        ("reward", c_void_p),
        ("terminal", c_void_p),
        ("flags", c_int32),
        ("priorities_ready", c_void_p),
        ("loss_weights", c_void_p),  # float32 [B] importance-sampling weights or NULL (include/isdqn_hip.h)
    ]


class BatchDiscount(Batch):  # isdqn_batch_discount: the batch, then the discounts that flags & BATCH_DISCOUNT announces
    _fields_ = [("discount", c_void_p)]  # float32 [B] per-transition discounts in cfg.gamma_n's place (include/isdqn_hip.h)


class BatchDecay(BatchDiscount):  # isdqn_batch_decay: the batch (and its discount slot), then what flags & BATCH_WEIGHT_DECAY announces
    _fields_ = [("weight_decay", c_float), ("decay_kinds", c_int32)]  # AdamW's decay and the tensor kinds it acts on (include/isdqn_hip.h)


class BatchConservative(BatchDecay):  # isdqn_batch_conservative: the batch (its discount and decay slots), then what flags & BATCH_CONSERVATIVE announces
    _fields_ = [("cql_alpha", c_float), ("reserved", c_int32)]  # the weight of the conservative term (include/isdqn_hip.h)


class BatchMixture(BatchConservative):  # isdqn_batch_mixture: the batch (its discount, decay and cql slots), then what flags & BATCH_MIXTURE announces
    _fields_ = [("alpha", c_void_p), ("n_mix", c_int32), ("reserved2", c_int32)]  # float32 [n_mix] mixture weights (include/isdqn_hip.h)


_SIGNATURES = {
    "isdqn_version": (c_char_p, []),
    "isdqn_last_error": (c_char_p, []),
    "isdqn_tree_layout": (c_int32, [c_int64, POINTER(c_int32), POINTER(c_int64), POINTER(c_int64)]),
    "isdqn_tree_set": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "isdqn_tree_swap_remove": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "isdqn_tree_query": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "isdqn_tree_query_weighted": (
        c_int32,
        [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_replay_apply_staged": (
        c_int32,
        [c_void_p, POINTER(StagedUpdates), c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_replay_gather_rows": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_replay_materialize": (
        c_int32,
        [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_replay_deinterleave": (
        c_int32,
        [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p],
    ),
    # random-shift augmentation of a sampled batch's frames into a scratch pool (include/isdqn_hip.h, isdqn_replay_augment_shift)
    "isdqn_replay_augment_shift": (
        c_int32,
        [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    # horizon windows: the scatter of their staged rows, and the gather at a horizon / discount read from device memory
    "isdqn_replay_apply_staged_horizon": (
        c_int32,
        [c_void_p, c_int32, c_int64, c_int64, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_replay_gather_horizon": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_param_layout": (
        c_int32,
        [POINTER(NetConfig), POINTER(c_int64), POINTER(TensorInfo), c_int32, POINTER(c_int32)],
    ),
    "isdqn_net_workspace_bytes": (c_int32, [POINTER(NetConfig), POINTER(c_int64)]),
    "isdqn_net_workspace_region": (c_int32, [POINTER(NetConfig), c_char_p, POINTER(c_int64), POINTER(c_int64)]),
    "isdqn_net_forward": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_learn_on_batch": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, POINTER(Batch), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_learn_on_batch_debug": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, POINTER(Batch), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_loss_on_batch": (
        c_int32,
        [POINTER(NetConfig), c_void_p, POINTER(Batch), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_learn_on_batch_target": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(Batch), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_loss_on_batch_target": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, POINTER(Batch), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_grad_on_batch": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, POINTER(Batch), c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_refresh_mirror": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p, c_void_p]),
    "isdqn_net_bn_commit_running": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p, c_void_p]),
    "isdqn_net_shift_params": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p]),
    "isdqn_net_best_action": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_best_actions": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    ),
    "isdqn_net_analysis_layout": (c_int32, [POINTER(NetConfig), POINTER(c_int32), POINTER(c_int64), c_int32]),
    "isdqn_net_analysis": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "isdqn_net_redo_layout": (c_int32, [POINTER(NetConfig), POINTER(c_int32), POINTER(c_int32), c_int32]),
    "isdqn_net_redo": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_float,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    # noisy Dense layers (include/isdqn_hip.h, isdqn_noisy_layout): layout, sample, compose, learn
    "isdqn_noisy_layout": (
        c_int32,
        [POINTER(NetConfig), POINTER(c_int32), POINTER(c_int64), POINTER(c_int32), POINTER(c_int32), c_int32, POINTER(c_int64)],
    ),
    "isdqn_noisy_sample": (c_int32, [POINTER(NetConfig), c_uint64, c_int32, c_void_p, c_void_p, c_void_p]),
    "isdqn_noisy_compose": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "isdqn_noisy_learn_on_batch": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         POINTER(Batch), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    # periodic resets and EMA targets (include/isdqn_hip.h, isdqn_net_reset / isdqn_net_ema)
    "isdqn_net_reset_layout": (c_int32, [POINTER(NetConfig), POINTER(c_int32), POINTER(c_int32)]),
    "isdqn_net_reset": (
        c_int32,
        [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float, c_float, c_float, c_void_p, c_void_p],
    ),
    "isdqn_net_ema": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p, c_float, c_void_p]),
    # soft head shift (include/isdqn_hip.h, isdqn_net_soft_shift): cfg, params, tau, workspace or NULL, stream
    "isdqn_net_soft_shift": (c_int32, [POINTER(NetConfig), c_void_p, c_float, c_void_p, c_void_p]),
    # gradual magnitude pruning (include/isdqn_hip.h, isdqn_net_prune_*): layout: cfg, &n_tensors, infos [n][4] int64, max_infos,
    # &mask_words, &scratch_bytes; update: cfg, params, n_pruned, mask, scratch, workspace or NULL, stream; apply: cfg, params, mask,
    # workspace or NULL, stream
    "isdqn_net_prune_layout": (c_int32, [POINTER(NetConfig), POINTER(c_int32), c_void_p, c_int32, POINTER(c_int64), POINTER(c_int64)]),
    "isdqn_net_prune_update": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "isdqn_net_prune_apply": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p]),
    # Normalize-and-Project (include/isdqn_hip.h, isdqn_net_project_*): layout: cfg, &n_tensors, infos [n][4] int64, max_infos,
    # &scratch_bytes; norms: cfg, params, norms, scratch, stream; apply: cfg, params, target_norms, norms, scales, scratch, workspace or
    # NULL, stream
    "isdqn_net_project_layout": (c_int32, [POINTER(NetConfig), POINTER(c_int32), c_void_p, c_int32, POINTER(c_int64)]),
    "isdqn_net_project_norms": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p]),
    "isdqn_net_project_apply": (c_int32, [POINTER(NetConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # random ensemble mixture (include/isdqn_hip.h, isdqn_mixture_draw): n_heads, seed, draw count, alpha, stream
    "isdqn_mixture_draw": (c_int32, [c_int32, c_uint64, c_void_p, c_void_p, c_void_p]),
    "isdqn_selftest_gemm": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p],
    ),
}

# entry points declared by include/isdqn_hip.h (the debug hook is exported but not part of the header)
PUBLIC_SYMBOLS = [s for s in _SIGNATURES if s != "isdqn_net_learn_on_batch_debug"]

_lib = None


def lib() -> ctypes.CDLL:
    """The loaded C-ABI library; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm bundles its own libamdhip64; import it first so that this library binds to the SAME HIP
        # runtime (streams and device pointers are shared with torch) instead of loading a second one.
        import torch  # noqa: F401

        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first (python is-dqn_amd/build.py). "
                "There is no CPU fallback for the iS-DQN hot path."
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def last_error() -> str:
    return lib().isdqn_last_error().decode()


def check(rc: int, what: str = "") -> None:
    """Map C-ABI status codes onto the reference's exception types (error conventions)."""
    if rc == OK:
        return
    msg = f"{what}: {last_error()}" if what else last_error()
    if rc in (ERR_CAPACITY, ERR_NEGATIVE, ERR_SHAPE, ERR_EMPTY):
        raise AssertionError(msg)
    if rc == ERR_RANGE:
        raise ValueError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(f"isdqn_hip error {rc}: {msg}")


def ptr(t) -> int:
    """Device pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


def default_device():
    """The GPU this process drives.  One process per GPU: under torchrun / experiments/launch.py the rank's
    LOCAL_RANK selects it (a launcher that sets HIP_VISIBLE_DEVICES per child leaves exactly one visible device, cuda:0);
    a plain single-process run gets cuda:0."""
    import torch

    idx = int(os.environ.get("ISDQN_DEVICE_INDEX", os.environ.get("LOCAL_RANK", "0")))
    n = torch.cuda.device_count()
    if n and idx >= n:
        idx = 0  # the launcher narrowed HIP_VISIBLE_DEVICES to this rank's GPU
    return torch.device("cuda", idx)


def resolve_device(device):
    import torch

    dev = default_device() if device is None else torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    return dev


_CUDA_OK = None


def _cuda_ok() -> bool:
    """torch.cuda.is_available(), asked once: it is a driver call (~80 us), and the per-call device binding below sits on the
    acting / update path."""
    global _CUDA_OK
    if _CUDA_OK is None:
        import torch

        _CUDA_OK = bool(torch.cuda.is_available())
    return _CUDA_OK


def bind_device(device) -> None:
    """Make `device` the calling thread's current HIP device: the library launches on the current device (per-device
    side stream, function attributes), so an object on cuda:k must only ever be driven with cuda:k current."""
    import torch

    if device.type == "cuda" and _cuda_ok() and torch.cuda.current_device() != device.index:
        torch.cuda.set_device(device)


def stream_ptr(device=None) -> int:
    """HIP stream the C-ABI call is enqueued on: torch's current stream OF THE OBJECT'S DEVICE.  Fails loudly when the
    thread's current device is another one (kernels would be launched on device A against pointers of device B)."""
    import torch

    if device is not None and device.type == "cuda" and device.index is not None and device.index != torch.cuda.current_device():
        raise RuntimeError(
            f"isdqn_hip: object lives on {device} but the calling thread's current device is cuda:{torch.cuda.current_device()}; "
            f"one process drives one GPU -- call torch.cuda.set_device({device.index}) (experiments/launch.py does)")
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("the iS-DQN HIP path needs a ROCm GPU (torch.cuda.is_available() is False)")
    lib()
