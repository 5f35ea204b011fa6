"""Optimizer options that travel behind the batch (include/isdqn_hip.h, isdqn_batch_decay): the rules and their messages.

AdamW's decoupled weight decay is an option of the learn CALL, not of the network configuration: ``QNetEngine.set_weight_decay`` checks it
here and ``make_batch`` hands it to the library in every batch.  The engine imports this module, never its names."""
from __future__ import annotations

import math

from slimdqn import _hip

WEIGHT_DECAY_REFUSED = "weight_decay must be finite and >= 0 (0 = off: plain Adam, the bits of a run without the option)"
WEIGHT_DECAY_NOISY_REFUSED = (
    "weight_decay > 0 with noisy layers is a follow-up: the noisy optimizer kernel walks the flat parameter buffer and does not know "
    "which tensors are kernels (ISDQN_ERR_UNSUPPORTED)")


def check_weight_decay(weight_decay, noisy: bool = False) -> float:
    """The weight decay of an engine, an agent or a command line: a finite float >= 0 (NaN and inf refused), and 0 under noisy layers."""
    wd = float(weight_decay)
    if not (math.isfinite(wd) and wd >= 0.0):
        raise ValueError(WEIGHT_DECAY_REFUSED)
    if wd > 0.0 and noisy:
        raise ValueError(WEIGHT_DECAY_NOISY_REFUSED)
    return wd


def decay_kinds(all_kinds: bool = False) -> int:
    """Bit mask over ``TensorInfo.kind`` of the tensors that decay: the conv and dense kernels (the mask of the optax and torch recipes),
    or with ``all_kinds`` everything Adam updates -- biases and the LayerNorm / BatchNorm scales and biases too; never the running statistics."""
    return _hip.DECAY_KINDS_ALL if all_kinds else _hip.DECAY_KINDS_KERNELS
