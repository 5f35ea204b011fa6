"""Normalize-and-Project (include/isdqn_hip.h, isdqn_net_project_*): the rules and their messages.

Lyle, Zheng, Khetarpal, Martens, van Hasselt, Pascanu & Dabney, "Normalization and effective learning rates in reinforcement learning",
NeurIPS 2024.  The norms, the scales and the projection live on the device; what is decided on the host is decided here: which networks
can be projected at all.  The engine and the command line import this module, never its names."""
from __future__ import annotations

NAP_LAYER_NORM_REFUSED = ("-nap / weight_projection needs -ln / layer_norm: without a normalisation behind every projected kernel the "
                          "projection changes the function at every step")
NAP_NOISY_REFUSED = "weight projection with noisy layers is a follow-up: the norm would have to cover the mu and sigma buffers (ISDQN_ERR_UNSUPPORTED)"
NAP_BATCH_NORM_REFUSED = "weight projection is not built for batch_norm (ISDQN_ERR_UNSUPPORTED)"
NAP_IMPALA_REFUSED = "weight projection is not built for architecture_type 'impala' (ISDQN_ERR_UNSUPPORTED)"
NAP_NOT_SET_REFUSED = "project_weights / project_norms need set_weight_projection() first: the engine has no target norms"
NAP_TARGETS_REFUSED = "set_weight_projection takes one target norm per projected tensor"


def check_engine(*, noisy: bool = False, batch_norm: bool = False, architecture_type: str = "cnn") -> None:
    """What no engine's projection entry points run on (the library's own refusals, and noisy layers), in the order of the messages."""
    if noisy:
        raise ValueError(NAP_NOISY_REFUSED)
    if batch_norm:
        raise ValueError(NAP_BATCH_NORM_REFUSED)
    if architecture_type == "impala":
        raise ValueError(NAP_IMPALA_REFUSED)


def check_network(*, layer_norm: bool, noisy: bool = False, batch_norm: bool = False, architecture_type: str = "cnn") -> None:
    """What no projected agent can be: ``check_engine`` first, then the rule of the option itself -- LayerNorm behind every projected
    kernel, or the projection is no reparametrisation."""
    check_engine(noisy=noisy, batch_norm=batch_norm, architecture_type=architecture_type)
    if not layer_norm:
        raise ValueError(NAP_LAYER_NORM_REFUSED)


def check_targets(target_norms, n_tensors: int) -> list:
    """One float per projected tensor (a value that is not finite or <= 0 is allowed: the device leaves such a tensor alone)."""
    t = [float(x) for x in target_norms]
    if len(t) != int(n_tensors):
        raise ValueError(NAP_TARGETS_REFUSED)
    return t


def scale_logs(scales) -> dict:
    """The logs of a target update from the scales of the last step: at 1 the run is not growing its norms; at 0.99 it would lose 2 % of
    its effective learning rate per step without the option."""
    s = [float(x) for x in scales]
    return {"weight_scale_min": min(s), "weight_scale_max": max(s)} if s else {}
