"""Gradual magnitude pruning (include/isdqn_hip.h, isdqn_net_prune_*): the rules, their messages and the schedule.

Zhu & Gupta 2017; Graesser et al. 2022; Obando-Ceron, Courville & Castro 2024; the behaviour of JaxPruner's GMP.  The mask and its
selection live on the device; what is decided on the host is decided here, in float64 and integers: the sparsity of a gradient step and
the pruned count of every tensor.  The engine and the command line import this module, never its names."""
from __future__ import annotations

import math

PRUNE_SPARSITY_REFUSED = "-prune / final sparsity must be in [0, 1) (0 = off: the calls and the bits of a run without the option)"
PRUNE_SCHEDULE_REFUSED = "-prunes / -prunee: the schedule needs integers 0 <= start < end (gradient steps)"
PRUNE_PERIOD_REFUSED = "-prunef must be a positive multiple of -tuf: the mask is updated at target updates, as -redo and -reset run"
PRUNE_NOISY_REFUSED = "pruning with noisy layers is a follow-up: the mask would have to cover the mu and sigma buffers (ISDQN_ERR_UNSUPPORTED)"
PRUNE_BATCH_NORM_REFUSED = "pruning is not built for batch_norm (ISDQN_ERR_UNSUPPORTED)"
PRUNE_IMPALA_REFUSED = "pruning is not built for architecture_type 'impala' (ISDQN_ERR_UNSUPPORTED)"
PRUNE_NOT_SET_REFUSED = "prune_update / prune_apply need set_pruning() first: the engine has no mask"
PRUNE_COUNTS_REFUSED = "prune_update takes one integer count per prunable tensor, each in [0, the tensor's real element count]"


def check_network(*, noisy: bool = False, batch_norm: bool = False, architecture_type: str = "cnn") -> None:
    """What no pruned network can be, in the order of the messages above."""
    if noisy:
        raise ValueError(PRUNE_NOISY_REFUSED)
    if batch_norm:
        raise ValueError(PRUNE_BATCH_NORM_REFUSED)
    if architecture_type == "impala":
        raise ValueError(PRUNE_IMPALA_REFUSED)


def check_sparsity(sparsity) -> float:
    s = float(sparsity)
    if not (0.0 <= s < 1.0):  # (NaN fails both comparisons)
        raise ValueError(PRUNE_SPARSITY_REFUSED)
    return s


def check_schedule(start, end) -> tuple:
    if int(start) != start or int(end) != end or not 0 <= int(start) < int(end):
        raise ValueError(PRUNE_SCHEDULE_REFUSED)
    return int(start), int(end)


def check_period(period, target_update_frequency) -> int:
    if int(period) != period or int(period) <= 0 or int(period) % int(target_update_frequency) != 0:
        raise ValueError(PRUNE_PERIOD_REFUSED)
    return int(period)


def sparsity_at(step: int, final: float, start: int, end: int) -> float:
    """The cubic schedule of Zhu & Gupta in float64: 0 before ``start``, ``final`` from ``end`` on, and in between
    ``final * (1 - (1 - (step - start) / (end - start)) ** 3)``."""
    if step < start:
        return 0.0
    if step >= end:
        return float(final)
    return float(final) * (1.0 - (1.0 - (step - start) / (end - start)) ** 3)


def pruned_counts(sparsity: float, n_real, previous=None) -> list:
    """Uniform distribution over the tensors: ``floor(sparsity * n_i)`` of each, never below what ``previous`` already pruned (the masks
    stay nested) and never above ``n_i``."""
    counts = [min(int(n), int(math.floor(float(sparsity) * int(n)))) for n in n_real]
    if previous is not None:
        counts = [max(k, int(p)) for k, p in zip(counts, previous)]
    return counts


def pruned_share(counts, n_real) -> float:
    """The logged ``sparsity``: the pruned share of all real prunable elements, from the host's own counts."""
    total = sum(int(n) for n in n_real)
    return sum(int(k) for k in counts) / total if total else 0.0


class Schedule:
    """The state of one run: final sparsity, start, end, and the counts handed to the last mask update."""

    def __init__(self, final: float, start: int, end: int, n_real):
        self.final = check_sparsity(final)
        self.start, self.end = check_schedule(start, end)
        self.n_real = [int(n) for n in n_real]
        self.counts = [0] * len(self.n_real)

    def step(self, t: int) -> list:
        """The counts of a mask update at gradient step ``t`` (remembered: the next ones are no smaller)."""
        self.counts = pruned_counts(sparsity_at(int(t), self.final, self.start, self.end), self.n_real, self.counts)
        return list(self.counts)

    @property
    def active(self) -> bool:
        return any(k > 0 for k in self.counts)

    @property
    def sparsity(self) -> float:
        return pruned_share(self.counts, self.n_real)
