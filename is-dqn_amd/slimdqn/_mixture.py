"""REM, the random ensemble mixture (Agarwal, Schuurmans, Norouzi 2020; include/isdqn_hip.h, isdqn_batch_mixture): the rules and their
messages.

Like the conservative term the mixture is an option of the learn CALL, not of the network configuration: the network is an ordinary
one with ``n_heads = H``, ``QNetEngine.set_mixture`` owns the step's weights and ``make_batch`` hands them to the library in every
batch.  The engine imports this module, never its names."""
from __future__ import annotations

MAX_HEADS = 1024  # isdqn_mixture_draw: one workgroup draws them all

REM_HEADS_REFUSED = "rem_heads must be an integer in [0, 1024] (0 = off: a plain DQN, the bits of a run without the option)"
REM_NOISY_REFUSED = "rem_heads > 0 with noisy layers is not built (isdqn_noisy_learn_on_batch refuses the mixture)"
REM_HISTOGRAM_REFUSED = "rem_heads > 0 with histogram heads (n_bins > 0) is not built: the mixture is defined on scalar heads"
REM_QUANTILE_REFUSED = "rem_heads > 0 with quantile heads (n_quantiles > 0) is not built: the mixture is defined on scalar heads"
REM_MUNCHAUSEN_REFUSED = "rem_heads > 0 with Munchausen targets is not built"
REM_CQL_REFUSED = "rem_heads > 0 with cql_alpha > 0 is not built: a conservative term on the mixture is a follow-up"
REM_AGENT_REFUSED = "-rem / rem_heads is an option of DQN (dqn.py): the other agents have no mixture"


def check_rem_heads(rem_heads, *, noisy=False, n_bins=0, n_quantiles=0, munchausen_tau=0.0, cql_alpha=0.0) -> int:
    """The number of mixture heads of an agent or a command line: an int in [0, 1024]; above 0 the options the library refuses with
    the mixture are refused here, before anything is built, in this order."""
    if isinstance(rem_heads, bool) or not isinstance(rem_heads, int) and not (isinstance(rem_heads, float) and rem_heads == int(rem_heads)):
        raise ValueError(REM_HEADS_REFUSED)
    H = int(rem_heads)
    if not 0 <= H <= MAX_HEADS:
        raise ValueError(REM_HEADS_REFUSED)
    if H == 0:
        return 0
    if noisy:
        raise ValueError(REM_NOISY_REFUSED)
    if int(n_bins) > 0:
        raise ValueError(REM_HISTOGRAM_REFUSED)
    if int(n_quantiles) > 0:
        raise ValueError(REM_QUANTILE_REFUSED)
    if float(munchausen_tau) > 0.0:
        raise ValueError(REM_MUNCHAUSEN_REFUSED)
    if float(cql_alpha) > 0.0:
        raise ValueError(REM_CQL_REFUSED)
    return H


def mixture_seed(seed: int) -> int:
    """The Philox key of an agent's draws from its seed (the draws have a counter domain of their own: the key may be the seed itself)."""
    return int(seed) & (2**64 - 1)
