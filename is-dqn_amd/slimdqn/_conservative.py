"""The conservative (CQL) term, an option that travels behind the batch (include/isdqn_hip.h, isdqn_batch_conservative): the rule and
its message.

Like AdamW's decay it is an option of the learn CALL, not of the network configuration: ``QNetEngine.set_conservative`` checks it here
and ``make_batch`` hands it to the library in every batch.  The engine imports this module, never its names."""
from __future__ import annotations

import math

CQL_ALPHA_REFUSED = "cql_alpha must be finite and >= 0 (0 = off: no conservative term, the bits of a run without the option)"


def check_cql_alpha(cql_alpha) -> float:
    """The weight of the conservative term of an engine, an agent or a command line: a finite float >= 0 (NaN and inf refused)."""
    alpha = float(cql_alpha)
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError(CQL_ALPHA_REFUSED)
    return alpha
