"""The geometry of the three distributional loss kernels (csrc/head_loss.h), restated, and THE table of cases the GPU tests of
tests/test_gpu_head_geometry.py parametrize over.  No GPU, no torch.

A workgroup of hl_loss_kernel / c51_loss_kernel / qr_loss_kernel takes R = clamp(8192 / (K * nb), 1, 4) transitions (rows_per_wg) and
leaves dL/d(output) of its R * K (transition, pair)s in dynamic LDS, s_dl [R][K][nb]; a lane owns the outputs lane + 64 t of a (head,
action), t < ceil(nb / 64).  tests/test_head_geometry_host.py holds this restatement to the header's text and the table to its coverage."""
import collections
import math

MAX_ROWS = 4        # head_loss.h: MAX_ROWS
LDS_FLOATS = 8192   # head_loss.h: rows_per_wg keeps s_dl within 32 KB
MAX_K = 64          # net_plan.h: at most 64 regressed heads (LossStage's arrays are [MAX_ROWS * 64])
MAX_ROW = 5456      # net_plan.h: n_heads * n_actions * width at most (dense_post_kernel: three rows in 64 KB of LDS)
MAX_WIDTH = 256     # net_plan.h: n_bins / n_quantiles in [2, 256]

LOSSES = ("hl", "c51", "qr")


def rows_per_wg(K, nb):
    """Transitions per workgroup (head_loss.h, rows_per_wg)."""
    return min(max(LDS_FLOATS // (K * nb), 1), MAX_ROWS)


def groups_per_lane(nb):
    """64-value groups of a (head, action) a lane owns."""
    return -(-nb // 64)


def workgroups(B, R):
    return -(-B // R)


def dyadic_support(nb):
    """(1, 1 + nb eta) with eta the power of two nearest 20 / nb: every edge and every centre is exact in float32 (nb <= 256), so the
    support itself puts no rounding between a float32 kernel and its float64 restatement; and it does not straddle zero -- an
    expectation is a float32 sum of nb terms softmax_j c_j, which over a symmetric support cancel to a Q near zero that no relative
    bound covers (tests/test_gpu_double_q.py, HIST_POS: the same choice, for the same reason)."""
    eta = 2.0 ** round(math.log2(20.0 / nb))
    return 1.0, 1.0 + nb * eta


class Case(collections.namedtuple("Case", "id K A nb B note")):
    """n_heads = K + 1; for the quantile loss nb is n_quantiles."""

    @property
    def n_heads(self):
        return self.K + 1

    @property
    def R(self):
        return rows_per_wg(self.K, self.nb)

    @property
    def n_wg(self):
        return workgroups(self.B, self.R)

    @property
    def row(self):
        return self.n_heads * self.A * self.nb


CASES = [
    Case("r3-ragged", 9, 2, 256, 5, "workgroups of 3 + 2 rows"),
    Case("r3-short", 9, 2, 256, 2, "B < R"),
    Case("r3-c5-heads", 32, 2, 65, 7, "3 + 3 + 1, two groups per lane, one live lane in the second"),
    Case("r3-widest", 10, 2, 248, 4, "11 * 2 * 248 = 5456"),
    Case("r3-k64", 64, 2, 40, 4, "K at its limit"),
    Case("r4-k64", 64, 2, 2, 5, "64 pairs per wave, nb at its minimum"),
    Case("r2", 12, 1, 256, 5, "2 + 2 + 1, A = 1"),
    Case("r1", 20, 1, 256, 3, "one row per workgroup"),
]
BY_ID = {c.id: c for c in CASES}
VARIANT_IDS = ("r3-ragged", "r2", "r1")  # the cases every variant (discount, double_q, CQL, loss-only, gradient-only) runs on

# HL-Gauss over bin counts, sigma and support edges: K = 2, A = 3, B = 7 (R = 4: the subject is the per-lane arithmetic).
# Grid A: edges exact in float32; grid B: edges that are not.  (support, bin counts, sigma / eta)
GRID_K, GRID_A, GRID_B = 2, 3, 7
GRID_EXACT = ((-8.0, 8.0), (2, 64, 128, 256), (0.02, 0.75, 20.0, 200.0))
GRID_INEXACT = ((-10.0, 10.0), (51, 65, 130, 200), (0.75, 3.0))


def grid_cases():
    """[(id, vmin, vmax, nb, sigma / eta)] of both grids."""
    out = []
    for tag, ((vmin, vmax), nbs, ratios) in (("A", GRID_EXACT), ("B", GRID_INEXACT)):
        for nb in nbs:
            for ratio in ratios:
                out.append((f"{tag}-nb{nb}-s{ratio:g}", vmin, vmax, nb, ratio))
    return out


def grid_bin_counts():
    return sorted(set(GRID_EXACT[1]) | set(GRID_INEXACT[1]))


def within_plan_limits(K, A, nb, B):
    return 1 <= K <= MAX_K and A >= 1 and B >= 1 and 2 <= nb <= MAX_WIDTH and (K + 1) * A * nb <= MAX_ROW


def coverage_gaps(cases=None, grid=None):
    """What the table no longer covers, as a list of sentences (empty: nothing)."""
    cases = CASES if cases is None else cases
    grid = grid_cases() if grid is None else grid
    gaps = []
    for R in (1, 2, 3, 4):
        mine = [c for c in cases if c.R == R]
        if not mine:
            gaps.append(f"no case with R = {R}")
        if R in (2, 3) and not any(c.B % R != 0 for c in mine):
            gaps.append(f"no case with R = {R} and B mod R != 0")
        if R == 1 and not any(c.n_wg >= 2 for c in mine):  # (B mod 1 is 0 for every B: at R = 1 the ragged edge does not exist)
            gaps.append("no case with R = 1 and more than one workgroup")
    if not any(c.R == 3 and c.B < 3 for c in cases):
        gaps.append("no case with R = 3 and B < R")
    if not any(c.K == MAX_K for c in cases):
        gaps.append(f"no case with K = {MAX_K}")
    if not any(c.row == MAX_ROW for c in cases):
        gaps.append(f"no case with a row of exactly {MAX_ROW} outputs")
    groups = {groups_per_lane(c.nb) for c in cases} | {groups_per_lane(g[3]) for g in grid}
    for n in (1, 2, 3, 4):
        if n not in groups:
            gaps.append(f"no HL-Gauss case with {n} groups per lane")
    for c in cases:
        if not within_plan_limits(c.K, c.A, c.nb, c.B):
            gaps.append(f"{c.id} is outside the plan's limits")
    for g in grid:
        if not within_plan_limits(GRID_K, GRID_A, g[3], GRID_B):
            gaps.append(f"{g[0]} is outside the plan's limits")
    return gaps
