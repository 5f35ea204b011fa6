"""The case table of tests/helpers/head_geometry.py, without a GPU: it keeps the coverage tests/test_gpu_head_geometry.py exists for, every
case lies inside the plan's limits, and the rule it restates (csrc/head_loss.h, rows_per_wg) is still the header's text.  If the rule
changes, this test fails and the table is revisited."""
import os
import re

import pytest

from tests.helpers import head_geometry as hg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "is-dqn_amd", "csrc")


def test_the_table_keeps_its_coverage():
    assert hg.coverage_gaps() == []
    # written out once more, by hand, for the rows the table was built around
    by_r = {R: [c for c in hg.CASES if c.R == R] for R in (1, 2, 3, 4)}
    assert all(by_r[R] for R in by_r)  # (one table for the three losses: every loss meets every R)
    assert any(c.B % 3 for c in by_r[3]) and any(c.B % 2 for c in by_r[2]) and any(c.B < 3 for c in by_r[3])
    assert any(c.K == 64 for c in hg.CASES) and any(c.row == 5456 for c in hg.CASES)
    assert {hg.groups_per_lane(nb) for nb in hg.grid_bin_counts()} | {hg.groups_per_lane(c.nb) for c in hg.CASES} == {1, 2, 3, 4}
    assert set(hg.VARIANT_IDS) <= set(hg.BY_ID) and {hg.BY_ID[i].R for i in hg.VARIANT_IDS} == {1, 2, 3}


REQUIRED = {  # id: (K, A, nb, B, R, workgroups)
    "r3-ragged": (9, 2, 256, 5, 3, 2),
    "r3-short": (9, 2, 256, 2, 3, 1),
    "r3-c5-heads": (32, 2, 65, 7, 3, 3),
    "r3-widest": (10, 2, 248, 4, 3, 2),
    "r3-k64": (64, 2, 40, 4, 3, 2),
    "r4-k64": (64, 2, 2, 5, 4, 2),
    "r2": (12, 1, 256, 5, 2, 3),
    "r1": (20, 1, 256, 3, 1, 3),
}


@pytest.mark.parametrize("cid", list(REQUIRED))
def test_the_required_rows_are_in_the_table(cid):
    c = hg.BY_ID[cid]
    assert (c.K, c.A, c.nb, c.B, c.R, c.n_wg) == REQUIRED[cid] and c.n_heads == c.K + 1


def test_removing_any_row_that_is_alone_in_its_class_is_noticed():
    """Every required row but r3-ragged and r3-k64 is the only one of its kind: without it coverage_gaps() is not empty.  (r3-ragged's
    classes -- R = 3, B mod 3 != 0, four groups -- are shared with r3-c5-heads, r3-widest and r3-k64: REQUIRED above holds those.)"""
    alone = {"r3-short": "B < R", "r3-widest": "5456", "r4-k64": "R = 4", "r2": "R = 2", "r1": "R = 1"}
    for cid, word in alone.items():
        gaps = hg.coverage_gaps([c for c in hg.CASES if c.id != cid])
        assert gaps and any(word in g for g in gaps), (cid, gaps)
    assert any("K = 64" in g for g in hg.coverage_gaps([c for c in hg.CASES if c.K != 64]))
    assert any("3 groups" in g for g in hg.coverage_gaps(grid=[g for g in hg.grid_cases() if hg.groups_per_lane(g[3]) != 3]))


def test_every_case_respects_the_plans_limits():
    for c in hg.CASES:
        assert hg.within_plan_limits(c.K, c.A, c.nb, c.B), c
        assert c.R * c.K * c.nb <= hg.LDS_FLOATS or c.R == 1, c  # s_dl stays within the 32 KB the rule is written for
        assert c.R * c.K <= hg.MAX_ROWS * 64  # LossStage's [MAX_ROWS * 64] arrays
        assert 3 <= c.B <= 7 or c.id == "r3-short"
    for gid, vmin, vmax, nb, ratio in hg.grid_cases():
        assert hg.within_plan_limits(hg.GRID_K, hg.GRID_A, nb, hg.GRID_B) and hg.rows_per_wg(hg.GRID_K, nb) == 4 and vmax > vmin and ratio > 0
    assert not hg.within_plan_limits(10, 2, 249, 4) and not hg.within_plan_limits(65, 1, 2, 4)


def test_the_limits_are_the_plans():
    text = open(os.path.join(CSRC, "net_plan.h")).read()
    assert len(re.findall(r"P\.nlog\s*<=\s*5456", text)) == 2  # histogram and quantile heads
    assert len(re.findall(r"P\.K\s*<=\s*64", text)) >= 2
    assert re.search(r"n_bins\s*>=\s*2\s*&&\s*cfg->n_bins\s*<=\s*256", text) and re.search(r"n_quantiles\s*>=\s*2\s*&&\s*cfg->n_quantiles\s*<=\s*256", text)


def test_the_rule_is_still_the_headers():
    text = open(os.path.join(CSRC, "head_loss.h")).read()
    assert re.search(r"constexpr\s+int\s+MAX_ROWS\s*=\s*4\s*;", text)
    assert re.search(r"8192\s*/\s*\(\s*K\s*\*\s*nb\s*\)", text)
    assert re.search(r"R\s*<\s*1\s*\?\s*1\s*:\s*R\s*>\s*MAX_ROWS\s*\?\s*MAX_ROWS\s*:\s*R", text)
    assert re.search(r"constexpr\s+int\s+MAX_GROUP\s*=\s*256\s*;", text) and re.search(r"PER_LANE\s*=\s*MAX_GROUP\s*/\s*64", text)
    # the restatement at the thresholds the header's integer division puts them at
    for K_nb, R in ((2048, 4), (2049, 3), (2730, 3), (2731, 2), (4096, 2), (4097, 1), (8192, 1), (8193, 1), (16384, 1), (2, 4)):
        assert hg.rows_per_wg(1, K_nb) == R, K_nb
    assert [hg.groups_per_lane(nb) for nb in (2, 64, 65, 128, 129, 192, 193, 256)] == [1, 1, 2, 2, 3, 3, 4, 4]


def test_dyadic_supports_are_exact_in_float32():
    import numpy as np

    for nb in sorted({c.nb for c in hg.CASES}):
        vmin, vmax = hg.dyadic_support(nb)
        eta = (vmax - vmin) / nb
        e = vmin + np.arange(nb + 1) * eta
        c = vmin + (np.arange(nb) + 0.5) * eta
        assert vmin == 1.0 and 14.0 <= vmax - vmin <= 28.0 and np.log2(eta) == round(np.log2(eta))
        assert (e.astype(np.float32).astype(np.float64) == e).all() and (c.astype(np.float32).astype(np.float64) == c).all()
