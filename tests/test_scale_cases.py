"""CPU: the inputs of tests/test_gpu_scale_edges.py have the properties their cases are named for — per-round sums of per-tile counts, heads of the
sorted labels by tile, the trip of the box kernel that holds the extremes.  numpy alone: no device, no library."""
import numpy as np
import pytest

import compact_cases as cc
import merge_cases as mc
import reorder_cases as rc
import time_window_cases as tw


@pytest.mark.parametrize("n", cc.ROUND_SIZES)
def test_the_round_patterns_are_what_they_are_named_for(n):
    for pattern in cc.ROUND_PATTERNS:
        mask = cc.round_mask(pattern, n)
        cc.assert_round_pattern(pattern, n, mask)
        if n == cc.ROUND + 1:                                  # both tables keep exactly the mask
            assert np.array_equal(cc.keeps(cc.round_table(mask), cc.RULES["visible"]), mask)
            assert np.array_equal(tw.keeps(tw.mask_table(mask), 24.0, 26.0), mask)


def test_a_degenerate_round_pattern_is_refused():
    n = cc.ROUND + 1
    m = cc.round_mask("seam", n)
    m[cc.ROUND] = False                                        # nothing kept in round 2
    with pytest.raises(AssertionError):
        cc.assert_round_pattern("seam", n, m)
    m = cc.round_mask("first_round", n)
    m[n - 1] = True                                            # a kept row behind round 1
    with pytest.raises(AssertionError):
        cc.assert_round_pattern("first_round", n, m)
    with pytest.raises(AssertionError):
        cc.assert_round_pattern("sparse", n, cc.round_mask("last_round", n))


class _Stat:
    RECORD_STAT = cc.STAT                                      # (the binding's dtype has the same fields; only `pixels` is looked at here)


@pytest.mark.parametrize("case", mc.ROUND_CASES)
def test_the_merge_labels_have_heads_where_the_case_says(case):
    labels, stats, _ = mc.round_labels(case, _Stat)
    member = labels != mc.ID_NONE                              # (every record of the pool is a member by itself: round_records)
    if stats is not None:
        member &= mc.passes(stats)
    assert mc.assert_round_labels(case, labels, member) > 250_000


@pytest.mark.parametrize("trip", rc.STRIDE_TRIPS)
def test_the_extremes_sit_in_the_named_trip(trip):
    pos = rc.stride_positions(trip)
    rc.assert_stride_positions(trip, pos)
    other = "first" if trip == "second" else "second"
    with pytest.raises(AssertionError):
        rc.assert_stride_positions(other, pos)
