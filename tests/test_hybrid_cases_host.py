"""CPU: the premises of tests/hybrid_cases.py, for every span the depth sort's hybrid is planned for — so that no case of
tests/test_gpu_sort_hybrid_edges.py is vacuous.  Through gs4d.build_records_4d, gs4d.key_bounds (the library's host code), oracle.keygen and numpy;
no GPU.  Nothing here is skipped on a condition: a premise that does not hold for the chosen inputs fails."""
import numpy as np
import pytest

import hybrid_cases as hc
import sort_cases as sc

# (w0, w1, LB) of k_os_tail for spans of 19..27 bits, written out by hand from csrc/sort.hip: rem = bits - 9, w0 = (rem + 1) >> 1, w1 = rem >> 1,
# k_os_tail<256> for plan.top = rem <= 16
EDGES = {19: (5, 5, 256), 20: (6, 5, 256), 21: (6, 6, 256), 22: (7, 6, 256), 23: (7, 7, 256), 24: (8, 7, 256), 25: (8, 8, 256), 26: (9, 8, 512), 27: (9, 9, 512)}


def _keys(gs4d, oracle, targets, bits):
    """(bias, proven bits, keys) of the record set built for the targets"""
    rec = hc._records(gs4d, targets, hc.span_for(bits))
    bias, proven = hc._proven(gs4d, rec)
    _, ek = oracle.keygen(rec[:len(targets)], 0.0, np.array(hc.CAM0, np.float32))
    return bias, proven, ek.view(np.uint32)


def test_the_edges_are_the_kernels():
    assert hc.WIDTHS == tuple(EDGES)
    for bits, (w0, w1, lb) in EDGES.items():
        assert hc.edges(bits) == (bits - 9, w0, w1, lb) and w0 + w1 == bits - 9 and w1 <= w0 <= 9 and (1 << w0) <= lb
    assert {lb for _, _, lb in EDGES.values()} == {256, 512} and EDGES[25][2] != EDGES[26][2]      # both sides of the switch
    assert hc.TOP_TILE == sc.tile_keys(6) and sc.SHAPES[6] == (512, 12)


def test_the_size_and_digit_tables():
    assert hc.SLOW_SIZES[:len(hc.FIT_SIZES)] == hc.FIT_SIZES and max(hc.FIT_SIZES) == hc.TAIL_TILE
    assert [s for s in hc.SLOW_SIZES if s > hc.TAIL_TILE] == [hc.TAIL_TILE + 1, 2 * hc.TAIL_TILE]
    assert sum(hc.SLOW_SIZES) == 46787
    fit, slow = hc.digits_for(hc.FIT_SIZES), hc.digits_for(hc.SLOW_SIZES)
    assert slow == hc.DIGITS and fit[0] == slow[0] == 0 and fit[-1] == slow[-1] == 511
    assert dict(zip(fit, hc.FIT_SIZES))[511] == 8192 and dict(zip(slow, hc.SLOW_SIZES))[510] == 8193 and dict(zip(slow, hc.SLOW_SIZES))[511] == 16384


@pytest.mark.parametrize("bits", hc.WIDTHS)
@pytest.mark.parametrize("which", ["fit", "slow"])
def test_a_profile_gives_its_buckets_at_every_width(gs4d, oracle, bits, which):
    sizes = hc.FIT_SIZES if which == "fit" else hc.SLOW_SIZES
    digits = hc.digits_for(sizes)
    targets = hc.fit_profile(bits) if which == "fit" else hc.slow_profile(bits)
    assert targets.size == sum(sizes)
    bias, proven, keys = _keys(gs4d, oracle, targets, bits)
    assert (bias, proven) == (hc.KEY_LO, bits), "the box does not prove the width the case is about"
    assert np.abs(keys.astype(np.int64) - targets.astype(np.int64)).max() <= 1, "a record's key is further from its target than one bit pattern"
    assert keys.min() >= bias and int(keys.max() - bias) <= hc.span_for(bits)
    top = np.bincount(hc.top_digit(keys, bias, bits), minlength=512)
    assert np.array_equal(top, hc.profile_counts(sizes, digits)), "top-digit counts"
    assert top[0] == sizes[0] and top[511] == sizes[-1]             # bucket 0 and bucket 511 hold keys
    rem, w0, w1, _ = hc.edges(bits)
    low = (keys - np.uint32(bias)) & np.uint32((1 << rem) - 1)
    if which == "slow":                                             # every value of both local digits occurs
        assert np.unique(low & np.uint32((1 << w0) - 1)).size == 1 << w0 and np.unique(low >> np.uint32(w0)).size == 1 << w1
    # ties at both ends of every bucket of 64 keys and more: each extreme is held at least twice
    for d, size in zip(digits, sizes):
        mine = np.sort(keys[hc.top_digit(keys, bias, bits) == d])
        if size >= 64:
            assert mine[0] == mine[1] and mine[-1] == mine[-2], f"bucket {d}"
    # the payload is not the index, and the two checkers agree on the sort
    vals = hc.payload(keys.size, bits)
    assert np.array_equal(np.sort(vals), np.arange(keys.size)) and not np.array_equal(vals, np.arange(keys.size))
    want = sc.reference(keys, vals)
    got = oracle.sort_pairs(keys, vals, "std")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("bits", [24, 27])
def test_the_six_values_of_the_one_digit_bucket(gs4d, oracle, bits):
    targets, six = hc.one_digit_case(gs4d, oracle, bits, 20000, 40 + bits)
    bias, proven, keys = _keys(gs4d, oracle, targets, bits)
    assert (bias, proven) == (hc.KEY_LO, bits)
    top = hc.top_digit(keys, bias, bits)
    counts = np.bincount(top, minlength=512)
    assert counts[hc.ONE_DIGIT_TOP] == hc.ONE_DIGIT_BUCKET == 3 * 8192 + 5 and np.count_nonzero(counts > hc.TAIL_TILE) == 1
    rem, w0, w1, _ = hc.edges(bits)
    values = np.unique(keys[top == hc.ONE_DIGIT_TOP])
    assert values.size == 6
    low = (values - np.uint32(bias)) & np.uint32((1 << rem) - 1)
    d0, d1 = (low & np.uint32((1 << w0) - 1)).astype(np.int64), (low >> np.uint32(w0)).astype(np.int64)
    # three values that bits [0, w0) alone tell apart, three that bits [w0, rem) alone tell apart
    by_d1, by_d0 = np.unique(d1, return_counts=True), np.unique(d0, return_counts=True)
    assert by_d1[1].max() == 3 and np.unique(d0[d1 == by_d1[0][by_d1[1].argmax()]]).size == 3
    assert by_d0[1].max() == 3 and np.unique(d1[d0 == by_d0[0][by_d0[1].argmax()]]).size == 3
    assert min(np.bincount(np.searchsorted(values, keys[top == hc.ONE_DIGIT_TOP]))) > 3000       # every value is a long run of ties


def test_the_large_uniform_set_fits_and_its_prefixes_are_the_tile_counts(gs4d, oracle):
    sizes = hc.lookback_sizes()
    assert [t for t, _ in sizes] == [549, 17, 257, 273, 549] and sizes[0][1] == sizes[-1][1] == 548 * 6144 + 1 == 3366913
    assert [n % hc.TOP_TILE for _, n in sizes] == [1, 6141, 1, 6141, 1]
    assert max(t for t, _ in sizes) == sc.resident_bound(6, 9) + 37 > sc.resident_bound(6, 9)      # persistent workgroups on any build
    assert 17 > sc.OS_GROUP and 257 > sc.TILES_PER_SUPER and 273 == sc.TILES_PER_SUPER + sc.OS_GROUP + 1
    bias, proven, keys = _keys(gs4d, oracle, hc._uniform(hc.LOOKBACK_N, hc.span_for(24), 548), 24)
    assert (bias, proven) == (hc.KEY_LO, 24)
    for _, n in sizes[:4]:
        top = np.bincount(hc.top_digit(keys[:n], bias, 24), minlength=512)
        print(f"n = {n}: largest bucket {top.max()}")
        assert 0 < top.max() <= hc.TAIL_TILE and top[0] > 0 and top[511] > 0
    starts = np.cumsum(np.bincount(hc.top_digit(keys, bias, 24), minlength=512))
    assert starts[-2] > 1 << 21                                     # bucket starts above 2^21


def test_descending_keys_stay_descending(gs4d, oracle):
    n = 272 * hc.TOP_TILE + 1
    bias, proven, keys = _keys(gs4d, oracle, hc.descending(n), 24)
    assert (bias, proven) == (hc.KEY_LO, 24)
    assert (np.diff(keys.astype(np.int64)) < 0).all()
    top = np.bincount(hc.top_digit(keys, bias, 24), minlength=512)
    assert top.max() <= hc.TAIL_TILE and np.count_nonzero(top) > 500
    # a tile of the top pass holds at most three top digits: its words are as large as they come
    per_tile = [np.unique(hc.top_digit(keys[t * hc.TOP_TILE:(t + 1) * hc.TOP_TILE], bias, 24)).size for t in (0, 100, 271)]
    assert max(per_tile) <= 3


def test_describe_mismatch_names_the_bucket():
    keys = hc.slow_profile(24)
    want = np.sort(keys)
    got = want.copy()
    start = int(np.bincount(hc.top_digit(keys, hc.KEY_LO, 24), minlength=512)[:510].sum())
    got[start + 8192] ^= np.uint32(1)
    text = hc.describe_mismatch("keys", got, want, keys, hc.KEY_LO, 24)
    assert hc.describe_mismatch("keys", want, want, keys, hc.KEY_LO, 24) == ""
    assert f"first at {start + 8192}" in text and "bucket 510" in text and "8193 keys (slow path, slot 8192 of it, chunk 1)" in text and "(8, 7, 256)" in text
