"""The premises of tests/test_gpu_sort_forms.py, checked on the CPU (tests/sort_cases.py is the table): so that the GPU test cannot quietly
test less than it claims.

Every legal instantiation of k_os_pass is listed; its static LDS fits a CU; every form is run at a tile count no device can hold at once,
and at the counts on either side of each group / super-group condition; the sizes give exactly those tile counts; the banded keys put one
digit into whole tiles, groups and super-groups of the banded pass, which is what drives the packed look-back fields {epoch:18, count:14}
and {arrivals:8, sum:24} to their largest values, and those values fit; the bar (numpy's stable argsort) agrees with std::stable_sort."""
import re
import os

import numpy as np
import pytest

import sort_cases as sc

SORT_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "4dgaussiansplatrendering_amd", "csrc", "sort.hip")


def test_forms_are_the_24_legal_instantiations():
    assert len(sc.FORMS) == 24 and len(set(sc.FORMS)) == 24
    for shape, rb, rank in sc.FORMS:
        threads, items = sc.SHAPES[shape]
        assert rb in (8, 9) and rank in (1, 2) and (1 << rb) <= threads            # one thread per digit
    assert {(s, rb) for s, rb, _ in sc.FORMS} == {(s, 8) for s in sc.SHAPES} | {(s, 9) for s in (2, 3, 5, 6, 7)}
    assert [sc.SHAPES[s] for s in range(1, 8)] == [(256, 8), (512, 8), (1024, 8), (256, 16), (512, 16), (512, 12), (512, 4)]
    assert len(sc.DEEP) == 4 and sc.SHAPES[sc.DEEP_SHAPE] == (512, 4)


def test_shapes_and_shared_arrays_are_those_of_the_source():
    """the table against the text of sort.hip: the switch of radix_sort_pairs and the __shared__ declarations lds_bytes() counts"""
    src = open(SORT_HIP).read()
    switch = {int(k): (int(t), int(i)) for k, t, i in re.findall(r"case (\d): return [^;]*?GS4D_OS8?\((\d+), (\d+)\)", src)}
    switch[7] = tuple(int(x) for x in re.search(r"default: return GS4D_OS\((\d+), (\d+)\)", src).groups())
    assert switch == sc.SHAPES
    kernel = src[src.index("void k_os_pass("):src.index("void k_lds_order_test(")]
    decl = re.findall(r"__shared__ uint32_t (\w+)((?:\[[^\]]+\])*);", kernel)
    assert decl == [("skeys", "[TILE_KEYS]"), ("svals", "[TILE_KEYS]"), ("wcnt", "[WAVES][BINS]"), ("loff", "[BINS]"), ("gpos", "[BINS]"),
                    ("s_tmp", "[BINS / 64]"), ("s_dead", ""), ("s_tile", "")]
    assert "constexpr uint32_t OS_GROUP = 16;" in src and "constexpr uint32_t OS_SUPER = 16;" in src


def test_lds_fits_and_resident_bounds():
    bounds = {}
    for shape, rb, _ in sc.FORMS:
        assert sc.lds_bytes(shape, rb) <= 160 * 1024
        bounds[shape, rb] = sc.resident_bound(shape, rb)
    print(bounds)
    assert [sc.lds_bytes(s, 8) for s in range(1, 8)] == [22552, 43032, 83992, 38936, 75800, 59416, 26648]
    assert [bounds[s, 8] for s in range(1, 8)] == [1792, 768, 256, 1024, 512, 512, 1024]
    assert [bounds[s, 9] for s in (2, 3, 5, 6, 7)] == [768, 256, 256, 512, 1024]


@pytest.mark.parametrize("shape,rb,rank", sc.FORMS)
def test_tile_counts_of_every_form(shape, rb, rank):
    tk = sc.tile_keys(shape)
    cases = sc.edge_tile_counts(shape, rb)
    assert [t for t, _ in cases[:-1]] == [16, 17, 33, 256, 257, 273]
    assert cases[-1][0] == sc.resident_bound(shape, rb) + 37 > max(t for t, _ in cases[:-1])      # the persistent loop, on any build
    for t, n in cases:
        assert -(-n // tk) == t and n % 4 != 0 and n < 2 ** 31
    last = [n - (t - 1) * tk for t, n in cases]
    assert set(last) == {1, tk - 3} and last[-1] == 1                                # nearly empty and nearly full
    # either side of each condition of the kernel
    ngroups = lambda t: -(-t // sc.OS_GROUP)
    nsuper = lambda t: -(-ngroups(t) // sc.OS_SUPER)
    assert [ngroups(t) for t, _ in cases[:3]] == [1, 2, 3]
    assert [nsuper(t) for t, _ in cases[3:6]] == [1, 2, 2] and [ngroups(t) for t, _ in cases[3:6]] == [16, 17, 18]
    assert nsuper(cases[-1][0]) >= 2                                                 # the large size hands group totals up


def test_deep_case_reaches_the_second_round_of_super_groups():
    assert sc.tile_keys(sc.DEEP_SHAPE) == 2048 and -(-sc.DEEP_N // 2048) == sc.DEEP_TILES and sc.DEEP_N % 4 != 0
    sup_last = (sc.DEEP_TILES - 1) // sc.TILES_PER_SUPER
    assert sup_last >= 17 and 4352 // sc.TILES_PER_SUPER == 17                       # for (t = 0; t < sup; t += 16): t = 16 runs
    assert sc.DEEP_TILES > sc.resident_bound(sc.DEEP_SHAPE, 8) and sc.DEEP_TILES > sc.resident_bound(sc.DEEP_SHAPE, 9)
    assert sorted(sc.DEEP) == [(8, 1), (8, 2), (9, 1), (9, 2)]


def _largest_count(digit, per, bins):
    """largest count of one digit within consecutive runs of `per` keys"""
    run = np.arange(digit.size) // per
    return int(np.bincount(run * bins + digit, minlength=(int(run[-1]) + 1) * bins).max())


@pytest.mark.parametrize("rb", [8, 9])
@pytest.mark.parametrize("tk", sorted({sc.tile_keys(s) for s in sc.SHAPES}))
def test_banded_keys_fill_the_packed_fields(tk, rb):
    """one super-group, one group and five keys more, at the real tile sizes"""
    n = (sc.TILES_PER_SUPER + sc.OS_GROUP) * tk + 5
    rng = np.random.default_rng(tk + rb)
    bins = 1 << rb
    for gen, shift, full in ((sc.super_bands, 24, ("tile", "group", "super")), (sc.group_bands, 16, ("tile", "group"))):
        keys = gen(n, tk, rng)
        p = sc.banded_pass(rb, shift)
        assert rb * p >= shift > rb * (p - 1) and p < 4
        digit = ((keys >> np.uint32(rb * p)) & np.uint32(bins - 1)).astype(np.int64)
        got = {"tile": _largest_count(digit, tk, bins), "group": _largest_count(digit, sc.OS_GROUP * tk, bins),
               "super": _largest_count(digit, sc.TILES_PER_SUPER * tk, bins)}
        for level in full:
            assert got[level] == {"tile": tk, "group": sc.OS_GROUP * tk, "super": sc.TILES_PER_SUPER * tk}[level], (gen.__name__, level, got)
        assert got["tile"] < 2 ** 14 and got["group"] < 2 ** 24 and got["super"] < 2 ** 24
        # below the band the bits are random: the lower passes are ordinary
        assert np.unique(keys & np.uint32(0xFF)).size == 256 and np.unique((keys >> np.uint32(8)) & np.uint32(0xFF)).size == 256
    # group_bands gives every group a band of its own (the group's accumulator holds one digit, its neighbours' another)
    g = sc.group_bands(n, tk, rng) >> np.uint32(16)
    assert np.array_equal(g, np.arange(n) // (sc.OS_GROUP * tk))
    s = sc.super_bands(n, tk, rng) >> np.uint32(24)
    assert np.array_equal(s, np.arange(n) // (sc.TILES_PER_SUPER * tk))


def test_band_numbers_fit_the_key_at_the_largest_sizes():
    for shape, rb, _ in sc.FORMS:
        tk, (t, n) = sc.tile_keys(shape), sc.edge_tile_counts(shape, rb)[-1]
        assert (n - 1) // (sc.TILES_PER_SUPER * tk) < 2 ** 8
    assert (sc.DEEP_N - 1) // (sc.TILES_PER_SUPER * 2048) == 17 and (sc.DEEP_N - 1) // (sc.OS_GROUP * 2048) < 2 ** 16


def test_generators():
    rng = np.random.default_rng(5)
    n, tk = 5003, 64
    assert np.unique(sc.few(n, tk, rng)).size == 37
    assert np.array_equal(sc.ascending(n, tk, rng), np.arange(n)) and np.array_equal(sc.descending(n, tk, rng), np.arange(n)[::-1])
    k = sc.one_stray(n, tk, rng)
    assert k[-1] < k[0] and np.all(k[:-1] == k[0])
    diff = int(np.bitwise_or.reduce(k ^ k[0]))
    assert sum(1 for b in range(4) if (diff >> (8 * b)) & 0xFF) == sc.STRAY_LIVE_BYTES == 1
    for rb in (8, 9):                                                                # "two live digits at most": here one at either width
        assert sum(1 for p in range(4) if (diff >> (rb * p)) & ((1 << rb) - 1)) == 1
    for name, gen in sc.GENERATORS.items():
        out = gen(n, tk, np.random.default_rng(1))
        assert out.dtype == np.uint32 and out.shape == (n,) and out.flags.c_contiguous, name


@pytest.mark.parametrize("gen", list(sc.GENERATORS))
def test_reference_agrees_with_stable_sort(oracle, gen):
    n, tk = 6007, 8                                                                  # 751 tiles of 8: bands of 128 and 2048 keys
    keys, vals, ek, ev = sc.case(gen, n, tk)
    assert np.array_equal(np.sort(vals), np.arange(n))
    ok, ov = oracle.sort_pairs(keys, vals, "std")
    assert np.array_equal(ek, ok) and np.array_equal(ev, ov)
    assert not keys.flags.writeable and not ev.flags.writeable
    assert sc.case(gen, n, tk)[0] is keys                                            # computed once
    assert sc.describe_mismatch("keys", ek, ek, keys, tk, (1, 8, 1), n) == ""
    wrong = ek.copy()
    wrong[4000] ^= 1
    msg = sc.describe_mismatch("keys", wrong, ek, keys, tk, (1, 8, 1), n)
    assert "first at 4000 (tile 500, group 31, super-group 1)" in msg and "n = 6007" in msg and "(1, 8, 1)" in msg
