"""The instantiations of the radix sort's pass kernel (csrc/sort.hip, k_os_pass<THREADS, ITEMS, ATOMIC_RANK, RB>) and the sorts that take each
of them through every branch of its cooperation between workgroups.

Test infrastructure only (tests/test_sort_cases_host.py pins this table on the CPU, tests/test_gpu_sort_forms.py runs it).  Plain numpy; the bar is
reference(): numpy's stable argsort, which shares nothing with the kernel, the LSD checker or oracle.sort_pairs.

What a tile count means.  A pass cuts the keys into tiles of TILE_KEYS = threads x items; tile t belongs to group t // 16 and super-group
t // 256.  A tile publishes its per-digit counts in three places and sums its exclusive prefix from three levels (os_lookback):

* the grid is min(tiles, resident workgroups).  Up to `resident` tiles every tile has a workgroup of its own and the kernel leaves behind the
  write-out; above it the workgroups are persistent: second ticket draw, wcnt zeroed again, skeys/svals/loff/gpos reused, digit_base kept.
  resident_bound() is an upper bound of what the runtime can answer, so resident_bound + 37 tiles reach the loop on any build;
* `grp + 1 < ngroups` decides whether a tile adds to its group's accumulator at all: 16 tiles against 17, 32 + 1 = 33;
* `sup + 1 < nsuper` decides whether the add returns the old word and the sixteenth arrival hands the group's total up: 256 tiles against 257
  (one super-group and one tile) and 272 + 1 = 273 (a second group in the last super-group);
* the loop over earlier super-groups reads 16 accumulators a round: its second round needs sup >= 17, more than 4352 tiles (DEEP).

resident_bound(shape, rb) = 256 CUs x min(160 KiB // lds_bytes, 32 waves // (threads / 64)), with lds_bytes counted from the __shared__
declarations of k_os_pass.  Occupancy can only be lower (registers).  For 8-bit digits, shapes 1 to 7:
    lds_bytes       22552  43032  83992  38936  75800  59416  26648
    workgroups / CU     7      3      1      4      2      2      4       (shape 7: the wave cap, LDS would allow 6)
    resident_bound   1792    768    256   1024    512    512   1024
and for 9-bit digits (512 bins), shapes 2, 3, 5, 6, 7:
    lds_bytes       53288 102440  86056  69672  36904
    resident_bound    768    256    256    512   1024                     (512 x 16 drops to one workgroup per CU)
"""
import functools
import zlib

import numpy as np

OS_GROUP, OS_SUPER = 16, 16                            # tiles per group, groups per super-group (csrc/sort.hip)
TILES_PER_SUPER = OS_GROUP * OS_SUPER
CUS, LDS_PER_CU, WAVES_PER_CU = 256, 160 * 1024, 32

# GS4D_SORT_SHAPE -> (threads, keys per thread): the switch of radix_sort_pairs
SHAPES = {1: (256, 8), 2: (512, 8), 3: (1024, 8), 4: (256, 16), 5: (512, 16), 6: (512, 12), 7: (512, 4)}
# (shape, digit bits GS4D_SORT_RB, ranking GS4D_SORT_RANK: 1 ballot, 2 LDS atomic).  9-bit digits need a thread per bin: no 256-thread form.
# The forms of a shape are neighbours, so that they find each other's cases in the cache below (the sizes depend on the tile and the bound).
FORMS = [(shape, rb, rank) for shape in SHAPES for rb in (8, 9) if rb == 8 or SHAPES[shape][0] >= 512 for rank in (1, 2)]


def tile_keys(shape):
    threads, items = SHAPES[shape]
    return threads * items


def lds_bytes(shape, rb):
    """static LDS of k_os_pass<threads, items, *, rb>: skeys, svals [TILE_KEYS]; wcnt [WAVES][BINS]; loff, gpos [BINS]; s_tmp [BINS / 64];
    s_dead; s_tile — all uint32"""
    threads, items = SHAPES[shape]
    tile, waves, bins = threads * items, threads // 64, 1 << rb
    return 4 * (2 * tile + waves * bins + 2 * bins + bins // 64 + 2)


def resident_bound(shape, rb):
    """no device holds more workgroups of this form at once"""
    waves = SHAPES[shape][0] // 64
    return CUS * min(LDS_PER_CU // lds_bytes(shape, rb), WAVES_PER_CU // waves)


def edge_tile_counts(shape, rb):
    """[(tiles, n)]: the tile counts a form is run at, the largest last.  The last tile holds 1 key or TILE_KEYS - 3 in turn; n % 4 != 0
    (k_os_hist reads uint4 and has a tail)."""
    tk = tile_keys(shape)
    counts = [16, 17, 33, 256, 257, 273, resident_bound(shape, rb) + 37]
    return [(t, (t - 1) * tk + (1 if i % 2 == 0 else tk - 3)) for i, t in enumerate(counts)]


# the third look-back level's second round: shape 7 (2048-key tiles, both digit widths); tiles 4352 .. 4399 have sup = 17
DEEP_SHAPE, DEEP_TILES = 7, 4400
DEEP_N = (DEEP_TILES - 1) * 2048 + 5
DEEP = [(rb, rank) for rb in (8, 9) for rank in (1, 2)]


def banded_pass(rb, shift):
    """the pass whose digit lies wholly in the band bits (>= shift) of super_bands / group_bands"""
    return -(-shift // rb)


# ---- keys: each generator takes (n, tile_keys, rng) ----
def random32(n, tk, rng):
    return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def few(n, tk, rng):
    pool = np.unique(rng.integers(0, 2 ** 32, 64, dtype=np.uint64))[:37].astype(np.uint32)
    assert pool.size == 37
    return pool[rng.integers(0, 37, n)]


def ascending(n, tk, rng):
    """a tile is one digit in the upper passes: tile counts of TILE_KEYS"""
    return np.arange(n, dtype=np.uint32)


def descending(n, tk, rng):
    return np.arange(n, dtype=np.uint32)[::-1].copy()


def _bands(n, per_band, shift, rng):
    band = (np.arange(n, dtype=np.uint64) // np.uint64(per_band)) << np.uint64(shift)
    assert int(band[-1]) < 2 ** 32
    return (band | rng.integers(0, 1 << shift, n, dtype=np.uint64)).astype(np.uint32)


def super_bands(n, tk, rng):
    """super-group s holds digit s of the top pass and nothing else: every tile word, group sum and super-group sum of that digit is as
    large as it can be"""
    return _bands(n, TILES_PER_SUPER * tk, 24, rng)


def group_bands(n, tk, rng):
    return _bands(n, OS_GROUP * tk, 16, rng)


STRAY_KEY, STRAY_SMALLER = 0x3A5C7E91, 0x3A1C7E91      # they differ in byte 2 alone: one live digit at either width (bit 22)
STRAY_LIVE_BYTES = 1


def one_stray(n, tk, rng):
    """one constant, and a smaller key at the very end: it goes to the front and every other element moves by one, across every tile"""
    keys = np.full(n, STRAY_KEY, np.uint32)
    keys[-1] = STRAY_SMALLER
    return keys


GENERATORS = {f.__name__: f for f in (random32, few, ascending, descending, super_bands, group_bands, one_stray)}


def reference(keys, vals):
    """THE bar: the stable ascending sort"""
    order = np.argsort(keys, kind="stable")
    return keys[order], vals[order]


@functools.lru_cache(maxsize=20)                        # the 16 sorts of one form, and the large ones of the next where its bound differs
def case(gen, n, tk):
    """(keys, vals, sorted keys, sorted vals) of one sort, computed once and shared by the tests that run it (read-only).  The values are a
    random permutation of arange(n): a payload that merely follows the index is caught."""
    rng = np.random.default_rng(zlib.crc32(f"{gen}-{n}-{tk}".encode()))
    keys = GENERATORS[gen](n, tk, rng)
    vals = rng.permutation(n).astype(np.uint32)
    out = (keys, vals) + reference(keys, vals)
    for a in out:
        a.setflags(write=False)
    return out


def describe_mismatch(what, got, want, keys, tk, form, n):
    """where a sort went wrong, in the kernel's terms: the first bad output slot, and the tile, group and super-group that slot lies in
    and the element that belongs there came from"""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    p = int(bad[0])
    src = int(np.argsort(keys, kind="stable")[p])
    where = lambda i: f"tile {i // tk}, group {i // tk // OS_GROUP}, super-group {i // tk // TILES_PER_SUPER}"
    return (f"{what} differ: form (shape, rb, rank) = {form}, n = {n}, {-(-n // tk)} tiles of {tk}; {bad.size} bad slots, the first at {p} "
            f"({where(p)}): got {int(got[p]):#x}, want {int(want[p]):#x}, which the input holds at {src} ({where(src)})")
