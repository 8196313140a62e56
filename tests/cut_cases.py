"""gs4d_stat_cut (include/gs4d.h) restated in numpy, and the tables of its tests.

Test infrastructure only (tests/test_cut_host.py pins it on the CPU, tests/test_gpu_cut.py runs it).  The bar is restate(): a descending sort and
two counts, which share nothing with the kernels' radix select.  An integer problem: every comparison is exact.

Sizes: the histogram kernel walks the table in tiles of TILE rows (256 threads, 8 rows each; CUT_TILE in csrc/gs4d_internal.h) with at most GROUPS
workgroups (CUT_GROUPS) and a grid stride beyond.  SIZES hits a wave, a workgroup's round of 256 rows and the edges of a tile; STRIDE_SIZE gives
every workgroup of the capped grid a second tile and the first one a third, so the grid stride runs everywhere.
"""
import numpy as np

import compact_cases as cc

STAT = cc.STAT
FIELDS = ("pixels", "wmax", "wsum")                        # GS4D_STAT_PIXELS, GS4D_STAT_WMAX, GS4D_STAT_WSUM = 0, 1, 2
FIELD_BITS = {"pixels": 32, "wmax": 32, "wsum": 64}
DIGIT_BITS = 8                                             # CUT_DIGIT_BITS
TILE = 2048                                                # CUT_TILE
GROUPS = 1024                                              # CUT_GROUPS
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 1)
STRIDE_SIZE = 2 * GROUPS * TILE + 1                        # 2 * GROUPS + 1 tiles
CUT = np.dtype([("value", "<u8"), ("above", "<u4"), ("equal", "<u4")])
GENERATORS = ("equal", "distinct", "top_digit", "bottom_digit", "high_half", "weights", "mostly_zero", "ties")


def field_u64(table, field):
    """f of gs4d.h: the field of every row as a uint64 (pixels and wmax zero-extended, wmax as its bit pattern)"""
    return np.ascontiguousarray(table[field]).astype(np.uint64)


def descending(f):
    return np.sort(f)[::-1]


def restate(f, budget, desc=None):
    """-> (value, above, equal) of gs4d.h for the uint64 array f and a budget >= 1; desc: descending(f), where the caller shares one sort among
    budgets"""
    n = len(f)
    if n == 0:
        return 0, 0, 0
    k = min(int(budget), n)
    v = (descending(f) if desc is None else desc)[k - 1]
    return int(v), int((f > v).sum()), int((f == v).sum())


def loop_restate(f, budget):
    """the contract as a plain Python loop (small tables): the largest value v with at least k rows >= v, found by trying every row's value"""
    vals = [int(x) for x in f]
    n = len(vals)
    if n == 0:
        return 0, 0, 0
    k = min(int(budget), n)
    best = None
    for v in vals:
        at_least = 0
        for x in vals:
            if x >= v:
                at_least += 1
        if at_least >= k and (best is None or v > best):
            best = v
    above = equal = 0
    for x in vals:
        if x > best:
            above += 1
        elif x == best:
            equal += 1
    return best, above, equal


def expected_bytes(table, field, budget, desc=None):
    """the 16 bytes `out` must hold"""
    e = np.zeros(1, CUT)
    e["value"], e["above"], e["equal"] = restate(field_u64(table, field), budget, desc)
    return e.view(np.uint8)


def tie_layout(n):
    """(t, a, b): t distinct rows above everything, an upper tie group of a rows, a lower one of b rows; t + a + b == n"""
    t = n // 4
    a = (n - t) // 2
    return t, a, n - t - a


def tie_budgets(n):
    """the budget that lands on the last member of the upper tie group (above + equal == k) and the one that lands on the first member of the
    lower one, of the `ties` table of n rows; only budgets >= 1"""
    t, a, _ = tie_layout(n)
    return [k for k in (t + a, t + a + 1) if 1 <= k <= max(n, 1)]


def budgets(n):
    """1, 2, n/2, n - 1, n, n + 7 (the clamp) and the two tie-boundary budgets: those that are >= 1, each once, ascending"""
    return sorted({k for k in [1, 2, n // 2, n - 1, n, n + 7] + tie_budgets(n) if k >= 1})


def _spread(r, field, lo_bit):
    """r placed at bit lo_bit of the field's width, over a constant pattern in the bits below"""
    const = {"pixels": 0x00A1B2C3, "wmax": 0x003D5E7F, "wsum": 0x0011223344556677}[field]
    return (r.astype(np.uint64) << np.uint64(lo_bit)) | np.uint64(const & ((1 << lo_bit) - 1))


def table(gen, n):
    """the STAT table of n rows of a generator; every field carries the generator's pattern at its own width"""
    rng = np.random.default_rng(cc.seed(f"cut/{gen}/{n}"))
    st = np.zeros(n, STAT)
    if gen == "equal":                                      # equal == n at every budget
        st["pixels"], st["wmax"], st["wsum"] = 7, cc.BITS_1_255, cc.WSUM_MIN
    elif gen == "distinct":                                 # no ties: above == k - 1, equal == 1; the values spread over every digit
        for field, mul in (("pixels", 1001), ("wmax", 997), ("wsum", (1 << 40) + 12345)):
            st[field] = (rng.permutation(n).astype(np.uint64) * np.uint64(mul) + np.uint64(3)).astype(STAT[field])
    elif gen == "top_digit":                                # the first pass decides; every later one sees one bin
        for field in FIELDS:
            st[field] = _spread(rng.integers(0, 1 << DIGIT_BITS, n), field, FIELD_BITS[field] - DIGIT_BITS).astype(STAT[field])
    elif gen == "bottom_digit":                             # every pass but the last sees one bin
        for field in FIELDS:
            base = {"pixels": 0x12345600, "wmax": 0x3F7FFF00, "wsum": (cc.WSUM_MIN << 24) & ~0xFF}[field]
            st[field] = (np.uint64(base) | rng.integers(0, 1 << DIGIT_BITS, n).astype(np.uint64)).astype(STAT[field])
    elif gen == "high_half":                                # wsum differs at bit 32 and above only (equal low words): compare and prefix must be 64-bit
        st["pixels"] = _spread(rng.integers(0, 1 << 16, n), "pixels", 16).astype(np.uint32)
        st["wmax"] = _spread(rng.integers(0, 1 << 14, n), "wmax", 16).astype(np.uint32)
        st["wsum"] = (rng.integers(0, 1 << 20, n).astype(np.uint64) << np.uint64(32)) | np.uint64(cc.WSUM_MIN & 0xFFFFFFFF)
    elif gen == "weights":                                  # what a draw leaves: wmax real float32 weights in (0, 1], counts, sums in units of 2^-24
        w = (1.0 - rng.uniform(0.0, 1.0, n)).astype(np.float32)
        w[w <= 0] = 1.0
        st["wmax"] = w.view(np.uint32)
        st["pixels"] = rng.integers(1, 5000, n)
        st["wsum"] = st["pixels"].astype(np.uint64) * np.rint(w.astype(np.float64) * 0.5 * (1 << 24)).astype(np.uint64)
    elif gen == "mostly_zero":                              # a few rows that showed, the rest zero: budgets beyond them land in the zeros
        hot = rng.permutation(n)[:n // 50 + min(n, 1)]
        st["pixels"][hot] = rng.integers(1, 300, hot.size)
        st["wmax"][hot] = (1.0 - rng.uniform(0.0, 1.0, hot.size)).astype(np.float32).view(np.uint32)
        st["wsum"][hot] = rng.integers(1, 1 << 40, hot.size).astype(np.uint64)
    elif gen == "ties":                                     # tie_layout: distinct rows on top, then two tie groups; shuffled over the table
        t, a, b = tie_layout(n)
        for field, hi in (("pixels", 0x00010000), ("wmax", 0x3F000000), ("wsum", cc.WSUM_MIN + (1 << 32))):
            v = np.concatenate([hi + 1 + np.arange(t, dtype=np.uint64), np.full(a, hi, np.uint64), np.full(b, hi - (1 << 8), np.uint64)])
            st[field] = v.astype(STAT[field])
        st = st[rng.permutation(n)]
    else:
        raise KeyError(gen)
    return np.ascontiguousarray(st)
