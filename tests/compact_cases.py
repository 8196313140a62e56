"""gs4d_compact_records (include/gs4d.h) restated in numpy, and the tables of its tests.

Test infrastructure only (tests/test_compact_host.py pins this table on the CPU, tests/test_gpu_compact.py runs it).  Plain numpy; the bar is
reference(): np.flatnonzero on the keep rule, which shares nothing with the kernels.  An integer problem: every comparison is exact.

Sizes: the kernels cut the records into tiles of a power of two between 256 and 4096 (COMPACT_TILE), waves of 64 inside them.  SIZES hits the
edges of every such tile; LARGE has more tiles than one round of workgroups on 256 compute units and 100 MB of 96-byte records.
"""
import zlib

import numpy as np

STAT = np.dtype([("pixels", "<u4"), ("wmax", "<u4"), ("wsum", "<u8")])       # wmax as its bit pattern: the rule compares bit patterns
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 1, 33 * 4096 - 3)
LARGE = (1 << 20) + 5
STRIDES = (16, 48, 96, 288, 1024)
STRIDE_SIZES = (65, 4097, 33 * 4096 - 3)
PATTERNS = ("none", "all", "first", "last", "alternating", "tile", "p03", "p50", "p97")
TILE_SPAN = 4096                                          # `tile`: records [TILE_SPAN, 2 * TILE_SPAN) kept — whole tiles of any size, empty ones around
BITS_1_255 = int(np.array([1.0 / 255.0], np.float32).view(np.uint32)[0])
WSUM_MIN = (1 << 32) + 12345                              # a threshold above 2^32: the compare must be a 64-bit one
# name -> (min_pixels, min_wmax bit pattern, min_wsum)
RULES = {"visible": (1, 0, 0), "prune": (1, BITS_1_255, 0), "all_fields": (5, BITS_1_255, WSUM_MIN), "anything": (0, 0, 0)}


def seed(name):
    return zlib.crc32(name.encode())


def keeps(stats, rule, invert=False):
    """the keep rule of gs4d.h on a STAT table: a bool per record"""
    min_pixels, min_wmax, min_wsum = rule
    k = (stats["pixels"] >= np.uint32(min_pixels)) & (stats["wmax"] >= np.uint32(min_wmax)) & (stats["wsum"] >= np.uint64(min_wsum))
    return k != bool(invert)


def reference(stats, rule, src, stride, cap_dst, cap_idx, invert=False):
    """-> (dst_prefix, idx_prefix, kept, written): the first `written` records (rows of `stride` bytes; None without src) and indices (uint32) of
    the outputs, the true kept count and written = min(kept, cap_dst, cap_idx).  A capacity of None: that output is not given."""
    idx = np.flatnonzero(keeps(stats, rule, invert)).astype(np.uint32)
    kept = int(idx.size)
    caps = [c for c in (cap_dst, cap_idx) if c is not None]
    written = min([kept] + caps)
    dst = None if src is None else np.ascontiguousarray(src).view(np.uint8).reshape(len(stats), stride)[idx[:written]]
    return dst, idx[:written].copy(), kept, written


def pattern_mask(pattern, n):
    """which of n records a pattern keeps"""
    m = np.zeros(n, bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[:1] = True
    elif pattern == "last":
        m[n - 1:] = True
    elif pattern == "alternating":
        m[::2] = True
    elif pattern == "tile":
        m[TILE_SPAN:2 * TILE_SPAN] = True
    elif pattern in ("p03", "p50", "p97"):
        m = np.random.default_rng(seed(f"{pattern}/{n}")).uniform(size=n) < {"p03": 0.03, "p50": 0.5, "p97": 0.97}[pattern]
    elif pattern != "none":
        raise KeyError(pattern)
    return m


def pattern_kept(pattern, n):
    """the documented kept count of a pattern (the random ones: whatever their seeded draw gives)"""
    if pattern in ("p03", "p50", "p97"):
        return int(pattern_mask(pattern, n).sum())
    return {"none": 0, "all": n, "first": min(n, 1), "last": min(n, 1), "alternating": (n + 1) // 2, "tile": max(0, min(n, 2 * TILE_SPAN) - TILE_SPAN)}[pattern]


def pattern_table(pattern, n, rule=RULES["prune"]):
    """A STAT table of n rows whose rows pass `rule` exactly where the pattern keeps.  A dropped row fails on exactly ONE of the three fields, by
    one unit where the threshold allows (a zero threshold cannot be failed: the next field takes its turn); a kept row sits on or just above every
    threshold."""
    min_pixels, min_wmax, min_wsum = rule
    rng = np.random.default_rng(seed(f"table/{pattern}/{n}"))
    m = pattern_mask(pattern, n)
    st = np.zeros(n, STAT)
    st["pixels"] = min_pixels + rng.integers(0, 2, n)
    st["wmax"] = min_wmax + rng.integers(0, 2, n)
    st["wsum"] = np.uint64(min_wsum) + rng.integers(0, 2, n).astype(np.uint64)
    fields = [f for f, t in (("pixels", min_pixels), ("wmax", min_wmax), ("wsum", min_wsum)) if t > 0]
    assert fields or m.all(), "a rule without a threshold keeps everything"
    if fields:
        which = rng.integers(0, len(fields), n)
        for k, f in enumerate(fields):
            drop = ~m & (which == k)
            st[f][drop] = {"pixels": min_pixels, "wmax": min_wmax, "wsum": min_wsum}[f] - 1
    return st


def threshold_table(n=None):
    """Rows that straddle each threshold of RULES['all_fields'] separately: every combination of pixels in {min - 1, min, min + 1}, wmax bit
    patterns around bits(1/255f) with 0 and 0x3F800000 (1.0f), and wsum around WSUM_MIN — below it by one, by 2^32 (equal low words), with a low
    word above and a high word below, and 0.  Returns the table (3 * 5 * 6 = 90 rows, tiled past one wave), or its first n rows repeated to n rows:
    the period of 90 against waves of 64 and tiles of a power of two puts every edge row on many lanes, wave offsets and tile boundaries."""
    min_pixels, min_wmax, min_wsum = RULES["all_fields"]
    px = [min_pixels - 1, min_pixels, min_pixels + 1]
    wm = [0, min_wmax - 1, min_wmax, min_wmax + 1, 0x3F800000]
    ws = [0, min_wsum - 1, min_wsum, min_wsum + 1, min_wsum - (1 << 32), 0xFFFFFFFF]
    rows = [(p, w, s) for p in px for w in wm for s in ws]
    st = np.zeros(len(rows), STAT)
    st["pixels"], st["wmax"], st["wsum"] = [r[0] for r in rows], [r[1] for r in rows], np.array([r[2] for r in rows], np.uint64)
    return np.tile(st, 3) if n is None else np.resize(st, n)


def records(n, stride):
    """n records of `stride` bytes whose contents are a function of (record, byte offset): uint32 word w of record i holds i * 2654435761 + w * 40503
    (mod 2^32) — a 16-byte piece that lands in the wrong record or the wrong place of its record is seen."""
    words = stride // 4
    i = np.arange(n, dtype=np.uint64)[:, None]
    w = np.arange(words, dtype=np.uint64)[None, :]
    return ((i * np.uint64(2654435761) + w * np.uint64(40503)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- past one round of the scan ------------------------------------------------------------------------------------------------------------------
# k_compact_scan (csrc/compact.hip) is ONE workgroup of 1024 threads that walks the per-tile counts in rounds of 1024 words; what the earlier rounds
# kept travels in one LDS word.  Round r covers tiles [1024 r, 1024 (r + 1)), records [r * ROUND, (r + 1) * ROUND).
COMPACT_TILE = 2048                                       # records per tile (gs4d_internal.h)
SCAN_THREADS = 1024                                       # tile counts per round of the scan
ROUND = SCAN_THREADS * COMPACT_TILE                       # records per round: 2 097 152
ROUND_SIZES = (ROUND, ROUND + 1, ROUND + COMPACT_TILE + 1, 2 * ROUND + 1)      # one full round and nothing behind it; one tile in round 2; two; three rounds
ROUND_PATTERNS = ("sparse", "seam", "first_round", "last_round")


def tile_counts(mask):
    """kept rows per tile of COMPACT_TILE records: what k_compact_count stores"""
    return np.add.reduceat(mask.astype(np.int64), np.arange(0, mask.size, COMPACT_TILE))


def round_sums(mask):
    """kept rows per round of the scan: the sums of SCAN_THREADS consecutive tile counts"""
    t = tile_counts(mask)
    return np.add.reduceat(t, np.arange(0, t.size, SCAN_THREADS))


def round_mask(pattern, n):
    """which of n > ROUND - COMPACT_TILE records a pattern keeps:
    sparse       about 3 % of the rows, the first and the last row among them: kept rows in every tile of every round;
    seam         about half of the rows of the last tile of round 1 and of the first tile of round 2 (where n has one), nothing else;
    first_round  about 3 % of the rows of round 1, nothing behind it: the count comes out of the carry alone;
    last_round   about 3 % of the rows of the last round (its last row among them), nothing in front of it."""
    rng = np.random.default_rng(seed(f"round/{pattern}/{n}"))
    m = np.zeros(n, bool)
    last = (n - 1) // ROUND * ROUND                       # first record of the last round
    if pattern == "sparse":
        m = rng.uniform(size=n) < 0.03
        for t0 in range(0, n, COMPACT_TILE):              # every tile, whatever the draw gave
            if not m[t0:t0 + COMPACT_TILE].any():
                m[t0] = True
        m[0] = m[n - 1] = True
    elif pattern == "seam":
        lo, hi = ROUND - COMPACT_TILE, min(n, ROUND + COMPACT_TILE)
        m[lo:hi] = rng.uniform(size=hi - lo) < 0.5
        m[ROUND - 1] = True
        if n > ROUND:
            m[ROUND] = True
    elif pattern == "first_round":
        m[:ROUND] = rng.uniform(size=ROUND) < 0.03
        m[ROUND - 1] = True
    elif pattern == "last_round":
        m[last:] = rng.uniform(size=n - last) < 0.03
        m[n - 1] = True
    else:
        raise KeyError(pattern)
    return m


def assert_round_pattern(pattern, n, mask):
    """the property a round pattern is named for, from the per-tile and per-round sums (numpy alone: runs without a device).  A case that has
    degenerated — no second round, an empty seam tile, a kept row in a round that should be empty — fails here."""
    tiles, rounds = tile_counts(mask), round_sums(mask)
    ntiles = -(-n // COMPACT_TILE)
    nrounds = -(-ntiles // SCAN_THREADS)
    assert tiles.size == ntiles and rounds.size == nrounds and int(rounds.sum()) == int(mask.sum())
    assert nrounds == {ROUND: 1, ROUND + 1: 2, ROUND + COMPACT_TILE + 1: 2, 2 * ROUND + 1: 3}[n], "the sizes are named for their rounds"
    assert ntiles - SCAN_THREADS * (nrounds - 1) == {ROUND: 1024, ROUND + 1: 1, ROUND + COMPACT_TILE + 1: 2, 2 * ROUND + 1: 1}[n], "tiles in the last round"
    if pattern == "sparse":
        assert (tiles > 0).all() and (rounds > 0).all() and 0.02 * n < mask.sum() < 0.04 * n
    elif pattern == "seam":
        seam = [t for t in (SCAN_THREADS - 1, SCAN_THREADS) if t < ntiles]
        assert (tiles[seam] > 0).all() and int(tiles[seam].sum()) == int(mask.sum()), "kept rows in the two tiles at the seam and nowhere else"
        assert len(seam) == (2 if n > ROUND else 1)
    elif pattern == "first_round":
        assert rounds[0] > 1000 and not rounds[1:].any() and tiles[SCAN_THREADS - 1] > 0, "kept rows in round 1 (its last tile too) and in no other"
    elif pattern == "last_round":
        assert rounds[-1] > 0 and not rounds[:-1].any() and mask[n - 1], "kept rows in the last round and in no other"
    else:
        raise KeyError(pattern)


def round_table(mask):
    """a STAT table that RULES['visible'] (min_pixels = 1) keeps exactly where mask says: pixels 1 or 0"""
    st = np.zeros(mask.size, STAT)
    st["pixels"] = mask
    st["wmax"] = BITS_1_255
    st["wsum"] = 1
    return st


def loop_reference(stats, rule, cap_dst, cap_idx, invert=False):
    """the contract as a plain Python loop (small tables): -> (indices written, kept, written)"""
    min_pixels, min_wmax, min_wsum = rule
    out, kept = [], 0
    cap = min([c for c in (cap_dst, cap_idx) if c is not None], default=None)
    for i in range(len(stats)):
        ok = int(stats["pixels"][i]) >= min_pixels and int(stats["wmax"][i]) >= min_wmax and int(stats["wsum"][i]) >= min_wsum
        if ok != bool(invert):
            if cap is None or kept < cap:
                out.append(i)
            kept += 1
    return out, kept, len(out)
