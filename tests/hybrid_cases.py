"""The decision points of the depth sort's MSD/LSD hybrid (csrc/sort.hip: k_os_pass<512, 12, true, 9> on the 9-bit top digit, then k_os_tail, one
workgroup per bucket) and the record sets that visit each of them.

Test infrastructure only (tests/test_hybrid_cases_host.py pins this table on the CPU; tests/test_gpu_sort_hybrid.py and
tests/test_gpu_sort_hybrid_edges.py run it).  Plain numpy; the bar is sort_cases.reference: numpy's stable argsort.

The hybrid is planned from the key span the host proves from the records' bounding box, so every case is a record set: record i lies on the x axis
at distance 1 / key_i from a camera at the origin, and two records BEHIND the n keyed ones pin the box — hence bias and span — to the case's range
whatever the keyed keys are (the box covers the whole buffer).  1 / (1 / k) is not k to the last bit: the key a record yields is within one bit
pattern of its target, so targets keep 8 patterns away from every boundary that matters (the ends of the span, the ends of a top digit), and what
the tests sort and expect is always what oracle.keygen computes from the records.

What k_os_tail decides on, restated by edges(bits): a proven span of `bits` bits (19..27) leaves rem = bits - 9 bits below the top digit, sorted as
two local digits of w0 = (rem + 1) >> 1 and w1 = rem >> 1 bits; k_os_tail<256> runs while rem <= 16 (both digits <= 8 bits), k_os_tail<512> above.
A bucket of at most `cap` keys (8192 = OT_TILE, or GS4D_SORT_TAILCAP) is sorted in LDS, wave w looking after whole rows of 64 keys
(ot_wave_range); a larger one goes through global memory in chunks of 8192.
"""
import numpy as np

CAM0 = (0.0, 0.0, 0.0)
KEY_LO = int(np.float32(0.26).view(np.uint32))              # the smallest key of every case: the bias
TOP_BITS = 9                                                # the top digit: 512 buckets
TAIL_TILE = 8192                                            # k_os_tail's LDS tile (OT_TILE)
TOP_TILE = 512 * 12                                         # the tile of the top pass, k_os_pass<512, 12, true, 9>
MARGIN = 8                                                  # target keys stay this far inside whatever they must not cross
WIDTHS = tuple(range(19, 28))                               # the spans the hybrid is planned for


# ---- record sets (moved here from test_gpu_sort_hybrid.py, unchanged) --------------------------------------------------------------------------------
def _records(gs4d, key_bits, span):
    """records whose keys are (about) the float bit patterns key_bits, then the two records that pin the box to [KEY_LO, KEY_LO + span]"""
    bits = np.concatenate([np.asarray(key_bits, np.uint32), np.array([KEY_LO, KEY_LO + span], np.uint32)])
    d = (np.float32(1.0) / bits.view(np.float32)).astype(np.float32)
    m = d.size
    pos4 = np.zeros((m, 4), np.float32)
    pos4[:, 0] = d
    q = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (m, 1))
    one3 = np.ones((m, 3), np.float32)
    return gs4d.build_records_4d(pos4, q, one3, np.ones(m, np.float32), np.full(m, 0.5, np.float32), np.zeros((m, 3), np.float32), np.ones((m, 4), np.float32))


def _proven(gs4d, rec):
    """(bias, key bits) the library proves for the buffer: the box of its x positions (everything else is zero)"""
    lo7, hi7 = np.zeros(7, np.float32), np.zeros(7, np.float32)
    lo7[0], hi7[0] = rec[:, 0].min(), rec[:, 0].max()
    bias, span = gs4d.key_bounds(lo7, hi7, 0.0, CAM0)
    return bias, max(1, int(span).bit_length())


def _uniform(n, span, seed):
    rng = np.random.default_rng(seed)
    return (KEY_LO + 8 + rng.integers(0, span - 16, n, dtype=np.int64)).astype(np.uint32)      # (a few patterns inside the box: 1 / (1 / k) is not k to the last bit)


def _crowded(n, share, seed):
    """`share` of the keys inside top digit 200 of a 24-bit span, the rest uniform"""
    keys = _uniform(n, (1 << 24) - (1 << 19), seed)
    rng = np.random.default_rng(seed + 1)
    m = int(n * share)
    where = rng.choice(n, m, replace=False)
    keys[where] = (KEY_LO + (200 << 15) + (1 << 13) + rng.integers(0, 1 << 14, m, dtype=np.int64)).astype(np.uint32)
    return keys, m


# ---- the widths --------------------------------------------------------------------------------------------------------------------------------------
def span_for(bits):
    """a span that proves exactly `bits` key bits, with its last top digit (511) reachable"""
    return (1 << bits) - 64


def edges(bits):
    """(rem, w0, w1, LB): the bits below the top digit, the two local digits of k_os_tail, and which instantiation radix_sort_pairs launches
    (`plan.top <= 16`)"""
    rem = bits - TOP_BITS
    return rem, (rem + 1) >> 1, rem >> 1, 256 if rem <= 16 else 512


def top_digit(keys, bias, bits):
    return (np.asarray(keys, np.uint32) - np.uint32(bias)) >> np.uint32(bits - TOP_BITS)


# ---- bucket profiles ---------------------------------------------------------------------------------------------------------------------------------
# Bucket sizes either side of: a lane, a wave's row of 64, one row per wave (512 = 8 waves x 64: ot_wave_range's share goes from 64 to 128 and
# the last waves start past the end), the LDS tile with every lane and item valid; on the slow path a second chunk of one key and two full chunks.
FIT_SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 4096, 8191, 8192]
SLOW_SIZES = FIT_SIZES + [8193, 16384]
# Top digits: the first and the last thread of a wave of digit_excl_scan<512, 512>, neighbours (a bucket's range ends where the next starts), and
# 511, whose range ends at n.
DIGITS = [0, 1, 2, 3, 100, 101, 102, 255, 256, 257, 509, 510, 511]


def digits_for(sizes):
    """DIGITS cut to the size list, keeping its ends: the smallest size sits in digit 0 and the largest in digit 511 (the fit list's 8192, the slow
    list's 16384 with 8193 in 510)"""
    assert 2 <= len(sizes) <= len(DIGITS)
    return DIGITS[:len(sizes) - 1] + DIGITS[-1:]


def profile(bits, sizes, digits, seed):
    """target keys with exactly sizes[i] keys in top digit digits[i] of a span_for(bits) span above KEY_LO, in random order.  Low bits uniform in
    [8, 2^rem - 8) — in digit 511 [8, 2^rem - 80): the pin record sits at KEY_LO + span, 64 below the digit's end; in every bucket of at least 64
    keys the two extreme low values are held twice each (ties at both ends of the bucket's range)."""
    rem = bits - TOP_BITS
    assert len(sizes) == len(digits) == len(set(digits)) and all(0 <= d < 512 for d in digits)
    rng = np.random.default_rng(seed)
    parts = []
    for size, d in zip(sizes, digits):
        hi = (1 << rem) - (64 + 2 * MARGIN if d == 511 else MARGIN)
        low = rng.integers(MARGIN, hi, size, dtype=np.int64)
        if size >= 64:
            low[0:2], low[2:4] = MARGIN, hi - 1
        parts.append(KEY_LO + (d << rem) + low)
    keys = np.concatenate(parts)
    assert int(keys.max()) <= KEY_LO + span_for(bits) - MARGIN
    return rng.permutation(keys).astype(np.uint32)


def profile_counts(sizes, digits):
    c = np.zeros(512, np.int64)
    c[list(digits)] = sizes
    return c


def fit_profile(bits):
    return profile(bits, FIT_SIZES, digits_for(FIT_SIZES), 1000 + bits)


def slow_profile(bits):
    return profile(bits, SLOW_SIZES, digits_for(SLOW_SIZES), 2000 + bits)


def payload(n, seed):
    """a payload that does not follow the index: a random permutation of arange(n)"""
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


# ---- a bucket that only one local digit orders -------------------------------------------------------------------------------------------------------
ONE_DIGIT_BUCKET = 3 * TAIL_TILE + 5                        # three full chunks of the slow path and one of 5 keys
ONE_DIGIT_TOP = 300


def record_keys(gs4d, oracle, targets, span):
    """the keys the records built for `targets` yield (oracle.keygen), as bit patterns"""
    rec = _records(gs4d, targets, span)
    _, ek = oracle.keygen(rec[:len(targets)], 0.0, np.array(CAM0, np.float32))
    return ek.view(np.uint32)


def one_digit_values(gs4d, oracle, bits, seed):
    """six target keys of top digit ONE_DIGIT_TOP whose record keys are: a, and two more that differ from a in bits [0, w0) alone, and three that
    share one value of bits [0, w0) and differ in bits [w0, rem) alone.  Chosen from the keys a pool of records really yields, since a record's
    key is its target only to the last bit."""
    rem, w0, w1, _ = edges(bits)
    rng = np.random.default_rng(seed)
    pool = np.unique(KEY_LO + (ONE_DIGIT_TOP << rem) + rng.integers(MARGIN, (1 << rem) - MARGIN, 8192, dtype=np.int64)).astype(np.uint32)
    got = record_keys(gs4d, oracle, pool, span_for(bits))
    low = (got - np.uint32(KEY_LO)) & np.uint32((1 << rem) - 1)
    d0, d1 = low & np.uint32((1 << w0) - 1), low >> np.uint32(w0)
    assert (top_digit(got, KEY_LO, bits) == ONE_DIGIT_TOP).all()
    taken = np.zeros(pool.size, bool)

    def pick(same, other):
        """three keys not taken yet with one value of `same` and three values of `other`"""
        for v in np.unique(same):
            idx = np.flatnonzero((same == v) & ~taken)
            _, first = np.unique(other[idx], return_index=True)
            if first.size >= 3:
                taken[idx[first[:3]]] = True
                return pool[idx[first[:3]]]
        raise AssertionError("the pool holds no such three keys")

    return np.concatenate([pick(d1, d0), pick(d0, d1)]).astype(np.uint32)


def one_digit_case(gs4d, oracle, bits, n_rest, seed):
    """target keys: ONE_DIGIT_BUCKET keys drawn from one_digit_values in top digit ONE_DIGIT_TOP, and n_rest uniform keys in the other digits"""
    rem = bits - TOP_BITS
    rng = np.random.default_rng(seed)
    six = one_digit_values(gs4d, oracle, bits, seed + 1)
    rest = _uniform(n_rest, span_for(bits), seed + 2)
    inside = top_digit(rest, KEY_LO, bits) == ONE_DIGIT_TOP
    rest[inside] += np.uint32(1 << rem)                     # (the next digit: the crowded bucket holds the six values and nothing else)
    keys = np.concatenate([six[rng.integers(0, 6, ONE_DIGIT_BUCKET)], rest])
    return rng.permutation(keys).astype(np.uint32), six


# ---- the top pass past its look-back edges -----------------------------------------------------------------------------------------------------------
# tiles of the top pass: 17 (a second group: the first tiles add to their group's accumulator), 257 (a second super-group: group totals are handed
# up), 273 (a second group in the last super-group), 549 (more tiles than any device holds workgroups of this form: sort_cases.resident_bound(6, 9)
# + 37, the persistent loop).  The largest comes first and again last; the last tile holds 1 key or TOP_TILE - 3 in turn, as
# sort_cases.edge_tile_counts does.
LOOKBACK_TILES = [549, 17, 257, 273, 549]
LOOKBACK_N = 548 * TOP_TILE + 1


def lookback_sizes():
    """[(tiles, n)] in the order they are sorted"""
    out = [(t, (t - 1) * TOP_TILE + (1 if i % 2 == 0 else TOP_TILE - 3)) for i, t in enumerate(LOOKBACK_TILES)]
    assert all(-(-n // TOP_TILE) == t and n <= LOOKBACK_N for t, n in out) and out[0][1] == LOOKBACK_N
    return out


def descending(n, bits=24, step=10):
    """strictly descending targets `step` apart (more than the two bit patterns a pair of record keys can move): a tile of the top pass is one or
    two top digits, every tile word of a digit as large as it can be"""
    keys = KEY_LO + MARGIN + step * np.arange(n - 1, -1, -1, dtype=np.int64)
    assert int(keys[0]) <= KEY_LO + span_for(bits) - 64 - 2 * MARGIN
    return keys.astype(np.uint32)


def describe_mismatch(what, got, want, keys, bias, bits, cap=TAIL_TILE):
    """where a hybrid sort went wrong, in the kernel's terms: the first bad output slot, the bucket (top digit) it lies in with that bucket's range,
    size and path, and (w0, w1, LB)"""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    p = int(bad[0])
    counts = np.bincount(top_digit(keys, bias, bits), minlength=512)
    ends = np.cumsum(counts)
    d = int(np.searchsorted(ends, p, side="right"))
    start = int(ends[d] - counts[d])
    rem, w0, w1, lb = edges(bits)
    return (f"{what} differ: {bad.size} of {len(want)} slots, the first at {p}: got {int(got[p]):#x}, want {int(want[p]):#x}; bucket {d} = slots "
            f"[{start}, {int(ends[d])}), {int(counts[d])} keys ({'LDS' if counts[d] <= cap else 'slow'} path, slot {p - start} of it, chunk "
            f"{(p - start) // TAIL_TILE}); {bits} bits: rem = {rem}, (w0, w1, LB) = ({w0}, {w1}, {lb})")
