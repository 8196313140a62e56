"""gs4d_edit_colours (include/gs4d.h) restated in numpy, and the records, tables and rules of its tests.

Test infrastructure only (tests/test_edit_host.py pins the restatement on the CPU against a scalar loop of the header's text and against
gs4d_host_edit_colours; tests/test_gpu_edit.py runs the device call against it).  Plain numpy: float32 arrays, one ufunc per operation of the
definition, so every product and every sum is rounded on its own.

Sizes: the kernel gives one workgroup of TILE threads a tile of TILE records, waves of 64 inside it.  SIZES hits the edges of both.
"""
import numpy as np

f32 = np.float32
TILE = 256                                                # EDIT_TILE (csrc/gs4d_internal.h)
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1)
EXTRA = 3                                                 # records behind n that no call may change
SET, MUL, LERP, COPY = 0, 1, 2, 3                         # GS4D_EDIT_*
OPS = {"set": SET, "mul": MUL, "lerp": LERP, "copy": COPY}
MASKS = (1, 8, 7, 15, 10)                                 # r; a; rgb; rgba; g and a
STAT = np.dtype([("pixels", "<u4"), ("wmax", "<u4"), ("wsum", "<u8")])       # wmax as its bit pattern: the rule compares bit patterns
VALUE, AMOUNT = (0.25, 1.5, -0.75, 0.375), 0.3125
WSUM_MIN = (1 << 32) + 12345                              # a threshold above 2^32: the compare must be a 64-bit one
INF_BITS = 0x7F800000


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want):
    """equal as bit patterns, a word that is a NaN on both sides counting as equal (gs4d.h: the sign and payload of a NaN that MUL or LERP
    makes are not fixed)"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


# ---- records ---------------------------------------------------------------------------------------------------------------------------------------
def records(n, seed=0x4544):
    """n 96-byte records [n, 24]: every word a function of (seed, record, word) and a float in [0.5, 1), so that a word that moves shows; the
    colours (floats 4..7) spread over [-1, 3)"""
    w = np.arange(n * 24, dtype=np.uint64).reshape(n, 24) + np.uint64(seed) * np.uint64(7919)
    word = ((w * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rec = ((word >> np.uint32(9)) | np.uint32(0x3F000000)).view(f32).copy()
    rec[:, 4:8] = (rec[:, 4:8] - f32(0.5)) * f32(8.0) - f32(1.0)
    return rec


HOSTILE = (np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, 1e-40, -1e-40, 1e-45, 0.0, -0.0)


def hostile_records(n, seed=0x4545):
    """records whose colours run through HOSTILE (NaN, +-Inf, huge, denormal, signed zeros) between ordinary ones"""
    rec = records(n, seed)
    col = rec[:, 4:8].reshape(-1)                               # (a copy: the slice is not contiguous)
    idx = np.arange(0, col.size, 3)
    col[idx] = np.array(HOSTILE, f32)[np.arange(idx.size) % len(HOSTILE)]
    rec[:, 4:8] = col.reshape(n, 4)
    return rec


def hostile_operands():
    """(value, amount) pairs: every HOSTILE number as an operand on some channel, and as the amount"""
    h = HOSTILE
    out = [((h[k % len(h)], h[(k + 3) % len(h)], h[(k + 5) % len(h)], h[(k + 7) % len(h)]), AMOUNT) for k in range(len(h))]
    out += [(VALUE, a) for a in h]
    out += [((np.nan, np.inf, 1e30, 1e-40), np.inf), ((3e38, -3e38, 3e38, -3e38), 3e38)]
    return out


# ---- the selection -----------------------------------------------------------------------------------------------------------------------------------
def selected(n, stats=None, rule=(1, 0, 0), invert=False):
    """which of the n records are selected: all of them without a table, else the predicate of gs4d_compact_records on row i"""
    if stats is None:
        return np.ones(n, bool)
    min_pixels, min_wmax, min_wsum = rule
    st = stats[:n]
    k = (st["pixels"] >= np.uint32(min_pixels)) & (st["wmax"] >= np.uint32(min_wmax)) & (st["wsum"] >= np.uint64(min_wsum))
    return k != bool(invert)


def rule_keywords(rule, invert=False):
    """a (min_pixels, min_wmax bit pattern, min_wsum) rule as the keywords of Context.edit_colours / compact_records (min_wmax is a weight there)"""
    return dict(min_pixels=int(rule[0]), min_wmax=float(np.array([rule[1]], np.uint32).view(f32)[0]), min_wsum=int(rule[2]), invert=bool(invert))


def mask_table(mask, rule=(1, 0, 0)):
    """a STAT table whose row i passes `rule` iff mask[i]: a failing row misses exactly one field that has a threshold, by one unit"""
    n = len(mask)
    st = np.zeros(n, STAT)
    st["pixels"] = rule[0] + (np.arange(n) % 3)
    st["wmax"] = rule[1] + (np.arange(n) % 2)
    st["wsum"] = np.uint64(rule[2]) + (np.arange(n) % 5).astype(np.uint64)
    fields = [f for f, t in zip(("pixels", "wmax", "wsum"), rule) if t > 0]
    assert fields or mask.all(), "a rule without a threshold selects everything"
    for k, f in enumerate(fields):
        drop = ~mask & (np.arange(n) % len(fields) == k)
        st[f][drop] = dict(zip(("pixels", "wmax", "wsum"), rule))[f] - 1
    return st


def tables(n):
    """name -> (STAT table of n rows, rule, invert): all, none, every other record, one record in the last tile only, and the inverted forms"""
    all_, none, alt, one = np.ones(n, bool), np.zeros(n, bool), np.arange(n) % 2 == 0, np.zeros(n, bool)
    one[n - 1 - (n - 1) % TILE // 2] = True                    # in the middle of the last tile's records
    wide = (5, 0x3B808081, WSUM_MIN)                           # every field has a threshold (wmax: the bits of 1/255)
    out = {}
    for name, m, rule in (("all", all_, (1, 0, 0)), ("none", none, (1, 0, 0)), ("alternating", alt, wide), ("one_in_the_last_tile", one, (1, 0, 0))):
        st = mask_table(m, rule)
        assert np.array_equal(selected(n, st, rule), m)
        out[name] = (st, rule, False)
        out[name + "_inverted"] = (st, rule, True)
    return out


def edge_table(n):
    """rows that straddle each threshold of EDGE_RULE separately: pixels around its minimum, wmax bit patterns at 0, around the threshold and at
    0x7F800000 (+inf), wsum around a threshold above 2^32 — below it by one, by 2^32 (equal low words), a low word above with a high word below"""
    px = [EDGE_RULE[0] - 1, EDGE_RULE[0], EDGE_RULE[0] + 1]
    wm = [0, EDGE_RULE[1] - 1, EDGE_RULE[1], EDGE_RULE[1] + 1, INF_BITS]
    ws = [0, WSUM_MIN - 1, WSUM_MIN, WSUM_MIN + 1, WSUM_MIN - (1 << 32), 0xFFFFFFFF, (1 << 40) + 1]
    rows = [(p, w, s) for p in px for w in wm for s in ws]
    st = np.zeros(len(rows), STAT)
    st["pixels"], st["wmax"], st["wsum"] = [r[0] for r in rows], [r[1] for r in rows], np.array([r[2] for r in rows], np.uint64)
    return np.resize(st, n)


EDGE_RULE = (5, 0x3B808081, WSUM_MIN)
EDGE_RULES = (EDGE_RULE, (0, 0, 0), (1, 0, 0), (0, INF_BITS, 0), (0, 0, 1 << 40), (0, 0, 0xFFFFFFFF))


# ---- the edit ----------------------------------------------------------------------------------------------------------------------------------------
def edit(rec, op, channels, value=VALUE, amount=AMOUNT, stats=None, rule=(1, 0, 0), invert=False, from_=None, n=None):
    """a copy of rec [total, 24] with the first n records (default: all) edited as gs4d.h defines: float32, one rounding per operation"""
    out = np.array(rec, f32, copy=True)
    n = out.shape[0] if n is None else n
    op = OPS.get(op, op)
    sel = selected(n, stats, rule, invert)
    v, a = np.array(value, f32), f32(amount)
    with np.errstate(all="ignore"):
        for ch in range(4):
            if not (channels >> ch) & 1:
                continue
            c = out[:n, 4 + ch]
            if op == SET:
                new = np.full(n, v[ch], f32)
            elif op == MUL:
                new = c * v[ch]
            elif op == LERP:
                d = v[ch] - c
                step = a * d
                new = c + step
            else:
                new = np.ascontiguousarray(from_, f32)[:n, 4 + ch]
            # (np.where on the bit patterns: a copy of a signalling NaN keeps its bits)
            out[:n, 4 + ch] = np.where(sel, bits(new), bits(c)).view(f32)
    return out
