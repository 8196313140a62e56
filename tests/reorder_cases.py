"""gs4d_spatial_order and gs4d_gather_records (include/gs4d.h) restated in numpy, and the tables of their tests.

keys() is the header's definition operation by operation in float32 (numpy rounds each float32 operation to nearest and never contracts, and its
float32 division is correctly rounded: the operations of the device code), order() the stable argsort of the identity by those keys: the device's
order_index must equal it byte for byte."""
import zlib

import numpy as np

import compact_cases as cc

UNPLACED = np.uint32(0x40000000)
SIZES = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 70_001)
STRIDES = cc.STRIDES                                       # (16, 48, 96, 288, 1024)
GATHER_STRIDES = (4, 8) + STRIDES                          # rows of words and of time spans as well
STRIDE_SIZES = (65, 2049, 70_001)
PATTERNS = ("uniform", "identical", "clusters", "sorted", "reversed")
HOSTILE = ("nan", "inf", "big", "zeros", "overflow", "flat1", "flat3", "unplaced_all", "mixed")
F32_MAX = np.float32(3.4028234663852886e38)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def seed(name):
    return zlib.crc32(name.encode())


def spread10(v):
    """10 bits -> every third bit of 30 (uint32)"""
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def placed(pos):
    return np.isfinite(f32(pos)).all(1)


def cells(pos):
    """(n, 3) uint32 cells of the PLACED records of pos (rows of unplaced records: 0), and the placed mask"""
    pos = f32(pos)
    ok = placed(pos)
    cell = np.zeros(pos.shape, np.uint32)
    if ok.any():
        p = pos[ok]
        lo, hi = p.min(0), p.max(0)
        with np.errstate(all="ignore"):
            d, e = p - lo, hi - lo
            g = (d / e) * np.float32(1023.0)
            assert d.dtype == e.dtype == g.dtype == np.float32
            cell[ok] = np.where(g >= 0, np.minimum(g, np.float32(1023.0)), np.float32(0.0)).astype(np.uint32)      # (a NaN fails g >= 0)
    return cell, ok


def keys(pos):
    """the uint32 sort key of every record"""
    cell, ok = cells(pos)
    k = spread10(cell[:, 0]) | (spread10(cell[:, 1]) << np.uint32(1)) | (spread10(cell[:, 2]) << np.uint32(2))
    return np.where(ok, k, UNPLACED).astype(np.uint32)


def order(pos):
    """order_index: the stable ascending sort of the identity by key (uint32)"""
    return np.argsort(keys(pos), kind="stable").astype(np.uint32)


# ---- an independent slow reference: one record at a time, bit by bit ----
def loop_order(pos):
    pos = f32(pos)
    n = pos.shape[0]
    fin = [i for i in range(n) if all(np.isfinite(pos[i, a]) for a in range(3))]
    ks = [int(UNPLACED)] * n
    if fin:
        lo = [min(pos[i, a] for i in fin) for a in range(3)]
        hi = [max(pos[i, a] for i in fin) for a in range(3)]
        for i in fin:
            code = 0
            for a in range(3):
                with np.errstate(all="ignore"):
                    g = np.float32(np.float32(np.float32(pos[i, a] - lo[a]) / np.float32(hi[a] - lo[a])) * np.float32(1023.0))
                c = 0
                if g >= 0:                                  # (False for a NaN)
                    c = 1023 if g >= 1023 else int(g)
                for b in range(10):
                    code |= ((c >> b) & 1) << (3 * b + a)
            ks[i] = code
    return np.array(sorted(range(n), key=lambda i: (ks[i], i)), np.uint32), np.array(ks, np.uint32)


# ---- positions ----
def uniform(n, name="uniform"):
    rng = np.random.default_rng(seed(f"reorder/{name}/{n}"))
    return f32(rng.uniform(-3.0, 5.0, (n, 3)))


def pattern_positions(pattern, n):
    if pattern == "uniform":
        return uniform(n)
    if pattern == "identical":
        return f32(np.tile([[0.25, -1.5, 7.0]], (n, 1)))
    if pattern == "clusters":                               # 8 points, every record on one of them: massive ties
        rng = np.random.default_rng(seed(f"reorder/clusters/{n}"))
        return uniform(8, "centres")[rng.integers(0, 8, n)]
    if pattern in ("sorted", "reversed"):
        p = uniform(n, "presorted")
        p = p[order(p)]
        return f32(p[::-1]) if pattern == "reversed" else p
    raise KeyError(pattern)


def hostile_positions(kind, n):
    """a random set of n positions with rows of the hostile class `kind` mixed in (about one row in five, at least one when n allows)"""
    rng = np.random.default_rng(seed(f"reorder/hostile/{kind}/{n}"))
    p = uniform(n, f"hostile/{kind}")
    if kind == "zeros":
        p = np.abs(p)                                       # the box starts at a zero whose sign depends on which record is looked at first
    at = np.flatnonzero(rng.random(n) < 0.2)
    if at.size == 0:
        at = np.array([n - 1])
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    big, edge = np.float32(1e30), np.float32(3.0e38)
    rows = {
        "nan": [[nan, 0, 0], [0, nan, 0], [0, 0, nan], [nan, nan, nan]],
        "inf": [[inf, 0, 0], [0, -inf, 0], [0, 0, inf], [-inf, inf, nan]],
        "big": [[big, 0, 0], [0, -big, 0], [big, big, -big], [-big, 1, 1]],
        "zeros": [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 1.0], [-0.0, 2.0, 0.0]],
        "overflow": [[edge, 0, 0], [-edge, 0, 0], [0, edge, -edge], [F32_MAX, -F32_MAX, F32_MAX], [-F32_MAX, F32_MAX, -F32_MAX]],
        "mixed": [[nan, 0, 0], [0, inf, 0], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [big, 0, 0], [0, 0, -inf], [-big, -big, big]],
    }
    if kind in rows:
        r = f32(rows[kind])
        p[at] = r[np.arange(at.size) % r.shape[0]]
    elif kind == "flat1":
        p[:, 1] = np.float32(-2.5)                          # one degenerate axis
    elif kind == "flat3":
        p[:] = p[0]                                         # three
        p[at] = f32([nan, 1, 1])                            # ... with unplaced records in between
    elif kind == "unplaced_all":
        p[np.arange(n), rng.integers(0, 3, n)] = f32([nan, inf, -inf])[rng.integers(0, 3, n)]      # one bad coordinate in every record
    else:
        raise KeyError(kind)
    return f32(p)


def positions(name, n):
    return hostile_positions(name[len("hostile/"):], n) if name.startswith("hostile/") else pattern_positions(name, n)


ALL_PATTERNS = PATTERNS + tuple(f"hostile/{k}" for k in HOSTILE)

# ---- past the grid of the box kernel ----
# k_order_box (csrc/reorder.hip) has at most ORDER_BOX_GROUPS workgroups of 256 threads; past ORDER_BOX_GROUPS * 256 records every thread strides.
ORDER_BOX_GROUPS = 1024                                    # gs4d_internal.h
FIRST_TRIP = ORDER_BOX_GROUPS * 256                        # records the grid covers in one trip of the stride loop
STRIDE_SIZE = FIRST_TRIP + 257                             # a second trip for every thread of the first workgroup and one thread of the second
STRIDE_TRIPS = ("second", "first")                         # the trip whose records hold the six extremes of the box


def stride_positions(trip):
    """STRIDE_SIZE positions in [-3, 5]^3 whose six box extremes (-100 or +100 on one axis each) are held by six records of the given trip of
    k_order_box's stride loop alone — "second": records >= FIRST_TRIP, on the first and last lane of a wave, the last thread of the workgroup and
    the one record of the second workgroup; "first": records < FIRST_TRIP.  The second trip also holds three unplaced records and eleven that
    share their position, and so their key, with a record of the first trip."""
    p = uniform(STRIDE_SIZE, "stride")
    at = FIRST_TRIP + np.array([0, 63, 64, 130, 255, 256]) if trip == "second" else np.array([0, 255, 256, 70_001, FIRST_TRIP - 257, FIRST_TRIP - 1])
    for k, i in enumerate(at):
        p[i, k % 3] = np.float32(-100.0 if k < 3 else 100.0)
    p[FIRST_TRIP + 1], p[FIRST_TRIP + 65], p[FIRST_TRIP + 200] = f32([np.nan, 0, 0]), f32([0, np.inf, 0]), f32([1, 1, -np.inf])
    p[FIRST_TRIP + 10:FIRST_TRIP + 21] = p[5]
    return f32(p)


def assert_stride_positions(trip, pos):
    """the property the case is named for (numpy alone): every extreme of the box is reached in the named trip only, and strictly"""
    ok = placed(pos)
    idx = np.flatnonzero(ok)
    here = idx >= FIRST_TRIP if trip == "second" else idx < FIRST_TRIP
    assert pos.shape[0] == STRIDE_SIZE and 0 < (~ok).sum() and (np.flatnonzero(~ok) >= FIRST_TRIP).all()
    for a in range(3):
        v = pos[ok, a]
        assert v[here].min() == -100.0 and v[here].max() == 100.0 and v[~here].min() > -4.0 and v[~here].max() < 6.0, f"axis {a}"


# ---- records ----
def records_with_positions(pos, stride, pos_offset):
    """(n, stride / 4) uint32: cc.records with the position's bits in the three words at pos_offset"""
    rec = cc.records(pos.shape[0], stride)
    w = pos_offset // 4
    rec[:, w:w + 3] = f32(pos).view(np.uint32)
    return rec


def pos_offsets(stride):
    return sorted({0, 4, stride - 12})


def side_table(n):
    """8-byte rows that name their record: (i, ~i)"""
    i = np.arange(n, dtype=np.uint32)
    return np.stack([i, ~i], axis=1)


# ---- gather ----
def gather_reference(index, src, dst):
    """dst (m rows) after the gather: row j <- src[index[j]] where index[j] < nsrc"""
    out = np.array(dst)
    ok = index < src.shape[0]
    out[ok] = src[index[ok]]
    return out


def index_lists(nsrc):
    """name -> uint32 index list over nsrc records"""
    rng = np.random.default_rng(seed(f"reorder/lists/{nsrc}"))
    ident = np.arange(nsrc, dtype=np.uint32)
    wild = rng.integers(0, nsrc, 2 * nsrc + 3).astype(np.uint32)
    bad = np.array(wild)
    bad[rng.random(bad.size) < 0.3] = np.uint32(0xFFFFFFFF)
    bad[rng.random(bad.size) < 0.1] = np.uint32(nsrc)                                     # the first index that does not exist
    bad[rng.random(bad.size) < 0.1] = np.uint32(min(0xFFFFFFFF, nsrc + (1 << 28)))        # * stride: past 2^32 bytes
    bad[0], bad[-1] = np.uint32(0xFFFFFFFF), np.uint32(nsrc)
    return {"identity": ident, "reversed": ident[::-1].copy(), "repeated": np.sort(wild)[: max(1, nsrc // 2)] // np.uint32(3),
            "longer": wild, "shorter": rng.permutation(nsrc)[: max(1, nsrc // 3)].astype(np.uint32), "out_of_range": bad}
