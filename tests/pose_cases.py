"""Inputs for the gs4d_pose_records tests (include/gs4d.h): tables of gs4d_affine4 rows, bind tables of both forms, and the definition
restated as a numpy float32 loop of the header's text.

sets      those of tests/transform_cases.py: clean 3D, 4D_VEL and 4D_2Q sets and the hostile block.
tables    m rows taken round and round from transform_cases.NAMES (NaN, Inf and 1e30 rows included); the rows past the first round are shifted in o[0]
          so that no two rows of a table are equal, and every "zero" row has an L of -0 elements (its o holds a -0 too).
bind      INDEX: every j < m, then j == m, j == m + 1 and GS4D_ID_NONE, then a random mix of all of them.
          BLEND4: row i has the slots of the bits of i % 16 taking part (0, 1, 2, 3 and 4 slots, in every position), the others holding m, m + 1 or
          GS4D_ID_NONE under a weight that must not matter (NaN, Inf, 1, 0); the weights of the slots that take part go through seven kinds: 0, 1,
          -0, normalised, unnormalised, one NaN, one Inf.  Rows 16 q + (1, 2, 4, 8) of kind 1 are weight-1 single slots; some of them fall on a "zero"
          row once m > 7.
"""
import functools

import numpy as np

import transform_cases as tc

f32 = np.float32
u32 = np.uint32
ID_NONE = 0xFFFFFFFF
INDEX, BLEND4 = 0, 1                                          # GS4D_POSE_INDEX, GS4D_POSE_BLEND4
FORMS = {"index": INDEX, "blend4": BLEND4}
SIZES = tc.SIZES                                             # one record, either side of a tile of 256, three tiles plus one
SETS = tc.SETS
TILE, LDS_ROWS = 256, 128                                    # POSE_TILE, POSE_LDS_ROWS (csrc/gs4d_internal.h)
# no table, one row, a few; the capacity of the workgroup's LDS copy and one past it (the rows then come from global memory)
TABLE_SIZES = (0, 1, 3, LDS_ROWS, LDS_ROWS + 1)
# seven tiles, the last a short one.  The shipped kernel gives every workgroup one tile; in the POSE_WALK=4 build of the Makefile two workgroups take
# four and three of these
WALK_N = 6 * TILE + 1
STRIDES = {INDEX: (4, 12), BLEND4: (32, 48)}
KINDS = ("zero", "one", "negative zero", "normalised", "unnormalised", "nan", "inf")
bits, same_bits = tc.bits, tc.same_bits


# ---- tables --------------------------------------------------------------------------------------------------------------------------------------
def xf_table(m, call=0):
    """[m, 20] float32: row k is transform NAMES[(3 call + k) % 11]"""
    rows = np.zeros((m, 20), f32)
    for k in range(m):
        name = tc.NAMES[(3 * call + k) % len(tc.NAMES)]
        r = tc.transforms()[name].copy()
        if name == "zero":
            r[:16] = f32(-0.0)
        r[16] += f32(k // len(tc.NAMES))
        rows[k] = r
    return rows


def outside(rng, n, m):
    """n words that name no row of a table of m"""
    return np.array([m, m + 1, ID_NONE], np.uint64)[rng.integers(3, size=n)].astype(u32)


def index_bind(n, m, seed=1):
    """uint32 [n]"""
    rng = np.random.default_rng([0x504F, n, m, seed])
    values = np.array(list(range(m)) + [m, m + 1, ID_NONE], np.uint64).astype(u32)
    j = values[rng.integers(values.size, size=n)]
    k = min(n, values.size)
    j[:k] = values[(np.arange(k) + seed) % values.size] if n < values.size else values
    return np.ascontiguousarray(j)


def blend_bind(n, m, seed=1):
    """(joints uint32 [n, 4], weights float32 [n, 4])"""
    rng = np.random.default_rng([0x5042, n, m, seed])
    i = np.arange(n) + seed
    part = ((i[:, None] >> np.arange(4)[None, :]) & 1).astype(bool) & (m > 0)
    j = np.where(part, rng.integers(max(m, 1), size=(n, 4)).astype(u32), outside(rng, 4 * n, m).reshape(n, 4)).astype(u32)
    kind = (i // 16) % len(KINDS)
    w = rng.uniform(-2.0, 2.0, (n, 4)).astype(f32)                                        # unnormalised
    w[kind == 0], w[kind == 1], w[kind == 2] = f32(0.0), f32(1.0), f32(-0.0)
    norm = np.abs(w) + f32(0.05)
    norm = (norm / np.where(part, norm, 0).sum(1, keepdims=True).clip(1e-3)).astype(f32)
    w[kind == 3] = norm[kind == 3]
    slot = rng.integers(4, size=n)
    w[kind == 5, slot[kind == 5]] = f32(np.nan)
    w[kind == 6, slot[kind == 6]] = f32(np.inf) * np.where(rng.integers(2, size=int((kind == 6).sum())), f32(1), f32(-1))
    # a slot that takes no part: its weight must not matter
    junk = np.array([np.nan, np.inf, 1.0, 0.0], f32)[rng.integers(4, size=(n, 4))]
    w = np.where(part, w, junk).astype(f32)
    return np.ascontiguousarray(j), np.ascontiguousarray(w)


def packed(words, stride, fill=0xC3):
    """rows of `words` (uint32 [n] or [n, k]) at a pitch of `stride` bytes, the padding filled: uint8 [n * stride]"""
    w = np.ascontiguousarray(words, u32).reshape(len(words), -1)
    out = np.full((w.shape[0], stride), fill, np.uint8)
    out[:, :4 * w.shape[1]] = w.view(np.uint8)
    return out.reshape(-1)


def bind_bytes(gs4d, form, n, m, stride, seed=1):
    """the bind table of a call as uint8 [n * stride]"""
    if form == INDEX:
        return packed(index_bind(n, m, seed), stride)
    return packed(gs4d.bind_rows(*blend_bind(n, m, seed)), stride)


def unpacked(table, form, n, stride):
    """(joints [n, 1 or 4], weights [n, 4] or None) read back from the bytes"""
    rows = np.ascontiguousarray(table, np.uint8).reshape(-1)[:n * stride].reshape(n, stride)
    if form == INDEX:
        return np.ascontiguousarray(rows[:, :4]).view(u32), None
    return np.ascontiguousarray(rows[:, :16]).view(u32), np.ascontiguousarray(rows[:, 16:32]).view(f32)


# ---- the definition, restated -------------------------------------------------------------------------------------------------------------------
def record_by_the_text(rec, a):
    """the four lines of gs4d_transform_records' definition with a row of its own per record: rec [n, 24], a [n, 20]"""
    l, o = [a[:, e] for e in range(16)], [a[:, 16 + e] for e in range(4)]
    out = np.empty_like(rec)
    p = [rec[:, k] for k in range(4)]
    for r in range(4):
        out[:, r] = ((((l[r] * p[0]) + (l[4 + r] * p[1])) + (l[8 + r] * p[2])) + (l[12 + r] * p[3])) + o[r]
    out[:, 4:8] = rec[:, 4:8]
    S = [[rec[:, 8 + 4 * c + k] for k in range(4)] for c in range(4)]
    T = [[(((l[r] * S[c][0]) + (l[4 + r] * S[c][1])) + (l[8 + r] * S[c][2])) + (l[12 + r] * S[c][3]) for r in range(4)] for c in range(4)]
    for c in range(4):
        for r in range(4):
            out[:, 8 + 4 * c + r] = (((T[0][r] * l[c]) + (T[1][r] * l[4 + c])) + (T[2][r] * l[8 + c])) + (T[3][r] * l[12 + c])
    return out


def by_the_text(rec, xf, table, form, stride):
    """the header's text in numpy float32, one operation at a time (numpy rounds every product and every sum on its own).  Returns (out [n, 24],
    transformed bool [n]): the records that are not transformed are copies, byte for byte"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    xf = np.ascontiguousarray(xf, f32).reshape(-1, 20)
    n, m = rec.shape[0], xf.shape[0]
    j, w = unpacked(table, form, n, stride)
    rows = np.concatenate([xf, np.zeros((1, 20), f32)])                                   # (row m: never used where it matters)
    part = j < m
    pick = np.where(part, j, m)
    with np.errstate(all="ignore"):
        if form == INDEX:
            a, moved = rows[pick[:, 0]], part[:, 0]
        else:
            a, moved = np.zeros((n, 20), f32), np.zeros(n, bool)
            for k in range(4):
                prod = w[:, k, None] * rows[pick[:, k]]
                first, later = part[:, k] & ~moved, part[:, k] & moved
                a = np.where(first[:, None], prod, np.where(later[:, None], a + prod, a))
                moved = moved | part[:, k]
        assert a.dtype == f32
        out = record_by_the_text(rec, a)
    assert out.dtype == f32
    out.view(u32)[~moved] = rec.view(u32)[~moved]
    return out, moved


def expected(gs4d, rec, xf, table, form, stride):
    """what a call writes, from the host definition: [n, 24]"""
    return gs4d.pose_records_host(rec, xf, table, form, stride)


def assert_records(got, want, rec, moved, what):
    """the rule of gs4d.h: a transformed record equal as uint32 but for NaN = NaN, a copied record byte-equal"""
    got, want = np.ascontiguousarray(got, f32).reshape(-1, 24), np.ascontiguousarray(want, f32).reshape(-1, 24)
    ok = same_bits(got, want)
    assert ok.all(), f"{what}: {int((~ok).any(1).sum())} of {got.shape[0]} records differ, first word at {np.argwhere(~ok)[0].tolist()}"
    assert np.array_equal(got.view(u32)[~moved], np.ascontiguousarray(rec, f32).reshape(-1, 24).view(u32)[~moved]), f"{what}: a copied record is not byte-equal"


# ---- the weight-1 property ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight_one_table(names=tc.NAMES):
    """every transform, and every transform again with each +0 of its L turned into -0"""
    rows = tc.rows(names)
    neg = rows.copy()
    z = neg[:, :16].view(u32) == 0
    neg[:, :16].view(u32)[z] = 0x80000000
    out = np.concatenate([rows, neg])
    out.setflags(write=False)
    return out


def weight_one_binds(gs4d, n, m):
    """(index uint32 [n], bind_rows [n, 8]): row i names row i % m; the BLEND4 row holds it in slot i % 4 under weight 1.0f, the other slots outside
    the table under weights that must not matter"""
    rng = np.random.default_rng([0x5031, n, m])
    idx = (np.arange(n) % m).astype(u32)
    j = outside(rng, 4 * n, m).reshape(n, 4)
    w = np.array([np.nan, np.inf, 0.5, 0.0], f32)[rng.integers(4, size=(n, 4))]
    j[np.arange(n), np.arange(n) % 4] = idx
    w[np.arange(n), np.arange(n) % 4] = f32(1.0)
    return idx, gs4d.bind_rows(j, w)
