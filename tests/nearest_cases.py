"""gs4d_nearest_neighbours (include/gs4d.h) restated in numpy, and the parameter matrix of its tests.

Test infrastructure only (tests/test_nearest_host.py pins gs4d_host_nearest_neighbours to the restatement on the CPU; tests/test_gpu_nearest.py runs
the device call against the host definition).  The record sets, radii, sources and tables are neighbour_cases'.  Plain numpy: who takes part is
neighbour_cases.takes_part, the selection edit_cases.selected; dist2 is an n x n float32 matrix, one ufunc per operation of the definition in the
order of its parentheses, so every product and every sum is rounded on its own; the order is a stable argsort of bits(dist2) along j — equal
distances keep ascending j, which is np.lexsort((j, bits(dist2))) by another name (the host test asserts that the two agree) and a radix sort
instead of a comparison sort, which is what makes n = 4097 affordable.
"""
import functools
import importlib

import numpy as np

import edit_cases as ec
import neighbour_cases as nc

f32 = np.float32
HIT = np.dtype([("record", "<u4"), ("dist2", "<u4")])      # dist2 as its bit pattern: rows are compared as bytes
SKIP_HIDDEN, SKIP_DEAD, INCLUDE_SELF = 1, 2, 4            # GS4D_NN_*
KS = (1, 3, 4, 5, 8, 9, 16)                               # the smallest, an inner and the largest k of each kernel instantiation (K = 4, 8, 16)
K_MAX = 16
ID_NONE, INF_BITS = 0xFFFFFFFF, 0x7F800000
NOT_A_CANDIDATE = np.uint32(0xFFFFFFFF)                   # above the bits of every dist2 >= +0, +inf included
SENTINEL = 0xA5
STAT = nc.STAT
COMBOS = 56                                               # 3 forms, 7 values of k and 8 flag values are pairwise coprime: 56 consecutive combinations hold every k 8 times, every flag value 7 times
BIG_COMBOS = 4                                            # at n = 4097


def _gs4d():
    return importlib.import_module("4dgaussiansplatrendering_amd")


def stride_for(k):
    return 16 * ((8 * k + 15) // 16)


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------------
def dist2_bits(m):
    """[n, n] uint32: the bits of ((d.x * d.x) + (d.y * d.y)) + (d.z * d.z), d = m_i - m_j per component, in float32"""
    m = np.ascontiguousarray(m, f32)
    with np.errstate(all="ignore"):
        d = m[:, None, 0] - m[None, :, 0]
        s = d * d
        d = m[:, None, 1] - m[None, :, 1]
        s = s + (d * d)
        d = m[:, None, 2] - m[None, :, 2]
        s = s + (d * d)
    return s.view(np.uint32)


@functools.lru_cache(maxsize=2)
def case_dist2(case):
    """the dist2 matrix of a neighbour_cases.Case (it does not depend on the flags, k or the source); only the latest two are kept"""
    return dist2_bits(nc.takes_part(case.rec, case.t, 0)[1])


def candidates(rec, t, r, flags, source=None, rule=nc.RULE, invert=False, d2=None):
    """(bits [n, n] uint32: bits(dist2) where j is a candidate of i, NOT_A_CANDIDATE elsewhere; part [n])"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    n = rec.shape[0]
    part, m = nc.takes_part(rec, t, flags & (SKIP_HIDDEN | SKIP_DEAD))
    if d2 is None:
        d2 = dist2_bits(m)
    src = part & ec.selected(n, source, rule, invert)
    rr = f32(r) * f32(r)
    with np.errstate(all="ignore"):
        cand = (d2.view(f32) <= rr) & part[:, None] & src[None, :]                       # (a NaN is not near)
    if not flags & INCLUDE_SELF:
        cand[np.arange(n), np.arange(n)] = False
    return np.where(cand, d2, NOT_A_CANDIDATE), part


def ordered(bits):
    """(j [n, 16], bits [n, 16]) of the first 16 of every row by (bits(dist2), j) ascending, NOT_A_CANDIDATE behind the candidates"""
    n = bits.shape[0]
    if bits.shape[1] < K_MAX:
        bits = np.concatenate([bits, np.full((n, K_MAX - bits.shape[1]), NOT_A_CANDIDATE, np.uint32)], 1)
    order = np.argsort(bits, axis=1, kind="stable")[:, :K_MAX]
    return order, np.take_along_axis(bits, order, 1)


def restate(rec, t, r, k, flags, hits, table=None, source=None, rule=nc.RULE, invert=False, d2=None):
    """(the hit table after the call: a copy of `hits`, uint8 [n, hit_stride], with the first 8 k bytes of every row written; the table after the
    call: a copy of `table` (STAT) with the rows of f >= 1 updated, or None without one; f [n]; the number of candidates [n])"""
    bits, part = candidates(rec, t, r, flags, source, rule, invert, d2)
    n = bits.shape[0]
    j, b = ordered(bits)
    j, b = j[:, :k], b[:, :k]
    filled = b != NOT_A_CANDIDATE
    slots = np.zeros((n, k), HIT)
    slots["record"] = np.where(filled, j, ID_NONE)
    slots["dist2"] = np.where(filled, b, INF_BITS)
    out = np.array(hits, np.uint8, copy=True).reshape(n, -1)
    out[:, :8 * k] = slots.view(np.uint8).reshape(n, 8 * k)
    f = filled.sum(1)
    st = None
    if table is not None:
        st = np.array(table, STAT, copy=True)
        rows = np.flatnonzero(f >= 1)
        add = f[rows].astype(np.uint64)
        last = b[rows, f[rows] - 1]
        st["pixels"][rows] = (st["pixels"][rows].astype(np.uint64) + add).astype(np.uint32)
        st["wmax"][rows] = np.maximum(st["wmax"][rows], last)
        st["wsum"][rows] = st["wsum"][rows] + (add << np.uint64(24))
    return out, st, f, (bits != NOT_A_CANDIDATE).sum(1)


def struct(t, r, k, flags):
    """the query as the binding's NearestQuery"""
    q = _gs4d().NearestQuery()
    q.t, q.radius, q.k, q.flags = float(f32(t)), float(f32(r)), int(k), int(flags)
    return q


def host(rec, t, r, k, flags, hits, table=None, source=None, rule=nc.RULE, invert=False):
    """gs4d_host_nearest_neighbours through the binding: (the hit table uint8 [n, hit_stride], the STAT table or None) after the call"""
    kw = ec.rule_keywords(rule, invert) if source is not None else {}
    hits = np.ascontiguousarray(hits, np.uint8)
    ht, st = _gs4d().nearest_neighbours_host(rec, source=source, query=struct(t, r, k, flags), hits=hits, hit_stride=hits.shape[1], stats=table,
                                             with_stats=table is not None, **kw)
    return ht, None if st is None else st.view(STAT)


def slots(table, k):
    """the (n, k) HIT view (dist2 as bits) of a hit table uint8 [n, hit_stride]"""
    t = np.ascontiguousarray(table, np.uint8)
    return np.ascontiguousarray(t[:, :8 * k]).view(HIT).reshape(t.shape[0], k)


def sentinel_hits(n, hit_stride):
    return np.full((n, hit_stride), SENTINEL, np.uint8)


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------------------------
def stride_of(k, c):
    """the stride of combination c: the smallest one, now and then a wider one (k = 3 in 32 bytes, k = 1 in 1024 among them)"""
    if c % 5 == 1:
        return {1: 1024, 3: 32}.get(k, stride_for(k) + 16 * (c % 3))
    return stride_for(k)


def matrix(kind, sizes=nc.SIZES):
    """(n, form, k, flags, hit_stride, with_stats, prefilled) for one kind: at every size COMBOS consecutive combinations (BIG_COMBOS at n = 4097)
    of the cycle through forms x KS x flags, starting where the last size stopped and at another place for every kind — every k, flag value and
    form appears per kind many times over"""
    c = 11 * nc.KINDS.index(kind)
    for n in sizes:
        for _ in range(BIG_COMBOS if n > 1024 else COMBOS):
            k = KS[c % 7]
            yield n, nc.FORMS[c % 3], k, c % 8, stride_of(k, c), c % 4 != 3, c % 2 == 1
            c += 1


def hostile_matrix():
    """(case, form, k, flags, hit_stride, with_stats, prefilled) over neighbour_cases.hostile_sets(): every set with flags 0 and 7 at least"""
    c = 0
    for case in nc.hostile_sets():
        for flags in (0, 7, c % 8):
            k = KS[c % 7]
            yield case, nc.FORMS[c % 3], k, flags, stride_of(k, c), c % 4 != 3, c % 2 == 1
            c += 1
