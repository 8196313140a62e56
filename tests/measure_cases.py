"""gs4d_measure_records (include/gs4d.h) restated in numpy, and the record sets, selections and queries of its tests.

Test infrastructure only (tests/test_measure_host.py pins gs4d_host_measure_records to the restatement on the CPU; tests/test_gpu_measure.py runs the
device call against the host definition).  Plain numpy: float32 arrays, one ufunc per operation of the definition, so every product and every sum is
rounded on its own; numpy's float32 division and square root are correctly rounded.  The centre is centre_cases.centre, the selection
edit_cases.selected: the texts the header refers to.

Sizes: the two walking kernels give a workgroup of THREADS threads one record per thread and round, at most GROUPS workgroups (a grid stride beyond);
the final kernel folds one partial row per workgroup with THREADS threads.
"""
import functools
import importlib

import numpy as np

import centre_cases as cc
import edit_cases as ec
import hostile_cases
import scenes

f32, f64 = np.float32, np.float64
THREADS = 256                                             # MEASURE_THREADS (csrc/gs4d_internal.h)
GROUPS = 1024                                             # MEASURE_GROUPS: the grid cap
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
N_PARTIALS = THREADS * THREADS + 1                        # THREADS + 1 workgroups: more partial rows than the final workgroup has threads
N_STRIDE = GROUPS * THREADS + THREADS + 1                 # the capped grid, and its first THREADS + 1 threads walk a second record
EXTRA = 3                                                 # records behind n that no call may look at
W, H = 64, 48                                             # the image of every context of these tests
SKIP_HIDDEN, SKIP_DEAD = 1, 2                             # GS4D_MS_*
FLAGS = (0, SKIP_HIDDEN, SKIP_DEAD, SKIP_HIDDEN | SKIP_DEAD)
T = cc.T                                                  # part of a 4D set of centre_cases.records is dead at T
TIMES = (0.0, T - 0.25, T)
KINDS = ("static3d", "symmetric", "edges")                # static 3D, true 4D with velocity (build_records_4d_tvar), hand-made edge records
FORMS = ("all", "rule", "inverted")                       # no table; a table and a rule; the same with GS4D_KEEP_INVERT
RULE = (5, 0x3B808081, ec.WSUM_MIN)                       # every field has a threshold
NAN, INF = float("nan"), float("inf")
MEASURE = np.dtype([("count", "<u4"), ("unplaced", "<u4"), ("skipped", "<u4"), ("reserved0", "<u4"), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)),
                    ("ext_lo", "<f4", (3,)), ("ext_hi", "<f4", (3,)), ("cell_sum", "<u8", (3,)), ("reserved1", "<u8")])
assert MEASURE.itemsize == 96


def _gs4d():
    return importlib.import_module("4dgaussiansplatrendering_amd")


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------------
def key(v):
    """the total order of the box ends: bits ^ (sign ? 0xFFFFFFFF : 0x80000000), as uint32"""
    b = np.ascontiguousarray(v, f32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.asarray(k, np.uint32)
    return (k ^ np.where(k >> np.uint32(31) != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(f32)


def keyed_min(v, empty=INF):
    return unkey(key(v).min()) if v.size else f32(empty)


def keyed_max(v, empty=-INF):
    return unkey(key(v).max()) if v.size else f32(empty)


def parts(rec, t, flags, stats=None, rule=RULE, invert=False):
    """the definition's intermediate results, for the premises of the tests: selected, skipped, measured [n] (bool), m, reach, the reach ends [n, 3]"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    n = rec.shape[0]
    sel = ec.selected(n, stats, rule, invert)
    m, dt, inv = cc.centre(rec, t)
    with np.errstate(all="ignore"):
        skip = np.zeros(n, bool)
        if flags & SKIP_HIDDEN:
            skip |= ~(rec[:, 7] > f32(0.0))
        if flags & SKIP_DEAD:
            skip |= (((f32(-0.5) * dt) * inv) * dt) < cc.DEAD_ARG
        placed = np.isfinite(m).all(1)
        sig3 = rec[:, 20:23]
        var = rec[:, [8, 13, 18]] - ((sig3 * sig3) * inv[:, None])
        reach = np.where(var > f32(0.0), f32(3.0) * np.sqrt(var), f32(0.0)).astype(f32)
        e0, e1 = m - reach, m + reach
    return dict(selected=sel, skipped=sel & skip, unplaced=sel & ~skip & ~placed, measured=sel & ~skip & placed, m=m, var=var, reach=reach, e0=e0, e1=e1)


def restate(rec, t, flags, stats=None, rule=RULE, invert=False):
    """the 96 bytes of the measurement as one MEASURE record, and parts()"""
    p = parts(rec, t, flags, stats, rule, invert)
    out = np.zeros(1, MEASURE)
    o = out[0]
    on = p["measured"]
    o["count"], o["unplaced"], o["skipped"] = int(on.sum()), int(p["unplaced"].sum()), int(p["skipped"].sum())
    m = p["m"][on]
    for a in range(3):
        o["lo"][a], o["hi"][a] = keyed_min(m[:, a]), keyed_max(m[:, a])
        e0, e1 = p["e0"][on, a], p["e1"][on, a]
        o["ext_lo"][a], o["ext_hi"][a] = keyed_min(e0[np.isfinite(e0)]), keyed_max(e1[np.isfinite(e1)])
        with np.errstate(all="ignore"):
            d, e = m[:, a] - o["lo"][a], o["hi"][a] - o["lo"][a]
            g = (d / e) * f32(1048576.0)
            cell = np.where(g >= f32(0.0), np.minimum(g, f32(1048576.0)), f32(0.0)).astype(np.uint64)
        o["cell_sum"][a] = cell.sum(dtype=np.uint64)
    return out, p


def struct(t, flags):
    """the query as the binding's MeasureQuery"""
    q = _gs4d().MeasureQuery()
    q.t, q.flags = float(f32(t)), int(flags)
    return q


def host(rec, t, flags, stats=None, rule=RULE, invert=False):
    """gs4d_host_measure_records through the binding, as one MEASURE record"""
    g = _gs4d()
    kw = ec.rule_keywords(rule, invert) if stats is not None else {}
    m = g.measure_records_host(rec, stats=stats, query=struct(t, flags), **kw)
    return np.frombuffer(bytes(m), MEASURE).copy()


# ---- record sets -------------------------------------------------------------------------------------------------------------------------------------
def edge_records(n):
    """hand-made records, all of z = 7 exactly (e == 0 on that axis) and cycling through: a plain one; S[0][0] == 0 and a negative S[1][1] (var <= 0);
    var = NaN; S[0][0] = +inf (the reach is +inf: both ends on x are left out); centres at 3e38 and -3e38 on x (e overflows); a
    moving one with sig3 large against S (var < 0 through the subtraction); a position of +inf, NaN, and s44 == 0 (not placed); hidden ones; dead ones;
    a +0 and a -0 on x (sig3.x = -0: the centre keeps the sign)."""
    rec = np.zeros((n, 24), f32)
    i = np.arange(n)
    u = scenes.uniform(n, 0, seed=0x4D53) * 2.0 - 1.0
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = 30.0 * u, 20.0 * np.roll(u, 1), 7.0, T
    rec[:, 4:8] = (0.5, 0.25, 0.75, 0.9)
    rec[:, 8], rec[:, 13], rec[:, 18], rec[:, 23] = 4.0, 2.25, 1.0, 1.0
    k = i % 13
    rec[k == 1, 8], rec[k == 1, 13] = 0.0, -1.0
    rec[k == 2, 8] = NAN
    rec[k == 3, 8] = INF
    rec[k == 4, 0] = np.where((i[k == 4] // 13) % 2 == 0, f32(3e38), f32(-3e38))          # hi - lo overflows on x once both are there
    rec[k == 5, 3], rec[k == 5, 20], rec[k == 5, 8] = T - 0.5, 3.0, 1.0                 # var = 1 - 9 < 0; the centre moves by 1.5 at T
    rec[k == 6, 0] = INF
    rec[k == 7, 1] = NAN
    rec[k == 8, 23] = 0.0                                                               # 1 / s44 = inf, dt = 0: k = NaN
    rec[k == 9, 7] = np.array([0.0, -0.5, -0.0], f32)[(i[k == 9] // 13) % 3]
    rec[k == 10, 3] = T + 20.0                                                          # the argument is -200
    rec[k == 11, 0], rec[k == 11, 20] = 0.0, -0.0
    rec[k == 12, 0], rec[k == 12, 20] = -0.0, -0.0
    return rec


@functools.lru_cache(maxsize=None)
def records(kind, n):
    if kind == "edges":
        rec = edge_records(n)
        rec.setflags(write=False)
        return rec
    return cc.records(kind, n)


@functools.lru_cache(maxsize=None)
def big_records(n):
    """a large true-4D set made by tiling a small one with a per-copy offset (cheap to make; every record differs)"""
    base = cc.records("symmetric", 4097)
    reps = -(-n // base.shape[0])
    rec = np.tile(base, (reps, 1))[:n].copy()
    rec[:, 0] += (np.arange(n) // base.shape[0]).astype(f32) * f32(0.125)
    rec.setflags(write=False)
    return rec


def selection(n, form, seed=0x4D54):
    """(stats, rule, invert) of a selection form: about half of the records pass RULE; a failing row misses one threshold by one unit"""
    if form == "all":
        return None, RULE, False
    mask = scenes.uniform(n, 1, seed=seed) < 0.5
    if n > 1:
        mask[0], mask[n - 1] = True, False                    # (neither form selects everything or nothing)
    return ec.mask_table(mask, RULE), RULE, form == "inverted"


def one_selected(n, index):
    """a table and rule that select record `index` alone"""
    mask = np.zeros(n, bool)
    mask[index] = True
    return ec.mask_table(mask, RULE), RULE, False


def matrix(kinds=KINDS, sizes=SIZES):
    """(kind, n, t, flags, form): the case matrix of the issue"""
    for kind in kinds:
        for n in sizes:
            for t in TIMES:
                for flags in FLAGS:
                    for form in FORMS:
                        yield kind, n, t, flags, form


def hostile_sets():
    return hostile_cases.all_cases()
