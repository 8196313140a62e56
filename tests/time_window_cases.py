"""gs4d_record_time_spans and gs4d_compact_time_window (include/gs4d.h) restated in numpy, and the tables of their tests.

Test infrastructure only (tests/test_time_window_host.py pins it on the CPU, tests/test_gpu_time_window.py runs the device against it).  The span
of a record is defined by float32 operations, so every comparison is exact: arg() evaluates the draw's expression with numpy float32 arrays (IEEE
round to nearest, one rounding per operation), spans() bisects over the ordered bit patterns of t exactly as the header describes, and
brute_alive() — which shares nothing with the bisection — evaluates arg() at every float in a neighbourhood.
"""
import zlib

import numpy as np

DEAD_ARG = np.float32(-106.0)                              # GS4D_TIME_DEAD_ARG
SPAN = np.dtype([("t_first", "<f4"), ("t_last", "<f4")])   # gs4d_time_span
FLT_MAX = np.float32(np.finfo(np.float32).max)
INF = np.float32(np.inf)
NEVER, ALWAYS = (INF, -INF), (-INF, INF)
SPAN_SIZES = (1, 63, 64, 65, 2049)                         # one thread per record, workgroups of 256: below, on and above a wave, past eight workgroups
COMPACT_SIZES = (0, 1, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1)      # tiles of 2048 records, waves of 64
STRIDES = (96, 16)


def seed(name):
    return zlib.crc32(name.encode())


def f32(x):
    return np.asarray(x, np.float32)


def arg(t, mu, inv):
    """((-0.5f * dt) * inv) * dt with dt = t - mu, every operation in float32"""
    with np.errstate(all="ignore"):
        dt = f32(t) - f32(mu)
        return ((np.float32(-0.5) * dt) * f32(inv)) * dt


def key(t):
    """float32 -> int64 in the order of the floats (-0 just below +0)"""
    b = f32(t).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)


def unkey(k):
    k = np.asarray(k, np.int64)
    return np.where(k & 0x80000000, k & 0x7FFFFFFF, 0xFFFFFFFF - k).astype(np.uint32).view(np.float32)


def edge(mu, inv, end):
    """per record: the last float32 from mu towards `end` (+-FLT_MAX) with arg >= DEAD_ARG — bisection between an alive and a dead key"""
    mu, inv = f32(mu), f32(inv)
    endv = np.full(mu.shape, end, np.float32)
    done = arg(endv, mu, inv) >= DEAD_ARG
    a, d = key(mu), key(endv)
    for _ in range(32):
        go = ~done & (np.abs(d - a) > 1)
        if not go.any():
            break
        m = np.minimum(a, d) + np.abs(d - a) // 2
        alive = arg(unkey(m), mu, inv) >= DEAD_ARG
        a = np.where(go & alive, m, a)
        d = np.where(go & ~alive, m, d)
    assert (done | (np.abs(d - a) == 1)).all(), "32 halvings did not close an interval"
    return np.where(done, endv, unkey(a))


def spans_of(mu, cw, s44, min_opacity):
    """the SPAN table of records given by their three floats"""
    mu, cw, s44 = f32(mu).reshape(-1), f32(cw).reshape(-1), f32(s44).reshape(-1)
    min_opacity = np.float32(min_opacity)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / s44
        never = ~(cw > 0)
        always = ~never & (bool(not (min_opacity <= 0)) | ~((s44 > 0) & (s44 < INF)) | ~((inv > 0) & (inv < INF)) | ~(np.abs(mu) < INF))
    out = np.zeros(mu.shape[0], SPAN)
    out["t_first"], out["t_last"] = np.where(never, INF, -INF), np.where(never, -INF, INF)
    b = ~never & ~always
    if b.any():
        out["t_first"][b] = edge(mu[b], inv[b], -FLT_MAX)
        out["t_last"][b] = edge(mu[b], inv[b], FLT_MAX)
    return out


def spans(rec, min_opacity=0.0):
    """the SPAN table of (n, 24) float32 SplatData records: mu = float 3, colour alpha = float 7, s44 = float 23"""
    rec = f32(rec).reshape(-1, 24)
    return spans_of(rec[:, 3], rec[:, 7], rec[:, 23], min_opacity)


def brute_alive(mu, inv, centre, radius):
    """(keys, alive): arg >= DEAD_ARG evaluated at every float32 within `radius` bit patterns of `centre` (finite ones), per record: (n, 2 * radius + 1)"""
    k = key(centre)[:, None] + np.arange(-radius, radius + 1, dtype=np.int64)[None, :]
    k = np.clip(k, int(key(-FLT_MAX)), int(key(FLT_MAX)))
    return k, arg(unkey(k), f32(mu)[:, None], f32(inv)[:, None]) >= DEAD_ARG


# ---- the classes, hand-written: (mu, colour alpha, s44, min_opacity) -> NEVER, ALWAYS or "span" -------------------------------------------------
NAN = np.float32(np.nan)
CLASS_TABLE = (
    ("plain", 25.0, 0.7, 0.25, 0.0, "span"),
    ("negative zero floor", 25.0, 0.7, 0.25, -0.0, "span"),
    ("negative floor", 25.0, 0.7, 0.25, -1.0, "span"),
    ("alpha +inf", 25.0, np.inf, 0.25, 0.0, "span"),
    ("mu -0", -0.0, 1.0, 1.0, 0.0, "span"),
    ("mu FLT_MAX", FLT_MAX, 1.0, 1.0, 0.0, "span"),
    ("mu -FLT_MAX, huge s44", -FLT_MAX, 1.0, 1e38, 0.0, "span"),
    ("smallest normal s44", 1.0, 1.0, 2.0 ** -126, 0.0, "span"),
    ("s44 = FLT_MAX: a subnormal reciprocal", 1.0, 1.0, FLT_MAX, 0.0, "span"),
    ("alpha 0", 25.0, 0.0, 0.25, 0.0, NEVER),
    ("alpha -0", 25.0, -0.0, 0.25, 0.0, NEVER),
    ("alpha negative", 25.0, -0.5, 0.25, 0.0, NEVER),
    ("alpha NaN", 25.0, NAN, 0.25, 0.0, NEVER),
    ("alpha -inf", 25.0, -np.inf, 0.25, 0.0, NEVER),
    ("alpha 0 under a floor", 25.0, 0.0, 0.25, 0.5, NEVER),
    ("alpha NaN, s44 NaN", 25.0, NAN, NAN, 0.0, NEVER),
    ("s44 0", 25.0, 0.7, 0.0, 0.0, ALWAYS),
    ("s44 -0", 25.0, 0.7, -0.0, 0.0, ALWAYS),
    ("s44 negative", 25.0, 0.7, -0.25, 0.0, ALWAYS),
    ("s44 inf", 25.0, 0.7, np.inf, 0.0, ALWAYS),
    ("s44 NaN", 25.0, 0.7, NAN, 0.0, ALWAYS),
    ("s44 subnormal: its reciprocal is inf", 25.0, 0.7, 2.0 ** -140, 0.0, ALWAYS),
    ("mu inf", np.inf, 0.7, 0.25, 0.0, ALWAYS),
    ("mu -inf", -np.inf, 0.7, 0.25, 0.0, ALWAYS),
    ("mu NaN", NAN, 0.7, 0.25, 0.0, ALWAYS),
    ("a floor", 25.0, 0.7, 0.25, 0.05, ALWAYS),
    ("the smallest floor", 25.0, 0.7, 0.25, 2.0 ** -149, ALWAYS),
    ("a NaN floor", 25.0, 0.7, 0.25, NAN, ALWAYS),
)


def class_records(min_opacity):
    """(records (k, 24), expected class per record) of the CLASS_TABLE rows that are stated for this min_opacity (compared as bit patterns: -0, NaN)"""
    want = f32(min_opacity).view(np.uint32)
    rows = [r for r in CLASS_TABLE if f32(r[4]).view(np.uint32) == want]
    rec = np.zeros((len(rows), 24), np.float32)
    rec[:, 20] = 1.0                                       # a covariance that is otherwise the identity
    rec[:, 10] = rec[:, 15] = 1.0
    for i, (_, mu, cw, s44, _, _) in enumerate(rows):
        rec[i, 3], rec[i, 7], rec[i, 23] = mu, cw, s44
    return rec, [r[5] for r in rows]


CLASS_FLOORS = (0.0, -0.0, -1.0, 0.5, 0.05, 2.0 ** -149, NAN)


def synthetic(n, extreme):
    """(mu, s44): n pairs as a long 4D sequence has them (mu ~ U[0, 50], s44 from 0.06 to 1) followed by `extreme` pairs with s44 log-uniform over
    1e-12 .. 1e12 and mu up to +-1e6, some of them exactly 0"""
    rng = np.random.default_rng(seed("time_window/synthetic"))
    mu = np.concatenate([rng.uniform(0.0, 50.0, n), rng.uniform(-1e6, 1e6, extreme) * (rng.uniform(size=extreme) < 0.9)])
    s44 = np.concatenate([rng.uniform(0.06, 1.0, n), 10.0 ** rng.uniform(-12.0, 12.0, extreme)])
    return f32(mu), f32(s44)


# ---- the window ------------------------------------------------------------------------------------------------------------------------------------
def keeps(table, t0, t1):
    """the rule of gs4d_compact_time_window on a SPAN table: the span meets [t0, t1]"""
    return (table["t_first"] <= np.float32(t1)) & (table["t_last"] >= np.float32(t0))


def reference(table, t0, t1, src, stride, cap_dst, cap_idx):
    """-> (dst_prefix, idx_prefix, kept, written), as compact_cases.reference: the first `written` records (rows of `stride` bytes; None without
    src) and indices of the outputs, the true kept count and written = min(kept, cap_dst, cap_idx).  A capacity of None: that output is not given."""
    idx = np.flatnonzero(keeps(table, t0, t1)).astype(np.uint32)
    kept = int(idx.size)
    written = min([kept] + [c for c in (cap_dst, cap_idx) if c is not None])
    dst = None if src is None else np.ascontiguousarray(src).view(np.uint8).reshape(len(table), stride)[idx[:written]]
    return dst, idx[:written].copy(), kept, written


def window_table(n, finite=False):
    """finite: the first eleven kinds only — finite spans, so that a far window keeps none and an infinite one all.  A SPAN table of n rows for the window [24, 26] with every kind of row, each sitting ON the rule's edge or one float beside it: spans that
    end at 24 exactly (kept) and one float below (dropped), that begin at 26 and one float above, that cover the window, lie inside it, are a
    single point, never and always rows, and a NaN row (dropped: a NaN compares false)."""
    lo, hi = np.float32(24.0), np.float32(26.0)
    below, above = np.nextafter(lo, -INF), np.nextafter(hi, INF)
    kinds = [(0.0, lo), (0.0, below), (hi, 50.0), (above, 50.0), (0.0, 50.0), (24.5, 25.5), (25.0, 25.0), (lo, lo), (hi, hi), (below, below), (above, above),
             NEVER, ALWAYS, (-INF, below), (above, INF), (-INF, lo), (hi, INF), (NAN, NAN), (NAN, 50.0), (0.0, NAN)]
    pick = np.random.default_rng(seed(f"time_window/table/{n}")).integers(0, 11 if finite else len(kinds), n)
    out = np.zeros(n, SPAN)
    out["t_first"], out["t_last"] = f32([kinds[k][0] for k in pick]), f32([kinds[k][1] for k in pick])
    return out


def mask_table(mask):
    """a SPAN table that the window [24, 26] keeps exactly where mask says: a kept span ends at 24 exactly, a dropped one one float below"""
    out = np.zeros(mask.size, SPAN)
    out["t_last"] = np.where(mask, np.float32(24.0), np.nextafter(np.float32(24.0), -INF))
    return out
