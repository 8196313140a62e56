"""GPU: gs4d_nearest_neighbours — for every record the k nearest source records within a radius as a row of {record, dist2} hits, and optionally
the number of hits and the last distance as rows of a record-statistics table (include/gs4d.h).

Both tables are checked byte for byte against gs4d_host_nearest_neighbours, the brute-force definition (which tests/test_nearest_host.py pins to the
numpy restatement of the header's text on the CPU, over the same matrix, together with the premises: rows without a hit, rows that are not full,
truncated rows, cuts inside a tie of dist2, a smaller-index twin in front of the record itself, records that take no part), with guard buffers
around data, source, hits and stats; every kernel instantiation is named; refusals write nothing; the call orders itself with draws that add to the
source table and with later uploads, shares its scratch with gs4d_count_neighbours and gs4d_label_components, never builds a shadow, and closes
three chains: scales from the 3 nearest points, density-adaptive floaters, and the symmetry of the neighbour lists.  All calls go through the
Python binding over the C ABI; contexts are 64 x 48."""
import ctypes

import numpy as np
import pytest

import edit_cases as ec
import nearest_cases as nn
import neighbour_cases as nc

pytestmark = pytest.mark.gpu
SENTINEL = nn.SENTINEL
GUARD = 4096
f32 = np.float32
W, H = nc.W, nc.H


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


class Bench:
    """the buffers of one record set between sentinel guard buffers: data (the n records, EXTRA more behind them — copies of the first ones, so
    they would be the nearest neighbours of those if they were looked at — and a sentinel tail), a source table of n rows with EXTRA rows behind
    them that pass every rule of these tests, a hit table with room for n rows of the widest stride and a tail, and a stats table of exactly n rows"""

    def __init__(self, ctx, case):
        self.ctx, self.case, self.n = ctx, case, case.n
        held = np.concatenate([case.rec, np.resize(case.rec, (nc.EXTRA, 24))])
        self.host_data = np.concatenate([held.view(np.uint8).reshape(-1), np.full(GUARD, SENTINEL, np.uint8)])
        self.g0, self.data, self.g1 = fill(ctx, GUARD), ctx.buffer(self.host_data), fill(ctx, GUARD)
        self.source, self.g2 = ctx.buffer(nbytes=16 * (self.n + nc.EXTRA)), fill(ctx, GUARD)
        self.hits, self.g3 = ctx.buffer(nbytes=self.n * 1024 + GUARD), fill(ctx, GUARD)
        self.stats, self.g4 = ctx.buffer(nbytes=max(16, 16 * self.n)), fill(ctx, GUARD)
        self.src_form = None

    def check(self, form, k, flags, hit_stride, with_stats, prefilled, what):
        """one call: all n * hit_stride bytes of the hit table, the tail behind them and the stats table against the host definition; returns the
        slots [n, k] and the table"""
        c, case, n = self.ctx, self.case, self.n
        source, rule, invert = nc.selection(n, form)
        if source is not None and form != self.src_form:
            self.src_all = np.concatenate([source, ec.mask_table(np.full(nc.EXTRA, not invert), rule)])
            c.subdata(self.source, self.src_all)
            self.src_form = form
        table = nc.table("random" if prefilled else "zero", n)
        c.subdata(self.stats, table)
        span = n * hit_stride + GUARD
        c.subdata(self.hits, np.full(span, SENTINEL, np.uint8))
        kw = ec.rule_keywords(rule, invert) if source is not None else {}
        c.nearest_neighbours(n, self.data, source=self.source if source is not None else None, hits=self.hits, hit_stride=hit_stride,
                             stats=self.stats if with_stats else None, query=nn.struct(case.t, case.r, k, flags), **kw)
        got = c.read(self.hits, np.uint8, span)
        got_s = c.read(self.stats, nc.STAT, n)
        want, want_s = nn.host(case.rec, case.t, case.r, k, flags, nn.sentinel_hits(n, hit_stride), table if with_stats else None, source, rule, invert)
        rows = got[:n * hit_stride].reshape(n, hit_stride)
        assert rows.tobytes() == want.tobytes(), f"{what}: rows {np.flatnonzero((rows != want).any(1))[:8]}\n{nn.slots(rows, k)[(rows != want).any(1)][:3]}\n{nn.slots(want, k)[(rows != want).any(1)][:3]}"
        assert (rows[:, 8 * k:] == SENTINEL).all() and (got[n * hit_stride:] == SENTINEL).all(), f"{what}: bytes past 8 k or past row n - 1 were written"
        assert got_s.tobytes() == (want_s if with_stats else table).tobytes(), f"{what}: table rows {np.flatnonzero(got_s != (want_s if with_stats else table))[:8]}"
        slots = nn.slots(rows, k)
        assert ((slots["record"] < n) | (slots["record"] == nn.ID_NONE)).all(), f"{what}: a record behind n is a hit"
        return slots, got_s

    def check_the_rest(self, what):
        c = self.ctx
        assert all(untouched(c, g) for g in (self.g0, self.g1, self.g2, self.g3, self.g4)), f"{what}: a guard buffer changed"
        assert np.array_equal(c.read(self.data, np.uint8, self.host_data.size), self.host_data), f"{what}: data changed"
        if self.src_form is not None:
            assert c.read(self.source, nc.STAT, self.n + nc.EXTRA).tobytes() == self.src_all.tobytes(), f"{what}: the source table changed"

    def delete(self):
        for b in (self.g0, self.data, self.g1, self.source, self.g2, self.hits, self.g3, self.stats, self.g4):
            self.ctx.delete(b)


# ---- 1. bits, and nothing else is written ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", nc.KINDS)
def test_both_tables_equal_the_host_definition_byte_for_byte(gs4d, kind):
    """the matrix of tests/test_nearest_host.py: every size, k, flag value and source form, minimal and wide strides, without a table, into a
    zeroed and into a pre-filled one"""
    ctx = gs4d.Context(W, H)
    filled, bench = 0, None
    for n, form, k, flags, hit_stride, with_stats, prefilled in nn.matrix(kind):
        if bench is None or bench.n != n:
            if bench is not None:
                bench.check_the_rest(f"{kind}, n = {bench.n}")
                bench.delete()
            bench = Bench(ctx, nc.case(kind, n))
        slots, _ = bench.check(form, k, flags, hit_stride, with_stats, prefilled, f"{kind}, n = {n}, {form}, k = {k}, flags = {flags}, stride {hit_stride}")
        filled += int((slots["record"] != nn.ID_NONE).sum())
    bench.check_the_rest(f"{kind}, n = {bench.n}")
    bench.delete()
    assert filled > 0
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_hostile_record_sets(gs4d):
    ctx = gs4d.Context(W, H)
    filled, bench = 0, None
    for case, form, k, flags, hit_stride, with_stats, prefilled in nn.hostile_matrix():
        if bench is None or bench.case is not case:
            if bench is not None:
                bench.check_the_rest(bench.case.name)
                bench.delete()
            bench = Bench(ctx, case)
        slots, _ = bench.check(form, k, flags, hit_stride, with_stats, prefilled, f"{case.name}, {form}, k = {k}, flags = {flags}")
        filled += int((slots["record"] != nn.ID_NONE).sum())
    bench.check_the_rest(bench.case.name)
    bench.delete()
    assert filled > 0
    ctx.finish()
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(W, H)
    data, source, hits, stats = fill(ctx, 96 * 4), fill(ctx, 64), fill(ctx, 64), fill(ctx, 64)
    ctx.nearest_neighbours(0, data, 1.0, hits=hits)
    ctx.nearest_neighbours(0, data, 1.0, k=16, source=source, hits=hits, hit_stride=128, stats=stats, include_self=True, min_pixels=1)
    ctx.finish()
    assert untouched(ctx, data, 96 * 4) and untouched(ctx, source, 64) and untouched(ctx, hits, 64) and untouched(ctx, stats, 64)
    assert ctx.read_hits(hits, 0, 3).shape == (0, 3)
    ctx.close()


# ---- 2. every instantiation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", (False, True), ids=("COL=off", "COL=on"))
@pytest.mark.parametrize("k", (4, 8, 16, 1, 5, 9))
def test_every_instantiation(gs4d, col, k):
    """k_nn_query<COL, K>: COL is GS4D_NN_SKIP_HIDDEN, K the least of 4, 8, 16 that holds k — its largest and its smallest k.  A clump of 257
    records in one cell: the rows overflow k = 16"""
    case = nc.case("clump", 257)
    flags = (nn.SKIP_HIDDEN if col else 0) | nn.SKIP_DEAD
    _, _, f, ncand = nn.restate(case.rec, case.t, case.r, k, flags, nn.sentinel_hits(case.n, nn.stride_for(k)), d2=nn.case_dist2(case))
    assert (ncand > 16).sum() > 100 and (f == k).sum() > 100
    ctx = gs4d.Context(W, H)
    b = Bench(ctx, case)
    for form, prefilled in (("all", False), ("rule", True)):
        slots, st = b.check(form, k, flags, nn.stride_for(k), True, prefilled, f"COL = {col}, k = {k}, {form}")
        assert (slots["record"][:, k - 1] != nn.ID_NONE).sum() > 50
    b.check_the_rest(f"COL = {col}, k = {k}")
    b.delete()
    ctx.finish()
    ctx.close()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_tables_as_they_were(gs4d):
    case = nc.case("cube", 257)
    n = case.n
    ctx, lib = gs4d.Context(W, H), gs4d._lib
    src_table, rule, _ = nc.selection(n, "rule")
    table = nc.table("random", n)
    hit_bytes = nn.sentinel_hits(n, 1024)
    data, source, stats, hits = ctx.buffer(case.rec), ctx.buffer(src_table), ctx.buffer(table), ctx.buffer(hit_bytes)
    short_data, short_source, short_stats, dead = ctx.buffer(case.rec.reshape(-1)[:-1]), ctx.buffer(src_table[:-1]), ctx.buffer(table[:-1]), fill(ctx, 64)
    short_hits = fill(ctx, n * 32 - 1)
    ctx.delete(dead)
    NO = object()
    good_rule = gs4d._keep_rule(**ec.rule_keywords(rule))

    def call(data=data, n=n, q=None, source=source, rule=good_rule, hits=hits, stride=32, stats=stats, r=case.r, k=3, flags=7, reserved=None, rule_flags=None,
             rule_reserved=None):
        s = nn.struct(case.t, r, k, flags)
        if reserved is not None:
            s.reserved[reserved] = 1
        kr = None if rule is None else rule.copy()
        if rule_flags is not None:
            kr["flags"] = rule_flags
        if rule_reserved is not None:
            kr["reserved"] = rule_reserved
        return lib.gs4d_nearest_neighbours(ctx._h, data, ctypes.c_size_t(n), None if q is NO else ctypes.byref(s), source, None if kr is None else kr.ctypes.data,
                                           hits, ctypes.c_size_t(stride), stats)

    def short_stride(k):
        """8 k - 8 rounded up to 16, when that is below 8 k: the stride that holds k - 1 hits"""
        s = 16 * ((8 * k - 8 + 15) // 16)
        return s if s < 8 * k else None

    bad = {
        "query == NULL": dict(q=NO), "flag 8": dict(flags=8 | 1), "flag bit 31": dict(flags=0x80000000), "k == 0": dict(k=0), "k == 17": dict(k=17, stride=256),
        **{f"reserved[{j}]": dict(reserved=j) for j in range(4)},
        "r = 0": dict(r=0.0), "r < 0": dict(r=-1.0), "r = NaN": dict(r=np.nan), "r = inf": dict(r=np.inf), "r * r overflows": dict(r=2.0 ** 64),
        "r * r below FLT_MIN": dict(r=float(np.nextafter(f32(2.0 ** -63), f32(0.0)))),
        "n == 0xFFFFFFFF": dict(n=0xFFFFFFFF), "n > 0xFFFFFFFF": dict(n=1 << 32), "no data": dict(data=0), "dead data": dict(data=dead),
        "unknown data": dict(data=9999), "dead stats": dict(stats=dead), "unknown stats": dict(stats=9999),
        "data too small": dict(data=short_data), "stats too small": dict(stats=short_stats), "source without a rule": dict(rule=None),
        "a rule without source": dict(source=0), "rule flag 2": dict(rule_flags=2), "rule reserved": dict(rule_reserved=1),
        "dead source": dict(source=dead), "unknown source": dict(source=9999), "source too small": dict(source=short_source),
        "no hits": dict(hits=0), "dead hits": dict(hits=dead), "unknown hits": dict(hits=9999), "hits too small": dict(hits=short_hits),
        "stride 0": dict(stride=0), "stride 8": dict(stride=8, k=1), "stride 24": dict(stride=24), "stride 1040": dict(stride=1040),
        **{f"stride {short_stride(k)} for k = {k}": dict(stride=short_stride(k), k=k) for k in range(1, 17) if short_stride(k)},
        "hits == data": dict(hits=data), "hits == source": dict(hits=source), "hits == stats": dict(hits=stats),
        "data == stats": dict(stats=data), "data == source": dict(source=data), "source == stats": dict(source=stats),
        "hits == data without a source": dict(hits=data, source=0, rule=None, stats=0),
    }
    assert sum(what.startswith("stride") for what in bad) == 4 + 7                # (every odd k from 3 on has a stride that holds k - 1 hits only)
    for what, kw in bad.items():
        assert call(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    assert call(n=0, flags=8) == -1 and call(n=0, hits=dead) == -1 and call(n=0, r=0.0) == -1 and call(n=0, stride=24) == -1      # ... with no records too
    ctx.finish()
    assert ctx.read(stats, nc.STAT, n).tobytes() == table.tobytes() and ctx.read(hits, np.uint8, hit_bytes.size).tobytes() == hit_bytes.tobytes(), "a refused call wrote something"
    assert ctx.read(short_stats, nc.STAT, n - 1).tobytes() == table[:-1].tobytes() and untouched(ctx, short_hits, n * 32 - 1)
    assert np.array_equal(ctx.read(data, f32, n * 24).view(np.uint32), case.rec.reshape(-1).view(np.uint32))
    assert ctx.read(source, nc.STAT, n).tobytes() == src_table.tobytes()
    # the call works after the refusals, at the ends of the radius range too
    assert call() == 0
    want, want_s = nn.host(case.rec, case.t, case.r, 3, 7, nn.sentinel_hits(n, 32), table, src_table, rule, False)
    assert ctx.read(hits, np.uint8, n * 32).tobytes() == want.tobytes() and ctx.read(stats, nc.STAT, n).tobytes() == want_s.tobytes()
    assert want_s.tobytes() != table.tobytes() and untouched(ctx, hits, n * 32) is False
    for r in (2.0 ** -63, float(np.nextafter(f32(2.0 ** 64), f32(0.0)))):
        ctx.subdata(stats, table)
        assert call(source=0, rule=None, r=r, flags=4, k=16, stride=128) == 0
        want, want_s = nn.host(case.rec, case.t, r, 16, 4, nn.sentinel_hits(n, 128), table)
        assert ctx.read(hits, np.uint8, n * 128).tobytes() == want.tobytes() and ctx.read(stats, nc.STAT, n).tobytes() == want_s.tobytes()
    ctx.finish()
    ctx.close()


# ---- 4. ordering ------------------------------------------------------------------------------------------------------------------------------------
def test_the_call_sees_a_draw_that_adds_to_the_source_and_not_the_uploads_behind_it(gs4d):
    import test_gpu_centres as tc
    rec = tc.record_set(gs4d, "symmetric")
    n = rec.shape[0]
    r = nc.radius_for(n, 80.0, 6.0)
    s = tc.Scene(gs4d, rec)
    c = s.ctx
    assert c.stats()["lanes"] > 1
    s.frame(gs4d.MODE_4D_SORTED, 0)                             # the shadow exists and is current
    builds = c.shadow_builds(s.db)
    assert builds == 1
    # the draw alone, read back: the source table the call has to see
    alone = c.record_stats(n)
    tc.stats_frame(s, alone, 1)
    drawn = c.read(alone, ec.STAT, n)
    rule = (1, 0, int(np.median(drawn["wsum"])))                # what the draw shows most of: about half of the set
    assert 0 < int(ec.selected(n, drawn, rule).sum()) < n
    zero = nc.table("zero", n)
    blank = nn.sentinel_hits(n, 64)
    want, want_s = nn.host(rec, tc.T, r, 8, nn.INCLUDE_SELF, blank, zero, drawn, rule, False)
    assert want.tobytes() != nn.host(rec, tc.T, r, 8, nn.INCLUDE_SELF, blank, zero, zero, rule, False)[0].tobytes()
    # the same draw; the next lane; the call by the draw's table — nothing read or finished in between; then uploads right behind the call
    src, out, hits = c.record_stats(n), c.record_stats(n), c.buffer(blank)
    tc.stats_frame(s, src, 1)
    c.clear()                                                   # a new frame: the call is queued on another lane than the draw
    c.nearest_neighbours(n, s.db, r, k=8, t=tc.T, source=src, include_self=True, hits=hits, hit_stride=64, stats=out, **ec.rule_keywords(rule))
    c.subdata(src, np.zeros(n, ec.STAT))
    c.subdata(s.db, np.zeros_like(rec))
    got = c.read(hits, np.uint8, n * 64).reshape(n, 64)
    assert got.tobytes() == want.tobytes(), f"rows {np.flatnonzero((got != want).any(1))[:8]}"
    assert c.read(out, nc.STAT, n).tobytes() == want_s.tobytes()
    assert c.shadow_builds(s.db) == builds, "the call built or invalidated a shadow"
    c.finish()
    c.close()


# ---- 5. scratch re-use ------------------------------------------------------------------------------------------------------------------------------
def test_the_scratch_is_shared_with_count_neighbours_and_label_components_at_other_sizes(gs4d):
    """large, then small, then large again on one lane, a gs4d_count_neighbours or gs4d_label_components call of another size in between: the
    layout of the shared scratch (candidates, table, keys) depends on n"""
    ctx = gs4d.Context(W, H)
    other = nc.case("cube", 1025)
    odata, ostats = ctx.buffer(other.rec), ctx.record_stats(other.n)
    want_counts = nc.host(other.rec, other.t, other.r, 0xFFFFFFFF, 0, nc.table("zero", other.n))
    want_labels = gs4d.label_components_host(other.rec, other.r, with_stats=False)[0]
    for step, (kind, n, form, k, flags) in enumerate((("4d", 4097, "rule", 3, 7), ("cube", 65, "all", 16, 4), ("twins", 2, "all", 1, 4), ("lattice", 4097, "inverted", 4, 0),
                                                      ("far", 257, "all", 9, 5), ("cube", 4097, "all", 8, 4))):
        b = Bench(ctx, nc.case(kind, n))
        slots, _ = b.check(form, k, flags, nn.stride_for(k), True, False, f"{kind}, n = {n}")
        assert n == 2 or (slots["record"] != nn.ID_NONE).any()
        if step % 2 == 0:
            ctx.subdata(ostats, nc.table("zero", other.n))
            ctx.count_neighbours(ostats, other.n, odata, other.r)
        else:
            labels = ctx.label_components(other.n, odata, other.r)
        slots2, _ = b.check(form, k, flags, nn.stride_for(k), True, True, f"{kind}, n = {n}, again")
        assert slots2.tobytes() == slots.tobytes()
        if step % 2 == 0:
            assert ctx.read(ostats, nc.STAT, other.n).tobytes() == want_counts.tobytes()
        else:
            assert np.array_equal(ctx.read(labels, np.uint32, other.n), want_labels)
            ctx.delete(labels)
        b.check_the_rest(f"{kind}, n = {n}")
        b.delete()
    ctx.finish()
    ctx.close()


# ---- 6. a size of several sort tiles -----------------------------------------------------------------------------------------------------------------
def test_a_size_of_several_sort_tiles_and_three_radix_passes(gs4d):
    """n = 70001, about 200 neighbours each, k = 8.  The host's double loop is too slow to be the yardstick here: a fixed sample of 2000 rows
    against the numpy restatement of those rows, and the invariants of every row"""
    n, k, flags = nc.N_BIG, 8, nn.SKIP_HIDDEN | nn.SKIP_DEAD
    assert nc.bucket_bits(n) + 1 == 19 and n > 8 * 8192
    case = nc.dense_case()
    ctx = gs4d.Context(W, H)
    data, stats = ctx.buffer(case.rec), ctx.record_stats(n)
    hits, _ = ctx.nearest_neighbours(n, data, case.r, k=k, skip_hidden=True, skip_dead=True, stats=stats)
    raw = ctx.read(hits, np.uint8, n * 64).reshape(n, 64)
    got, st = nn.slots(raw, k), ctx.read(stats, nc.STAT, n)
    ctx.finish()
    ctx.close()
    part, m = nc.takes_part(case.rec, case.t, flags)
    rr = f32(case.r) * f32(case.r)
    # the sample, in chunks of 250 rows of the dist2 matrix
    sample = np.sort(np.random.default_rng(0x4E71).choice(n, 2000, replace=False))
    full = 0
    for rows in sample.reshape(8, 250):
        with np.errstate(all="ignore"):
            d = m[rows, None, 0] - m[None, :, 0]
            s = d * d
            d = m[rows, None, 1] - m[None, :, 1]
            s = s + (d * d)
            d = m[rows, None, 2] - m[None, :, 2]
            s = s + (d * d)
            cand = (s <= rr) & part[rows, None] & part[None, :]
        cand[np.arange(rows.size), rows] = False
        bits = s.view(np.uint32)
        for a, i in enumerate(rows):
            js = np.flatnonzero(cand[a])
            js = js[np.lexsort((js, bits[a, js]))][:k]
            want = np.zeros(k, nn.HIT)
            want["record"], want["dist2"] = nn.ID_NONE, nn.INF_BITS
            want["record"][:js.size], want["dist2"][:js.size] = js, bits[a, js]
            assert got[i].tobytes() == want.tobytes(), f"row {i}: {got[i]} != {want}"
            full += int(js.size == k)
    assert full > 1000 and (~part[sample]).sum() > 100
    # every row
    filled = got["record"] != nn.ID_NONE
    key = (got["dist2"].astype(np.uint64) << np.uint64(32)) | got["record"]
    assert (key[:, 1:] > key[:, :-1])[filled[:, 1:]].all(), "keys ascend (and no record is in a row twice)"
    assert (filled[:, :-1] | ~filled[:, 1:]).all(), "filled slots come before empty ones"
    assert (got["dist2"][~filled] == nn.INF_BITS).all() and (got["dist2"].view(f32)[filled] <= rr).all() and (got["record"][filled] < n).all()
    assert not filled[~part].any() and (got["record"] != np.arange(n)[:, None]).all()
    srt = np.sort(got["record"], axis=1)
    assert ((srt[:, 1:] != srt[:, :-1]) | (srt[:, 1:] == nn.ID_NONE)).all(), "no duplicate record in a row"
    f = filled.sum(1)
    assert np.array_equal(st["pixels"], f) and np.array_equal(st["wsum"], f.astype(np.uint64) << np.uint64(24))
    assert np.array_equal(st["wmax"][f > 0], got["dist2"][f > 0, f[f > 0] - 1]) and (st["wmax"][f == 0] == 0).all()


# ---- 7. the chains ----------------------------------------------------------------------------------------------------------------------------------
def test_scales_from_the_three_nearest_points_then_build_records(gs4d):
    """points -> nearest_neighbours(k = 3) -> knn_mean_dist2 -> build_records with those scales: the records of the host builder on scales
    computed from the host definition's hits"""
    n, r = 1000, 12.0
    rng = np.random.default_rng(0x4E72)
    pos = (nc._uniform3(n, 0x4E73) * 80.0 - 40.0).astype(f32)
    pos[-3:] = [(400.0, 0.0, 0.0), (0.0, -400.0, 0.0), (0.0, 0.0, 400.0)]                       # three points with nobody within r: the fallback r * r
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0], f32), (n, 1))
    rgba = rng.uniform(0.1, 0.9, (n, 4)).astype(f32)
    ones = np.ones((n, 3), f32)

    def scales(hit_array):
        d2 = gs4d.knn_mean_dist2(hit_array, radius=r)
        assert d2.dtype == f32 and d2.shape == (n,)
        return np.repeat(np.sqrt(d2)[:, None], 3, 1).astype(f32)

    host_hits = gs4d.hits_of(gs4d.nearest_neighbours_host(gs4d.build_records_3d(pos, rot, ones, rgba), r, k=3, with_stats=False)[0], 3)
    want_scales = scales(host_hits)
    assert (want_scales[-3:] == f32(r)).all() and (want_scales[:-3] < f32(r)).all() and (host_hits["record"][:-3, 2] != nn.ID_NONE).sum() > n // 2
    ctx = gs4d.Context(W, H)
    bpos, brot, brgba, bscale = ctx.buffer(pos), ctx.buffer(rot), ctx.buffer(rgba), ctx.buffer(ones)
    points = ctx.build_records(gs4d.PARAMS_3D, n, pos=bpos, rot=brot, scale=bscale, rgba=brgba)
    hits = ctx.nearest_neighbours(n, points, r, k=3)
    got_hits = ctx.read_hits(hits, n, 3)
    assert got_hits.tobytes() == host_hits.tobytes()
    ctx.subdata(bscale, scales(got_hits))
    built = ctx.build_records(gs4d.PARAMS_3D, n, pos=bpos, rot=brot, scale=bscale, rgba=brgba)
    got = ctx.read(built, f32, n * 24).reshape(n, 24)
    want = gs4d.build_records_3d(pos, rot, want_scales, rgba)
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    ctx.finish()
    ctx.close()


def fibonacci_sphere(count, radius):
    i = np.arange(count) + 0.5
    z = 1.0 - 2.0 * i / count
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)


def test_floaters_where_density_varies_sparse_records_then_stat_cut_then_compact_records(gs4d):
    """A dense blob (600 points within 2 of the origin, spacing about 0.3), a sparse shell (300 points evenly on the sphere of radius 30, spacing
    about 6) and five planted outliers 14 from the origin, 12 from the blob and 16 from the shell: their third neighbour is farther than anybody
    else's.  isolated(r, 3) does not give them at a radius that fits the blob (0.5, 1, 2: the whole shell is marked too) nor at one that fits the
    shell with a margin (25, 40: the outliers reach the blob, nothing is marked) — only a radius between the shell's spacing and 12 would, which
    is knowing the answer.  sparse_records -> stat_cut over wmax with a budget of 5 -> compact_records gives exactly the planted indices."""
    k, r = 3, 25.0
    blob = (nc._uniform3(600, 0x4E74) * 2.0 - 1.0) * (2.0 / np.sqrt(3.0))
    pos = np.concatenate([blob, fibonacci_sphere(305, 30.0)])
    n = pos.shape[0]
    planted = np.array([3, 250, 251, 640, 904])
    pos[planted] = [(14.0, 0.0, 0.0), (-14.0, 0.5, 0.0), (0.0, 14.0, 0.25), (0.0, -14.0, 0.0), (0.5, 0.0, 14.0)]
    rec = nc.static_records(pos)
    rec[:, 7], rec[:, 3] = 0.9, 0.0                             # nobody is hidden or dead: every record takes part
    for radius in (0.5, 1.0, 2.0, 25.0, 40.0):                  # the premise, on the CPU
        c = nc.host(rec, 0.0, radius, k, 0, nc.table("zero", n))["pixels"]
        lonely = np.flatnonzero(c < k)
        assert not np.array_equal(lonely, planted), radius
        assert lonely.size == 0 or lonely.size > 100, radius
    host_h, host_s = nn.host(rec, 0.0, r, k, 0, nn.sentinel_hits(n, 32), nc.table("zero", n))
    assert np.array_equal(np.sort(np.argsort(host_s["wmax"], kind="stable")[-5:]), planted) and (host_s["pixels"] == k).all()
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(rec)
    hits, stats = ctx.sparse_records(n, data, r, k)
    value, above, equal = ctx.read_stat_cut(ctx.stat_cut(stats, n, 5, "wmax"))
    assert above + equal == 5
    kept_index = fill(ctx, 4 * n)
    count = ctx.compact_records(stats, n, kept_index=kept_index, min_pixels=0, min_wmax=float(np.array([value], np.uint32).view(f32)[0]))
    assert ctx.read_compact_count(count) == (planted.size, planted.size)
    assert np.array_equal(ctx.read(kept_index, np.uint32, planted.size), planted)
    assert ctx.read(stats, nc.STAT, n).tobytes() == host_s.tobytes()
    assert np.array_equal(ctx.read_hits(hits, n, k).view(nn.HIT), nn.slots(host_h, k))
    ctx.finish()
    ctx.close()


def test_neighbour_lists_are_symmetric_without_truncation(gs4d):
    """source == 0, k = 16 and a set whose rows never fill: j is a hit of i iff i is a hit of j"""
    case = nc.case("cube", 4097)
    n = case.n
    ctx = gs4d.Context(W, H)
    hits = ctx.nearest_neighbours(n, ctx.buffer(case.rec), case.r, k=16)
    got = ctx.read_hits(hits, n, 16)
    ctx.finish()
    ctx.close()
    filled = got["record"] != nn.ID_NONE
    assert not filled[:, 15].any() and filled.sum() > n, "no row is full: nothing was truncated"
    i, j = np.broadcast_to(np.arange(n)[:, None], filled.shape)[filled], got["record"][filled].astype(np.int64)
    pairs = set(zip(i.tolist(), j.tolist()))
    assert len(pairs) == i.size and all((b, a) in pairs for a, b in pairs)
    d2 = dict(zip(zip(i.tolist(), j.tolist()), got["dist2"].view(np.uint32)[filled].tolist()))
    assert all(d2[(a, b)] == d2[(b, a)] for a, b in pairs), "dist2 is symmetric bit for bit"
