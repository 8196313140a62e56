"""GPU: gs4d_count_neighbours — for every record the number of source records whose centre lies within a radius of its own, as rows of a
record-statistics table (include/gs4d.h).

The table is checked against gs4d_host_count_neighbours, the brute-force definition (which tests/test_neighbours_host.py pins to the numpy
restatement of the header's text on the CPU, from the same generator, together with the premises: rows of c == 0, of 0 < c < cap and saturated rows
in every kind, pairs at exactly r, buckets shared inside a query range and between occupied cells), with guard buffers around data, source and
stats; the call orders itself with draws that add to the source table and with later uploads, re-uses its scratch at other sizes, never builds a
shadow, and closes the two chains: floaters (isolated -> compact_records) and grow (select_volume -> grow_selection -> measure_records).  All calls
go through the Python binding over the C ABI; contexts are 64 x 48."""
import ctypes

import numpy as np
import pytest

import centre_cases as cc
import edit_cases as ec
import measure_cases as mc
import neighbour_cases as nc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
f32 = np.float32
W, H = nc.W, nc.H


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


class Bench:
    """the buffers of one record set between sentinel guard buffers: data (the n records, EXTRA more behind them — copies of the first ones, so
    they would be neighbours of those if they were looked at — and a sentinel tail), a source table of n rows with EXTRA rows behind them that
    pass every rule of these tests, and a stats table of exactly n rows"""

    def __init__(self, ctx, case):
        self.ctx, self.case, self.n = ctx, case, case.n
        held = np.concatenate([case.rec, np.resize(case.rec, (nc.EXTRA, 24))])
        self.host_data = np.concatenate([held.view(np.uint8).reshape(-1), np.full(GUARD, SENTINEL, np.uint8)])
        self.g0, self.data, self.g1 = fill(ctx, GUARD), ctx.buffer(self.host_data), fill(ctx, GUARD)
        self.source, self.g2 = ctx.buffer(nbytes=16 * (self.n + nc.EXTRA)), fill(ctx, GUARD)
        self.stats, self.g3 = ctx.buffer(nbytes=max(16, 16 * self.n)), fill(ctx, GUARD)
        self.src_form = None

    def check(self, form, cap, flags, prefilled, what):
        """one call: the table against the host definition; returns the rows"""
        c, case, n = self.ctx, self.case, self.n
        source, rule, invert = nc.selection(n, form)
        if source is not None and form != self.src_form:
            self.src_all = np.concatenate([source, ec.mask_table(np.full(nc.EXTRA, not invert), rule)])
            c.subdata(self.source, self.src_all)
            self.src_form = form
        table = nc.table("random" if prefilled else "zero", n)
        c.subdata(self.stats, table)
        kw = ec.rule_keywords(rule, invert) if source is not None else {}
        c.count_neighbours(self.stats, n, self.data, source=self.source if source is not None else None, query=nc.struct(case.t, case.r, cap, flags), **kw)
        got = c.read(self.stats, nc.STAT, n)
        want = nc.host(case.rec, case.t, case.r, cap, flags, table, source, rule, invert)
        assert got.tobytes() == want.tobytes(), f"{what}: rows {np.flatnonzero(got != want)[:8]}\n{got[got != want][:4]}\n{want[got != want][:4]}"
        return got

    def check_the_rest(self, what):
        c = self.ctx
        assert all(untouched(c, g) for g in (self.g0, self.g1, self.g2, self.g3)), f"{what}: a guard buffer changed"
        assert np.array_equal(c.read(self.data, np.uint8, self.host_data.size), self.host_data), f"{what}: data changed"
        if self.src_form is not None:
            assert c.read(self.source, nc.STAT, self.n + nc.EXTRA).tobytes() == self.src_all.tobytes(), f"{what}: the source table changed"

    def delete(self):
        for b in (self.g0, self.data, self.g1, self.source, self.g2, self.stats, self.g3):
            self.ctx.delete(b)


# ---- 1. bits, 2. nothing else is written ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", nc.KINDS)
def test_the_table_equals_the_host_definition_byte_for_byte(gs4d, kind):
    """every size, source form, cap and flag combination, into a zeroed and into a pre-filled table (rows of pixels at 2^32 - 1 among them)"""
    ctx = gs4d.Context(W, H)
    counted = 0
    for n in nc.SIZES:
        b = Bench(ctx, nc.case(kind, n))
        for k, (_, form, cap, flags) in enumerate(nc.matrix((n,))):
            prefilled = k % 2 == 1
            got = b.check(form, cap, flags, prefilled, f"{kind}, n = {n}, {form}, cap = {cap}, flags = {flags}")
            counted += 0 if prefilled else int(got["pixels"].astype(np.int64).sum())
        b.check_the_rest(f"{kind}, n = {n}")
        b.delete()
    assert counted > 0
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_hostile_record_sets(gs4d):
    ctx = gs4d.Context(W, H)
    counted = 0
    for k, case in enumerate(nc.hostile_sets()):
        b = Bench(ctx, case)
        for j, form in enumerate(nc.FORMS):
            for flags in (nc.FLAGS if (k + j) % 5 == 0 else (0, 7)):
                got = b.check(form, nc.CAPS[(k + j + flags) % 3], flags, (k + j) % 2 == 0, f"{case.name}, {form}, flags = {flags}")
                counted += int(got["pixels"].astype(np.int64).sum())
        b.check_the_rest(case.name)
        b.delete()
    assert counted > 0
    ctx.finish()
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(W, H)
    data, source, stats = fill(ctx, 96 * 4), fill(ctx, 64), fill(ctx, 64)
    ctx.count_neighbours(stats, 0, data, 1.0)
    ctx.count_neighbours(stats, 0, data, 1.0, source=source, count_self=True, min_pixels=1)
    ctx.finish()
    assert untouched(ctx, data, 96 * 4) and untouched(ctx, source, 64) and untouched(ctx, stats, 64)
    ctx.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_as_it_was(gs4d):
    case = nc.case("cube", 257)
    n = case.n
    ctx, lib = gs4d.Context(W, H), gs4d._lib
    src_table, rule, _ = nc.selection(n, "rule")
    table = nc.table("random", n)
    data, source, stats = ctx.buffer(case.rec), ctx.buffer(src_table), ctx.buffer(table)
    short_data, short_source, short_stats, dead = ctx.buffer(case.rec.reshape(-1)[:-1]), ctx.buffer(src_table[:-1]), ctx.buffer(table[:-1]), fill(ctx, 64)
    ctx.delete(dead)
    NO = object()
    good_rule = gs4d._keep_rule(**ec.rule_keywords(rule))

    def call(data=data, n=n, q=None, source=source, rule=good_rule, stats=stats, r=case.r, cap=3, flags=7, reserved=None, rule_flags=None, rule_reserved=None):
        s = nc.struct(case.t, r, cap, flags)
        if reserved is not None:
            s.reserved[reserved] = 1
        k = None if rule is None else rule.copy()
        if rule_flags is not None:
            k["flags"] = rule_flags
        if rule_reserved is not None:
            k["reserved"] = rule_reserved
        return lib.gs4d_count_neighbours(ctx._h, data, ctypes.c_size_t(n), None if q is NO else ctypes.byref(s), source, None if k is None else k.ctypes.data, stats)

    bad = {
        "query == NULL": dict(q=NO), "flag 8": dict(flags=8 | 1), "flag bit 31": dict(flags=0x80000000), "cap == 0": dict(cap=0),
        **{f"reserved[{k}]": dict(reserved=k) for k in range(4)},
        "r = 0": dict(r=0.0), "r < 0": dict(r=-1.0), "r = NaN": dict(r=np.nan), "r = inf": dict(r=np.inf), "r * r overflows": dict(r=2.0 ** 64),
        "r * r below FLT_MIN": dict(r=float(np.nextafter(f32(2.0 ** -63), f32(0.0)))),
        "n == 0xFFFFFFFF": dict(n=0xFFFFFFFF), "n > 0xFFFFFFFF": dict(n=1 << 32), "no data": dict(data=0), "dead data": dict(data=dead),
        "unknown data": dict(data=9999), "no stats": dict(stats=0), "dead stats": dict(stats=dead), "unknown stats": dict(stats=9999),
        "data too small": dict(data=short_data), "stats too small": dict(stats=short_stats), "source without a rule": dict(rule=None),
        "a rule without source": dict(source=0), "rule flag 2": dict(rule_flags=2), "rule reserved": dict(rule_reserved=1),
        "dead source": dict(source=dead), "unknown source": dict(source=9999), "source too small": dict(source=short_source),
        "data == stats": dict(stats=data), "data == source": dict(source=data), "source == stats": dict(source=stats),
        "data == stats without a source": dict(stats=data, source=0, rule=None),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    assert call(n=0, flags=8) == -1 and call(n=0, stats=dead) == -1 and call(n=0, r=0.0) == -1      # ... with no records too
    ctx.finish()
    assert ctx.read(stats, nc.STAT, n).tobytes() == table.tobytes(), "a refused call wrote something"
    assert ctx.read(short_stats, nc.STAT, n - 1).tobytes() == table[:-1].tobytes()
    assert np.array_equal(ctx.read(data, f32, n * 24).view(np.uint32), case.rec.reshape(-1).view(np.uint32))
    assert ctx.read(source, nc.STAT, n).tobytes() == src_table.tobytes()
    # the call works after the refusals, at the ends of the radius range too
    assert call() == 0
    want = nc.host(case.rec, case.t, case.r, 3, 7, table, src_table, rule, False)
    assert ctx.read(stats, nc.STAT, n).tobytes() == want.tobytes() and want.tobytes() != table.tobytes()
    for r in (2.0 ** -63, float(np.nextafter(f32(2.0 ** 64), f32(0.0)))):
        ctx.subdata(stats, table)
        assert call(source=0, rule=None, r=r, flags=4, cap=0xFFFFFFFF) == 0
        assert ctx.read(stats, nc.STAT, n).tobytes() == nc.host(case.rec, case.t, r, 0xFFFFFFFF, 4, table).tobytes()
    ctx.finish()
    ctx.close()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------------------------
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
    want = nc.host(rec, tc.T, r, 0xFFFFFFFF, nc.COUNT_SELF, zero, drawn, rule, False)
    assert want.tobytes() != nc.host(rec, tc.T, r, 0xFFFFFFFF, nc.COUNT_SELF, zero, zero, rule, False).tobytes()
    # the same draw; the next lane; the call by the draw's table — nothing read or finished in between; then uploads right behind the call
    src, out = c.record_stats(n), c.record_stats(n)
    tc.stats_frame(s, src, 1)
    c.clear()                                                   # a new frame: the call is queued on another lane than the draw
    c.count_neighbours(out, n, s.db, r, t=tc.T, source=src, count_self=True, **ec.rule_keywords(rule))
    c.subdata(src, np.zeros(n, ec.STAT))
    c.subdata(s.db, np.zeros_like(rec))
    got = c.read(out, nc.STAT, n)
    assert got.tobytes() == want.tobytes(), f"rows {np.flatnonzero(got != want)[:8]}"
    assert c.shadow_builds(s.db) == builds, "the call built or invalidated a shadow"
    c.finish()
    c.close()


def test_the_scratch_is_re_used_at_other_sizes(gs4d):
    """large, then small, then large again on one lane: the layout of the scratch (candidates, table, keys) depends on n"""
    ctx = gs4d.Context(W, H)
    for kind, n, form, cap, flags in (("4d", 4097, "rule", 3, 7), ("cube", 65, "all", 0xFFFFFFFF, 4), ("twins", 2, "all", 1, 4), ("lattice", 4097, "inverted", 0xFFFFFFFF, 0),
                                      ("far", 257, "all", 3, 5), ("cube", 4097, "all", 0xFFFFFFFF, 4)):
        b = Bench(ctx, nc.case(kind, n))
        got = b.check(form, cap, flags, False, f"{kind}, n = {n}")
        assert n == 2 or got["pixels"].any()
        b.check_the_rest(f"{kind}, n = {n}")
        b.delete()
    ctx.finish()
    ctx.close()


def test_a_size_of_several_sort_tiles_and_three_radix_passes(gs4d):
    """n = 70001.  A dense cube with cap 3 against the host definition (its double loop ends early), and the lattice without a cap against
    neighbour_cases.lattice_counts (the reasoning is there; the host test pins it to the host definition at n = 4097).
    Which sort runs: the call sorts kb + 1 = 19 key bits on the lane's pair_sort scratch with a histogram launch of its own (k_os_hist).  19 bits
    are inside the spans the MSD/LSD hybrid is planned for, but that scratch plans the hybrid only when GS4D_SORT_HYBRID asks for it: with the
    variable unset, as here, this is k_os_hist and three 8-bit LSD passes.  tests/test_gpu_sort_hybrid_edges.py runs the same calls with the
    hybrid on (local digits of 5 + 5 bits, slow buckets) and off and compares the tables."""
    n = nc.N_BIG
    assert nc.bucket_bits(n) + 1 == 19 and n > 8 * 8192
    ctx = gs4d.Context(W, H)
    b = Bench(ctx, nc.dense_case())
    for form, flags in (("rule", nc.COUNT_SELF | nc.SKIP_HIDDEN), ("all", nc.SKIP_DEAD)):
        got = b.check(form, 3, flags, True, f"dense, {form}")
        part = nc.takes_part(b.case.rec, 0.0, flags)[0]
        assert (got["pixels"][~part] == nc.table("random", n)["pixels"][~part]).all() and part.sum() < n
    b.check_the_rest("dense")
    b.delete()
    case = nc.case("lattice", n)
    data, stats = ctx.buffer(case.rec), ctx.record_stats(n)
    ctx.count_neighbours(stats, n, data, case.r)
    c = nc.lattice_counts(n)
    want = np.zeros(n, nc.STAT)
    want["pixels"], want["wmax"], want["wsum"] = c, np.where(c > 0, nc.ONE_BITS, 0), c.astype(np.uint64) << np.uint64(24)
    assert ctx.read(stats, nc.STAT, n).tobytes() == want.tobytes() and c.min() >= 1 and (c == 6).sum() > n // 2
    ctx.finish()
    ctx.close()


# ---- 5. the chains -------------------------------------------------------------------------------------------------------------------------------
def test_floaters_isolated_then_compact_records_gives_the_planted_records(gs4d):
    n, k, r = 1000, 2, 20.0
    planted = np.array([3, 250, 251, 640, 999])
    pos = nc._uniform3(n, 0x4E36) * 80.0 - 40.0
    pos[planted] = [(500.0, 500.0, 500.0), (-500.0, 500.0, 0.0), (500.0, -500.0, 100.0), (-500.0, -500.0, -500.0), (0.0, 900.0, 0.0)]
    rec = nc.static_records(pos)
    c_host = nc.host(rec, 0.0, r, k, 0, nc.table("zero", n))["pixels"]
    assert np.array_equal(np.flatnonzero(c_host < k), planted) and (c_host[planted] == 0).all()      # the premise: nobody else is that lonely
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(rec)
    stats = ctx.isolated(n, data, r, k)
    kept_index = fill(ctx, 4 * n)
    count = ctx.compact_records(stats, n, kept_index=kept_index, min_pixels=k, invert=True)
    assert ctx.read_compact_count(count) == (planted.size, planted.size)
    assert np.array_equal(ctx.read(kept_index, np.uint32, planted.size), planted)
    assert np.array_equal(ctx.read(stats, nc.STAT, n)["pixels"], c_host)
    # the other direction: the well-supported records
    count = ctx.compact_records(stats, n, min_pixels=k)
    assert ctx.read_compact_count(count)[0] == n - planted.size
    ctx.finish()
    ctx.close()


def test_grow_select_volume_then_grow_selection_then_measure_records(gs4d):
    n = 1000
    rec = cc.records("symmetric", n)
    sphere, r = ((5.0, -4.0, 3.0), 18.0), 7.0
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(rec)
    _, _, kept, a = ctx.select_volume(n, data, sphere=sphere, t=nc.T, skip_dead=True)
    a_host = gs4d.count_centres_host(rec, gs4d.centre_query(sphere=sphere, t=nc.T, skip_dead=True), W, H).view(nc.STAT)
    assert 10 < kept < n // 4 and kept == int((a_host["pixels"] > 0).sum())
    one = (1, 0, 0)
    source, grown = a, a_host
    for step in range(2):                                       # grow, then grow again from the result
        b = ctx.grow_selection(n, data, source, r, t=nc.T, skip_dead=True)
        b_host = nc.host(rec, nc.T, r, 1, nc.SKIP_DEAD | nc.COUNT_SELF, nc.table("zero", n), grown, one, False)
        assert ctx.read(b, nc.STAT, n).tobytes() == b_host.tobytes(), step
        before, after = ec.selected(n, grown, one), ec.selected(n, b_host, one)
        assert (after | ~before).all() and int(after.sum()) > int(before.sum()), "the grown set holds the selection and more"
        m = ctx.read(ctx.measure_records(data, n, t=nc.T, stats=b, min_pixels=1), mc.MEASURE, 1)
        m_host = mc.host(rec, nc.T, 0, b_host, one, False)
        assert m.tobytes() == m_host.tobytes() and int(m["count"][0]) == int(after.sum()), step
        source, grown = b, b_host
    ctx.finish()
    ctx.close()
