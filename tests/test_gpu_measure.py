"""GPU: gs4d_measure_records — the counts, the box of the centres, the box of what they reach and the cell sums of the centroid of selected records,
as one 96-byte gs4d_measure (include/gs4d.h).

The 96 bytes are checked against gs4d_host_measure_records (which tests/test_measure_host.py pins to the numpy restatement of the header's text on
the CPU, from the same generator) with guard buffers around data, table and out; the call re-uses an out buffer, orders itself with draws that add
to the table and with later uploads, never builds a shadow, and closes the chain select_volume -> measure -> hide -> measure.  All calls go through
the Python binding over the C ABI; contexts are 64 x 48."""
import ctypes

import numpy as np
import pytest

import centre_cases as cc
import edit_cases as ec
import measure_cases as mc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
f32 = np.float32
W, H = mc.W, mc.H


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD, offset=0):
    return bool((ctx.read(buf, np.uint8, nbytes, offset) == SENTINEL).all())


class Bench:
    """the buffers of one record set between sentinel guard buffers: data (the n records, EXTRA more behind them — copies of the first ones, so
    they would be measured if they were looked at — and a sentinel tail), a table of exactly n rows, and out: 96 bytes at the start of a larger
    sentinel-filled buffer of its own"""

    def __init__(self, ctx, rec):
        self.ctx, self.n = ctx, rec.shape[0]
        self.rec = np.ascontiguousarray(rec)
        held = np.concatenate([self.rec, np.resize(self.rec, (mc.EXTRA, 24))])
        self.host = np.concatenate([held.view(np.uint8).reshape(-1), np.full(GUARD, SENTINEL, np.uint8)])
        self.g0, self.data, self.g1 = fill(ctx, GUARD), ctx.buffer(self.host), fill(ctx, GUARD)
        self.stats, self.g2 = ctx.buffer(nbytes=max(16, 16 * self.n)), fill(ctx, GUARD)
        self.out, self.g3 = fill(ctx, 96 + GUARD), fill(ctx, GUARD)
        self.table = None

    def check(self, t, flags, sel, what):
        """one call: the 96 bytes against the host definition; returns the measurement"""
        c = self.ctx
        stats, rule, invert = sel
        if stats is not None and stats is not self.table:
            c.subdata(self.stats, stats)
            self.table = stats
        kw = ec.rule_keywords(rule, invert) if stats is not None else {}
        c.measure_records(self.data, self.n, stats=self.stats if stats is not None else None, out=self.out, query=mc.struct(t, flags), **kw)
        got = c.read(self.out, mc.MEASURE, 1)
        want = mc.host(self.rec, t, flags, stats, rule, invert)
        assert got.tobytes() == want.tobytes(), f"{what}:\n{got}\n{want}"
        return got[0]

    def check_the_rest(self, what):
        c = self.ctx
        assert all(untouched(c, g) for g in (self.g0, self.g1, self.g2, self.g3)), f"{what}: a guard buffer changed"
        assert untouched(c, self.out, GUARD, 96), f"{what}: bytes past the 96 of out changed"
        assert np.array_equal(c.read(self.data, np.uint8, self.host.size), self.host), f"{what}: data changed"
        if self.table is not None:
            assert c.read(self.stats, ec.STAT, self.n).tobytes() == self.table.tobytes(), f"{what}: the table changed"

    def delete(self):
        for b in (self.g0, self.data, self.g1, self.stats, self.g2, self.out, self.g3):
            self.ctx.delete(b)


# ---- 1. bits, 2. nothing else is written ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mc.KINDS)
def test_the_measurement_equals_the_host_definition_byte_for_byte(gs4d, kind):
    """every combination of the flags, every selection form, every time, every size (the premises — no case is vacuous — are
    tests/test_measure_host.py's, asserted on the CPU from the same generator)"""
    ctx = gs4d.Context(W, H)
    counted = 0
    for n in mc.SIZES:
        b = Bench(ctx, mc.records(kind, n))
        for form in mc.FORMS:
            sel = mc.selection(n, form)
            for t in mc.TIMES:
                for flags in mc.FLAGS:
                    counted += int(b.check(t, flags, sel, f"{kind}, n = {n}, t = {t}, flags = {flags}, {form}")["count"])
        b.check_the_rest(f"{kind}, n = {n}")
        b.delete()
    assert counted > 0
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_hostile_record_sets(gs4d):
    ctx = gs4d.Context(W, H)
    unplaced = 0
    for k, case in enumerate(mc.hostile_sets()):
        b = Bench(ctx, case.rec)
        for j, form in enumerate(mc.FORMS):
            sel = mc.selection(case.n, form)
            for flags in (mc.FLAGS if (k + j) % 3 == 0 else (0, 3)):
                unplaced += int(b.check(case.t, flags, sel, f"{case.name}, flags = {flags}, {form}")["unplaced"])
        b.check_the_rest(case.name)
        b.delete()
    assert unplaced > 0
    ctx.finish()
    ctx.close()


@pytest.mark.parametrize("n", (mc.N_PARTIALS, mc.N_STRIDE), ids=("more_partial_rows_than_final_threads", "a_thread_walks_two_records"))
def test_sizes_past_the_final_workgroup_and_past_the_capped_grid(gs4d, n):
    assert mc.N_PARTIALS > mc.THREADS * mc.THREADS and -(-mc.N_PARTIALS // mc.THREADS) <= mc.GROUPS      # THREADS + 1 workgroups, below the cap
    assert mc.N_STRIDE > mc.GROUPS * mc.THREADS + mc.THREADS                                              # a whole workgroup iterates twice, and one more thread
    ctx = gs4d.Context(W, H)
    b = Bench(ctx, mc.big_records(n))
    for form, t, flags in (("all", mc.T, 0), ("rule", mc.T, 3), ("inverted", mc.T - 0.25, 2)):
        m = b.check(t, flags, mc.selection(n, form), f"n = {n}, {form}")
        assert m["count"] > n // 8
    # one selected record in the last workgroup only, and one in the first only
    for index in (n - 1, 0):
        m = b.check(mc.T, 0, mc.one_selected(n, index), f"n = {n}, record {index} alone")
        assert m["count"] == 1 and np.array_equal(m["lo"], m["hi"]) and not m["cell_sum"].any()
    b.check_the_rest(f"n = {n}")
    b.delete()
    ctx.finish()
    ctx.close()


def test_one_selected_record_in_the_last_or_the_first_workgroup(gs4d):
    ctx = gs4d.Context(W, H)
    for n in (257, 4097):
        rec = mc.records("symmetric", n)
        assert rec[n - 1, 7] > 0 and rec[0, 7] > 0
        b = Bench(ctx, rec)
        for index in (n - 1, 0):
            m = b.check(mc.T - 0.25, 1, mc.one_selected(n, index), f"n = {n}, record {index} alone")
            want = cc.centre(rec[index:index + 1], mc.T - 0.25)[0][0]
            assert m["count"] == 1 and np.array_equal(m["lo"], want) and np.array_equal(m["hi"], want)
        b.check_the_rest(f"n = {n}")
        b.delete()
    ctx.finish()
    ctx.close()


def test_both_zeros_on_an_axis_and_no_records(gs4d):
    ctx = gs4d.Context(W, H)
    rec = np.zeros((300, 24), f32)
    rec[:, 8], rec[:, 13], rec[:, 18], rec[:, 23], rec[:, 7], rec[:, 20] = 1.0, 1.0, 1.0, 1.0, 1.0, -0.0
    rec[:, 0] = np.where(np.arange(300) % 2 == 0, f32(0.0), f32(-0.0))
    for order in (rec, rec[::-1].copy()):
        b = Bench(ctx, order)
        m = b.check(0.0, 0, (None, mc.RULE, False), "zeros")
        assert m["lo"][:1].view(np.uint32)[0] == 0x80000000 and m["hi"][:1].view(np.uint32)[0] == 0
        b.delete()
    data, out = fill(ctx, 96 * 4), fill(ctx, 96 + GUARD)
    ctx.measure_records(data, 0, t=1.0, skip_dead=True, out=out)
    empty = mc.host(rec[:0], 1.0, 2)
    assert ctx.read(out, mc.MEASURE, 1).tobytes() == empty.tobytes() and untouched(ctx, out, GUARD, 96) and untouched(ctx, data, 96 * 4)
    assert ctx.read_measure(out)["centre"] is None and ctx.read_measure(out)["lo"][0] == np.inf
    ctx.close()


# ---- 3. re-use -----------------------------------------------------------------------------------------------------------------------------------
def test_a_second_query_into_the_same_out_does_not_carry_the_first(gs4d):
    ctx = gs4d.Context(W, H)
    rec = mc.records("symmetric", 4097)
    data, out = ctx.buffer(rec), ctx.buffer(nbytes=96)
    first = mc.host(rec, mc.T, 0)
    second = mc.host(rec, mc.T - 0.25, 3, *mc.selection(4097, "rule"))
    assert first["cell_sum"].all() and second["cell_sum"].all() and first.tobytes() != second.tobytes()
    stats, rule, invert = mc.selection(4097, "rule")
    table = ctx.buffer(stats)
    ctx.measure_records(data, 4097, t=mc.T, out=out)
    ctx.measure_records(data, 4097, stats=table, out=out, query=mc.struct(mc.T - 0.25, 3), **ec.rule_keywords(rule, invert))      # back to back
    assert ctx.read(out, mc.MEASURE, 1).tobytes() == second.tobytes()
    ctx.measure_records(data, 4097, t=mc.T, out=out)
    d = ctx.read_measure(out)
    assert ctx.read(out, mc.MEASURE, 1).tobytes() == first.tobytes()
    assert d["count"] == int(first["count"][0]) and np.array_equal(d["cell_sum"], first["cell_sum"][0]) and d["centre"] is not None
    assert (d["lo"] <= d["centre"]).all() and (d["centre"] <= d["hi"]).all()
    ctx.close()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------------------------
def test_the_call_orders_itself_with_draws_that_add_to_the_table_and_with_later_uploads(gs4d):
    import test_gpu_centres as tc
    rec = tc.record_set(gs4d, "symmetric")
    n = rec.shape[0]
    s = tc.Scene(gs4d, rec)
    c = s.ctx
    assert c.stats()["lanes"] > 1
    s.frame(gs4d.MODE_4D_SORTED, 0)                             # the shadow exists and is current
    builds = c.shadow_builds(s.db)
    assert builds == 1
    # the draw alone, read back: the table the measurement has to see
    alone = c.record_stats(n)
    tc.stats_frame(s, alone, 1)
    drawn = c.read(alone, ec.STAT, n)
    rule = (1, 0, int(np.median(drawn["wsum"])))                # what the draw shows most of: about half of the set
    seen = ec.selected(n, drawn, rule)
    assert 0 < int(seen.sum()) < n
    want = mc.host(rec, tc.T, 0, drawn, rule, False)
    # the same draw, and — nothing read or finished in between — the measurement by its table; then uploads right behind the call
    t = c.record_stats(n)
    tc.stats_frame(s, t, 1)
    out = c.measure_records(s.db, n, t=tc.T, stats=t, **ec.rule_keywords(rule))
    c.subdata(t, np.zeros(n, ec.STAT))
    c.subdata(s.db, np.zeros_like(rec))
    got = c.read(out, mc.MEASURE, 1)
    assert got.tobytes() == want.tobytes(), f"\n{got}\n{want}"
    assert got["count"][0] == int(seen.sum())
    assert c.shadow_builds(s.db) == builds, "the call built or invalidated a shadow"
    c.subdata(s.db, rec)
    # a current shadow stays current through the call, on the next lane too
    s.frame(gs4d.MODE_4D_SORTED, 0)
    builds = c.shadow_builds(s.db)
    c.clear()
    out2 = c.measure_records(s.db, n, t=tc.T, skip_hidden=True, skip_dead=True)
    assert c.read(out2, mc.MEASURE, 1).tobytes() == mc.host(rec, tc.T, 3).tobytes()
    s.frame(gs4d.MODE_4D_SORTED, 1)
    s.read()
    assert c.shadow_builds(s.db) == builds, "the call made the shadow stale"
    c.finish()
    c.close()


def test_a_queued_keygen_that_names_the_table_runs_first(gs4d):
    """a key generation whose key buffer is then used as the table: the keys are written before the call reads them"""
    rec = cc.records("symmetric", 1000)
    n = 250                                                     # 4 n key bytes = n / 4 rows
    twin = gs4d.Context(W, H)
    d2, k2, i2 = twin.buffer(rec), twin.buffer(nbytes=16 * n), twin.buffer(nbytes=4 * 4 * n)
    twin.keygen(d2, mc.T, cc.CAM[0], k2, i2, 4 * n)
    keys = twin.read(k2, ec.STAT, n)
    twin.close()
    rule = (int(np.median(keys["pixels"])), 0, 0)
    assert 0 < int(ec.selected(n, keys, rule).sum()) < n
    ctx = gs4d.Context(W, H)
    data, kb, ib = ctx.buffer(rec), ctx.buffer(nbytes=16 * n), ctx.buffer(nbytes=4 * 4 * n)
    ctx.keygen(data, mc.T, cc.CAM[0], kb, ib, 4 * n)            # queued, not launched
    out = ctx.measure_records(data, n, t=mc.T, stats=kb, **ec.rule_keywords(rule))
    assert ctx.read(out, mc.MEASURE, 1).tobytes() == mc.host(rec[:n], mc.T, 0, keys, rule, False).tobytes()
    ctx.close()


# ---- 5. the chain --------------------------------------------------------------------------------------------------------------------------------
def test_select_volume_then_measure_then_hide_then_measure(gs4d):
    import test_gpu_centres as tc
    rec = tc.record_set(gs4d, "symmetric")
    n = rec.shape[0]
    assert np.isfinite(rec).all() and (rec[:, 23] > 0).all() and (rec[:, 7] > 0).all()
    box = ((-30.0, -40.0, -20.0), (20.0, 20.0, 40.0))
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(rec)
    _, kept_index, kept, stats = ctx.select_volume(n, data, box=box, t=tc.T)
    assert n // 5 <= kept <= 4 * n // 5
    m = ctx.read_measure(ctx.measure_records(data, n, t=tc.T, stats=stats, min_pixels=1))
    assert m["count"] == kept and m["unplaced"] == 0 and m["skipped"] == 0
    assert (m["lo"] >= np.array(box[0], f32)).all() and (m["hi"] <= np.array(box[1], f32)).all() and (m["lo"] < m["hi"]).all()
    assert (m["ext_lo"] < m["lo"]).all() and (m["ext_hi"] > m["hi"]).all()
    inside = cc.takes_part(rec, cc.query(cc.BOX, t=tc.T, box_lo=box[0], box_hi=box[1]))
    mean = cc.centre(rec[inside], tc.T)[0].astype(np.float64).mean(0)
    assert (np.abs(m["centre"].astype(np.float64) - mean) <= (m["hi"].astype(np.float64) - m["lo"]) * 2.0 ** -19).all()
    ctx.hide(data, n, stats, min_pixels=1)
    m2 = ctx.read_measure(ctx.measure_records(data, n, t=tc.T, stats=stats, skip_hidden=True, min_pixels=1))
    assert m2["count"] == 0 and m2["skipped"] == kept and m2["centre"] is None and m2["lo"][0] == np.inf
    # the complement is still there
    m3 = ctx.read_measure(ctx.measure_records(data, n, t=tc.T, skip_hidden=True))
    assert m3["count"] == n - kept and m3["skipped"] == kept
    ctx.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_as_it_was(gs4d):
    n = 300
    ctx, lib = gs4d.Context(W, H), gs4d._lib
    rec = mc.records("symmetric", n)
    table, rule, _ = mc.selection(n, "rule")
    data, stats, out = ctx.buffer(rec), ctx.buffer(table), fill(ctx, 96 + GUARD)
    short_data, short_stats, short_out, dead = ctx.buffer(rec.reshape(-1)[:-1]), ctx.buffer(table[:-1]), fill(ctx, 95), fill(ctx, 64)
    ctx.delete(dead)
    NO = object()
    good_rule = gs4d._keep_rule(**ec.rule_keywords(rule))

    def call(data=data, n=n, q=None, stats=stats, rule=good_rule, out=out, flags=3, reserved=(0, 0), rule_flags=None, rule_reserved=None):
        s = mc.struct(mc.T, flags)
        s.reserved[0], s.reserved[1] = reserved
        k = None if rule is None else rule.copy()
        if rule_flags is not None:
            k["flags"] = rule_flags
        if rule_reserved is not None:
            k["reserved"] = rule_reserved
        return lib.gs4d_measure_records(ctx._h, data, ctypes.c_size_t(n), None if q is NO else ctypes.byref(s), stats,
                                        None if k is None else k.ctypes.data, out)

    bad = {
        "query == NULL": dict(q=NO), "flag 4": dict(flags=4 | 1), "flag bit 31": dict(flags=0x80000000), "reserved[0]": dict(reserved=(1, 0)),
        "reserved[1]": dict(reserved=(0, 7)), "n > 0xFFFFFFFF": dict(n=1 << 32), "no data": dict(data=0), "dead data": dict(data=dead),
        "unknown data": dict(data=9999), "no out": dict(out=0), "dead out": dict(out=dead), "unknown out": dict(out=9999),
        "data too small": dict(data=short_data), "out too small": dict(out=short_out), "stats without a rule": dict(rule=None),
        "a rule without stats": dict(stats=0), "rule flag 2": dict(rule_flags=2), "rule reserved": dict(rule_reserved=1),
        "dead stats": dict(stats=dead), "unknown stats": dict(stats=9999), "stats too small": dict(stats=short_stats),
        "data == out": dict(out=data), "data == stats": dict(stats=data), "stats == out": dict(out=stats),
        "data == out without a table": dict(out=data, stats=0, rule=None),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    assert call(n=0, flags=4) == -1 and call(n=0, out=dead) == -1                   # ... with no records too
    ctx.finish()
    assert untouched(ctx, out, 96 + GUARD) and untouched(ctx, short_out, 95), "a refused call wrote something"
    assert np.array_equal(ctx.read(data, f32, n * 24).view(np.uint32), rec.reshape(-1).view(np.uint32))
    assert ctx.read(stats, ec.STAT, n).tobytes() == table.tobytes()
    # the call works after the refusals
    assert call() == 0
    assert ctx.read(out, mc.MEASURE, 1).tobytes() == mc.host(rec, mc.T, 3, table, rule, False).tobytes() and untouched(ctx, out, GUARD, 96)
    assert call(stats=0, rule=None, flags=0) == 0
    assert ctx.read(out, mc.MEASURE, 1).tobytes() == mc.host(rec, mc.T, 0).tobytes()
    ctx.close()
