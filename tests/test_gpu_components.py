"""GPU: gs4d_label_components — one label per record, the smallest record index of its connected component, and optionally the component's size as
rows of a record-statistics table — and gs4d_count_labels, the records whose label a seed selection touches (include/gs4d.h).

Labels and tables are checked byte for byte against gs4d_host_label_components / gs4d_host_count_labels, the brute-force definitions (which
tests/test_components_host.py pins to a numpy restatement on the CPU, from the same generators, together with the premises: the component sizes
of every construction, pairs at exactly r and at the next float above it, the bridge record that is no member, the clumps isolated() does not
flag), with guard buffers around data, source, labels and stats and records behind n that would join components if they were looked at.  The
calls order themselves with draws that add to the source table and with later uploads, re-use the lane's scratch at other sizes and between
gs4d_count_neighbours calls, never build a shadow, and close the two chains: floater clumps (small_components -> compact_records) and select
connected (count_centres -> select_connected -> measure_records).  All calls go through the Python binding over the C ABI; contexts are 64 x 48."""
import ctypes
import functools

import numpy as np
import pytest

import component_cases as cp
import edit_cases as ec
import measure_cases as mc
import neighbour_cases as nc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
f32 = np.float32
W, H = cp.W, cp.H


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def host_once(sc, form_or_own, flags, cap, prefilled):
    """the host definition of one call, computed once and shared (the arrays are read-only)"""
    source, rule, invert = sc.selection if form_or_own == "own" else nc.selection(sc.n, form_or_own)
    labels, table = cp.host(sc.case.rec, sc.case.t, sc.case.r, cap, flags, cp.table(prefilled, sc.n), source, rule, invert)
    labels.setflags(write=False)
    return labels, table


class Bench:
    """the buffers of one record set between sentinel guard buffers: data (the n records, EXTRA more behind them — copies of the first ones, which
    would join the components of those if they were looked at — and a sentinel tail), a source table of n rows with EXTRA rows behind them that
    pass every rule of these tests, n label words with EXTRA sentinel words behind them, and a stats table of exactly n rows"""

    def __init__(self, ctx, sc):
        self.ctx, self.sc, self.case, self.n = ctx, sc, sc.case, sc.n
        held = np.concatenate([self.case.rec, np.resize(self.case.rec, (cp.EXTRA, 24))])
        self.host_data = np.concatenate([held.view(np.uint8).reshape(-1), np.full(GUARD, SENTINEL, np.uint8)])
        self.g0, self.data, self.g1 = fill(ctx, GUARD), ctx.buffer(self.host_data), fill(ctx, GUARD)
        self.source, self.g2 = ctx.buffer(nbytes=16 * (self.n + cp.EXTRA)), fill(ctx, GUARD)
        self.blank = np.full(self.n + cp.EXTRA, cp.SENTINEL_WORD, np.uint32)
        self.labels, self.g3 = ctx.buffer(self.blank), fill(ctx, GUARD)
        self.stats, self.g4 = ctx.buffer(nbytes=max(16, 16 * self.n)), fill(ctx, GUARD)
        self.src_key = None

    def check(self, form_or_own, flags, cap, prefilled, what, repeat=1):
        """one call (prefilled None: without a table): labels and table against the host definition; returns the labels"""
        c, case, n = self.ctx, self.case, self.n
        source, rule, invert = self.sc.selection if form_or_own == "own" else nc.selection(n, form_or_own)
        if source is not None and form_or_own != self.src_key:
            self.src_all = np.concatenate([source, ec.mask_table(np.full(cp.EXTRA, not invert), rule)])
            c.subdata(self.source, self.src_all)
            self.src_key = form_or_own
        want_l, want_t = host_once(self.sc, form_or_own, flags, cap, prefilled)
        table = cp.table(prefilled, n)
        kw = ec.rule_keywords(rule, invert) if source is not None else {}
        for k in range(repeat):                                 # the same call again gives the same bytes
            c.subdata(self.labels, self.blank)
            if table is not None:
                c.subdata(self.stats, table)
            c.label_components(n, self.data, source=self.source if source is not None else None, query=cp.struct(case.t, case.r, cap, flags),
                               labels=self.labels, stats=self.stats if table is not None else None, **kw)
            got_l = c.read(self.labels, np.uint32, n + cp.EXTRA)
            assert (got_l[n:] == cp.SENTINEL_WORD).all(), f"{what}: a word behind the n labels changed"
            assert got_l[:n].tobytes() == want_l.tobytes(), f"{what}, call {k}: labels {np.flatnonzero(got_l[:n] != want_l)[:8]}\n{got_l[:n][got_l[:n] != want_l][:8]}\n{want_l[got_l[:n] != want_l][:8]}"
            if table is not None:
                got_t = c.read(self.stats, cp.STAT, n)
                assert got_t.tobytes() == want_t.tobytes(), f"{what}, call {k}: rows {np.flatnonzero(got_t != want_t)[:8]}\n{got_t[got_t != want_t][:4]}\n{want_t[got_t != want_t][:4]}"
        return got_l[:n]

    def check_the_rest(self, what):
        c = self.ctx
        assert all(untouched(c, g) for g in (self.g0, self.g1, self.g2, self.g3, self.g4)), f"{what}: a guard buffer changed"
        assert np.array_equal(c.read(self.data, np.uint8, self.host_data.size), self.host_data), f"{what}: data changed"
        if self.src_key is not None:
            assert c.read(self.source, cp.STAT, self.n + cp.EXTRA).tobytes() == self.src_all.tobytes(), f"{what}: the source table changed"

    def delete(self):
        for b in (self.g0, self.data, self.g1, self.source, self.g2, self.labels, self.g3, self.stats, self.g4):
            self.ctx.delete(b)


def run_scenario(ctx, sc, repeat_first=1):
    """every call of a scenario (component_cases.calls), then the guards; returns (members, records in components of two and more)"""
    b = Bench(ctx, sc)
    members = linked = 0
    for k, (selection, flags, cap, prefilled) in enumerate(cp.calls(sc)):
        form = "own" if k == 0 else cp.COMBOS[k - 1][0]
        labels = b.check(form, flags, cap, prefilled, f"{sc}, {form}, flags = {flags}, cap = {cap}, table {prefilled}", repeat=repeat_first if k == 0 else 1)
        sizes = cp.component_sizes(labels)
        members += sum(sizes); linked += sum(s for s in sizes if s > 1)
    b.check_the_rest(str(sc))
    b.delete()
    return members, linked


# ---- 1. bits, 2. nothing else is written ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cp.SIZES)
def test_labels_and_table_equal_the_host_definition_byte_for_byte(gs4d, n):
    """every scenario of the size — chains in three index orders with and without the gap, the lattice at r and just below, the two bodies at
    both times, the four bridges, the cube, clump, twins, far and 4d sets — with its own call three times in a row, then every selection form,
    flag pair and cap, into a zeroed table, a pre-filled one (rows of pixels at 2^32 - 1 among them) and without a table"""
    ctx = gs4d.Context(W, H)
    members = linked = 0
    for sc in cp.by_size(n):
        m, l = run_scenario(ctx, sc, repeat_first=3)
        members += m; linked += l
    assert members > 0 and (n == 1 or linked > 0)
    ctx.finish()                                                # reports device-side check failures: a union-find trip bound among them
    ctx.close()


def test_the_contention_clump_and_the_clumps_of_every_size(gs4d):
    """256 records within r / 2 of each other — 32 640 edges hooking onto one root from within the same waves — and clumps of 1 .. 64 records
    with cap 1, 3 and none, into zeroed and pre-filled tables"""
    ctx = gs4d.Context(W, H)
    for sc in (cp.clump(), cp.clumps()):
        b = Bench(ctx, sc)
        for cap in (1, 3, cp.NOCAP):
            for prefilled in (False, True, None):
                labels = b.check("own", 0, cap, prefilled, f"{sc}, cap = {cap}, table {prefilled}", repeat=3 if cap == 1 else 1)
        assert cp.component_sizes(labels) == sc.sizes
        b.check_the_rest(str(sc))
        b.delete()
    ctx.finish()
    ctx.close()


def test_hostile_record_sets(gs4d):
    ctx = gs4d.Context(W, H)
    none = some = 0
    for k, case in enumerate(nc.hostile_sets()):
        sc = cp.Scenario(case.name, case.rec, case.t, case.r)
        b = Bench(ctx, sc)
        for j, form in enumerate(nc.FORMS):
            for flags in (0, 3):
                labels = b.check(form, flags, nc.CAPS[(k + j + flags) % 3], (None, False, True)[(k + j) % 3], f"{case.name}, {form}, flags = {flags}")
                none += int((labels == cp.NONE).sum()); some += int((labels != cp.NONE).sum())
        b.check_the_rest(case.name)
        b.delete()
    assert none > 0 and some > 0
    ctx.finish()
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(W, H)
    data, source, labels, stats, seeds = fill(ctx, 96 * 4), fill(ctx, 64), fill(ctx, 64), fill(ctx, 64), fill(ctx, 64)
    ctx.label_components(0, data, 1.0, labels=labels)
    ctx.label_components(0, data, 1.0, source=source, labels=labels, stats=stats, min_pixels=1)
    ctx.count_labels(stats, 0, labels, seeds)
    ctx.finish()
    assert untouched(ctx, data, 96 * 4) and all(untouched(ctx, b, 64) for b in (source, labels, stats, seeds))
    ctx.close()


def test_a_size_of_several_sort_tiles_and_three_radix_passes(gs4d):
    """n = 70001: the lattice cut into slabs by gaps wider than r, against component_cases.slab_labels — the smallest index of each slab (the
    reasoning is there; the host test pins it to the host definition at n = 4097; no 70001^2 host loop is run) — and the slab sizes in the rows"""
    n = cp.N_BIG
    assert nc.bucket_bits(n) + 1 == 19 and n > 8 * 8192
    sc = cp.slabs(n)
    ctx = gs4d.Context(W, H)
    b = Bench(ctx, sc)
    want_l = cp.slab_labels(n)
    size = np.bincount(want_l)[want_l]
    for cap, prefilled in ((cp.NOCAP, False), (5000, True)):
        table = nc.table("random" if prefilled else "zero", n)
        ctx.subdata(b.labels, b.blank)
        ctx.subdata(b.stats, table)
        ctx.label_components(n, b.data, sc.case.r, cap=cap, labels=b.labels, stats=b.stats)
        got = ctx.read(b.labels, np.uint32, n + cp.EXTRA)
        assert np.array_equal(got[:n], want_l) and (got[n:] == cp.SENTINEL_WORD).all(), np.flatnonzero(got[:n] != want_l)[:8]
        want_t = cp.add_fragments(table, np.arange(n), np.minimum(size, cap))
        assert ctx.read(b.stats, cp.STAT, n).tobytes() == want_t.tobytes()
    assert size.max() == 5 * 42 * 42 and np.unique(want_l).size == 8
    b.check_the_rest("slabs")
    b.delete()
    ctx.finish()
    ctx.close()


def test_the_scratch_is_re_used_at_other_sizes_and_between_count_neighbours_calls(gs4d):
    """large, then small, then large again on one lane, a gs4d_count_neighbours call — which lays the same scratch out for its own n — before each"""
    ctx = gs4d.Context(W, H)
    other = nc.case("cube", 257)
    o_data, o_stats = ctx.buffer(other.rec), ctx.record_stats(other.n)
    o_want = nc.host(other.rec, other.t, other.r, 3, 0, nc.table("zero", other.n))
    for sc, form, flags, cap, prefilled in ((cp.generic("4d", 4097), "rule", 3, 3, True), (cp.chain(65, "shuffled"), "own", 0, cp.NOCAP, False),
                                            (cp.generic("twins", 2), "all", 0, 1, None), (cp.lattice(4097), "own", 0, cp.NOCAP, True),
                                            (cp.bridge(257, "dead"), "own", cp.SKIP_DEAD, 3, False), (cp.chain(4097, "descending", True), "own", 0, cp.NOCAP, False)):
        ctx.subdata(o_stats, nc.table("zero", other.n))
        ctx.count_neighbours(o_stats, other.n, o_data, other.r, cap=3)
        b = Bench(ctx, sc)
        labels = b.check(form, flags, cap, prefilled, f"{sc}")
        assert (labels != cp.NONE).any()
        b.check_the_rest(str(sc))
        b.delete()
        assert ctx.read(o_stats, nc.STAT, other.n).tobytes() == o_want.tobytes()
    ctx.finish()
    ctx.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(gs4d):
    sc = cp.generic("cube", 257)
    case, n = sc.case, sc.n
    ctx, lib = gs4d.Context(W, H), gs4d._lib
    src_table, rule, _ = nc.selection(n, "rule")
    table = nc.table("random", n)
    blank = np.full(n, cp.SENTINEL_WORD, np.uint32)
    data, source, labels, stats = ctx.buffer(case.rec), ctx.buffer(src_table), ctx.buffer(blank), ctx.buffer(table)
    short_data, short_source, short_stats, short_labels = ctx.buffer(case.rec.reshape(-1)[:-1]), ctx.buffer(src_table[:-1]), ctx.buffer(table[:-1]), ctx.buffer(blank[:-1])
    dead = fill(ctx, 64)
    ctx.delete(dead)
    NO = object()
    good_rule = gs4d._keep_rule(**ec.rule_keywords(rule))

    def call(data=data, n=n, q=None, source=source, rule=good_rule, labels=labels, stats=stats, r=case.r, cap=3, flags=3, reserved=None, rule_flags=None,
             rule_reserved=None):
        s = cp.struct(case.t, r, cap, flags)
        if reserved is not None:
            s.reserved[reserved] = 1
        k = None if rule is None else rule.copy()
        if rule_flags is not None:
            k["flags"] = rule_flags
        if rule_reserved is not None:
            k["reserved"] = rule_reserved
        return lib.gs4d_label_components(ctx._h, data, ctypes.c_size_t(n), None if q is NO else ctypes.byref(s), source, None if k is None else k.ctypes.data,
                                         labels, stats)

    bad = {
        "query == NULL": dict(q=NO), "flag 4": dict(flags=4 | 1), "flag 8": dict(flags=8), "flag bit 31": dict(flags=0x80000000), "cap == 0": dict(cap=0),
        **{f"reserved[{k}]": dict(reserved=k) for k in range(4)},
        "r = 0": dict(r=0.0), "r < 0": dict(r=-1.0), "r = NaN": dict(r=np.nan), "r = inf": dict(r=np.inf), "r * r overflows": dict(r=2.0 ** 64),
        "r * r below FLT_MIN": dict(r=float(np.nextafter(f32(2.0 ** -63), f32(0.0)))),
        "n == 0xFFFFFFFF": dict(n=0xFFFFFFFF), "n > 0xFFFFFFFF": dict(n=1 << 32), "no data": dict(data=0), "dead data": dict(data=dead),
        "unknown data": dict(data=9999), "dead stats": dict(stats=dead), "unknown stats": dict(stats=9999),
        "no labels": dict(labels=0), "dead labels": dict(labels=dead), "unknown labels": dict(labels=9999), "labels too small": dict(labels=short_labels),
        "no labels and no stats": dict(labels=0, stats=0),
        "data too small": dict(data=short_data), "stats too small": dict(stats=short_stats), "source without a rule": dict(rule=None),
        "a rule without source": dict(source=0), "rule flag 2": dict(rule_flags=2), "rule reserved": dict(rule_reserved=1),
        "dead source": dict(source=dead), "unknown source": dict(source=9999), "source too small": dict(source=short_source),
        "data == stats": dict(stats=data), "data == source": dict(source=data), "source == stats": dict(source=stats),
        "data == labels": dict(labels=data), "labels == stats": dict(labels=stats), "labels == source": dict(labels=source),
        "labels == stats as the only table": dict(labels=stats, source=0, rule=None), "data == labels without stats": dict(labels=data, stats=0),
        "data == stats without a source": dict(stats=data, source=0, rule=None),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    assert call(n=0, flags=8) == -1 and call(n=0, labels=dead) == -1 and call(n=0, r=0.0) == -1 and call(n=0, stats=dead) == -1      # ... with no records too

    # gs4d_count_labels' own
    seeds = source

    def count(labels=labels, n=n, seeds=seeds, rule=good_rule, stats=stats, rule_flags=None, rule_reserved=None):
        k = None if rule is None else rule.copy()
        if rule_flags is not None:
            k["flags"] = rule_flags
        if rule_reserved is not None:
            k["reserved"] = rule_reserved
        return lib.gs4d_count_labels(ctx._h, labels, ctypes.c_size_t(n), seeds, None if k is None else k.ctypes.data, stats)

    bad = {
        "n > 0xFFFFFFFF": dict(n=1 << 32), "rule == NULL": dict(rule=None), "rule flag 2": dict(rule_flags=2), "rule reserved": dict(rule_reserved=1),
        "no labels": dict(labels=0), "dead labels": dict(labels=dead), "unknown labels": dict(labels=9999), "labels too small": dict(labels=short_labels),
        "no seeds": dict(seeds=0), "dead seeds": dict(seeds=dead), "unknown seeds": dict(seeds=9999), "seeds too small": dict(seeds=short_source),
        "no stats": dict(stats=0), "dead stats": dict(stats=dead), "unknown stats": dict(stats=9999), "stats too small": dict(stats=short_stats),
        "labels == seeds": dict(seeds=labels), "labels == stats": dict(stats=labels), "seeds == stats": dict(seeds=stats),
    }
    for what, kw in bad.items():
        assert count(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    assert count(n=0, rule=None) == -1 and count(n=0, stats=dead) == -1

    ctx.finish()
    assert ctx.read(stats, cp.STAT, n).tobytes() == table.tobytes(), "a refused call wrote something"
    assert ctx.read(short_stats, cp.STAT, n - 1).tobytes() == table[:-1].tobytes()
    assert np.array_equal(ctx.read(labels, np.uint32, n), blank) and np.array_equal(ctx.read(short_labels, np.uint32, n - 1), blank[:-1])
    assert np.array_equal(ctx.read(data, f32, n * 24).view(np.uint32), case.rec.reshape(-1).view(np.uint32))
    assert ctx.read(source, cp.STAT, n).tobytes() == src_table.tobytes()
    # the calls work after the refusals, at the ends of the radius range and without a table too
    assert call() == 0
    want_l, want_t = cp.host(case.rec, case.t, case.r, 3, 3, table, src_table, rule, False)
    assert ctx.read(labels, np.uint32, n).tobytes() == want_l.tobytes() and ctx.read(stats, cp.STAT, n).tobytes() == want_t.tobytes()
    assert want_t.tobytes() != table.tobytes()
    ctx.subdata(stats, table)
    assert count() == 0
    assert ctx.read(stats, cp.STAT, n).tobytes() == cp.host_count_labels(want_l, src_table, rule, False, table).tobytes()
    for r in (2.0 ** -63, float(np.nextafter(f32(2.0 ** 64), f32(0.0)))):
        ctx.subdata(stats, table)
        assert call(source=0, rule=None, r=r, flags=0, cap=0xFFFFFFFF, stats=0) == 0
        assert ctx.read(labels, np.uint32, n).tobytes() == cp.host(case.rec, case.t, r, 0xFFFFFFFF, 0)[0].tobytes()
        assert ctx.read(stats, cp.STAT, n).tobytes() == table.tobytes()
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
    want_l, want_t = cp.host(rec, tc.T, r, cp.NOCAP, 0, zero, drawn, rule, False)
    assert want_l.tobytes() != cp.host(rec, tc.T, r, cp.NOCAP, 0, zero, zero, rule, False)[0].tobytes()
    assert max(cp.component_sizes(want_l)) > 1
    # the same draw; the next lane; the call by the draw's table — nothing read or finished in between; then uploads right behind the call
    src, out, labels = c.record_stats(n), c.record_stats(n), c.buffer(np.full(n, cp.SENTINEL_WORD, np.uint32))
    tc.stats_frame(s, src, 1)
    c.clear()                                                   # a new frame: the call is queued on another lane than the draw
    c.label_components(n, s.db, r, t=tc.T, source=src, labels=labels, stats=out, **ec.rule_keywords(rule))
    c.subdata(src, np.zeros(n, ec.STAT))
    c.subdata(s.db, np.zeros_like(rec))
    got_l, got_t = c.read(labels, np.uint32, n), c.read(out, cp.STAT, n)
    assert got_l.tobytes() == want_l.tobytes(), f"labels {np.flatnonzero(got_l != want_l)[:8]}"
    assert got_t.tobytes() == want_t.tobytes(), f"rows {np.flatnonzero(got_t != want_t)[:8]}"
    assert c.shadow_builds(s.db) == builds, "the call built or invalidated a shadow"
    c.finish()
    c.close()


# ---- 5. gs4d_count_labels ------------------------------------------------------------------------------------------------------------------------
def test_count_labels_equals_the_host_definition(gs4d):
    """seed tables that hit no, one, several and all components, plain and inverted, into zeroed and pre-filled tables; labels as
    label_components left them, and with out-of-range words planted by upload; guards around the three buffers and rows behind n that would hit"""
    from test_components_host import SEEDS, HITS
    sc = cp.clumps()
    n, rule = sc.n, nc.RULE
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(sc.case.rec)
    g0, labels, g1 = fill(ctx, GUARD), ctx.buffer(np.full(n + cp.EXTRA, cp.SENTINEL_WORD, np.uint32)), fill(ctx, GUARD)
    seeds, g2, stats, g3 = ctx.buffer(nbytes=16 * (n + cp.EXTRA)), fill(ctx, GUARD), ctx.buffer(nbytes=16 * n), fill(ctx, GUARD)
    ctx.label_components(n, data, sc.case.r, labels=labels)
    made = ctx.read(labels, np.uint32, n)
    assert made.tobytes() == cp.host(sc.case.rec, 0.0, sc.case.r, cp.NOCAP, 0)[0].tobytes()
    planted = made.copy()
    planted[[5, 70, 300, 2000]] = (n, n + 5, 0xFFFFFFFE, cp.NONE)
    behind = np.array([0, 1, 2], np.uint32)                     # label words behind n: labels of real components, whose seed rows pass
    for lab in (made, planted):
        ctx.subdata(labels, np.concatenate([lab, behind]))
        for name, seeds_of in SEEDS.items():
            mask = seeds_of(lab, n)
            for invert in (False, True):
                seed_rows = np.concatenate([ec.mask_table(mask ^ invert, rule), ec.mask_table(np.full(cp.EXTRA, not invert), rule)])
                ctx.subdata(seeds, seed_rows)
                for prefilled in (False, True):
                    table = nc.table("random" if prefilled else "zero", n)
                    ctx.subdata(stats, table)
                    for _ in range(2):                          # nothing zeroes the table: the second call adds again
                        ctx.count_labels(stats, n, labels, seeds, **ec.rule_keywords(rule, invert))
                    once = cp.host_count_labels(lab, seed_rows[:n], rule, invert, table)
                    want = cp.host_count_labels(lab, seed_rows[:n], rule, invert, once)
                    got = ctx.read(stats, cp.STAT, n)
                    assert got.tobytes() == want.tobytes(), (name, invert, prefilled, np.flatnonzero(got != want)[:8])
                    assert int((once["pixels"] != table["pixels"]).sum()) == HITS[name](lab, n)
                assert ctx.read(seeds, cp.STAT, n + cp.EXTRA).tobytes() == seed_rows.tobytes()
        assert np.array_equal(ctx.read(labels, np.uint32, n + cp.EXTRA), np.concatenate([lab, behind]))
    assert all(untouched(ctx, g) for g in (g0, g1, g2, g3))
    ctx.finish()
    ctx.close()


# ---- 6. the chains -------------------------------------------------------------------------------------------------------------------------------
def test_floater_clumps_small_components_then_compact_records_gives_the_planted_records(gs4d):
    """five clumps of 5 tight records far from a dense cube: isolated(k = 2) flags none of them (the premise, on the CPU: test_components_host),
    small_components(k = 10) -> compact_records(min_pixels = 10, invert) gives exactly the 25, in order"""
    rec, planted, r = cp.floaters()
    n, k = rec.shape[0], 10
    assert (nc.host(rec, 0.0, r, 2, 0, nc.table("zero", n))["pixels"] >= 2).all()
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(rec)
    lonely = ctx.isolated(n, data, r, 2)
    assert ctx.read_compact_count(ctx.compact_records(lonely, n, min_pixels=2, invert=True))[0] == 0
    labels, stats = ctx.small_components(n, data, r, k)
    kept_index = fill(ctx, 4 * n)
    count = ctx.compact_records(stats, n, kept_index=kept_index, min_pixels=k, invert=True)
    assert ctx.read_compact_count(count) == (planted.size, planted.size)
    assert np.array_equal(ctx.read(kept_index, np.uint32, planted.size), planted)
    want_l, want_t = cp.host(rec, 0.0, r, k, 0, nc.table("zero", n))
    assert ctx.read(labels, np.uint32, n).tobytes() == want_l.tobytes() and ctx.read(stats, cp.STAT, n).tobytes() == want_t.tobytes()
    # the other direction: the records of the cube
    assert ctx.read_compact_count(ctx.compact_records(stats, n, min_pixels=k))[0] == n - planted.size
    ctx.finish()
    ctx.close()


def test_select_connected_count_centres_then_select_connected_then_measure_records(gs4d):
    """two separate bodies and a seed table of one record, taken from count_centres: the selection is the seed's body, and its measurement equals
    the host chain byte for byte"""
    rec, first, r = cp.two_bodies()
    n, seed = rec.shape[0], 417
    sphere = (tuple(float(v) for v in rec[seed, :3]), 1e-3)
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(rec)
    seeds = ctx.record_stats(n)
    ctx.count_centres(seeds, n, data, sphere=sphere)
    seeds_host = gs4d.count_centres_host(rec, gs4d.centre_query(sphere=sphere), W, H).view(cp.STAT)
    assert np.array_equal(np.flatnonzero(seeds_host["pixels"]), [seed]) and ctx.read(seeds, cp.STAT, n).tobytes() == seeds_host.tobytes()
    labels, picked = ctx.select_connected(n, data, seeds, r)
    want_l, _ = cp.host(rec, 0.0, r, cp.NOCAP, 0)
    one = (1, 0, 0)
    want_t = cp.host_count_labels(want_l, seeds_host, one, False, nc.table("zero", n))
    assert ctx.read(labels, np.uint32, n).tobytes() == want_l.tobytes() and ctx.read(picked, cp.STAT, n).tobytes() == want_t.tobytes()
    m = ctx.read(ctx.measure_records(data, n, stats=picked, min_pixels=1), mc.MEASURE, 1)
    m_host = mc.host(rec, 0.0, 0, want_t, one, False)
    assert m.tobytes() == m_host.tobytes() and int(m["count"][0]) == n - first == int((want_t["pixels"] > 0).sum())
    # clicked again on the other body with the labels kept: no second labelling
    ctx.subdata(seeds, ec.mask_table(np.arange(n) == 5, one))
    _, other = ctx.select_connected(n, data, seeds, r, labels=labels)
    assert np.array_equal(np.flatnonzero(ctx.read(other, cp.STAT, n)["pixels"]), np.arange(first))
    ctx.finish()
    ctx.close()
