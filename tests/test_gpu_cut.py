"""GPU: gs4d_stat_cut — the threshold of one statistics field that fits a record budget, selected on the device (include/gs4d.h).

Contract: with f the chosen field of the n rows as uint64 and k = min(budget, n), `out` receives {value = the k-th largest of f, above = #{f > value},
equal = #{f == value}} in its first 16 bytes and nothing else is written anywhere.  An integer problem: every comparison is exact, against
cut_cases.restate (a descending numpy sort and two counts).  All calls go through the Python binding over the C ABI."""
import ctypes

import numpy as np
import pytest

import cut_cases as kc
import staged_cases
import stats_cases as sc
import test_gpu_compact as tgc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
OUT_BYTES = 256                                            # `out` is larger than the 16 bytes the call writes


class Cuts:
    """one context holding a statistics table of n rows and a sentinel-filled `out`; check() runs one cut against the restatement"""

    def __init__(self, gs4d, n):
        self.n = n
        self.ctx = gs4d.Context(64, 64)
        self.stats = self.ctx.buffer(nbytes=max(16, 16 * n))
        self.out = self.ctx.buffer(np.full(OUT_BYTES, SENTINEL, np.uint8))
        self.guard = self.ctx.buffer(np.full(4096, SENTINEL, np.uint8))      # created right after `out`

    def upload(self, table):
        self.table = table
        if self.n:
            self.ctx.subdata(self.stats, table)
        self.desc = {field: kc.descending(kc.field_u64(table, field)) for field in kc.FIELDS}      # one sort per field, shared among the budgets

    def check(self, field, budget, what=""):
        c = self.ctx
        c.subdata(self.out, np.full(16, SENTINEL, np.uint8))
        assert c.stat_cut(self.stats, self.n, budget, field, out=self.out) == self.out
        got = c.read(self.out, np.uint8, OUT_BYTES)
        want = kc.expected_bytes(self.table, field, budget, self.desc[field])
        assert np.array_equal(got[:16], want), (what, field, budget, got[:16].view(kc.CUT), want.view(kc.CUT))
        assert (got[16:] == SENTINEL).all(), "bytes of out beyond the first 16 changed"
        return tuple(int(x) for x in got[:16].view(kc.CUT)[0])

    def unchanged(self):
        assert (self.ctx.read(self.guard, np.uint8, 4096) == SENTINEL).all(), "the buffer created after out changed"
        if self.n:
            assert np.array_equal(self.ctx.read(self.stats, kc.STAT, self.n), self.table), "the table changed"

    def close(self):
        self.ctx.close()


def run_generator(t, gen):
    t.upload(kc.table(gen, t.n))
    for field in kc.FIELDS:
        for budget in kc.budgets(t.n):
            value, above, equal = t.check(field, budget, gen)
            if t.n:
                k = min(budget, t.n)
                assert above < k <= above + equal
    t.unchanged()


# ---- 1. results: every size x generator x field x budget, byte for byte ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", kc.SIZES)
def test_every_generator_field_and_budget_equals_the_restatement(gs4d, n):
    t = Cuts(gs4d, n)
    for gen in kc.GENERATORS:
        run_generator(t, gen)
    t.close()


@pytest.mark.parametrize("gen", kc.GENERATORS)
def test_the_grid_stride_size_equals_the_restatement(gs4d, gen):
    """cut_cases.STRIDE_SIZE: 2 * GROUPS + 1 tiles — every workgroup of the capped grid takes a second tile, the first one a third"""
    t = Cuts(gs4d, kc.STRIDE_SIZE)
    run_generator(t, gen)
    t.close()


def test_the_tie_budgets_land_on_the_group_boundary(gs4d):
    n = 3 * kc.TILE + 1
    t = Cuts(gs4d, n)
    t.upload(kc.table("ties", n))
    top, a, b = kc.tie_layout(n)
    k1, k2 = kc.tie_budgets(n)
    for field in kc.FIELDS:
        v1, above1, equal1 = t.check(field, k1)
        v2, above2, equal2 = t.check(field, k2)
        assert (above1, equal1) == (top, a) and above1 + equal1 == k1          # the last member of the upper group: min = value keeps exactly k
        assert (above2, equal2) == (top + a, b) and v2 < v1                    # the first member of the lower one: min = value + 1 keeps `above` < k
    t.close()


# ---- 2. argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_queue_nothing(gs4d):
    n = 300
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    fill = lambda nbytes: ctx.buffer(np.full(nbytes, SENTINEL, np.uint8))
    st = kc.table("distinct", n)
    stats, out, short_stats, short_out, dead = ctx.buffer(st), fill(OUT_BYTES), ctx.buffer(st[:-1]), fill(12), fill(64)
    ctx.delete(dead)

    def call(stats=stats, n=n, field=gs4d.STAT_WSUM, budget=10, out=out):
        return lib.gs4d_stat_cut(ctx._h, stats, ctypes.c_size_t(n), field, ctypes.c_size_t(budget), out)

    bad = {
        "n > 0xFFFFFFFF": dict(n=1 << 32),
        "budget == 0": dict(budget=0),
        "field 3": dict(field=3),
        "field -1": dict(field=-1),
        "stats is no buffer": dict(stats=0),
        "out is no buffer": dict(out=0),
        "unknown name": dict(out=9999),
        "dead stats": dict(stats=dead),
        "dead out": dict(out=dead),
        "stats == out": dict(out=stats),
        "stats too small": dict(stats=short_stats),
        "out too small": dict(out=short_out),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    for b, nbytes in ((out, OUT_BYTES), (short_out, 12)):
        assert (ctx.read(b, np.uint8, nbytes) == SENTINEL).all(), "a refused call wrote something"
    assert np.array_equal(ctx.read(stats, kc.STAT, n), st)
    assert call() == 0                                                          # the same arguments, valid: the call works after the refusals
    assert ctx.read_stat_cut(out) == kc.restate(kc.field_u64(st, "wsum"), 10)
    ctx.close()


# ---- 3. ordering without a finish ------------------------------------------------------------------------------------------------------------------
def cut_of(table, field, budget):
    return kc.restate(kc.field_u64(tgc.table_bits(table), field), budget)


def test_the_cut_waits_for_the_draws_of_every_lane(gs4d):
    rec = sc.records(gs4d, tgc.W5, tgc.H5, *tgc.layered_params())
    d = tgc.Direct(gs4d, tgc.W5, tgc.H5, rec)
    frames = 2 * d.ctx.stats()["lanes"] + 1
    for _ in range(frames):
        d.frame()
    budget = d.n // 4
    outs = {field: d.ctx.stat_cut(d.sb, d.n, budget, field) for field in kc.FIELDS}       # immediately: no read-back, no finish
    got = {field: d.ctx.read_stat_cut(outs[field]) for field in kc.FIELDS}
    d.ctx.close()
    # a fresh context that drew the same frames, its table read after finish
    f = tgc.Direct(gs4d, tgc.W5, tgc.H5, rec)
    for _ in range(frames):
        f.frame()
    f.ctx.finish()
    table = f.ctx.read_record_stats(f.sb, f.n)
    f.ctx.close()
    assert (table["pixels"] > 0).sum() > budget                                # the budget lies inside the counted records
    for field in kc.FIELDS:
        assert got[field] == cut_of(table, field, budget), field
        assert got[field][0] > 0


def test_the_cut_waits_for_a_rerun(gs4d, monkeypatch):
    """staged_cases' case a, as tests/test_gpu_compact.py runs it: frames at T0 teach the guesses, the frame at T1 outgrows a segment block; the
    library re-runs it with exact lists when the cut asks for the table"""
    monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    rec, _ = staged_cases.build(gs4d, "a")
    W, H, n = staged_cases.W, staged_cases.H, rec.shape[0]
    fresh = gs4d.Context(W, H)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    fb = (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n))
    fsb = fresh.record_stats(n)
    fresh.set_record_stats(fsb, n)
    tgc.sorted_frame(gs4d, fresh, fb, n, staged_cases.T1)
    fresh.finish()
    want = fresh.read_record_stats(fsb, n)
    fresh.close()
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    sb = ctx.record_stats(n)
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        tgc.sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    ctx.set_record_stats(sb, n)
    tgc.sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    budget = max(1, int((want["pixels"] > 0).sum()) // 3)
    out = ctx.stat_cut(sb, n, budget, "wsum")                                  # no read-back in between
    s1 = ctx.stats()
    assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    assert ctx.read_stat_cut(out) == cut_of(want, "wsum", budget)
    assert np.array_equal(tgc.table_bits(ctx.read_record_stats(sb, n)), tgc.table_bits(want))
    ctx.close()


def test_a_draw_or_a_host_write_after_the_cut_does_not_change_it(gs4d):
    """Statistics stay on: the cut, then at once a frame on the next lane that adds to the table; then a second cut with an upload of zeros behind
    it.  Both results are those of the table as it stood at the call."""
    rec = sc.records(gs4d, tgc.W5, tgc.H5, *tgc.layered_params())
    d = tgc.Direct(gs4d, tgc.W5, tgc.H5, rec)
    c = d.ctx
    d.frame()
    one = tgc.table_bits(c.read_record_stats(d.sb, d.n)).copy()
    budget = d.n // 5
    outs = {field: c.stat_cut(d.sb, d.n, budget, field) for field in ("pixels", "wsum")}
    d.frame()                                                                  # the next lane (where there is more than one), no read-back in between
    two = one.copy()                                                           # the statistics are deterministic: the frame adds what the first added
    two["pixels"] *= 2
    two["wsum"] *= 2
    for field in ("pixels", "wsum"):
        assert c.read_stat_cut(outs[field]) == kc.restate(kc.field_u64(one, field), budget), field
        assert kc.restate(kc.field_u64(one, field), budget) != kc.restate(kc.field_u64(two, field), budget)      # a cut that saw the draw would differ
    assert np.array_equal(tgc.table_bits(c.read_record_stats(d.sb, d.n)), two)  # ... and the draw did add
    out = c.stat_cut(d.sb, d.n, budget, "wsum")
    c.subdata(d.sb, np.zeros(d.n, gs4d.Context.RECORD_STAT))                   # a host write waits for the reader
    assert c.read_stat_cut(out) == kc.restate(kc.field_u64(two, "wsum"), budget)
    assert c.read_stat_cut(out)[0] > 0                                         # zeros would have given {0, 0, n}
    assert not c.read_record_stats(d.sb, d.n)["pixels"].any()
    c.close()


# ---- 4. end to end: prune_to_budget ------------------------------------------------------------------------------------------------------------------
def test_prune_to_budget_keeps_the_records_that_matter_most_and_the_set_draws(gs4d):
    W, H, params = sc.layered("edges")
    rec = sc.records(gs4d, W, H, *params)
    n = rec.shape[0]
    c = gs4d.Context(W, H)
    c.set_clear_color(gs4d.CLEAR_COLOR)
    view, proj = sc.mats(gs4d, W, H)
    c.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
    db, sb = c.buffer(rec), c.record_stats(n)
    c.set_mode(gs4d.MODE_4D_DIRECT)
    c.bind(1, db)
    c.set_record_stats(sb, n)
    c.clear()
    c.draw_instanced(n)
    c.set_record_stats(None)
    wsum = c.read_record_stats(sb, n)["wsum"]
    counted = int((wsum > 0).sum())
    assert 8 < counted < n                                                     # records off the image count nothing
    kb, ib = c.buffer(nbytes=4 * n), c.buffer(nbytes=4 * n)
    for budget in (counted // 3, counted + (n - counted) // 2 + 1):            # inside the counted records; beyond them, in the zero rows
        value, above, equal = kc.restate(wsum, budget)
        want = np.flatnonzero(wsum >= np.uint64(value if above + equal <= budget else value + 1)).astype(np.uint32)
        if budget > counted:
            assert value == 0 and want.size == counted                        # the tie of zero rows does not fit: every counted record, none of the others
        dst, kidx, kept = c.prune_to_budget(sb, n, db, budget)
        assert 0 < kept <= budget and kept == want.size
        index = c.read(kidx, np.uint32, kept)
        assert np.array_equal(index, want) and np.all(np.diff(index.astype(np.int64)) > 0)      # numpy's, ascending: the stable order
        assert np.array_equal(c.read(dst, np.float32, kept * 24).reshape(kept, 24).view(np.uint32), rec[index].view(np.uint32))
        # the pruned set draws
        c.clear()
        c.keygen(dst, 0.0, sc.CAM[0], kb, ib, kept)
        c.sort_pairs(kb, ib, kept)
        c.set_mode(gs4d.MODE_4D_SORTED)
        c.bind(1, ib)
        c.bind(2, dst)
        c.draw_instanced(kept)
        c.finish()                                                             # raises unless gs4d_finish returns 0
        img = c.read_pixels()
        assert float(np.abs(img - np.array(gs4d.CLEAR_COLOR, np.float32)).max()) > 0.05, "empty frame"
        for b in (dst, kidx):
            c.delete(b)
    # a table in which nothing exceeds a tie that does not fit: an empty set, no compaction
    flat = c.buffer(kc.table("equal", n))
    dst, kidx, kept = c.prune_to_budget(flat, n, db, n - 1)
    assert kept == 0 and dst and kidx
    # ... and every field by name
    for field in kc.FIELDS:
        st = kc.table("distinct", n)
        tb = c.buffer(st)
        dst, kidx, kept = c.prune_to_budget(tb, n, db, 100, field=field)
        assert kept == 100
        assert np.array_equal(c.read(kidx, np.uint32, kept), np.sort(np.argsort(st[field], kind="stable")[::-1][:100]).astype(np.uint32))
    c.close()
