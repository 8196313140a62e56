"""GPU: gs4d_count_ids — a region of the current frame's ID planes added into a record-statistics table on the device (include/gs4d.h).

Contract: every pixel of the rectangle whose record is not the sentinel and below nrecords, whose draw lies in [draw_first, draw_last], whose weight
bits are >= min_weight and whose mask byte is non-zero adds (1, bits(w), q(w)) to its record's (pixels, wmax, wsum) — and nothing else is written.
An integer problem: every comparison is exact, against select_cases.restate over the planes the test itself reads back with gs4d_read_ids on the
same frame (so nothing depends on how the draw broke a tie).  The new kernel alone is under test.  All calls go through the Python binding over
the C ABI."""
import ctypes

import numpy as np
import pytest

import cut_cases as kc
import select_cases as sel
import staged_cases
import stats_cases as sc

pytestmark = pytest.mark.gpu
NONE = sel.ID_NONE


class Frame:
    """one context that draws `rec` (96-byte records, GS4D_MODE_4D_DIRECT: instance k is record k) into frames with ID outputs"""

    def __init__(self, gs4d, W, H, rec):
        self.gs4d, self.W, self.H, self.n = gs4d, W, H, rec.shape[0]
        self.ctx = gs4d.Context(W, H)
        self.ctx.set_clear_color(gs4d.CLEAR_COLOR)
        self.ctx.set_id_outputs(True)
        self.db = self.ctx.buffer(rec)
        view, proj = sc.mats(gs4d, W, H)
        self.ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
        self.ctx.set_mode(gs4d.MODE_4D_DIRECT)
        self.ctx.bind(1, self.db)

    def frame(self, draws=1):
        self.ctx.clear()
        for _ in range(draws):
            self.ctx.draw_instanced(self.n)

    def table(self, rows):
        """a table buffer holding `rows` and TAIL_ROWS sentinel rows, and a sentinel-filled buffer created right after it"""
        return self.ctx.buffer(sel.table_bytes(rows)), self.ctx.buffer(np.full(4096, sel.SENTINEL, np.uint8))

    def read_table(self, buf, n):
        return self.ctx.read(buf, np.uint8, (n + sel.TAIL_ROWS) * 16)

    def close(self):
        self.ctx.close()


def count(f, buf, nrecords, reg, mask=0):
    """the C call with the fields of select_cases.region"""
    g = f.gs4d.IdRegion(*reg, 0)
    rc = f.gs4d._lib.gs4d_count_ids(f.ctx._h, ctypes.byref(g), int(mask), int(buf), ctypes.c_size_t(nrecords))
    assert rc == 0, f.gs4d._lib.gs4d_last_error(f.ctx._h)


def rows_of(raw, n):
    return raw[:n * 16].view(sel.STAT)


def check_call(f, planes, reg, nrecords, kind, mask_bytes=None, what=""):
    """one call into a fresh table of f.n rows against the restatement: the rows, the tail behind them and the neighbour buffer, byte for byte"""
    tin = sel.table(kind, f.n, what)
    buf, guard = f.table(tin)
    mb = f.ctx.buffer(mask_bytes) if mask_bytes is not None else 0
    count(f, buf, nrecords, reg, mb)
    got = f.read_table(buf, f.n)
    want = sel.table_bytes(sel.restate(*planes, reg, mask_bytes, tin, nrecords))
    assert np.array_equal(got, want), (what, reg, nrecords, kind, np.nonzero(rows_of(got, f.n) != rows_of(want, f.n))[0][:8])
    assert (f.ctx.read(guard, np.uint8, 4096) == sel.SENTINEL).all(), "the buffer created after the table changed"
    for b in (buf, guard) + ((mb,) if mb else ()):
        f.ctx.delete(b)
    return rows_of(got, f.n), tin


# ---- 1. results: every scene x rectangle x table, byte for byte -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sel.SCENES)
def test_every_scene_rectangle_and_table_equals_the_restatement(gs4d, name):
    W, H, rec = sel.scene(gs4d, name)
    f = Frame(gs4d, W, H, rec)
    f.frame(draws=0 if name == "clear" else 1)
    planes = f.ctx.read_ids()
    shown = planes[0] != NONE
    if name == "one":
        assert shown.all() and (planes[0] == 0).all(), "the premise: one record owns every pixel"
    elif name == "grid":
        assert 0.2 < shown.mean() < 0.8 and np.unique(planes[0][shown]).size > 0.9 * f.n, "the premise: small records, the sentinel between them"
        assert (planes[0][:, 1:] != planes[0][:, :-1]).mean() > 0.2, "the premise: neighbouring lanes differ"
    elif name == "layered":
        assert shown.mean() > 0.6 and np.unique(planes[0][shown]).size > 1000
    else:
        assert not shown.any()
    for rname, rect in sel.rectangles(W, H).items():
        for kind in sel.TABLES:
            for nrecords in (f.n, f.n // 2):
                got, tin = check_call(f, planes, sel.region(*rect), nrecords, kind, what=f"{name}/{rname}")
                if name == "clear":
                    assert np.array_equal(got, tin), "a cleared frame changed the table"
    f.close()


# ---- 2. filters ------------------------------------------------------------------------------------------------------------------------------------
def test_draw_filter_splits_a_frame_of_two_draws(gs4d):
    """two draws of two different record sets in one frame: the grid, then a few large records over a part of it"""
    W, H, rec = sel.scene(gs4d, "grid")
    f = Frame(gs4d, W, H, rec)
    rng = np.random.default_rng(5)
    k = 4
    over = sc.records(gs4d, W, H, rng.uniform(10, W - 10, k), rng.uniform(10, H - 10, k), np.full(k, 20.0), np.full(k, 2 * sc.S_LARGE),
                      np.concatenate([rng.uniform(0, 1, (k, 3)), np.full((k, 1), 0.6)], 1))
    ob = f.ctx.buffer(over)
    f.frame()
    f.ctx.bind(1, ob)
    f.ctx.draw_instanced(k)
    planes = f.ctx.read_ids()
    assert (planes[1] == 0).sum() > 50 and (planes[1] == 1).sum() > 50, "the premise: both draws show"
    full = sel.region(0, 0, W, H)
    every, _ = check_call(f, planes, full, f.n, "zero", what="draws/all")
    d0, _ = check_call(f, planes, sel.region(0, 0, W, H, draws=(0, 0)), f.n, "zero", what="draws/0")
    d1, _ = check_call(f, planes, sel.region(0, 0, W, H, draws=(1, 1)), f.n, "zero", what="draws/1")
    check_call(f, planes, sel.region(0, 0, W, H, draws=(0, 1)), f.n, "filled", what="draws/0-1")
    assert int(d0["pixels"].sum()) == int((planes[1] == 0).sum()) and int(d1["pixels"].sum()) == int((planes[1] == 1).sum())
    assert int(d0["pixels"].sum()) + int(d1["pixels"].sum()) == int(every["pixels"].sum()) == int((planes[0] != NONE).sum())
    assert (d1["pixels"][k:] == 0).all()
    # the binding's forms of the same filter
    for draws, want in ((0, d0), ((1, 1), d1), (None, every)):
        t = f.ctx.record_stats(f.n)
        f.ctx.count_ids(t, f.n, draws=draws)
        assert f.ctx.read(t, sel.STAT, f.n).tobytes() == want.tobytes()
    f.close()


def test_min_weight_is_inclusive_and_one_above_the_maximum_counts_nothing(gs4d):
    W, H, rec = sel.scene(gs4d, "layered")
    f = Frame(gs4d, W, H, rec)
    f.frame()
    planes = f.ctx.read_ids()
    wb = planes[2].view(np.uint32)[planes[0] != NONE]
    present = int(np.sort(wb)[wb.size // 2])                          # a weight the plane holds, half of the others below it
    full = (0, 0, W, H)
    got, _ = check_call(f, planes, sel.region(*full, min_weight=present), f.n, "zero", what="min_weight/present")
    assert int(got["pixels"].sum()) == int((wb >= present).sum()) > int((wb > present).sum())
    above, tin = check_call(f, planes, sel.region(*full, min_weight=int(wb.max()) + 1), f.n, "filled", what="min_weight/above")
    assert np.array_equal(above, tin)
    t = f.ctx.record_stats(f.n)
    f.ctx.count_ids(t, f.n, min_weight=float(np.array([present], np.uint32).view(np.float32)[0]))
    assert f.ctx.read(t, sel.STAT, f.n).tobytes() == got.tobytes()
    f.close()


@pytest.mark.parametrize("name", ["one", "layered"])
def test_masks(gs4d, name):
    W, H, rec = sel.scene(gs4d, name)
    f = Frame(gs4d, W, H, rec)
    f.frame()
    planes = f.ctx.read_ids()
    rects = sel.rectangles(W, H)
    for rname in ("full", "straddle", "column"):
        x, y, w, h = rects[rname]
        for kind in sel.MASKS:
            m = sel.mask(kind, w, h)
            got, tin = check_call(f, planes, sel.region(x, y, w, h), f.n, "filled" if kind == "random" else "zero", mask_bytes=m, what=f"mask/{rname}/{kind}")
            if kind == "zeros":
                assert np.array_equal(got, tin)
            elif kind == "ones":
                assert int(got["pixels"].sum()) == int((planes[0][y:y + h, x:x + w] != NONE).sum())
    # the binding uploads an (h, w) array
    x, y, w, h = rects["straddle"]
    m = sel.mask("checker", w, h)
    t = f.ctx.record_stats(f.n)
    f.ctx.count_ids(t, f.n, rect=(x, y, w, h), mask=m.astype(bool))
    want = sel.restate(*planes, sel.region(x, y, w, h), m, sel.table("zero", f.n), f.n)
    assert f.ctx.read(t, sel.STAT, f.n).tobytes() == want.tobytes()
    f.close()


# ---- 3. additivity ---------------------------------------------------------------------------------------------------------------------------------
def test_calls_add_up(gs4d):
    W, H, rec = sel.scene(gs4d, "layered")
    f = Frame(gs4d, W, H, rec)
    f.frame()
    planes = f.ctx.read_ids()
    n = f.n
    zero = sel.table("zero", n)
    whole = sel.restate(*planes, sel.region(0, 0, W, H), None, zero, n)
    # two disjoint rectangles into one table: one call on their union
    split = 37
    buf, _ = f.table(zero)
    count(f, buf, n, sel.region(0, 0, split, H))
    count(f, buf, n, sel.region(split, 0, W - split, H))
    assert rows_of(f.read_table(buf, n), n).tobytes() == whole.tobytes()
    # the same call twice: pixels and wsum double, wmax stays
    buf2, _ = f.table(zero)
    for _ in range(2):
        count(f, buf2, n, sel.region(0, 0, W, H))
    twice = rows_of(f.read_table(buf2, n), n)
    assert np.array_equal(twice["pixels"], 2 * whole["pixels"]) and np.array_equal(twice["wsum"], 2 * whole["wsum"]) and np.array_equal(twice["wmax"], whole["wmax"])
    assert int(whole["pixels"].sum()) == int((planes[0] != NONE).sum()) > 0
    f.close()


def stats_draw(f, table):
    """one frame without ID outputs whose draw adds its record statistics to `table`; ID outputs are on again afterwards"""
    c = f.ctx
    c.set_id_outputs(False)
    c.set_record_stats(table, f.n)
    f.frame()
    c.set_record_stats(None)
    c.set_id_outputs(True)


def test_a_count_adds_to_what_draws_have_added(gs4d):
    """draws with gs4d_set_record_stats into a table, then — nothing read in between — a count into the same table"""
    W, H, rec = sel.scene(gs4d, "layered")
    f = Frame(gs4d, W, H, rec)
    n = f.n
    alone = f.ctx.record_stats(n)
    stats_draw(f, alone)
    drawn = f.ctx.read(alone, sel.STAT, n)                             # integers: the same draw adds the same rows every time
    assert int(drawn["pixels"].sum()) > 0
    t = f.ctx.record_stats(n)
    stats_draw(f, t)
    f.frame()
    f.ctx.count_ids(t, n)
    planes = f.ctx.read_ids()
    got = f.ctx.read(t, sel.STAT, n)
    want = sel.add_tables(drawn, sel.restate(*planes, sel.region(0, 0, W, H), None, sel.table("zero", n), n))
    assert got.tobytes() == want.tobytes()
    f.close()


# ---- 4. argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_queue_nothing(gs4d):
    W, H, rec = sel.scene(gs4d, "grid")
    f = Frame(gs4d, W, H, rec)
    ctx, lib, n = f.ctx, gs4d._lib, f.n
    f.frame()
    tin = sel.table("filled", n, "errors")
    stats, guard = f.table(tin)
    fill = lambda nbytes: ctx.buffer(np.full(nbytes, sel.SENTINEL, np.uint8))
    rect = (3, 5, 40, 30)
    mask, short_mask, short_stats, dead = fill(40 * 30), fill(40 * 30 - 1), fill(16 * n - 1), fill(64)
    ctx.delete(dead)

    def call(rect=rect, draws=sel.EVERY_DRAW, reserved=0, mask=mask, stats=stats, nrecords=n, null_region=False):
        g = gs4d.IdRegion(*rect, draws[0], draws[1], 0, reserved)
        return lib.gs4d_count_ids(ctx._h, None if null_region else ctypes.byref(g), mask, stats, ctypes.c_size_t(nrecords))

    bad = {
        "empty rectangle (w)": dict(rect=(3, 5, 0, 30)),
        "empty rectangle (h)": dict(rect=(3, 5, 40, 0)),
        "negative width": dict(rect=(3, 5, -1, 30)),
        "negative x": dict(rect=(-1, 5, 40, 30)),
        "negative y": dict(rect=(3, -1, 40, 30)),
        "over the right edge": dict(rect=(W - 39, 5, 40, 30), mask=0),
        "over the top edge": dict(rect=(3, H - 29, 40, 30), mask=0),
        "x + w overflows": dict(rect=(0x7FFFFFFF, 0, 0x7FFFFFFF, 1), mask=0),
        "draw_first > draw_last": dict(draws=(2, 1)),
        "reserved != 0": dict(reserved=1),
        "nrecords > 0xFFFFFFFF": dict(nrecords=1 << 32),
        "stats is no buffer": dict(stats=0),
        "unknown stats": dict(stats=9999),
        "dead stats": dict(stats=dead),
        "stats too small": dict(stats=short_stats),
        "stats too small by the tail": dict(nrecords=n + sel.TAIL_ROWS + 1),
        "unknown mask": dict(mask=9999),
        "dead mask": dict(mask=dead),
        "mask too small": dict(mask=short_mask),
        "mask too small for the whole image": dict(null_region=True),
        "mask == stats": dict(mask=stats),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"count_ids" in lib.gs4d_last_error(ctx._h), what
    # a frame that was not cleared with ID outputs on
    ctx.set_id_outputs(False)
    f.frame()
    assert call() == -1 and b"ID outputs" in lib.gs4d_last_error(ctx._h)
    ctx.set_id_outputs(True)
    assert np.array_equal(f.read_table(stats, n), sel.table_bytes(tin)), "a refused call wrote to the table"
    for b in (guard, mask, short_mask, short_stats):
        assert (ctx.read(b, np.uint8, 16) == sel.SENTINEL).all()
    # nrecords == 0: a no-op; then the same call with valid arguments works
    f.frame()
    assert call(nrecords=0) == 0 and np.array_equal(f.read_table(stats, n), sel.table_bytes(tin))
    assert call() == 0 and call(null_region=True, mask=0) == 0
    planes = ctx.read_ids()                                            # of the frame the two calls read
    m = np.full((30, 40), sel.SENTINEL, np.uint8)
    want = sel.restate(*planes, sel.region(0, 0, W, H), None, sel.restate(*planes, sel.region(*rect), m, tin, n), n)
    assert np.array_equal(f.read_table(stats, n), sel.table_bytes(want))
    f.close()


# ---- 5. ordering without a finish ------------------------------------------------------------------------------------------------------------------
def test_a_count_right_after_the_draw_sees_the_finished_frame(gs4d):
    W, H, rec = sel.scene(gs4d, "layered")
    tables = []
    for finish in (False, True):
        f = Frame(gs4d, W, H, rec)
        t = f.ctx.record_stats(f.n)
        f.frame()
        if finish:
            f.ctx.finish()
        f.ctx.count_ids(t, f.n)
        tables.append(f.ctx.read(t, sel.STAT, f.n))
        if finish:
            want = sel.restate(*f.ctx.read_ids(), sel.region(0, 0, W, H), None, sel.table("zero", f.n), f.n)
        f.close()
    assert tables[0].tobytes() == tables[1].tobytes() == want.tobytes() and int(want["pixels"].sum()) > 0


def test_a_later_draw_and_a_later_mask_upload_do_not_change_the_count(gs4d):
    W, H, rec = sel.scene(gs4d, "layered")
    twin = Frame(gs4d, W, H, rec)                                       # stops after the first draw
    twin.frame()
    planes = twin.ctx.read_ids()
    twin.close()
    f = Frame(gs4d, W, H, rec)
    m = sel.mask("checker", W, H)
    mb, t = f.ctx.buffer(m), f.ctx.record_stats(f.n)
    f.frame()
    f.ctx.count_ids(t, f.n, mask=mb)
    f.ctx.draw_instanced(f.n)                                           # a second draw into the same frame: every plane changes
    f.ctx.subdata(mb, 1 - m)
    got = f.ctx.read(t, sel.STAT, f.n)
    after = f.ctx.read_ids()
    f.close()
    assert (after[1] == 1).any(), "the premise: the second draw shows"
    want = sel.restate(*planes, sel.region(0, 0, W, H), m, sel.table("zero", f.n), f.n)
    assert got.tobytes() == want.tobytes() and int(want["pixels"].sum()) > 0


def test_a_draw_the_library_runs_again_is_counted_once_it_stands(gs4d, monkeypatch):
    """staged_cases.py case a, as tests/test_gpu_ids.py runs it with ID outputs: frames at T0 teach the guesses, the frame at T1 overflows the last
    segment's block and is re-run exactly.  The count is issued right behind that draw; the planes it must have seen are those of a twin context
    that draws the same frame with exact lists (GS4D_STAGED=0) and never re-runs."""
    rec, times = staged_cases.build(gs4d, "a")
    view, proj = staged_cases.mats(gs4d)
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    n = rec.shape[0]

    def run(staged, warm):
        if staged:
            monkeypatch.delenv("GS4D_STAGED", raising=False)
        else:
            monkeypatch.setenv("GS4D_STAGED", "0")
        ctx = gs4d.Context(staged_cases.W, staged_cases.H)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_id_outputs(True)
        data, keys, idx, t = ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n), ctx.record_stats(n)
        for k, tm in enumerate([staged_cases.T0] * warm + [times[0]]):
            if warm and k == warm:
                ctx.finish()
            ctx.clear()
            ctx.set_uniforms(time=tm, min_opacity=0.0, view=view, proj=proj)
            ctx.keygen(data, tm, staged_cases.CAM[0], keys, idx, n)
            ctx.sort_pairs(keys, idx, n)
            ctx.set_mode(gs4d.MODE_4D_SORTED)
            ctx.bind(1, idx)
            ctx.bind(2, data)
            ctx.draw_instanced(n)
        ctx.count_ids(t, n)
        got = ctx.read(t, sel.STAT, n)
        planes = ctx.read_ids()
        st = ctx.stats()
        ctx.close()
        return got, planes, st

    exact, planes, st0 = run(False, 0)
    assert st0["staged_draws"] == 0 and st0["reruns"] == 0, st0
    got, _, st = run(True, 2 * 4 + 8)
    assert st["staged_misses"] >= 1 and st["reruns"] >= 1, st
    want = sel.restate(*planes, sel.region(0, 0, staged_cases.W, staged_cases.H), None, sel.table("zero", n), n)
    assert got.tobytes() == want.tobytes() == exact.tobytes() and int(want["pixels"].sum()) > 0


def test_a_statistics_draw_on_the_next_lane_adds_to_the_count(gs4d):
    W, H, rec = sel.scene(gs4d, "layered")
    f = Frame(gs4d, W, H, rec)
    n = f.n
    assert f.ctx.stats()["lanes"] > 1
    alone = f.ctx.record_stats(n)
    stats_draw(f, alone)
    drawn = f.ctx.read(alone, sel.STAT, n)
    twin = Frame(gs4d, W, H, rec)
    twin.frame()
    planes = twin.ctx.read_ids()
    twin.close()
    t = f.ctx.record_stats(n)
    f.frame()
    f.ctx.count_ids(t, n)                                               # on the frame's lane
    stats_draw(f, t)                                                    # clear: the next lane; its draw adds to the same table
    got = f.ctx.read(t, sel.STAT, n)
    f.close()
    want = sel.add_tables(drawn, sel.restate(*planes, sel.region(0, 0, W, H), None, sel.table("zero", n), n))
    assert got.tobytes() == want.tobytes()


# ---- 6. shards -------------------------------------------------------------------------------------------------------------------------------------
def test_the_tables_of_two_tile_row_shards_add_up(gs4d):
    W, H, rec = sel.scene(gs4d, "layered")
    tables = {}
    for rank in (None, 0, 1):
        f = Frame(gs4d, W, H, rec)
        if rank is not None:
            f.ctx.set_tile_shard(rank, 2)
        t = f.ctx.record_stats(f.n)
        f.frame()
        f.ctx.count_ids(t, f.n)
        tables[rank] = f.ctx.read(t, sel.STAT, f.n)
        planes = f.ctx.read_ids()
        assert tables[rank].tobytes() == sel.restate(*planes, sel.region(0, 0, W, H), None, sel.table("zero", f.n), f.n).tobytes()
        f.close()
    assert sel.add_tables(tables[0], tables[1]).tobytes() == tables[None].tobytes()
    assert int(tables[0]["pixels"].sum()) > 0 and int(tables[1]["pixels"].sum()) > 0


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------------------------
def test_select_builds_the_set_a_rectangle_shows(gs4d):
    W, H, rec = sel.scene(gs4d, "layered")
    f = Frame(gs4d, W, H, rec)
    c, n = f.ctx, f.n
    f.frame()
    rect = sel.rectangles(W, H)["straddle"]
    x, y, w, h = rect
    planes = c.read_ids()
    dst, kept_index, kept, stats = c.select(n, src=f.db, rect=rect)
    inside = planes[0][y:y + h, x:x + w]
    want = np.unique(inside[inside != NONE])
    assert 10 < kept == want.size < n
    assert np.array_equal(c.read(kept_index, np.uint32, kept), want)
    assert np.array_equal(c.read(dst, np.float32, kept * 24).reshape(kept, 24).view(np.uint32), rec[want].view(np.uint32))
    table = c.read(stats, sel.STAT, n)
    assert table.tobytes() == sel.restate(*planes, sel.region(*rect), None, sel.table("zero", n), n).tobytes()
    # the k most visible records of the rectangle
    for field in kc.FIELDS:
        budget = kept // 3
        assert c.read_stat_cut(c.stat_cut(stats, n, budget, field)) == kc.restate(kc.field_u64(table, field), budget)
    # the index list alone
    none, index_only, kept2, _ = c.select(n, rect=rect)
    assert none is None and kept2 == kept and np.array_equal(c.read(index_only, np.uint32, kept), want)
    # the compacted set draws: keygen, sort, draw
    keys, idx = c.buffer(nbytes=4 * kept), c.buffer(nbytes=4 * kept)
    c.clear()
    c.keygen(dst, 0.0, sc.CAM[0], keys, idx, kept)
    c.sort_pairs(keys, idx, kept)
    c.set_mode(gs4d.MODE_4D_SORTED)
    c.bind(1, idx)
    c.bind(2, dst)
    c.draw_instanced(kept)
    c.finish()
    img = c.read_pixels()
    assert float(np.abs(img - np.array(gs4d.CLEAR_COLOR, np.float32)).max()) > 0.05, "empty image"
    shown = c.read_ids()[0]
    assert (shown[shown != NONE] < kept).all()
    f.close()
