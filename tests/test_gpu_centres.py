"""GPU: gs4d_count_centres — the records whose time-conditioned centre lies in a volume or projects into a region of the screen, as rows of a
record-statistics table (include/gs4d.h).

The table is checked byte for byte against the numpy restatement (tests/centre_cases.py: the header's float32 operations) with guard buffers
around data, table and mask; the same query gives the same table from the records and from each layout of a current SoA shadow, and
gs4d_debug_shadow_builds does not move; the selection of a screen query is exactly what the draw's own projected centres say; the call orders
itself with draws that add to the table and with a later mask upload; select_volume + hide draws the bits of the compacted complement.  All calls
go through the Python binding over the C ABI; contexts are 64 x 48."""
import ctypes

import numpy as np
import pytest

import centre_cases as cc
import edit_cases as ec
import hostile_cases
import scenes

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
f32 = np.float32
W, H = cc.W, cc.H
GPU_SIZES = tuple(n for n in cc.SIZES if n > 0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


class Bench:
    """the buffers of one record set between sentinel guard buffers: data (the n records, EXTRA more behind them — copies of the first ones, so
    they would take part if they were looked at — and a sentinel tail), a table of exactly n rows, masks of exactly w * h bytes"""

    def __init__(self, ctx, rec, n=None):
        self.ctx, self.n = ctx, rec.shape[0] if n is None else n
        self.rec = np.ascontiguousarray(rec[:self.n])
        held = np.concatenate([self.rec, np.resize(self.rec, (cc.EXTRA, 24))]) if self.n else self.rec
        self.host = np.concatenate([held.view(np.uint8).reshape(-1), np.full(GUARD, SENTINEL, np.uint8)])
        self.g0, self.data, self.g1 = fill(ctx, GUARD), ctx.buffer(self.host), fill(ctx, GUARD)
        self.stats, self.g2 = ctx.buffer(nbytes=max(16, 16 * self.n)), fill(ctx, GUARD)
        self.masks, self.g3 = {}, fill(ctx, GUARD)

    def mask(self, rect):
        if rect not in self.masks:
            m = cc.mask_for(rect)
            self.masks[rect] = (self.ctx.buffer(m), m, fill(self.ctx, GUARD))
        return self.masks[rect]

    def check(self, q, table, masked, what):
        """one call on a freshly uploaded table: every byte of the table against the restatement; returns who takes part"""
        c = self.ctx
        buf, m = (self.mask(tuple(q["rect"]))[:2] if masked else (None, None))
        c.subdata(self.stats, table)
        c.count_centres(self.stats, self.n, self.data, mask=buf, query=cc.struct(q))
        got = c.read(self.stats, cc.STAT, self.n)
        want, part = cc.restate(self.rec, q, table, m)
        assert got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} rows differ from the restatement"
        return part

    def check_the_rest(self, what):
        c = self.ctx
        assert all(untouched(c, g) for g in (self.g0, self.g1, self.g2, self.g3)), f"{what}: a guard buffer changed"
        assert np.array_equal(c.read(self.data, np.uint8, self.host.size), self.host), f"{what}: data changed"
        for buf, m, guard in self.masks.values():
            assert np.array_equal(c.read(buf, np.uint8, m.size), m.reshape(-1)) and untouched(c, guard), f"{what}: a mask changed"

    def delete(self):
        for b in [self.g0, self.data, self.g1, self.stats, self.g2, self.g3] + [b for buf, _, g in self.masks.values() for b in (buf, g)]:
            self.ctx.delete(b)


# ---- 1. bits -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cc.KINDS)
def test_the_table_equals_the_restatement_byte_for_byte(gs4d, kind):
    """every subset of the six test bits, both ops, a zeroed and a random table, every size (the premises — no case is vacuous — are
    tests/test_centres_host.py's, asserted on the CPU from the same generator)"""
    ctx = gs4d.Context(W, H)
    for n in GPU_SIZES:
        b = Bench(ctx, cc.records(kind, n))
        zero, random = cc.table("zero", n), cc.table("random", n)
        for tests in cc.subsets():
            masked = bool(tests & cc.SCREEN)
            part = b.check(cc.query(tests), zero, masked, f"{kind}, n = {n}, tests = {tests}, add, zeroed table")
            b.check(cc.query(tests), random, masked, f"{kind}, n = {n}, tests = {tests}, add, random table")
            b.check(cc.query(tests, cc.REMOVE), random, masked, f"{kind}, n = {n}, tests = {tests}, remove")
            if masked:
                b.check(cc.query(tests), random, False, f"{kind}, n = {n}, tests = {tests}, no mask")
            if n >= cc.TILE - 1 and tests & ~cc.FRAME:
                assert 0 < int(part.sum()) < n
        b.check_the_rest(f"{kind}, n = {n}")
        b.delete()
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_rectangles_on_the_image_edges_and_non_finite_operands(gs4d):
    ctx = gs4d.Context(W, H)
    for kind in cc.KINDS:
        b = Bench(ctx, cc.records(kind, 1000))
        random = cc.table("random", 1000)
        for rect in cc.EDGE_RECTS:
            for tests in (cc.SCREEN, cc.ALL_BITS):
                for masked in (False, True):
                    part = b.check(cc.query(tests, rect=rect), random, masked, f"{kind}, rect = {rect}, tests = {tests}, mask = {masked}")
                    assert 0 < int(part.sum()) < 1000
        for name, q in cc.nonfinite_queries():
            b.check(q, random, bool(q["tests"] & cc.SCREEN), f"{kind}, {name}")
        b.check_the_rest(kind)
        b.delete()
    ctx.finish()
    ctx.close()


def test_hostile_record_sets(gs4d):
    ctx = gs4d.Context(W, H)
    total = 0
    for case in hostile_cases.all_cases():
        b = Bench(ctx, case.rec)
        random = cc.table("random", case.n)
        for k, q in enumerate(cc.hostile_queries(case)):
            total += int(b.check(q, random, bool(q["tests"] & cc.SCREEN and k % 2 == 0), f"{case.name}, query {k}").sum())
        b.check_the_rest(case.name)
        b.delete()
    assert total > 1000
    ctx.finish()                                                # no device error
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(W, H)
    data, stats, mask = fill(ctx, 96 * 4), fill(ctx, 16 * 4), fill(ctx, cc.RECT[2] * cc.RECT[3])
    ctx.count_centres(stats, 0, data, mask=mask, query=cc.struct(cc.query(cc.ALL_BITS)))
    ctx.count_centres(stats, 0, data, query=cc.struct(cc.query(0, cc.REMOVE)))
    ctx.finish()
    assert untouched(ctx, data, 96 * 4) and untouched(ctx, stats, 16 * 4) and untouched(ctx, mask, cc.RECT[2] * cc.RECT[3])
    ctx.close()


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_as_it_was(gs4d):
    n = 300
    ctx, lib = gs4d.Context(W, H), gs4d._lib
    rec, table, m = cc.records("symmetric", n), cc.table("random", n), cc.mask_for(cc.RECT)
    data, stats, mask = ctx.buffer(rec), ctx.buffer(table), ctx.buffer(m)
    short_data, short_stats, short_mask, dead = ctx.buffer(rec.reshape(-1)[:-1]), ctx.buffer(table[:-1]), ctx.buffer(m.reshape(-1)[:-1]), fill(ctx, 64)
    ctx.delete(dead)
    NO = object()

    def call(data=data, n=n, q=None, mask=0, stats=stats, **fields):
        s = cc.struct(cc.query(cc.ALL_BITS)) if q is None else q
        for k, v in fields.items():
            setattr(s, k, v)
        return lib.gs4d_count_centres(ctx._h, data, ctypes.c_size_t(n), None if q is NO else ctypes.byref(s), mask, stats)

    box = lambda: cc.struct(cc.query(cc.BOX))
    bad = {
        "query == NULL": dict(q=NO), "test bit 64": dict(tests=64 | cc.BOX), "test bit 31": dict(tests=0x80000000), "op 2": dict(op=2),
        "op 0xFFFFFFFF": dict(op=0xFFFFFFFF), "reserved": dict(reserved=1), "n > 0xFFFFFFFF": dict(n=1 << 32), "no data": dict(data=0),
        "dead data": dict(data=dead), "unknown data": dict(data=9999), "no stats": dict(stats=0), "dead stats": dict(stats=dead),
        "unknown stats": dict(stats=9999), "data too small": dict(data=short_data), "stats too small": dict(stats=short_stats),
        "dead mask": dict(mask=dead), "unknown mask": dict(mask=9999), "mask without SCREEN": dict(q=box(), mask=mask),
        "mask too small": dict(mask=short_mask), "x < 0": dict(x=-1), "y < 0": dict(y=-1), "w == 0": dict(w=0), "h == 0": dict(h=0), "w < 0": dict(w=-4),
        "past the right edge": dict(x=W - cc.RECT[2] + 1), "past the top edge": dict(y=H - cc.RECT[3] + 1), "wider than the image": dict(x=0, w=W + 1),
        "x + w overflows": dict(x=0x7FFFFFFF, w=0x7FFFFFFF), "data == stats": dict(data=stats), "data == mask": dict(mask=data), "stats == mask": dict(mask=stats),
        "data == stats without SCREEN": dict(q=box(), data=stats),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    assert call(n=0, tests=64) == -1 and call(n=0, mask=dead) == -1                 # ... with no records too
    ctx.finish()
    assert np.array_equal(ctx.read(stats, np.uint8, 16 * n), table.view(np.uint8)), "a refused call wrote something"
    assert np.array_equal(bits(ctx.read(data, f32, n * 24)), bits(rec).reshape(-1)) and np.array_equal(ctx.read(mask, np.uint8, m.size), m.reshape(-1))
    # the call works after the refusals; without SCREEN the rectangle is data nobody looks at
    assert call(mask=mask) == 0 and call(n=0) == 0 and call(q=box(), x=-7, w=0) == 0
    want, _ = cc.restate(rec, cc.query(cc.ALL_BITS), table, m)
    want, _ = cc.restate(rec, cc.query(cc.BOX), want)
    assert ctx.read(stats, cc.STAT, n).tobytes() == want.tobytes()
    ctx.close()


# ---- 3. each source ------------------------------------------------------------------------------------------------------------------------------
N = 300
T = cc.T
LAYOUT_BYTES = {"static3d": 64, "symmetric": 72, "full": 96}


def camera(k=0):
    return (4.0 * k - 6.0, 3.0 - 1.5 * k, 150.0 + 2.0 * k)


def record_set(gs4d, layout):
    """one record set per layout of the SoA shadow (as tests/test_gpu_edit.py builds them): static 3D splats (one mu_t: nothing is dead), a
    symmetric sig, a sig that is not symmetric"""
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(N, seed=0x4350)
    pos4 = pos4.copy()
    pos4[:, :3] *= 0.2
    pos4[:, 3] = T - 1.0 + pos4[:, 3] / 25.0
    if layout == "static3d":
        rec = gs4d.build_records_3d(pos4[:, :3].copy(), q, scale * 12.0, rgba)
        rec[:, 3] = T
        return rec
    rec = gs4d.build_records_4d(pos4, q, scale * 12.0, life * 4.0, fade, vel * 0.2, rgba)
    sig = rec[:, 8:].reshape(-1, 4, 4)
    iu = np.triu_indices(4, 1)
    sig[:, iu[0], iu[1]] = sig[:, iu[1], iu[0]]
    if layout == "full":
        rec[:, 8 + 1] *= f32(1.25)                              # sig[0][1] != sig[1][0]
    return rec


class Scene:
    def __init__(self, gs4d, rec, outputs=False, aux=False):
        self.gs4d, self.rec, self.n = gs4d, rec, rec.shape[0]
        self.ctx = c = gs4d.Context(W, H)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        if outputs:
            c.set_id_outputs(True)                              # (a frame with ID outputs has aux outputs too)
        elif aux:
            c.set_aux_outputs(True)
        self.outputs = outputs
        self.db = c.buffer(rec)
        self.kb, self.ib = c.buffer(nbytes=4 * self.n), c.buffer(nbytes=4 * self.n)
        self.proj = gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)

    def view(self, k=0):
        return self.gs4d.look_at(camera(k), (0.0, 0.0, -1.0))

    def frame(self, mode, k=0, t=T, data=None, count=None):
        c, gs4d, cam = self.ctx, self.gs4d, camera(k)
        data, count = (self.db, self.n) if data is None else (data, count)
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=self.view(k), proj=self.proj)
        if mode == gs4d.MODE_4D_SORTED:
            c.keygen(data, t, cam, self.kb, self.ib, count)
            c.sort_pairs(self.kb, self.ib, count)
        c.set_mode(mode)
        if mode == gs4d.MODE_4D_SORTED:
            c.bind(1, self.ib)
            c.bind(2, data)
        else:
            c.bind(1, data)                                     # (instance k is record k)
        c.draw_instanced(count)

    def read(self):
        c = self.ctx
        out = [c.read_pixels()]
        if self.outputs:
            out += [c.read_aux(), *c.read_ids()]
        return out


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w)), f"{int((bits(g) != bits(w)).sum())} words differ"


@pytest.mark.parametrize("layout", tuple(LAYOUT_BYTES))
def test_the_records_and_a_current_shadow_give_the_same_table(gs4d, layout):
    rec = record_set(gs4d, layout)
    s = Scene(gs4d, rec)
    c = s.ctx
    mask = cc.mask_for(cc.RECT)
    queries = [(cc.query(cc.ALL_BITS & ~cc.SKIP_HIDDEN, view=s.view(1), proj=s.proj), mask), (cc.query(cc.ALL_BITS, view=s.view(1), proj=s.proj), mask),
               (cc.query(cc.BOX), None), (cc.query(cc.SKIP_HIDDEN | cc.SPHERE | cc.FRAME, cc.REMOVE), None)]
    start = cc.table("random", N)
    stats, mb = c.buffer(start), c.buffer(mask)

    def tables(records, what):
        out = []
        for k, (q, m) in enumerate(queries):
            c.subdata(stats, start)
            c.count_centres(stats, N, s.db, mask=mb if m is not None else None, query=cc.struct(q))
            got = c.read(stats, cc.STAT, N)
            want, part = cc.restate(records, q, start, m)
            assert got.tobytes() == want.tobytes(), f"{layout}, {what}, query {k}: {int((got != want).sum())} rows differ"
            assert 0 < int(part.sum()) < N, (layout, what, k)
            out.append(got.tobytes())
        return out

    first = tables(rec, "no shadow")                            # right after the upload: the 96-byte records
    assert c.shadow_builds(s.db) == 0, "the call built a shadow"
    s.frame(gs4d.MODE_4D_SORTED, 0)                             # keygen + draw: the shadow exists and is current
    assert c.shadow_builds(s.db) == 1 and c.stats()["record_read_bytes"] == LAYOUT_BYTES[layout]
    assert tables(rec, "shadow current") == first
    assert c.shadow_builds(s.db) == 1
    # half the set hidden by gs4d_edit_colours: the shadow's colour plane is patched, and SKIP_HIDDEN reads the alpha from it
    half, rule, _ = ec.tables(N)["alternating"]
    hb = c.buffer(half)
    c.hide(s.db, N, hb, **ec.rule_keywords(rule))
    hidden = ec.edit(rec, "set", 8, (0.0, 0.0, 0.0, 0.0), stats=half, rule=rule)
    assert c.stats()["lanes"] > 1
    c.clear()                                                   # the frame is complete: the next lane — the patched shadow is read from another lane than the one that built and patched it
    patched = tables(hidden, "shadow patched")
    assert patched[1] != first[1] and patched[3] != first[3] and patched[0] == first[0] and patched[2] == first[2]
    assert c.shadow_builds(s.db) == 1, "the call or the edit made the shadow stale"
    s.frame(gs4d.MODE_4D_SORTED, 1)
    s.read()
    assert c.shadow_builds(s.db) == 1, "the call invalidated the shadow"
    # ... and the same tables from the records of a fresh upload of the hidden set
    c.subdata(s.db, hidden)
    assert tables(hidden, "after a host write") == patched and c.shadow_builds(s.db) == 1
    c.finish()
    c.close()


# ---- 4. the draw tie -----------------------------------------------------------------------------------------------------------------------------
def test_a_screen_query_selects_the_records_whose_drawn_centre_is_in_the_rectangle(gs4d):
    rec = cc.records("symmetric", 1000)
    n = rec.shape[0]
    s = Scene(gs4d, rec, aux=True)
    c = s.ctx
    s.frame(gs4d.MODE_4D_DIRECT, 1)
    pj = c.debug_projected(n)
    cx, cy, valid, depth = pj[:, 0], pj[:, 1], pj[:, 14] != 0, pj[:, 15]
    assert valid.sum() > 500
    lo, hi = np.sort(depth[valid])[[valid.sum() // 5, 4 * valid.sum() // 5]]
    stats = c.record_stats(n)
    for rect, masked in (((10, 8, 37, 25), False), ((0, 0, W, H), False), ((20, 12, 30, 23), True)):
        x, y, w, h = rect
        m = cc.mask_for(rect) if masked else None
        c.subdata(stats, np.zeros(n, cc.STAT))
        c.count_centres(stats, n, s.db, mask=m, screen=(s.view(1), s.proj), rect=rect, depth=(lo, hi), t=T)
        got = c.read(stats, cc.STAT, n)["pixels"] == 1
        want = (cx >= x) & (cx < x + w) & (cy >= y) & (cy < y + h) & (depth >= lo) & (depth <= hi)
        if masked:
            inside = want & valid
            col, row = np.where(inside, np.floor(cx), x).astype(np.int64) - x, np.where(inside, np.floor(cy), y).astype(np.int64) - y
            want &= m[row, col] != 0
        assert np.array_equal(got[valid], want[valid]), f"rect {rect}: {int((got[valid] != want[valid]).sum())} valid records differ from the draw's centres"
        assert 20 < int(want[valid].sum()) < int(valid.sum()) - 20, (rect, int(want[valid].sum()))
    c.finish()
    c.close()


# ---- 5. ordering ---------------------------------------------------------------------------------------------------------------------------------
def stats_frame(s, table, k):
    c = s.ctx
    c.set_record_stats(table, s.n)
    s.frame(s.gs4d.MODE_4D_DIRECT, k)
    c.set_record_stats(None)


def test_the_call_adds_to_a_table_draws_are_still_adding_to(gs4d):
    """statistics draws on three lanes, then — nothing read in between — the call into the same table, then a statistics draw on the next lane:
    the rows are the draws' plus the call's"""
    rec = record_set(gs4d, "symmetric")
    s = Scene(gs4d, rec)
    c = s.ctx
    assert c.stats()["lanes"] > 1
    drawn = []
    for k in range(4):
        alone = c.record_stats(N)
        stats_frame(s, alone, k)
        drawn.append(c.read(alone, cc.STAT, N))                 # integers: the same draw adds the same rows every time
    assert all(int(d["pixels"].sum()) > 0 for d in drawn)
    q = cc.query(cc.BOX | cc.SKIP_HIDDEN)
    t = c.record_stats(N)
    for k in range(3):
        stats_frame(s, t, k)
    c.count_centres(t, N, s.db, query=cc.struct(q))
    stats_frame(s, t, 3)                                        # clear: the next lane; its draw adds to the table behind the call
    got = c.read(t, cc.STAT, N)
    want = np.zeros(N, cc.STAT)
    for d in drawn[:3]:
        want["pixels"] += d["pixels"]
        want["wmax"] = np.maximum(want["wmax"], d["wmax"])
        want["wsum"] += d["wsum"]
    want, part = cc.restate(rec, q, want)
    want["pixels"] += drawn[3]["pixels"]
    want["wmax"] = np.maximum(want["wmax"], drawn[3]["wmax"])
    want["wsum"] += drawn[3]["wsum"]
    assert 0 < int(part.sum()) < N
    assert got.tobytes() == want.tobytes(), f"{int((got != want).sum())} rows differ"
    c.finish()
    c.close()


def test_a_later_mask_upload_and_a_later_data_upload_do_not_change_the_result(gs4d):
    rec = cc.records("symmetric", 1000)
    ctx = gs4d.Context(W, H)
    m = cc.mask_for(cc.RECT)
    data, mb, t = ctx.buffer(rec), ctx.buffer(m), ctx.record_stats(1000)
    q = cc.query(cc.SCREEN | cc.SKIP_DEAD)
    ctx.count_centres(t, 1000, data, mask=mb, query=cc.struct(q))
    ctx.subdata(mb, np.where(m != 0, 0, 1).astype(np.uint8))    # directly behind: the call must not see the inverted lasso ...
    ctx.subdata(data, np.zeros_like(rec))                       # ... nor the zeroed records
    got = ctx.read(t, cc.STAT, 1000)
    want, part = cc.restate(rec, q, cc.table("zero", 1000), m)
    assert got.tobytes() == want.tobytes() and 0 < int(part.sum()) < 1000
    ctx.close()


def test_a_queued_keygen_that_names_the_table_runs_first(gs4d):
    """a key generation whose key buffer is then used as the table: the keys are written before the call reads and updates them"""
    rec = cc.records("symmetric", 1000)
    n = 250                                                     # 4 n key bytes = n / 4 rows
    twin = gs4d.Context(W, H)
    d2, k2, i2 = twin.buffer(rec), twin.buffer(nbytes=16 * n), twin.buffer(nbytes=4 * 4 * n)
    twin.keygen(d2, T, cc.CAM[0], k2, i2, 4 * n)
    keys = twin.read(k2, cc.STAT, n)
    twin.close()
    ctx = gs4d.Context(W, H)
    data, kb, ib = ctx.buffer(rec), ctx.buffer(nbytes=16 * n), ctx.buffer(nbytes=4 * 4 * n)
    ctx.keygen(data, T, cc.CAM[0], kb, ib, 4 * n)               # queued, not launched
    q = cc.query(cc.SPHERE)
    ctx.count_centres(kb, n, data, query=cc.struct(q))
    got = ctx.read(kb, cc.STAT, n)
    want, part = cc.restate(rec[:n], q, keys)
    assert got.tobytes() == want.tobytes() and 0 < int(part.sum()) < n
    ctx.close()


# ---- 6. the chain --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_select_volume_then_hide_draws_the_compacted_complement(gs4d, mode):
    mode = {"sorted": gs4d.MODE_4D_SORTED, "direct": gs4d.MODE_4D_DIRECT}[mode]
    rec = record_set(gs4d, "symmetric")
    assert np.isfinite(rec).all() and (rec[:, 23] > 0).all() and (rec[:, 7] > 0).all()
    box = ((-30.0, -40.0, -20.0), (20.0, 20.0, 40.0))
    inside = cc.takes_part(rec, cc.query(cc.BOX, box_lo=box[0], box_hi=box[1]))
    assert N // 5 <= int(inside.sum()) <= 4 * N // 5
    kept = np.flatnonzero(~inside)
    s = Scene(gs4d, rec, outputs=True)
    c = s.ctx
    s.frame(mode, 1)
    shown = s.read()
    dst, kept_index, count, stats = c.select_volume(N, s.db, src=s.db, box=box, t=T)
    assert count == int(inside.sum()) and np.array_equal(c.read(kept_index, np.uint32, count), np.flatnonzero(inside))
    assert np.array_equal(bits(c.read(dst, f32, count * 24)).reshape(count, 24), bits(rec[inside]))
    assert np.array_equal(c.read_record_stats(stats, N)["pixels"], inside.astype(np.uint32))
    rest, rest_index, rest_count = c.prune(stats, N, s.db, min_pixels=1, invert=True)
    assert rest_count == kept.size and np.array_equal(c.read(rest_index, np.uint32, kept.size), kept)
    c.hide(s.db, N, stats, min_pixels=1)
    s.frame(mode, 1)
    got = s.read()
    s.frame(mode, 1, data=rest, count=kept.size)
    want = s.read()
    same(got[:2], want[:2])                                     # the colour image and the aux planes
    (rid, draw, weight), (crid, cdraw, cweight) = got[2:], want[2:]
    assert np.array_equal(bits(weight), bits(cweight)) and np.array_equal(draw, cdraw)
    seen = rid != gs4d.Context.ID_NONE
    assert seen.sum() > 200 and np.array_equal(crid != gs4d.Context.ID_NONE, seen)
    assert np.array_equal(kept[crid[seen]], rid[seen]) and not inside[rid[seen]].any()
    assert int((np.abs(shown[0] - got[0]).max(-1) > 1.0 / 255.0).sum()) > 100, "hiding changed nothing visible"
    # without src no records are copied
    none, index2, count2, stats2 = c.select_volume(N, s.db, sphere=((0.0, 0.0, 0.0), 30.0), t=T, skip_hidden=True)
    ball = cc.takes_part(c.read(s.db, f32, N * 24).reshape(N, 24), cc.query(cc.SPHERE | cc.SKIP_HIDDEN, sphere=(0.0, 0.0, 0.0, 30.0)))
    assert none is None and count2 == int(ball.sum()) > 0 and np.array_equal(c.read(index2, np.uint32, count2), np.flatnonzero(ball))
    c.finish()
    c.close()
