"""GPU: gs4d_transform_selected — the selected records of a set moved in place under a 4D affine map about a pivot (include/gs4d.h).

The whole data buffer — n records, three more and a sentinel tail — is compared with the header's text restated in numpy (tests/xfsel_cases.py: equal as
uint32, a word that is a NaN on both sides counting as equal; byte for byte wherever nothing is selected), with guard buffers around data, stats and
measure and the two read buffers compared against what was uploaded; the chain count_centres -> measure_records -> transform_selected runs without a
read-back against the host chain; pictures drawn from moved records are compared bit for bit with those of a fresh context that uploaded the
host-moved records; gs4d_debug_shadow_builds shows the one repack a call costs.  All calls go through the Python binding over the C ABI."""
import ctypes

import numpy as np
import pytest

import build_cases as bc
import edit_cases as ec
import scenes
import staged_cases
import transform_cases as tc
import xfsel_cases as xc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
TAIL = 32                                                       # sentinel bytes behind the last record of data
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


def data_bytes(rec):
    """the records and a sentinel tail, as uploaded"""
    return np.concatenate([np.ascontiguousarray(rec, f32).reshape(-1).view(np.uint8), np.full(TAIL, SENTINEL, np.uint8)])


def check_data(ctx, data, rec, want, sel, n, what):
    got = ctx.read(data, np.uint8, rec.size * 4 + TAIL)
    assert (got[rec.size * 4:] == SENTINEL).all(), f"{what}: bytes of data behind the last record changed"
    xc.assert_records(got[:rec.size * 4].view(f32), want, rec, sel, n, what)


# ---- 1. the bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", xc.SETS)
def test_the_data_buffer_equals_the_restatement(gs4d, which):
    """every size, table and pivot form; the transform rows taken round and round"""
    ctx = gs4d.Context(64, 64)
    call = 0
    for n in xc.SIZES:
        rec = tc.records(gs4d, which, n + xc.EXTRA)
        for tname, table in xc.tables(n).items():
            sel = xc.selected(n, table)
            guards = [fill(ctx, GUARD)]
            stats = None
            if table[0] is not None:
                stats = ctx.buffer(table[0])
                guards.append(fill(ctx, GUARD))
            for form in xc.PIVOT_FORMS:
                name = tc.NAMES[call % len(tc.NAMES)]
                call += 1
                xf = tc.transforms()[name]
                what = f"{which}, n = {n}, {tname}, pivot {form}, {name}"
                pivot, measure = xc.pivot_case(gs4d, form, rec, n, table, call)
                data = ctx.buffer(data_bytes(rec))
                after = [fill(ctx, GUARD)]
                mb = None
                if measure is not None:
                    mb = ctx.buffer(np.concatenate([xc.measure_bytes(measure), np.full(GUARD, SENTINEL, np.uint8)]))
                    after.append(fill(ctx, GUARD))
                ctx.transform_selected(data, n, xf, stats=stats, pivot=pivot, measure=mb, **(ec.rule_keywords(table[1], table[2]) if stats else {}))
                check_data(ctx, data, rec, xc.expected(gs4d, rec, xf, n, table, pivot, measure), sel, n, what)
                assert all(untouched(ctx, g) for g in guards + after), f"{what}: a guard buffer changed"
                if stats:
                    assert ctx.read(stats, np.uint8, 16 * n).tobytes() == table[0].tobytes(), f"{what}: stats changed"
                if mb:
                    got = ctx.read(mb, np.uint8, 96 + GUARD)
                    assert got[:96].tobytes() == bytes(measure) and (got[96:] == SENTINEL).all(), f"{what}: measure changed"
                for b in after + [data] + ([mb] if mb else []):
                    ctx.delete(b)
            for b in guards + ([stats] if stats else []):
                ctx.delete(b)
    assert call >= 5 * len(tc.NAMES)
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


# ---- 2. the chain without a read-back ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (257, 769))
def test_select_measure_move_without_a_read_back(gs4d, n):
    rec = bc.host_records(gs4d, "4d_vel", bc.picture_set(gs4d, "4d_vel", n + xc.EXTRA, seed=0x5854))
    box, t = ((-25.0, -40.0, -30.0), (30.0, 15.0, 40.0)), bc.T
    xf = tc.row(tc.block4(1.25 * tc.rotation(tc.RIGID_AXIS, tc.RIGID_ANGLE)), (3.0, -2.0, 1.0, 0.0))
    # the host chain
    table = gs4d.count_centres_host(rec[:n], gs4d.centre_query(box=box, t=t), 64, 64)
    measure = gs4d.measure_records_host(rec[:n], t=t, stats=table, min_pixels=1)
    assert n // 8 <= measure.count <= 7 * n // 8 and measure.as_dict()["centre"] is not None
    want = gs4d.transform_selected_host(rec, xf, stats=table, measure=measure, n=n, min_pixels=1)
    # the device chain: three calls back to back
    ctx = gs4d.Context(64, 64)
    data, stats = ctx.buffer(data_bytes(rec)), ctx.record_stats(n)
    ctx.count_centres(stats, n, data, box=box, t=t)
    mb = ctx.measure_records(data, n, t=t, stats=stats, min_pixels=1)
    ctx.transform_selected(data, n, xf, stats=stats, measure=mb, min_pixels=1)
    sel = table["pixels"] >= 1
    check_data(ctx, data, rec, want, sel, n, f"n = {n}")
    assert ctx.read(mb, np.uint8, 96).tobytes() == bytes(measure) and ctx.read(stats, np.uint8, 16 * n).tobytes() == table.tobytes()
    assert (bits(want[:n][sel]) != bits(rec[:n][sel])).any(1).all(), "a selected record did not move: the test shows nothing"
    ctx.finish()
    ctx.close()


# ---- 3. pictures and the repack ------------------------------------------------------------------------------------------------------------------
W, H, N = 64, 48, 300
CAM, CAM_DIR = (0.0, 0.0, 150.0), (0.0, 0.0, -1.0)
MOVE = tc.row(tc.block4(tc.rotation(tc.RIGID_AXIS, tc.RIGID_ANGLE)), (6.0, -4.0, 3.0, 0.0))      # rigid, about MOVE_PIVOT
MOVE_PIVOT = (5.0, -3.0, 2.0)


class Scene:
    """a context with an uploaded record buffer, key buffers and the camera of the picture sets"""

    def __init__(self, gs4d, rec, outputs=False):
        self.gs4d, self.n, self.outputs = gs4d, rec.shape[0], outputs
        self.ctx = c = gs4d.Context(W, H)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        if outputs:
            c.set_id_outputs(True)                              # (a frame with ID outputs has aux outputs too)
        self.db = c.buffer(rec)
        self.kb, self.ib = c.buffer(nbytes=4 * self.n), c.buffer(nbytes=4 * self.n)
        self.view, self.proj = gs4d.look_at(CAM, CAM_DIR), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)

    def frame(self, mode, t, move=None):
        """one frame; move: called first — the documented order transform_selected -> keygen -> sort_pairs -> draw"""
        c, gs4d = self.ctx, self.gs4d
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=self.view, proj=self.proj)
        if move is not None:
            move()
        if mode == gs4d.MODE_4D_SORTED:
            c.keygen(self.db, t, CAM, self.kb, self.ib, self.n)
            c.sort_pairs(self.kb, self.ib, self.n)
        c.set_mode(mode)
        if mode == gs4d.MODE_4D_SORTED:
            c.bind(1, self.ib)
            c.bind(2, self.db)
        else:
            c.bind(1, self.db)                                  # (instance k is record k)
        c.draw_instanced(self.n)

    def read(self):
        c = self.ctx
        out = [c.read_pixels()]
        if self.outputs:
            out += [c.read_aux(), *c.read_ids()]
        return out


def host_frame(gs4d, rec, mode, t, outputs=False):
    """the frame of a fresh context that uploaded the records"""
    s = Scene(gs4d, rec, outputs)
    s.frame(mode, t)
    out = s.read()
    s.ctx.close()
    return out


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w)), f"{int((bits(g) != bits(w)).sum())} words differ"


def picture_records(gs4d, seed=0x5855):
    return bc.host_records(gs4d, "4d_vel", bc.picture_set(gs4d, "4d_vel", N, seed))


@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_pictures_from_moved_records_equal_those_from_uploaded_records(gs4d, mode):
    mode, t = {"sorted": gs4d.MODE_4D_SORTED, "direct": gs4d.MODE_4D_DIRECT}[mode], bc.T
    rec = picture_records(gs4d)
    tables = xc.tables(N)
    alt, none = tables["alternating"], tables["none_selected"]
    moved = gs4d.transform_selected_host(rec, MOVE, pivot=MOVE_PIVOT, **xc.keywords(alt))
    want0, want1 = host_frame(gs4d, rec, mode, t, outputs=True), host_frame(gs4d, moved, mode, t, outputs=True)
    assert not np.array_equal(bits(want0[0]), bits(want1[0])), "the move does not show: the test shows nothing"
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert int((np.abs(want1[0] - clear).max(-1) > 1.0 / 255.0).sum()) > 100, "an empty frame"
    s = Scene(gs4d, rec, outputs=True)
    c = s.ctx
    st_alt, st_none = c.buffer(alt[0]), c.buffer(none[0])
    s.frame(mode, t)
    same(s.read(), want0)
    assert c.shadow_builds(s.db) == 1
    # one repack for the call followed by a draw, none for a second draw
    s.frame(mode, t, lambda: c.transform_selected(s.db, N, MOVE, stats=st_alt, pivot=MOVE_PIVOT, **ec.rule_keywords(alt[1], alt[2])))
    same(s.read(), want1)
    assert c.shadow_builds(s.db) == 2, "a call must make the next draw repack exactly once"
    s.frame(mode, t)
    same(s.read(), want1)
    assert c.shadow_builds(s.db) == 2, "a second draw repacked"
    # a table that selects nothing: the same picture, and still a full write of data
    s.frame(mode, t, lambda: c.transform_selected(s.db, N, MOVE, stats=st_none, pivot=MOVE_PIVOT, **ec.rule_keywords(none[1], none[2])))
    same(s.read(), want1)
    assert c.shadow_builds(s.db) == 3, "a call that selects nothing still counts as a full write"
    assert xc.same_bits(c.read(s.db, f32, N * 24).reshape(N, 24), moved).all()
    c.finish()
    c.close()


# ---- 4. ordering without a finish ----------------------------------------------------------------------------------------------------------------
def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch):
    """a call on the buffer that the previous lane's draw still reads: that frame keeps the old records; host writes into stats and measure right
    behind the call do not change its result; transform_selected, keygen, sort and draw are queued back to back"""
    monkeypatch.setenv("GS4D_LANES", "4")
    mode, t = gs4d.MODE_4D_SORTED, bc.T
    rec = picture_records(gs4d, seed=0x5856)
    table = xc.tables(N)["alternating"]
    measure = gs4d.measure_records_host(rec, t=t, **xc.keywords(table))
    new_rec = gs4d.transform_selected_host(rec, MOVE, measure=measure, **xc.keywords(table))
    ref = Scene(gs4d, rec)
    ref.frame(mode, t)
    ref_rgba8 = ref.ctx.buffer(nbytes=W * H * 4)
    ref.ctx.read_frame_rgba8_device(0, ref.ctx.device_ptr(ref_rgba8)[0], W * H * 4)
    ref.ctx.finish()
    want_prev = ref.ctx.read(ref_rgba8, np.uint8, W * H * 4)
    ref.ctx.close()
    want = host_frame(gs4d, new_rec, mode, t)
    s = Scene(gs4d, rec)
    c = s.ctx
    assert c.stats()["lanes"] == 4
    stats, mb, out = c.buffer(table[0]), c.buffer(xc.measure_bytes(measure)), c.buffer(nbytes=W * H * 4)
    for _ in range(3):
        s.frame(mode, t)                                        # frames in flight that read the old records and their shadow
    s.frame(mode, t, lambda: c.transform_selected(s.db, N, MOVE, stats=stats, measure=mb, **ec.rule_keywords(table[1], table[2])))
    c.subdata(stats, np.zeros(N, ec.STAT))                      # directly behind: the call must not see the zeros
    c.subdata(mb, xc.measure_bytes(xc.hostile_measures(gs4d)[0]))
    c.read_frame_rgba8_device(1, c.device_ptr(out)[0], W * H * 4)
    got = s.read()
    c.finish()
    assert np.array_equal(c.read(out, np.uint8, W * H * 4), want_prev), "the frame before the call shows other records than it was drawn with"
    same(got, want)
    assert not np.array_equal(bits(got[0]), bits(host_frame(gs4d, rec, mode, t)[0])), "the move does not show: the test shows nothing"
    assert xc.same_bits(c.read(s.db, f32, N * 24).reshape(N, 24), new_rec).all(), "the records are not those of stats and measure as they were at the call"
    assert c.shadow_builds(s.db) == 2
    c.close()


def test_two_calls_back_to_back_equal_the_hosts_two_calls(gs4d):
    """overlapping selections, the second about the pivot measured from the result of the first — measured on the device between the two"""
    n, t = 769, bc.T
    rec = bc.host_records(gs4d, "4d_2q", bc.picture_set(gs4d, "4d_2q", n, seed=0x5857))
    tables = xc.tables(n)
    one, two = tables["alternating"], tables["a_tile_unselected"]
    first = gs4d.transform_selected_host(rec, MOVE, pivot=MOVE_PIVOT, **xc.keywords(one))
    measure = gs4d.measure_records_host(first, t=t, **xc.keywords(two))
    second = gs4d.transform_selected_host(first, tc.transforms()["scale_shear"], measure=measure, **xc.keywords(two))
    ctx = gs4d.Context(64, 64)
    data, s1, s2 = ctx.buffer(rec), ctx.buffer(one[0]), ctx.buffer(two[0])
    ctx.transform_selected(data, n, MOVE, stats=s1, pivot=MOVE_PIVOT, **ec.rule_keywords(one[1], one[2]))
    mb = ctx.measure_records(data, n, t=t, stats=s2, **ec.rule_keywords(two[1], two[2]))
    ctx.transform_selected(data, n, tc.transforms()["scale_shear"], stats=s2, measure=mb, **ec.rule_keywords(two[1], two[2]))
    got = ctx.read(data, f32, n * 24).reshape(n, 24)
    ok = xc.same_bits(got, second)
    assert ok.all(), f"{int((~ok).any(1).sum())} records differ from the host's two calls"
    assert ctx.read(mb, np.uint8, 96).tobytes() == bytes(measure)
    ctx.finish()
    ctx.close()


def sorted_frame(gs4d, ctx, bufs, n, t):
    db, kb, ib = bufs
    view, proj = staged_cases.mats(gs4d)
    ctx.clear()
    ctx.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
    ctx.keygen(db, t, staged_cases.CAM[0], kb, ib, n)
    ctx.sort_pairs(kb, ib, n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.draw_instanced(n)


def test_a_call_waits_for_a_rerun(gs4d, monkeypatch):
    """staged_cases' case a (as tests/test_gpu_transform.py; its scene fixes the 640 x 360 context): frames at T0 teach the guesses, the frame at T1
    outgrows a segment block; the call on its record buffer settles the draw first — the re-run uses the old records"""
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    rec, _ = staged_cases.build(gs4d, "a")
    Wb, Hb, n = staged_cases.W, staged_cases.H, rec.shape[0]
    xf = tc.transforms()["scale_shear"]
    fresh = gs4d.Context(Wb, Hb)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    sorted_frame(gs4d, fresh, (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n)), n, staged_cases.T1)
    want = fresh.read_pixels()
    fresh.close()
    ctx = gs4d.Context(Wb, Hb)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    ctx.transform_selected(bufs[0], n, xf, pivot=xc.PIVOT)                        # no read-back in between
    s1 = ctx.stats()
    assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    got = ctx.read_pixels()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"
    assert xc.same_bits(ctx.read(bufs[0], f32, n * 24).reshape(n, 24), gs4d.transform_selected_host(rec, xf, pivot=xc.PIVOT)).all()
    ctx.finish()
    ctx.close()


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_everything_as_it_was(gs4d):
    n = 300
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    rec = tc.records(gs4d, "4d_vel", n)
    table = xc.tables(n)["alternating"]
    measure = gs4d.measure_records_host(rec, t=0.25, **xc.keywords(table))
    data, stats, mb = ctx.buffer(data_bytes(rec)), ctx.buffer(table[0]), ctx.buffer(xc.measure_bytes(measure))
    short_data, short_stats, short_mb, dead = ctx.buffer(rec.reshape(-1)[:-1]), ctx.buffer(table[0][:-1]), fill(ctx, 95), fill(ctx, 64)
    ctx.delete(dead)                                            # (last: a buffer made from here on could take its name)
    NO = object()
    good_rule = gs4d._keep_rule(**ec.rule_keywords(table[1], table[2]))
    xf = tc.transforms()["full"]

    def call(data=data, n=n, x=None, flags=gs4d.XS_PIVOT_MEASURE, stats=stats, rule=good_rule, measure=mb, rule_flags=None, rule_reserved=None):
        s = gs4d.selection_xf(xf, pivot=xc.PIVOT)
        s.flags = flags
        k = None if rule is None else rule.copy()
        if rule_flags is not None:
            k["flags"] = rule_flags
        if rule_reserved is not None:
            k["reserved"] = rule_reserved
        return lib.gs4d_transform_selected(ctx._h, data, ctypes.c_size_t(n), None if x is NO else ctypes.byref(s), stats,
                                           None if k is None else k.ctypes.data, measure)

    bad = {
        "xf == NULL": dict(x=NO), "flags 3": dict(flags=3), "flags 4": dict(flags=4, measure=0), "flag bit 31": dict(flags=0x80000000, measure=0),
        "n > 0xFFFFFFFF": dict(n=1 << 32), "no data": dict(data=0), "dead data": dict(data=dead), "unknown data": dict(data=9999),
        "data too small": dict(data=short_data), "stats without a rule": dict(rule=None), "a rule without stats": dict(stats=0),
        "rule flag 2": dict(rule_flags=2), "rule reserved": dict(rule_reserved=1), "dead stats": dict(stats=dead), "unknown stats": dict(stats=9999),
        "stats too small": dict(stats=short_stats), "GS4D_XS_PIVOT_MEASURE without measure": dict(measure=0), "dead measure": dict(measure=dead),
        "unknown measure": dict(measure=9999), "measure too small": dict(measure=short_mb), "measure without the flag": dict(flags=0),
        "measure with GS4D_XS_PIVOT": dict(flags=gs4d.XS_PIVOT), "data == stats": dict(stats=data), "data == measure": dict(measure=data),
        "stats == measure": dict(measure=stats), "data == measure without a table": dict(measure=data, stats=0, rule=None),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"transform_selected" in lib.gs4d_last_error(ctx._h), what
    assert call(n=0, flags=3) == -1 and call(n=0, measure=dead) == -1                # ... with no records too
    ctx.finish()

    def as_uploaded():
        return (ctx.read(data, np.uint8, n * 96 + TAIL).tobytes() == data_bytes(rec).tobytes() and ctx.read(stats, np.uint8, 16 * n).tobytes() == table[0].tobytes()
                and ctx.read(mb, np.uint8, 96).tobytes() == bytes(measure) and untouched(ctx, short_mb, 95)
                and ctx.read(short_data, np.uint8, n * 96 - 4).tobytes() == rec.tobytes()[:-4])

    assert as_uploaded(), "a refused call wrote something"
    assert ctx.shadow_builds(data) == 0
    # n == 0 is a no-op
    assert call(n=0) == 0 and call(n=0, stats=0, rule=None, measure=0, flags=0) == 0
    ctx.finish()
    assert as_uploaded(), "a call with n == 0 wrote something"
    # the call works after the refusals; stats == 0 gives every record
    sel = xc.selected(n, table)
    assert call() == 0
    check_data(ctx, data, rec, xc.expected(gs4d, rec, xf, n, table, None, measure), sel, n, "after the refusals")
    ctx.subdata(data, data_bytes(rec))
    assert call(stats=0, rule=None, measure=0, flags=gs4d.XS_PIVOT) == 0
    check_data(ctx, data, rec, xc.by_the_text(rec, xf, np.ones(n, bool), xc.PIVOT), np.ones(n, bool), n, "stats == 0")
    assert ctx.read(stats, np.uint8, 16 * n).tobytes() == table[0].tobytes() and ctx.read(mb, np.uint8, 96).tobytes() == bytes(measure)
    ctx.finish()
    ctx.close()
