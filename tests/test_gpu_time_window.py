"""GPU: gs4d_record_time_spans and gs4d_compact_time_window — the records of a 4D set that can show anything between two times (include/gs4d.h,
DESIGN.md §4).

The span table is bit-equal to the numpy restatement (tests/time_window_cases.py: float32 operations, so exact); the premise it rests on — the
device's expf is exactly 0 below GS4D_TIME_DEAD_ARG — is checked on the projected records; the compaction is exact against np.flatnonzero on the
window rule, with sentinel-filled outputs and guard buffers; and a draw of the compacted set gives the bits of a draw of the full set in every
output.  All calls go through the Python binding over the C ABI."""
import ctypes
import functools

import numpy as np
import pytest

import compact_cases as cc
import hostile_cases as hc
import scenes
import time_window_cases as tw

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
W, H, N = 320, 192, 4096
T0, T1 = 24.0, 26.0                                        # the window of the end-to-end tests


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=1)
def cube4d(gs4d):
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(N)
    rec = gs4d.build_records_4d(pos4, q, scale * 3.0, life, fade, vel, rgba)          # (the scale of the smoke frame: a few pixels per splat at 320 x 192)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=1)
def cube4d_spans(gs4d):
    table = tw.spans(cube4d(gs4d))
    table.setflags(write=False)
    return table


# ---- 1. spans -----------------------------------------------------------------------------------------------------------------------------------
def test_the_span_table_equals_the_reference_bit_for_bit(gs4d):
    ctx = gs4d.Context(64, 64)
    for n in tw.SPAN_SIZES:
        rec = cube4d(gs4d)[:n]
        db = ctx.buffer(rec)
        sb = ctx.buffer(np.full(n * 8 + 64, SENTINEL, np.uint8))
        ctx.record_time_spans(db, n, 0.0, sb)
        got = ctx.read(sb, np.uint8, n * 8 + 64)
        assert np.array_equal(got[:n * 8].view(np.uint32), bits(cube4d_spans(gs4d)[:n]).reshape(-1)), n
        assert (got[n * 8:] == SENTINEL).all(), "bytes behind the n spans changed"
        ctx.record_time_spans(db, n, 0.25, sb)              # a floor: every record always (their colour alpha is > 0)
        assert np.array_equal(ctx.read(sb, tw.SPAN, n), tw.spans(rec, 0.25)) and np.isinf(ctx.read(sb, np.float32, 2 * n)).all()
        ctx.delete(db)
        ctx.delete(sb)
    ctx.close()


def test_the_three_classes_on_the_device(gs4d):
    ctx = gs4d.Context(64, 64)
    for floor in tw.CLASS_FLOORS:
        rec, want = tw.class_records(floor)
        # the hand-written rows scattered among ordinary records (past one workgroup)
        mixed = np.array(cube4d(gs4d)[:300])
        at = np.linspace(0, 299, len(want)).astype(int)
        mixed[at] = rec
        db = ctx.buffer(mixed)
        sb = ctx.record_time_spans(db, 300, float(floor))
        got = ctx.read(sb, tw.SPAN, 300)
        ref = tw.spans(mixed, floor)
        assert np.array_equal(bits(got), bits(ref)), float(floor)
        for i, w in zip(at, want):
            if w != "span":
                assert (got["t_first"][i], got["t_last"][i]) == w
        ctx.delete(db)
        ctx.delete(sb)
    ctx.close()


def test_no_records_is_a_no_op_and_bad_arguments_queue_nothing(gs4d):
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    db = ctx.buffer(cube4d(gs4d)[:10])
    sb, dead = ctx.buffer(np.full(80, SENTINEL, np.uint8)), ctx.buffer(nbytes=64)
    ctx.delete(dead)
    call = lambda data, n, spans: lib.gs4d_record_time_spans(ctx._h, data, ctypes.c_size_t(n), 0.0, spans)
    assert call(db, 0, sb) == 0
    for what, args in {"n > 0xFFFFFFFF": (db, 1 << 32, sb), "data too small": (db, 11, sb), "data == spans": (db, 1, db),
                       "dead buffer": (db, 1, dead), "no data": (0, 1, sb), "no spans": (db, 1, 0), "unknown name": (db, 1, 9999)}.items():
        assert call(*args) == -1 and lib.gs4d_last_error(ctx._h), what
    small = ctx.buffer(np.full(72, SENTINEL, np.uint8))
    assert call(db, 10, small) == -1                        # nine spans of room
    ctx.finish()
    assert (ctx.read(sb, np.uint8, 80) == SENTINEL).all() and (ctx.read(small, np.uint8, 72) == SENTINEL).all()
    assert call(db, 10, sb) == 0
    assert np.array_equal(ctx.read(sb, tw.SPAN, 10), cube4d_spans(gs4d)[:10])
    ctx.close()


# ---- 2. the premise: the device's exponential is exactly 0 below GS4D_TIME_DEAD_ARG ----------------------------------------------------------------
def direct_frame(ctx, gs4d, db, n, t, view, proj, min_opacity=0.0):
    ctx.clear()
    ctx.set_uniforms(time=t, min_opacity=min_opacity, view=view, proj=proj)
    ctx.set_mode(gs4d.MODE_4D_DIRECT)
    ctx.bind(1, db)
    ctx.draw_instanced(n)


def test_the_exponential_is_zero_below_the_dead_argument(gs4d):
    """4096 static records (s44 = 1, no coupling of space and time) with colour alpha 1, drawn at t = 0 with mu_t chosen so that the argument of
    the opacity's exponential covers [-130, -106) — slot 6 of the projected record, the alpha, is exactly 0 — and, as the control that the slot
    says anything, (-80, -60]: the alpha is > 0 there."""
    pos, q, scale, rgba = scenes.cube_params(N)
    rgba = np.array(rgba)
    rgba[:, 3] = 1.0
    rec = gs4d.build_records_3d(pos, q, scale * 3.0, rgba)
    assert (rec[:, 23] == 1.0).all() and (rec[:, 7] == 1.0).all()
    view, proj = gs4d.look_at(*scenes.CAM_CUBE), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    ctx = gs4d.Context(W, H)
    for lo, hi, dead in ((106.0, 130.0, True), (60.0, 80.0, False)):
        a = np.linspace(lo, hi, N, endpoint=False) + (hi - lo) / N * 0.5                     # the arguments aimed at, strictly inside
        band = np.array(rec)
        band[:, 3] = np.sqrt(2.0 * a).astype(np.float32)                                      # t = 0: dt = -mu
        got_arg = tw.arg(np.float32(0.0), band[:, 3], np.float32(1.0))
        assert (got_arg >= -hi).all() and (got_arg < -lo).all() and np.unique(got_arg).size > N // 2
        db = ctx.buffer(band)
        direct_frame(ctx, gs4d, db, N, 0.0, view, proj)
        p = ctx.debug_projected(N)
        valid = p[:, 14] == 1.0
        assert valid.sum() > N // 4, "most records must be in front of the camera"
        if dead:
            assert (bits(p[:, 6]) == 0).all(), f"{int((bits(p[:, 6]) != 0).sum())} records have a non-zero alpha below the dead argument"
            assert tw.keeps(tw.spans(band), 0.0, 0.0).sum() == 0                                # ... and the spans say so
        else:
            assert (p[valid, 6] > 0.0).all() and tw.keeps(tw.spans(band), 0.0, 0.0).all()
        ctx.delete(db)
    ctx.close()


def test_the_alpha_is_zero_one_float_beyond_each_span(gs4d):
    """every cube_params_4d record alone, drawn at nextafter(t_last): slot 6, the alpha, is exactly 0; every 64th also at nextafter(t_first, -inf)"""
    rec, table = cube4d(gs4d), cube4d_spans(gs4d)
    view, proj = gs4d.look_at(*scenes.CAM_CUBE), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    ctx = gs4d.Context(64, 64)
    one = ctx.buffer(rec[:1])
    ctx.set_mode(gs4d.MODE_4D_DIRECT)
    ctx.bind(1, one)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
    after, before = np.nextafter(table["t_last"], tw.INF), np.nextafter(table["t_first"], -tw.INF)
    bad = 0
    for i in range(N):
        ctx.subdata(one, rec[i])
        for t in (after[i],) if i % 64 else (after[i], before[i]):
            ctx.set_uniforms(time=float(t))
            ctx.draw_instanced(1)
            bad += int(bits(ctx.debug_projected(1)[0, 6:7])[0] != 0)
    ctx.close()
    assert bad == 0, f"{bad} draws one float beyond a span had a non-zero alpha"


# ---- 3. compaction --------------------------------------------------------------------------------------------------------------------------------
WINDOWS = {"middle": (24.0, 26.0), "all": (-np.inf, np.inf), "none": (1e9, 2e9), "point": (25.0, 25.0)}


class Table:
    """one context holding n records of `stride` bytes and a span table of n rows; run() compacts into fresh sentinel-filled outputs and checks
    every byte of them, and of a guard buffer created right behind each, against the reference"""

    def __init__(self, gs4d, n, stride):
        self.n, self.stride = n, stride
        self.ctx = gs4d.Context(64, 64)
        self.src_host = cc.records(n, stride)
        self.src = self.ctx.buffer(self.src_host) if n else self.ctx.buffer(nbytes=16)
        self.spans = self.ctx.buffer(nbytes=max(16, 8 * n))
        self.upload(tw.window_table(n))
        self.count = self.ctx.buffer(np.full(8, SENTINEL, np.uint8))
        self.count_guard = self.ctx.buffer(np.full(4096, SENTINEL, np.uint8))

    def upload(self, table):
        self.table = table
        if self.n:
            self.ctx.subdata(self.spans, table)

    def sentinel(self, slots, unit):
        nbytes = max(16, slots * unit)
        return self.ctx.buffer(np.full(nbytes, SENTINEL, np.uint8)), self.ctx.buffer(np.full(4096, SENTINEL, np.uint8)), nbytes

    def run(self, window, cap_dst="n", cap_idx="n"):
        c, n, stride = self.ctx, self.n, self.stride
        cd, ci = (n if cap_dst == "n" else cap_dst), (n if cap_idx == "n" else cap_idx)
        dst = guard_d = idx = guard_i = None
        if cd is not None:
            dst, guard_d, dbytes = self.sentinel(cd, stride)
        if ci is not None:
            idx, guard_i, ibytes = self.sentinel(ci, 4)
        c.compact_time_window(self.spans, n, *window, src=self.src if dst else None, stride=stride, dst=dst, kept_index=idx, count=self.count)
        kept, written = c.read_compact_count(self.count)
        real_d, real_i = (None if cd is None else dbytes // stride), (None if ci is None else ibytes // 4)      # (a buffer is at least 16 bytes)
        want_d, want_i, want_kept, want_written = tw.reference(self.table, *window, self.src_host if dst else None, stride, real_d, real_i)
        assert (kept, written) == (want_kept, want_written), (kept, written, want_kept, want_written)
        if dst:
            got = c.read(dst, np.uint8, dbytes)
            assert np.array_equal(got[:written * stride].reshape(written, stride), want_d), "dst differs from the reference"
            assert (got[written * stride:] == SENTINEL).all(), "bytes of dst beyond the written slots changed"
            assert (c.read(guard_d, np.uint8, 4096) == SENTINEL).all(), "the buffer created after dst changed"
        if idx:
            got = c.read(idx, np.uint8, ibytes)
            assert np.array_equal(got[:written * 4].view(np.uint32), want_i), "kept_index differs from the reference"
            assert (got[written * 4:] == SENTINEL).all(), "bytes of kept_index beyond the written slots changed"
            assert (c.read(guard_i, np.uint8, 4096) == SENTINEL).all(), "the buffer created after kept_index changed"
        assert (c.read(self.count_guard, np.uint8, 4096) == SENTINEL).all(), "the buffer created after count changed"
        for b in (dst, guard_d, idx, guard_i):
            if b:
                c.delete(b)
        return kept, written


@pytest.mark.parametrize("stride", tw.STRIDES)
@pytest.mark.parametrize("n", tw.COMPACT_SIZES)
def test_every_window_equals_the_reference(gs4d, n, stride):
    t = Table(gs4d, n, stride)
    t.upload(tw.window_table(n, finite=True))                # finite spans: a far window keeps none, an infinite one all
    kept = {name: t.run(w)[0] for name, w in WINDOWS.items()}
    assert kept["none"] == 0 and kept["all"] == n and kept["point"] <= kept["middle"] <= n
    t.upload(tw.window_table(n))                             # every kind of row, never, always and NaN rows among them
    kept = {name: t.run(w)[0] for name, w in WINDOWS.items()}
    if n >= 64:
        assert 0 < kept["none"] < kept["point"] <= kept["middle"] < kept["all"] < n          # (always rows meet any window; never and NaN rows none)
    k = kept["middle"]
    # outputs smaller than the kept set: kept > written, nothing beyond the capacity
    for cap_dst, cap_idx in ((k // 2, k // 2), (max(k - 1, 0), "n"), ("n", k // 2), (k // 2, None), (None, max(k - 1, 0)), (0, 0)):
        got, written = t.run(WINDOWS["middle"], cap_dst=cap_dst, cap_idx=cap_idx)
        assert got == k and written <= k
    if k > 8:
        assert t.run(WINDOWS["middle"], cap_dst=k // 2, cap_idx=k // 2) == (k, k // 2)
    # the optional outputs
    assert t.run(WINDOWS["middle"], cap_dst=None) == (k, k)                         # index only
    assert t.run(WINDOWS["middle"], cap_idx=None) == (k, k)                         # records only
    assert t.run(WINDOWS["middle"], cap_dst=None, cap_idx=None) == (k, k)           # count only
    t.ctx.close()


def test_argument_errors_leave_the_outputs_as_they_were(gs4d):
    n, stride = 300, 96
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    fill = lambda nbytes: ctx.buffer(np.full(nbytes, SENTINEL, np.uint8))
    table = tw.window_table(n)
    spans, src, dst, idx, count = ctx.buffer(table), ctx.buffer(cc.records(n, stride)), fill(n * stride), fill(n * 4), fill(8)
    short_spans, short_src, short_count, dead = ctx.buffer(table[:-1]), ctx.buffer(cc.records(n, stride)[:-1]), fill(4), fill(64)
    ctx.delete(dead)

    def call(spans=spans, n=n, t0=24.0, t1=26.0, src=src, stride=stride, dst=dst, idx=idx, count=count):
        return lib.gs4d_compact_time_window(ctx._h, spans, ctypes.c_size_t(n), t0, t1, src, stride, dst, idx, count)

    bad = {
        "t0 NaN": dict(t0=np.nan), "t1 NaN": dict(t1=np.nan), "both NaN": dict(t0=np.nan, t1=np.nan), "t0 > t1": dict(t0=26.0, t1=24.0), "inf > -inf": dict(t0=np.inf, t1=-np.inf),
        "n > 0xFFFFFFFF": dict(n=1 << 32), "spans too small": dict(spans=short_spans), "src too small": dict(src=short_src), "count too small": dict(count=short_count),
        "dst without src": dict(src=0), "spans == src": dict(src=spans), "src == dst": dict(dst=src), "dst == kept_index": dict(idx=dst), "kept_index == count": dict(count=idx),
        "spans == count": dict(count=spans), "spans == dst": dict(dst=spans), "stride 0": dict(stride=0), "stride not a multiple of 16": dict(stride=100),
        "stride above 1024": dict(stride=1040), "no count": dict(count=0), "no spans": dict(spans=0), "dead buffer": dict(idx=dead), "unknown name": dict(dst=9999),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    for b, nbytes in ((dst, n * stride), (idx, n * 4), (count, 8), (short_count, 4)):
        assert (ctx.read(b, np.uint8, nbytes) == SENTINEL).all(), "a refused call wrote something"
    assert np.array_equal(bits(ctx.read(spans, tw.SPAN, n)), bits(table))
    for t0, t1 in ((24.0, 26.0), (-np.inf, np.inf), (25.0, 25.0), (np.inf, np.inf)):          # valid, infinite ends included: the call works after the refusals
        assert call(t0=t0, t1=t1) == 0
        _, want_i, kept, _ = tw.reference(table, t0, t1, None, stride, n, n)
        assert ctx.read_compact_count(count) == (kept, kept) and np.array_equal(ctx.read(idx, np.uint32, kept), want_i)
    ctx.close()


# ---- 4. end to end: the compacted set draws the same bits -----------------------------------------------------------------------------------------------
FAR = 3.0e6                                                # from this far away the cloud's depth keys (1 / distance) span ~2000 float32 steps: many equal keys


def cameras(gs4d):
    """near: the cube camera.  far: the same picture, but the depth keys are generated for a point FAR behind the camera along its axis (gs4d_keygen
    takes the position the keys are measured from as an argument of its own): the same back-to-front direction, in steps so coarse that most
    records share their key with others and the stable sort's index order decides"""
    pos, ori = np.array(scenes.CAM_CUBE[0]), np.array(scenes.CAM_CUBE[1])
    view, proj = gs4d.look_at(*scenes.CAM_CUBE), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    behind = tuple(float(x) for x in pos - FAR * ori / np.linalg.norm(ori))
    return (scenes.CAM_CUBE, view, proj), ((behind, scenes.CAM_CUBE[1]), view, proj)


class Scene:
    """a context with the full set and, through Context.time_window, its compaction to [T0, T1]"""

    def __init__(self, gs4d, rec=None, window=(T0, T1), min_opacity=0.0, w=W, h=H):
        self.gs4d = gs4d
        self.rec = cube4d(gs4d) if rec is None else rec
        self.n = self.rec.shape[0]
        self.min_opacity = min_opacity
        self.ctx = c = gs4d.Context(w, h)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        self.db = c.buffer(self.rec)
        self.kb, self.ib = c.buffer(nbytes=4 * self.n), c.buffer(nbytes=4 * self.n)
        self.cdb, kidx, self.kept = c.time_window(self.db, self.n, *window, min_opacity=min_opacity)
        self.index = c.read(kidx, np.uint32, self.kept)
        want = np.flatnonzero(tw.keeps(tw.spans(self.rec, min_opacity), *window))
        assert np.array_equal(self.index, want)
        assert np.array_equal(bits(c.read(self.cdb, np.float32, self.kept * 24)).reshape(-1, 24), bits(self.rec[self.index]))

    def frame(self, compacted, t, camera, sort):
        c, gs4d = self.ctx, self.gs4d
        data, count = (self.cdb, self.kept) if compacted else (self.db, self.n)
        cam, view, proj = camera
        c.clear()
        c.set_uniforms(time=t, min_opacity=self.min_opacity, view=view, proj=proj)
        if sort:
            c.keygen(data, t, cam[0], self.kb, self.ib, count)
            c.sort_pairs(self.kb, self.ib, count)
            c.set_mode(gs4d.MODE_4D_SORTED)
            c.bind(1, self.ib)
            c.bind(2, data)
        else:
            c.set_mode(gs4d.MODE_4D_DIRECT)
            c.bind(1, data)
        c.draw_instanced(count)


@pytest.mark.parametrize("path", ["sorted-staged", "sorted-exact", "direct"])
def test_the_compacted_set_draws_the_same_colour(gs4d, monkeypatch, path):
    if path == "sorted-exact":
        monkeypatch.setenv("GS4D_STAGED", "0")
    else:
        monkeypatch.delenv("GS4D_STAGED", raising=False)
    s = Scene(gs4d)
    assert 0.1 * s.n <= s.kept <= 0.9 * s.n, s.kept           # equality cannot hold vacuously
    near, far = cameras(gs4d)
    clear = np.array(gs4d.CLEAR_COLOR, np.float32)
    # staged lists are built from what the frames before held: the draws from frame `lanes` on, of one set in a row, take them (test_gpu_staged.py)
    repeat = 2 * s.ctx.stats()["lanes"] + 2 if path == "sorted-staged" else 1
    for t, camera in ((24.0, near), (25.0, near), (26.0, near), (25.5, far)):
        for _ in range(repeat):
            s.frame(False, t, camera, path != "direct")
        full = s.ctx.read_pixels()
        if camera is far and path != "direct":
            keys = s.ctx.read(s.kb, np.uint32, s.n)
            assert np.unique(keys).size < s.n // 2, "the far camera must give many equal keys"
        dead = int((bits(s.ctx.debug_projected(s.n)[:, 6]) == 0).sum()) if path == "direct" else None
        for _ in range(repeat):
            s.frame(True, t, camera, path != "direct")
        got = s.ctx.read_pixels()
        diff = int((bits(got) != bits(full)).any(-1).sum())
        assert diff == 0, f"{path}, t = {t}: {diff} pixels differ"
        touched, shown = int((bits(full) != bits(clear)).any(-1).sum()), int((np.abs(full - clear).max(-1) > 1.0 / 255.0).sum())
        print(f"{path}, t = {t}: {touched} pixels touched, {shown} by more than 1/255")
        assert touched > 200 and shown > 20, "an empty frame"           # (most of the kept records are far down their opacity's tail at any one time)
        if dead is not None:
            assert dead >= s.n - s.kept                       # every dropped record had alpha 0 at this time
    staged = s.ctx.stats()["staged_draws"]
    assert staged > 0 if path == "sorted-staged" else staged == 0 if path == "sorted-exact" else True, s.ctx.stats()
    s.ctx.close()


def test_the_compacted_set_gives_the_same_aux_and_id_planes(gs4d, monkeypatch):
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    s = Scene(gs4d)
    near, _ = cameras(gs4d)
    s.ctx.set_id_outputs(True)                                # (a frame with ID outputs has aux outputs too)
    s.frame(False, 25.0, near, True)
    full, aux, (rid, draw, weight) = s.ctx.read_pixels(), s.ctx.read_aux(), s.ctx.read_ids()
    s.frame(True, 25.0, near, True)
    got, caux, (crid, cdraw, cweight) = s.ctx.read_pixels(), s.ctx.read_aux(), s.ctx.read_ids()
    s.ctx.close()
    assert np.array_equal(bits(got), bits(full)) and np.array_equal(bits(caux), bits(aux))
    assert np.array_equal(bits(cweight), bits(weight)) and np.array_equal(cdraw, draw)
    seen = rid != gs4d.Context.ID_NONE
    assert seen.sum() > 200 and np.array_equal(crid != gs4d.Context.ID_NONE, seen)
    assert np.array_equal(s.index[crid[seen]], rid[seen])
    assert (aux[..., 1] > 0).sum() > 200


def test_the_compacted_set_gives_the_same_record_statistics(gs4d, monkeypatch):
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    s = Scene(gs4d)
    near, _ = cameras(gs4d)
    sb, csb = s.ctx.record_stats(s.n), s.ctx.record_stats(s.kept)
    s.ctx.set_record_stats(sb, s.n)
    s.frame(False, 25.0, near, True)
    s.ctx.set_record_stats(csb, s.kept)
    s.frame(True, 25.0, near, True)
    full, got = s.ctx.read_record_stats(sb, s.n), s.ctx.read_record_stats(csb, s.kept)
    s.ctx.close()
    assert np.array_equal(full[s.index].view(np.uint8), got.view(np.uint8))
    dropped = np.ones(s.n, bool)
    dropped[s.index] = False
    assert dropped.sum() >= 0.1 * s.n and not full[dropped].view(np.uint8).any(), "a dropped record has statistics"
    assert (full["pixels"] > 0).sum() > 100


@pytest.mark.parametrize("name", ["several_at_once", "nan_inf_colour"])
def test_hostile_records_compact_and_draw_the_same(gs4d, name):
    """tests/hostile_cases.py records (NaN and Inf in positions, covariances, colours; dead ones) at the case's own time and floor: the span table
    equals the reference, the compacted set draws the same bits, and no call or device check reports an error"""
    c = hc.get(name)
    s = Scene(gs4d, rec=c.rec, window=(c.t, c.t), min_opacity=c.min_opacity, w=hc.W, h=hc.H)
    sb = s.ctx.record_time_spans(s.db, s.n, c.min_opacity)
    assert np.array_equal(bits(s.ctx.read(sb, tw.SPAN, s.n)), bits(tw.spans(c.rec, c.min_opacity)))
    camera = (c.cam, c.view, c.proj)
    for sort in (True, False):
        s.frame(False, c.t, camera, sort)
        full = s.ctx.read_pixels()
        s.frame(True, c.t, camera, sort)
        got = s.ctx.read_pixels()
        assert np.array_equal(bits(got), bits(full)), f"{name}, sort = {sort}: {int((bits(got) != bits(full)).any(-1).sum())} pixels differ"
    s.ctx.finish()                                            # reports device-side check failures
    s.ctx.close()


# ---- 5. ordering ----------------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_ordered_without_a_finish(gs4d, monkeypatch):
    """record_time_spans, compact_time_window straight behind it, a host write into src behind that — with frames on other lanes before and after:
    the result is that of call order"""
    monkeypatch.setenv("GS4D_LANES", "4")
    rec, table = cube4d(gs4d), cube4d_spans(gs4d)
    near, _ = cameras(gs4d)
    s = Scene(gs4d)
    assert s.ctx.stats()["lanes"] == 4
    c = s.ctx
    for k in range(3):                                        # frames in flight on three lanes; the calls below land on the fourth
        s.frame(False, 24.0 + k, near, True)
    c.clear()
    sb = c.buffer(np.full(N * 8, SENTINEL, np.uint8))
    dst, idx = c.buffer(np.full(N * 96, SENTINEL, np.uint8)), c.buffer(np.full(N * 4, SENTINEL, np.uint8))
    c.record_time_spans(s.db, N, 0.0, sb)
    count = c.compact_time_window(sb, N, T0, T1, src=s.db, dst=dst, kept_index=idx)
    c.subdata(s.db, np.zeros((N, 24), np.float32))            # behind the compaction: it must not see the zeros
    c.subdata(sb, np.full(N * 8, SENTINEL, np.uint8))         # ... nor a rewritten table
    want_d, want_i, kept, written = tw.reference(table, T0, T1, rec, 96, N, N)
    assert c.read_compact_count(count) == (kept, written) and 0.1 * N <= kept <= 0.9 * N
    assert np.array_equal(c.read(idx, np.uint32, kept), want_i)
    assert np.array_equal(c.read(dst, np.uint8, kept * 96).reshape(kept, 96), want_d)
    # the dst of the call as the data of a frame on the next lane, and of a second spans call: the compacted records' own spans
    c.subdata(s.db, rec)
    s.frame(False, 25.0, near, True)
    full = c.read_pixels()
    s.cdb, s.kept = dst, kept
    sb2 = c.record_time_spans(dst, kept)
    s.frame(True, 25.0, near, True)
    assert np.array_equal(bits(c.read_pixels()), bits(full))
    assert np.array_equal(bits(c.read(sb2, tw.SPAN, kept)), bits(table[want_i]))
    c.close()
