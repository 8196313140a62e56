"""GPU: gs4d_slice_records — a 4D record set baked at one time into 3D records (include/gs4d.h).

The records are compared word for word with the host definition (tests/slice_cases.py: equal as uint32, a word that is a NaN on both sides counting as
equal; word 7, which goes through the device's expf, within 5e-6 relative of the host's and bit-equal to the alpha the device's own draw computes), with
the rest of dst, guard buffers and src compared against what was uploaded.  The guarantee — a draw of the slice at mu_t_out gives the bits of a draw of
the source at t — is checked on the colour image, the aux planes, the ID planes and the record statistics.  All calls go through the Python binding over
the C ABI."""
import ctypes

import numpy as np
import pytest

import build_cases as bc
import scenes
import slice_cases as sc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
f32 = np.float32
ALPHA_RTOL, ALPHA_FLOOR = 5e-6, 1e-30                       # the project's bar for the time opacity against the host (tests/test_gpu_splat_draw.py), held
                                                            # down to 1e-30; below, the same absolute error as at 1e-30 (the denormal end of expf)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


def unchanged(ctx, buf, a):
    return np.array_equal(ctx.read(buf, np.uint32, a.size), bits(a).reshape(-1))


def records_ok(got, want):
    """[n, 24] bool: the rule of gs4d.h — the host's bits but for word 7, which is within the bar of the host's"""
    ok = sc.same_bits(got, want)
    g, w = got[:, 7].astype(np.float64), want[:, 7].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok[:, 7] |= np.abs(g - w) <= ALPHA_RTOL * np.maximum(np.abs(w), ALPHA_FLOOR)
    return ok


# ---- 1. the records ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sc.SETS)
def test_records_equal_the_host_definition(gs4d, which):
    ctx = gs4d.Context(64, 64)
    extra, call = 3, 5 * sc.SETS.index(which)                   # records behind the last one that must stay as they are; the sets start at different queries
    worst = 0.0
    for n in sc.SIZES:
        rec = sc.records(gs4d, which, n)
        for first in sc.FIRSTS:
            q = sc.query_for(call)
            call += 1
            what = f"{which}, n = {n}, dst_first = {first}, query {q}"
            guards = [fill(ctx, GUARD)]
            src = ctx.buffer(rec)
            guards.append(fill(ctx, GUARD))
            host = np.full((first + n + extra) * 96 + 32, SENTINEL, np.uint8)
            dst = ctx.buffer(host)
            guards.append(fill(ctx, GUARD))
            assert ctx.slice_records(src, n, *q, dst=dst, dst_first=first) == dst
            got = ctx.read(dst, np.uint8, host.size)
            want = sc.expected(gs4d, rec, q)
            mine = got[first * 96:(first + n) * 96].view(f32).reshape(n, 24)
            ok = records_ok(mine, want)
            with np.errstate(all="ignore"):
                rel = np.abs(mine[:, 7].astype(np.float64) - want[:, 7]) / np.maximum(np.abs(want[:, 7].astype(np.float64)), ALPHA_FLOOR)
            worst = max(worst, float(np.nanmax(np.where(np.isfinite(rel), rel, 0.0))))
            assert ok.all(), f"{what}: {int((~ok).any(1).sum())} of {n} records differ from the host definition, first word at {np.argwhere(~ok)[0].tolist()}"
            assert (got[:first * 96] == SENTINEL).all(), f"{what}: bytes of dst in front of record dst_first changed"
            assert (got[(first + n) * 96:] == SENTINEL).all(), f"{what}: bytes of dst behind the last record changed"
            assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
            assert unchanged(ctx, src, rec), f"{what}: src changed"
            for b in guards + [src, dst]:
                ctx.delete(b)
    print(f"{which}: word 7 against the host, worst relative difference {worst:.3e}")
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_a_new_buffer_is_allocated_and_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    n, rec = 300, sc.records(gs4d, "4d_vel", 300)
    src = ctx.buffer(rec)
    dst = ctx.slice_records(src, n, 25.0, dst_first=2)
    assert ctx.device_ptr(dst)[1] >= (2 + n) * 96
    assert records_ok(ctx.read(dst, f32, n * 24, offset=2 * 96).reshape(n, 24), gs4d.slice_records_host(rec, 25.0)).all()
    untouched_dst = fill(ctx, 96 * 8)
    ctx.slice_records(src, 0, 25.0, dst=untouched_dst)
    ctx.slice_records(src, 0, 25.0, dst=untouched_dst, dst_first=8)
    ctx.finish()
    assert untouched(ctx, untouched_dst, 96 * 8) and unchanged(ctx, src, rec) and ctx.shadow_builds(untouched_dst) == 0
    ctx.close()


# ---- 2. word 7 against the device's own draw, 3. the guarantee ----------------------------------------------------------------------------------
W, H, N = 64, 48, 300
CAM, CAM_DIR = (0.0, 0.0, 150.0), (0.0, 0.0, -1.0)


def picture_records(gs4d, which):
    """N records of a set in front of the camera, part of them alive at the times of picture_queries"""
    if which in bc.FORMS:
        return bc.host_records(gs4d, which, bc.picture_set(gs4d, which, N, 0x5350))
    if which == "hostile":                                      # the implanted records among records that show something
        rec = bc.host_records(gs4d, "4d_vel", bc.picture_set(gs4d, "4d_vel", N, 0x5351))
        rec[1::2] = sc.records(gs4d, "hostile", N)[1::2]
        return rec
    rec = sc.records(gs4d, which, N).copy()                     # neg_zero: a third of it has mu_t = 25
    rec[:, :3] *= f32(0.2)
    return rec


def picture_queries(which):
    t0 = 0.0 if which == "3d" else 25.0                         # a 3D record has mu_t = 0 and Sigma44 = 1
    return ((t0, 0.0, t0, 1.0), (t0 + 0.3, 0.25, 0.0, 0.5), (t0 + 0.3, 0.0, 7.5, float("inf")))


class Scene:
    """a context with a record buffer, an index buffer, a statistics table and the camera of the picture sets"""

    def __init__(self, gs4d, n, rec=None, outputs=True, w=W, h=H, cam=(CAM, CAM_DIR)):
        self.gs4d, self.n, self.cam = gs4d, n, cam
        self.ctx = c = gs4d.Context(w, h)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        self.outputs = outputs
        self.db = c.buffer(rec) if rec is not None else c.buffer(nbytes=96 * n)
        self.kb, self.ib = c.buffer(nbytes=4 * n), c.buffer(nbytes=4 * n)
        self.sb = c.buffer(np.zeros(n, gs4d.RECORD_STAT))
        self.view, self.proj = gs4d.look_at(*cam), gs4d.perspective(scenes.FOV, w, h, scenes.ZNEAR, scenes.ZFAR)

    def frame(self, t, min_opacity=0.0, index=None, blend=None, n=None, data=None, stats=False):
        """one frame: the colour, and with the default blend function either the aux and ID planes or (stats=True) the record statistics — a draw
        with statistics into a frame with such planes, or with another blend function, is out of the library's scope.  index: the uint32 order
        of a GS4D_MODE_4D_SORTED draw, None: GS4D_MODE_4D_DIRECT"""
        c, gs4d = self.ctx, self.gs4d
        n, data = self.n if n is None else n, self.db if data is None else data
        planes = self.outputs and blend is None and not stats
        assert not (stats and blend is not None)
        c.set_id_outputs(planes)
        c.set_blend(*(blend or (gs4d.SRC_ALPHA, gs4d.ONE_MINUS_SRC_ALPHA)))
        if stats:
            c.subdata(self.sb, np.zeros(self.n, gs4d.RECORD_STAT))
        c.set_record_stats(self.sb if stats else None, self.n)
        c.clear()
        c.set_uniforms(time=t, min_opacity=min_opacity, view=self.view, proj=self.proj)
        if index is not None:
            c.subdata(self.ib, np.ascontiguousarray(index, np.uint32))
            c.set_mode(gs4d.MODE_4D_SORTED)
            c.bind(1, self.ib)
            c.bind(2, data)
        else:
            c.set_mode(gs4d.MODE_4D_DIRECT)
            c.bind(1, data)
        c.draw_instanced(n)
        out = {"colour": c.read_pixels()}
        if stats:
            out["stats"] = c.read(self.sb, np.uint8, 16 * self.n)
        if planes:
            rid, drw, wt = c.read_ids()
            out.update(aux=c.read_aux(), record=rid, draw=drw, weight=wt)
        return out

    def keys(self, t, key_mode, data=None):
        c = self.ctx
        c.set_uniforms(time=t, min_opacity=0.0, view=self.view, proj=self.proj)
        c.keygen(self.db if data is None else data, t, self.cam[0], self.kb, self.ib, self.n, key_mode=key_mode)
        return c.read(self.kb, np.uint32, self.n), c.read(self.ib, np.uint32, self.n)


def same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        g, w = bits(got[k]), bits(want[k])
        assert np.array_equal(g, w), f"{what}: {k}: {int((g != w).sum())} words differ"


@pytest.mark.parametrize("which", sc.SETS)
def test_word_7_is_the_alpha_of_the_devices_own_draw(gs4d, which):
    rec = picture_records(gs4d, which)
    s = Scene(gs4d, N, rec, outputs=False)
    seen = 0
    for q in picture_queries(which):
        t, m = q[0], q[1]
        s.frame(t, m)
        pj = s.ctx.debug_projected(N)
        valid = pj[:, 14] != 0
        dst = s.ctx.slice_records(s.db, N, *q)
        word7 = s.ctx.read(dst, f32, N * 24).reshape(N, 24)[:, 7]
        s.ctx.delete(dst)
        differ = valid & (bits(pj[:, 6]) != bits(word7))
        assert not differ.any(), f"{which}, {q}: the alpha of {int(differ.sum())} of {int(valid.sum())} valid records is not word 7 of the slice"
        seen += int(valid.sum())
    assert seen > N // 2, "hardly a valid record: the test shows nothing"
    s.ctx.close()


@pytest.mark.parametrize("which", sc.SETS)
def test_a_draw_of_the_slice_is_the_draw_of_the_source(gs4d, which):
    """colour, aux, ID planes and record statistics: DIRECT and SORTED with one shared index, the default blend and (ONE, ONE)"""
    rec = picture_records(gs4d, which)
    src = Scene(gs4d, N, rec)
    out = Scene(gs4d, N)
    data = out.ctx.buffer(rec)
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    for q in picture_queries(which):
        t, m, mu_t_out, _ = q
        assert out.ctx.slice_records(data, N, *q, dst=out.db) == out.db
        _, index = src.keys(t, gs4d.KEY_REF_INV_EUCLID)                              # the source's own order, shared by both
        src.ctx.sort_pairs(src.kb, src.ib, N)
        index = src.ctx.read(src.ib, np.uint32, N)
        assert sorted(index.tolist()) == list(range(N))
        for order in (None, index):
            for config, kw in (("planes", {}), ("statistics", dict(stats=True)), ("blend (ONE, ONE)", dict(blend=(gs4d.ONE, gs4d.ONE)))):
                what = f"{which}, {q}, {'direct' if order is None else 'sorted'}, {config}"
                want = src.frame(t, m, order, **kw)
                got = out.frame(mu_t_out, m, order, **kw)
                same(got, want, what)
                if which != "hostile" and config == "planes":
                    assert int((np.abs(want["colour"] - clear).max(-1) > 1.0 / 255.0).sum()) > 50, f"{what}: an empty frame"
                    assert int((want["record"] != gs4d.Context.ID_NONE).sum()) > 50
                if which != "hostile" and config == "statistics":
                    assert int(np.frombuffer(want["stats"].tobytes(), gs4d.RECORD_STAT)["pixels"].sum()) > 50
        if sc.symmetric(rec).all():                              # the two sets' own view-z keys
            assert which in ("3d", "4d_vel")
            kz, iz = src.keys(t, gs4d.KEY_VIEW_Z)
            kz1, iz1 = out.keys(mu_t_out, gs4d.KEY_VIEW_Z)
            assert np.array_equal(kz, kz1) and np.array_equal(iz, iz1), f"{which}, {q}: the view-z keys of the slice are not those of the source"
    assert sc.symmetric(rec).all() == (which in ("3d", "4d_vel"))
    src.ctx.finish()
    out.ctx.finish()
    src.ctx.close()
    out.ctx.close()


# ---- 4. the layout of the shadow, the repack ---------------------------------------------------------------------------------------------------
CW, CH, CN, CT = 320, 192, 4096, 20.0


def cube4d(gs4d, spread=20.0):
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(CN, seed=0x534C)
    return gs4d.build_records_4d(pos4, q, scale * 3.0, life * spread, fade, vel, rgba)


def test_a_slice_of_a_4d_set_is_drawn_from_the_64_byte_layout(gs4d, monkeypatch):
    monkeypatch.delenv("GS4D_SOA_FULL", raising=False)
    rec = cube4d(gs4d)
    s = Scene(gs4d, CN + 7, outputs=False, w=CW, h=CH, cam=scenes.CAM_CUBE)
    c = s.ctx
    src = c.buffer(rec)
    own = np.arange(CN, dtype=np.uint32)
    want_src = s.frame(CT, index=own, n=CN, data=src)
    assert c.stats()["record_read_bytes"] > 64, "the 4D source is not a static set"
    alone = c.slice_records(src, CN, CT)
    assert c.shadow_builds(alone) == 0
    got = s.frame(CT, index=own, n=CN, data=alone)
    assert c.stats()["record_read_bytes"] == 64
    assert c.shadow_builds(alone) == 1, "one repack for the call followed by a draw"
    same({"colour": got["colour"]}, {"colour": want_src["colour"]}, "the slice alone")
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert int((np.abs(got["colour"] - clear).max(-1) > 1.0 / 255.0).sum()) > 200, "an empty frame"
    s.frame(CT, index=own, n=CN, data=alone)
    assert c.shadow_builds(alone) == 1, "a second draw repacked"
    # behind seven records with other time words: not the static layout, the same picture of its own records
    behind = c.buffer(np.concatenate([rec[:7], np.zeros((CN, 24), f32)]))
    c.slice_records(src, CN, CT, dst=behind, dst_first=7)
    got7 = s.frame(CT, index=own + 7, n=CN, data=behind)
    assert c.stats()["record_read_bytes"] > 64
    same({"colour": got7["colour"]}, {"colour": got["colour"]}, "the slice behind seven 4D records")
    assert c.shadow_builds(behind) == 1
    c.slice_records(src, CN, CT, dst=behind, dst_first=7)
    s.frame(CT, index=own + 7, n=CN, data=behind)
    assert c.shadow_builds(behind) == 2, "a call must make the next draw repack exactly once"
    c.finish()
    c.close()


# ---- 5. freeze ---------------------------------------------------------------------------------------------------------------------------------
def test_freeze_keeps_the_live_records_in_their_order(gs4d):
    rec = cube4d(gs4d, spread=1.0)                              # lifetimes of 0.5 .. 2 against mu_t in [0, 50]: most records are dead at any time
    s = Scene(gs4d, CN, rec, w=CW, h=CH, cam=scenes.CAM_CUBE)
    c = s.ctx
    host7 = gs4d.slice_records_host(rec, CT)[:, 7]
    sliced = c.slice_records(s.db, CN, CT)
    dev = c.read(sliced, f32, CN * 24).reshape(CN, 24)
    live = dev[:, 7] > 0
    ties = (host7 > 0) != live                                  # the device's word 7 decides at exactly 0
    assert (np.abs(host7[ties]) < ALPHA_FLOOR).all() and 0.02 * CN < live.sum() < 0.9 * CN, int(live.sum())
    dst, kept_index, count = c.freeze(s.db, CN, CT)
    kept, written = c.read_compact_count(count)
    assert kept == written == int(live.sum())
    index = c.read(kept_index, np.uint32, kept)
    assert np.array_equal(index, np.flatnonzero(live))
    assert np.array_equal(bits(c.read(dst, f32, kept * 24)).reshape(kept, 24), bits(dev[live]))
    # the draw, mapped through kept_index
    want = s.frame(CT)
    got = s.frame(CT, n=kept, data=dst)
    assert c.stats()["record_read_bytes"] == 64
    for k in ("colour", "aux", "weight", "draw"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    seen = want["record"] != gs4d.Context.ID_NONE
    assert seen.sum() > 200 and np.array_equal(got["record"] != gs4d.Context.ID_NONE, seen)
    assert np.array_equal(index[got["record"][seen]], want["record"][seen])
    want, got = s.frame(CT, stats=True), s.frame(CT, n=kept, data=dst, stats=True)
    assert np.array_equal(bits(got["colour"]), bits(want["colour"]))
    st, st_want = np.frombuffer(got["stats"].tobytes(), gs4d.RECORD_STAT), np.frombuffer(want["stats"].tobytes(), gs4d.RECORD_STAT)
    assert np.array_equal(st[:kept], st_want[index]) and not st_want["pixels"][~live].any() and st_want["pixels"].sum() > 200
    c.close()


# ---- 6. ordering without a finish ----------------------------------------------------------------------------------------------------------------
def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch):
    """a call into the buffer that the previous lane's draw still reads: that frame keeps the old set; a host write into src right behind the call
    does not change its result"""
    monkeypatch.setenv("GS4D_LANES", "4")
    t = bc.T
    old_rec = picture_records(gs4d, "4d_vel")
    src_rec = picture_records(gs4d, "4d_2q")
    new_rec = gs4d.slice_records_host(src_rec, t)

    def rgba8(scene):
        b = scene.ctx.buffer(nbytes=W * H * 4)
        scene.ctx.read_frame_rgba8_device(0, scene.ctx.device_ptr(b)[0], W * H * 4)
        scene.ctx.finish()
        return scene.ctx.read(b, np.uint8, W * H * 4)

    ref = Scene(gs4d, N, old_rec, outputs=False)
    ref.frame(t)
    want_prev = rgba8(ref)
    ref.ctx.close()
    s = Scene(gs4d, N, old_rec, outputs=False)
    c = s.ctx
    assert c.stats()["lanes"] == 4
    src, out = c.buffer(src_rec), c.buffer(nbytes=W * H * 4)

    def queue(t):                                               # a frame without a read-back
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=s.view, proj=s.proj)
        c.set_mode(gs4d.MODE_4D_DIRECT)
        c.bind(1, s.db)
        c.draw_instanced(N)

    for _ in range(4):
        queue(t)                                                # frames in flight that read the old records and their shadow
    c.clear()                                                   # the next lane's frame: the call is its first kernel
    c.slice_records(src, N, t, dst=s.db)
    c.subdata(src, np.zeros_like(src_rec))                      # directly behind: the call must not see the zeros
    c.set_uniforms(time=t, min_opacity=0.0, view=s.view, proj=s.proj)
    c.set_mode(gs4d.MODE_4D_DIRECT)
    c.bind(1, s.db)
    c.draw_instanced(N)
    c.read_frame_rgba8_device(1, c.device_ptr(out)[0], W * H * 4)
    got = c.read_pixels()
    c.finish()
    assert np.array_equal(c.read(out, np.uint8, W * H * 4), want_prev), "the frame before the call shows another set than it was drawn with"
    assert records_ok(c.read(s.db, f32, N * 24).reshape(N, 24), new_rec).all(), "the records are not those of src as it was at the call"
    fresh = Scene(gs4d, N, src_rec, outputs=False)
    want = fresh.frame(t)["colour"]
    fresh.ctx.close()
    assert np.array_equal(bits(got), bits(want))
    ref = Scene(gs4d, N, old_rec, outputs=False)
    assert not np.array_equal(bits(got), bits(ref.frame(t)["colour"])), "the two sets give the same picture: the test shows nothing"
    ref.ctx.close()
    assert c.shadow_builds(s.db) == 2
    c.close()


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_everything_as_it_was(gs4d):
    n, first = 300, 5
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    rec = sc.records(gs4d, "4d_vel", n)
    src = ctx.buffer(rec)
    dst_bytes = (first + n) * 96
    dst, short_dst, dead = fill(ctx, dst_bytes), fill(ctx, dst_bytes - 16), fill(ctx, 64)
    short_src = ctx.buffer(rec.reshape(-1)[:-1])                # one float short
    ctx.delete(dead)                                            # (last: a buffer made from here on could take its name)
    good = dict(t=25.0, min_opacity=0.0, mu_t_out=25.0, s44_out=1.0)

    def call(src=src, n=n, dst=dst, first=first, q=True, **fields):
        query = gs4d.Slice(**{**good, **fields})
        return lib.gs4d_slice_records(ctx._h, src, n, ctypes.byref(query) if q else None, dst, first)

    big, nan, inf = 1 << 32, float("nan"), float("inf")
    bad = {"q == NULL": dict(q=False), "t NaN": dict(t=nan), "t +inf": dict(t=inf), "t -inf": dict(t=-inf), "mu_t_out NaN": dict(mu_t_out=nan),
           "mu_t_out inf": dict(mu_t_out=inf), "min_opacity NaN": dict(min_opacity=nan), "s44_out NaN": dict(s44_out=nan), "s44_out 0": dict(s44_out=0.0),
           "s44_out -0": dict(s44_out=-0.0), "s44_out < 0": dict(s44_out=-1.0), "s44_out -inf": dict(s44_out=-inf),
           "n > 0xFFFFFFFF": dict(n=big), "dst_first > 0xFFFFFFFF": dict(first=big), "dst_first + n > 0xFFFFFFFF": dict(first=big - n),
           "n near 2^64": dict(n=(1 << 64) - 1), "src too small": dict(src=short_src), "dst too small": dict(dst=short_dst),
           "dst too small for dst_first": dict(first=first + 1), "src == dst": dict(src=dst)}
    for k in ("src", "dst"):
        bad.update({f"dead {k}": {k: dead}, f"no {k}": {k: 0}, f"unknown {k}": {k: 9999}})
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"slice_records" in lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and untouched(ctx, short_dst, dst_bytes - 16), "a refused call wrote something"
    assert unchanged(ctx, src, rec)
    assert call(n=0) == 0 and call(n=0, first=0xFFFFFFFF) == -1      # (a no-op still needs room for dst_first records)
    assert call(n=0, t=nan) == -1                               # (and a valid query)
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and ctx.shadow_builds(dst) == 0
    # the call works after the refusals; +inf and a min_opacity outside [0, 1] are allowed
    assert call(s44_out=inf, min_opacity=-inf) == 0
    got = ctx.read(dst, np.uint8, dst_bytes)
    assert (got[:first * 96] == SENTINEL).all()
    assert records_ok(got[first * 96:].view(f32).reshape(n, 24), gs4d.slice_records_host(rec, 25.0, -inf, 25.0, inf)).all()
    assert unchanged(ctx, src, rec)
    ctx.close()
