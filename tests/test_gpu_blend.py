"""GPU: the general blend path — any glBlendFunc other than (SRC_ALPHA, ONE_MINUS_SRC_ALPHA) — against the CPU checker, on the scenes of
tests/blend_cases.py (tests/test_blend_host.py shows on the CPU that the scenes are well posed: distinct, well conditioned, clear of the
discard threshold).  Such a draw builds instance-ordered tile lists and k_composite<PREMULT_C, true, Colour, false> walks them in draw order
with blend_general (csrc/composite_common.h); the overlay lines blend with the same function (csrc/lines.hip).

* every one of the 196 factor pairs, after lines, a sorted 4D draw, quads, a 2D draw and a direct 4D draw;
* draw order exactly: under (ONE, ZERO) the last entry of lists of 1 .. 200 entries shows, bit for bit;
* a draw whose tile lists overflow is re-run and still blends once;
* state changes within a frame, the clear colour a lazily clear tile starts from, tile-row shards.
Bars: per-pixel L-infinity <= 1e-4 for float images (TOL), exact where a test says so.
"""
import importlib

import numpy as np
import pytest

import blend_cases as bc
from test_gpu_render import linf, TOL

pytestmark = pytest.mark.gpu
KNOBS = ("GS4D_DRAW_PATH", "GS4D_SLABS", "GS4D_LANES", "GS4D_STAGED", "GS4D_STAGED_BOX", "GS4D_SORT_RANK", "GS4D_SORT_SHAPE", "GS4D_SORT_RB")


def _ctx(gs4d, monkeypatch, w, h, clear, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx = gs4d.Context(w, h)
    ctx.set_clear_color(clear)
    return ctx


def _blend(ctx, pair):
    ctx.set_blend(*bc.enums(pair))


def _sorted_draw(ctx, gs4d, db, kb, ib, n, key_mode=None):
    ctx.keygen(db, 0.0, bc.CAM[0], kb, ib, n, **({} if key_mode is None else {"key_mode": key_mode}))
    ctx.sort_pairs(kb, ib, n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.draw_instanced(n)


# ---- 2. every pair, every fragment source ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf", bc.FACTORS)
def test_every_destination_factor_with_source_factor(gs4d, oracle, monkeypatch, sf):
    """Lines on the lazily clear image, a sorted 4D draw, 3D-Full quads, a 2D draw, a direct 4D draw: after every step the image is the checker's,
    for each of the 14 destination factors.  Factors of one class (ZERO and CONSTANT_*, ONE and ONE_MINUS_CONSTANT_*) give the same bits."""
    m = bc.matrix(gs4d, oracle)
    w, h = m.W, m.H
    ctx = _ctx(gs4d, monkeypatch, w, h, m.CLEAR)
    db, kb, ib = ctx.buffer(m.rec_b), ctx.buffer(nbytes=4 * m.NB), ctx.buffer(nbytes=4 * m.NB)
    vb, d2 = ctx.buffer(m.quads_c), ctx.buffer(m.rec_d)
    out8 = ctx.buffer(nbytes=w * h * 4)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=m.view, proj=m.proj)
    same_class = {}
    for df in bc.FACTORS:
        pair = (sf, df)
        unordered = ctx.stats()["unordered_draws"]
        _blend(ctx, pair)
        ctx.clear()
        got = []
        ctx.draw_lines(m.lines, m.LINE_COLOUR, width=m.LINE_WIDTH)
        got.append(ctx.read_pixels())
        _sorted_draw(ctx, gs4d, db, kb, ib, m.NB)
        got.append(ctx.read_pixels())
        assert np.array_equal(ctx.read(ib, np.uint32, m.NB), m.order_b)
        ctx.set_mode(gs4d.MODE_3D_FULL)
        ctx.draw_quads(vb, m.NC)
        got.append(ctx.read_pixels())
        ctx.set_mode(gs4d.MODE_2D)
        ctx.bind(1, d2)
        ctx.draw_instanced(m.ND)
        got.append(ctx.read_pixels())
        ctx.set_mode(gs4d.MODE_4D_DIRECT)
        ctx.bind(1, db)
        ctx.draw_instanced(m.NE)
        got.append(ctx.read_pixels())
        ctx.read_pixels_rgba8_device(ctx.device_ptr(out8)[0], w * h * 4)
        ctx.finish()
        got8 = ctx.read(out8, np.uint8, w * h * 4).reshape(h, w, 4).astype(np.int32)
        want = m.expected(pair)
        for k, (g, e) in enumerate(zip(got, want)):
            err = linf(g, e)
            print(f"{pair} step {'abcde'[k]}: {err:.3e}")
            assert err <= TOL, (pair, "abcde"[k], err)
        # only the default pair goes through the unordered lists; everything else is blended in draw order
        assert (ctx.stats()["unordered_draws"] > unordered) == (pair == bc.OVER), pair
        # RGBA8: the packed float image, up to one count where the float value is within the float bar of a rounding boundary
        assert np.array_equal(got8, bc.pack8(got[4])), pair                    # of the library's own float image: exactly
        off = got8 - bc.pack8(want[4])
        assert np.abs(off).max() <= 1 and not np.any((off != 0) & ~bc.pack8_slack(want[4])), pair
        cls = bc.CLASS[df]
        if cls in same_class:
            assert all(np.array_equal(a, b) for a, b in zip(got, same_class[cls])), pair
        else:
            same_class[cls] = got
    ctx.close()


# ---- 3. draw order, exactly -----------------------------------------------------------------------------------------------------------------
def _check_lists(o, img, way, drop, what):
    for li, k in enumerate(o.KS):
        r, c = o.probes(li)
        seq = o.list_order(way, li)
        if k - drop < 1:
            assert np.array_equal(img[r, c], np.broadcast_to(o.CLEAR, (1, 4))), (what, li)
        elif way != "quads":
            assert np.array_equal(img[r, c, :3], np.broadcast_to(o.rgba[seq[k - 1 - drop]][:3], (1, 3))), (what, li, k)     # src * 1 + dst * 0: bit for bit
    want = o.image(way, drop=drop)
    assert linf(img, want) <= TOL, (what, linf(img, want))


@pytest.mark.parametrize("way", ["ref", "viewz", "direct", "quads"])
def test_the_last_entry_of_a_list_shows_under_one_zero(gs4d, oracle, monkeypatch, way):
    """Under (ONE, ZERO) a pixel ends as the last fragment drawn on it: lists of 1, 63, 64, 65, 127, 128, 129 and 200 entries, one on the partial
    corner tile, drawn sorted by the reference's key (shuffled record indices), sorted by view depth with runs of equal keys (the stable sort
    puts the higher record index last; one run straddles entry 64), and in index order as 4D-direct records and as quads.  The colour channels
    of a 4D fragment carry no exp: they are the record's colour bit for bit.  (A quad's colour is premultiplied by c, and every alpha is
    alpha * c: those are held to TOL against the checker; test_blend_host shows that a wrong entry would miss by more than 100 TOL.)
    Then every list without its last instance (draw_instanced(K - 1)): entries 62, 63, 64 and 127, 128 — the ends of a chunk — show."""
    o = bc.order_scene(gs4d, oracle)
    w, h = o.W, o.H
    ctx = _ctx(gs4d, monkeypatch, w, h, o.CLEAR)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=o.view, proj=o.proj)
    _blend(ctx, bc.ONE_ZERO)
    ctx.clear()
    if way in ("ref", "viewz"):
        db, kb, ib = ctx.buffer(o.rec), ctx.buffer(nbytes=4 * o.n), ctx.buffer(nbytes=4 * o.n)
        _sorted_draw(ctx, gs4d, db, kb, ib, o.n, None if way == "ref" else gs4d.KEY_VIEW_Z)
        img = ctx.read_pixels()
        assert np.array_equal(ctx.read(ib, np.uint32, o.n), o.order(way))
    elif way == "direct":
        db = ctx.buffer(o.rec)
        ctx.set_mode(gs4d.MODE_4D_DIRECT)
        ctx.bind(1, db)
        ctx.draw_instanced(o.n)
        img = ctx.read_pixels()
    else:
        vb = ctx.buffer(o.quads)
        ctx.set_mode(gs4d.MODE_3D_FULL)
        ctx.draw_quads(vb, o.n)
        img = ctx.read_pixels()
    assert ctx.stats()["unordered_draws"] == 0
    _check_lists(o, img, way, 0, "all instances")
    # every list on its own, without its last instance, in one frame
    ctx.clear()
    for li, k in enumerate(o.KS):
        seq = o.list_order(way, li)
        if k == 1:
            continue                                            # nothing left to draw: the tile stays clear
        if way in ("ref", "viewz"):
            sub = ctx.buffer(np.ascontiguousarray(seq, np.uint32))
            ctx.set_mode(gs4d.MODE_4D_SORTED)
            ctx.bind(1, sub)
            ctx.bind(2, db)
            ctx.draw_instanced(k - 1)
        elif way == "direct":
            ctx.set_mode(gs4d.MODE_4D_DIRECT)
            ctx.bind(1, ctx.buffer(np.ascontiguousarray(o.rec[seq])))
            ctx.draw_instanced(k - 1)
        else:
            ctx.draw_quads(ctx.buffer(np.ascontiguousarray(o.quads[seq])), k - 1)
    _check_lists(o, ctx.read_pixels(), way, 1, "without the last instance")
    ctx.close()


# ---- 4. a re-run blends once ----------------------------------------------------------------------------------------------------------------
def _rerun_frame(ctx, gs4d, s, bufs, t):
    """default draw (some tiles into memory), the overflowing general draw, lines, the larger general draw; returns the two images and the
    re-runs the capacities before each general draw imply"""
    d0, d1 = bufs
    ctx.clear()
    ctx.set_uniforms(time=t, min_opacity=0.0, view=s.view, proj=s.proj)
    ctx.set_mode(gs4d.MODE_4D_DIRECT)
    _blend(ctx, bc.OVER)
    ctx.bind(1, d0)
    ctx.draw_instanced(s.N0)
    implied = []
    imgs = []
    ctx.bind(1, d1)
    _blend(ctx, bc.ONE_ONE)
    for n in (s.N1, s.N2):
        st = ctx.stats()                                        # (validates the draw before: the entry count and the capacity are final)
        implied.append(bc.expected_reruns(st["capacity"], st["entries"], n, s.entries(n, t))[0])
        if n == s.N2:
            ctx.draw_lines(s.lines, s.LINE_COLOUR, width=2.0)
        ctx.draw_instanced(n)
        imgs.append(ctx.read_pixels())
        assert ctx.stats()["reruns"] - st["reruns"] == implied[-1], (n, st, ctx.stats())
        assert ctx.stats()["entries"] == s.entries(n, t)
    return imgs, implied


@pytest.mark.parametrize("lanes", [None, 1])
def test_an_overflowing_general_draw_is_rerun_and_blends_once(gs4d, oracle, monkeypatch, lanes):
    """(ONE, ONE) is not idempotent: a draw whose tile lists overflow their capacity must leave the image alone until its re-run.  The first
    general draw of the frame finds tiles a default draw brought into memory and lazily clear ones; the second, larger one overflows the grown
    capacity again.  Blended twice, either would move every pixel by more than 100 TOL (test_blend_host)."""
    s = bc.rerun_scene(gs4d, oracle)
    ctx = _ctx(gs4d, monkeypatch, s.W, s.H, s.CLEAR, **({} if lanes is None else {"GS4D_LANES": lanes}))
    nlanes = ctx.stats()["lanes"]
    assert lanes is None or nlanes == lanes
    bufs = ctx.buffer(s.rec0), ctx.buffer(s.rec)
    frames = 2 * nlanes + 1                                     # every lane's image and ranges table is used twice under a general function
    for f in range(frames):
        t = 0.05 * f
        imgs, implied = _rerun_frame(ctx, gs4d, s, bufs, t)
        if f == 0:
            assert implied == [1, 1]                            # the design (test_blend_host): both general draws of a fresh context overflow
        for k, (g, e) in enumerate(zip(imgs, s.frame(t))):
            assert linf(g, e) <= TOL, (f, k, linf(g, e))
        assert ctx.stats()["unordered_draws"] == f + 1
    ctx.close()


# ---- 5. state changes and shards ------------------------------------------------------------------------------------------------------------
def test_blend_state_changes_within_a_frame(gs4d, oracle, monkeypatch):
    """default (unordered lists), (SRC_ALPHA, ONE), default again, lines under (ONE_MINUS_DST_COLOR, ONE_MINUS_SRC_ALPHA): each step is the
    checker's, and only the default draws take the unordered path."""
    m = bc.matrix(gs4d, oracle)
    w, h = m.W, m.H
    ctx = _ctx(gs4d, monkeypatch, w, h, m.CLEAR)
    db, vb, d2 = ctx.buffer(m.rec_b), ctx.buffer(m.quads_c), ctx.buffer(m.rec_d)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=m.view, proj=m.proj)
    ctx.clear()
    e = oracle.clear_image(w, h, m.CLEAR)
    additive, lines = ("SRC_ALPHA", "ONE"), ("ONE_MINUS_DST_COLOR", "ONE_MINUS_SRC_ALPHA")
    ctx.set_mode(gs4d.MODE_4D_DIRECT)
    ctx.bind(1, db)
    ctx.draw_instanced(m.NB)
    oracle.composite(m.eproj_b, None, oracle.MODE_4D, w, h, e)
    assert linf(ctx.read_pixels(), e) <= TOL and ctx.stats()["unordered_draws"] == 1
    _blend(ctx, additive)
    ctx.set_mode(gs4d.MODE_3D_FULL)
    ctx.draw_quads(vb, m.NC)
    oracle.composite(m.eproj_c, None, oracle.MODE_3D, w, h, e, blend=bc.enums(additive))
    assert linf(ctx.read_pixels(), e) <= TOL and ctx.stats()["unordered_draws"] == 1
    _blend(ctx, bc.OVER)
    ctx.set_mode(gs4d.MODE_2D)
    ctx.bind(1, d2)
    ctx.draw_instanced(m.ND)
    oracle.composite(m.eproj_d, None, oracle.MODE_2D, w, h, e)
    assert linf(ctx.read_pixels(), e) <= TOL and ctx.stats()["unordered_draws"] == 2
    _blend(ctx, lines)
    ctx.draw_lines(m.lines, m.LINE_COLOUR, width=m.LINE_WIDTH)
    before = e.copy()
    oracle.draw_lines(e, m.lines, m.LINE_COLOUR, m.LINE_WIDTH, blend=bc.enums(lines))
    assert linf(ctx.read_pixels(), e) <= TOL and ctx.stats()["unordered_draws"] == 2
    assert linf(e, before) > 100 * TOL
    ctx.close()


def test_a_general_draw_starts_from_the_colour_of_the_clear(gs4d, oracle, monkeypatch):
    """glClearColor after glClear: the lazily clear tiles a general draw starts from, and the tiles it does not touch, keep the colour the image
    was cleared with."""
    m = bc.matrix(gs4d, oracle)
    w, h = m.W, m.H
    pair = ("ONE_MINUS_DST_ALPHA", "DST_COLOR")
    ctx = _ctx(gs4d, monkeypatch, w, h, m.CLEAR)
    db = ctx.buffer(m.rec_b)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=m.view, proj=m.proj)
    ctx.clear()
    ctx.set_clear_color((0.9, 0.1, 0.3, 0.8))                  # for the NEXT clear
    _blend(ctx, pair)
    ctx.set_mode(gs4d.MODE_4D_DIRECT)
    ctx.bind(1, db)
    ctx.draw_instanced(m.NB)
    img = ctx.read_pixels()
    e = oracle.composite(m.eproj_b, None, oracle.MODE_4D, w, h, oracle.clear_image(w, h, m.CLEAR), blend=bc.enums(pair))
    assert linf(img, e) <= TOL
    for tx, ty in m.UNTOUCHED:
        assert np.array_equal(img[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8], np.broadcast_to(m.CLEAR, (min(8, h - ty * 8), 8, 4)))
    other = oracle.composite(m.eproj_b, None, oracle.MODE_4D, w, h, oracle.clear_image(w, h, (0.9, 0.1, 0.3, 0.8)), blend=bc.enums(pair))
    assert linf(e, other) > 100 * TOL
    ctx.clear()
    assert np.array_equal(ctx.read_pixels()[0, 0], np.array([0.9, 0.1, 0.3, 0.8], np.float32))
    ctx.close()


def test_tile_row_shards_under_a_general_function(gs4d, oracle, monkeypatch):
    """set_tile_shard(rank, 2) under (ONE, ONE): a context's own tile rows are the full image's, its other rows are exactly the clear colour, and
    the band read-back is the packed full read of those rows."""
    sh = importlib.import_module("4dgaussiansplatrendering_amd.sharding")
    m = bc.matrix(gs4d, oracle)
    w, h = m.W, m.H

    def render(rank, world):
        ctx = _ctx(gs4d, monkeypatch, w, h, m.CLEAR)
        ctx.set_tile_shard(rank, world)
        db, vb = ctx.buffer(m.rec_b), ctx.buffer(m.quads_c)
        ctx.set_uniforms(time=0.0, min_opacity=0.0, view=m.view, proj=m.proj)
        ctx.clear()
        _blend(ctx, bc.ONE_ONE)
        ctx.set_mode(gs4d.MODE_4D_DIRECT)
        ctx.bind(1, db)
        ctx.draw_instanced(m.NB)
        ctx.set_mode(gs4d.MODE_3D_FULL)
        ctx.draw_quads(vb, m.NC)
        rows = ctx.band_rows()
        band, full8 = ctx.buffer(nbytes=max(rows, 1) * w * 4), ctx.buffer(nbytes=w * h * 4)
        ctx.read_band_rgba8_device(ctx.device_ptr(band)[0], rows * w * 4)
        ctx.read_pixels_rgba8_device(ctx.device_ptr(full8)[0], w * h * 4)
        img = ctx.read_pixels()
        ctx.finish()
        out = img, ctx.read(band, np.uint8, rows * w * 4).reshape(rows, w, 4), ctx.read(full8, np.uint8, w * h * 4).reshape(h, w, 4)
        assert ctx.stats()["unordered_draws"] == 0
        ctx.close()
        return out

    e = oracle.clear_image(w, h, m.CLEAR)
    oracle.composite(m.eproj_b, None, oracle.MODE_4D, w, h, e, blend=bc.enums(bc.ONE_ONE))
    oracle.composite(m.eproj_c, None, oracle.MODE_3D, w, h, e, blend=bc.enums(bc.ONE_ONE))
    whole, _, whole8 = render(0, 1)
    assert linf(whole, e) <= TOL
    for rank in range(2):
        img, band, full8 = render(rank, 2)
        mine = sh.band_pixel_rows(rank, 2, h)
        others = sorted(set(range(h)) - set(mine))
        assert linf(img[mine], whole[mine]) <= TOL and linf(img[mine], e[mine]) <= TOL
        assert np.array_equal(img[others], np.broadcast_to(m.CLEAR, (len(others), w, 4)))
        assert np.array_equal(band, full8[mine]) and np.array_equal(band.astype(np.int32), bc.pack8(img[mine]))
        assert np.array_equal(full8[mine], whole8[mine])
