"""GPU: tile-list entries that cannot change a pixel are not built (csrc/preprocess.hip emit(), csrc/footprint_rect.h).

A. GS4D_CULL_ALPHA0 (default on): under the default blend function a record whose alpha compares equal to 0 gets no tile-list entry; its
   projected record stays what it was.  B. GS4D_TIGHT_RECT (default on): the pixel rectangle is the smaller, per axis, of the quad's box and
   the discard disc's box.

Every case renders the same frames in two contexts, knob on and knob off: image, aux plane, ID planes, record statistics, sorted keys and
permutation must be equal bit for bit, and the entry counts must differ by exactly the tiles of the culled records, recomputed on the CPU from
the device's own projected records.  256 x 128 image (512 tiles), 3 * 2048 + 100 records; the frames are repeated until the draws are staged
(stats()["staged_draws"] grows), and run again with GS4D_STAGED=0.  tests/test_cull_host.py asserts the premises of the record sets.
A context's first splat draw builds every entry whatever the knobs say: what is compared is the last frame of 2 * lanes + 2.
"""
import numpy as np
import pytest

import cull_cases as cc

pytestmark = pytest.mark.gpu
W, H, N = cc.W, cc.H, cc.N


def render(gs4d, monkeypatch, rec, *, knobs, t=0.0, min_opacity=0.0, staged=True, outputs="colour", ztest=False, stats=False, blend=None, shard=None, ordered=False, frames=None):
    """the frames of one context: Clear -> key loop -> sort -> Draw, repeated until the draws are staged; what the last frame left"""
    for k in ("GS4D_CULL_ALPHA0", "GS4D_TIGHT_RECT", "GS4D_STAGED", "GS4D_DRAW_PATH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    if not staged:
        monkeypatch.setenv("GS4D_STAGED", "0")
    if ordered:
        monkeypatch.setenv("GS4D_DRAW_PATH", "ordered")
    ctx = gs4d.Context(W, H)
    try:
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        n = rec.shape[0]
        db, kb, ib = ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
        view, proj = cc.mats(gs4d)
        if outputs == "aux":
            ctx.set_aux_outputs(True)
        if outputs == "ids":
            ctx.set_id_outputs(True)
        if ztest:
            z = np.full((H, W), np.inf, np.float32)
            z[:, : W // 2] = 560.0                          # the cube's centre is about 680 from the camera: the plane hides the far part of the left half
            ctx.set_depth_test(ctx.depth_plane(z))
        if shard:
            ctx.set_tile_shard(*shard)
        if blend:
            ctx.set_blend(*blend)
        sb = None
        L = ctx.stats()["lanes"]
        frames = frames or 2 * L + 2
        for f in range(frames):
            if stats:                                       # a fresh table for every frame: the last one is compared
                sb = ctx.record_stats(n)
                ctx.set_record_stats(sb, n)
            ctx.clear()
            ctx.set_uniforms(time=t, min_opacity=min_opacity, view=view, proj=proj)
            ctx.keygen(db, t, cc.CAM[0], kb, ib, n)
            ctx.sort_pairs(kb, ib, n)
            ctx.set_mode(gs4d.MODE_4D_SORTED)
            ctx.bind(1, ib)
            ctx.bind(2, db)
            ctx.draw_instanced(n)
        out = {"img": ctx.read_pixels(), "keys": ctx.read(kb, np.uint32, n), "perm": ctx.read(ib, np.uint32, n), "proj": ctx.debug_projected(n)}
        if outputs in ("aux", "ids"):
            out["aux"] = ctx.read_aux()
        if outputs == "ids":
            out["ids"] = ctx.read_ids()
        if stats:
            out["stats"] = ctx.read_record_stats(sb, n)
        out["st"] = ctx.stats()
        out["frames"], out["lanes"] = frames, L
        return out
    finally:
        ctx.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same_results(on, off, what):
    for k in ("img", "keys", "perm", "aux", "stats"):
        if k in off:
            assert np.array_equal(bits(on[k]), bits(off[k])), f"{what}: {k} differs between knob on and knob off"
    if "ids" in off:
        for a, b, name in zip(on["ids"], off["ids"], ("record", "draw", "weight")):
            assert np.array_equal(bits(a), bits(b)), f"{what}: ID plane {name} differs"
    # the projected records are what they were: valid, colour, alpha, rectangle and all
    assert np.array_equal(bits(on["proj"]), bits(off["proj"])), f"{what}: the projected records differ"


def assert_paths(on, off, staged, ordered=False):
    for r in (on, off):
        st = r["st"]
        assert st["reruns"] == 0 and st["staged_misses"] == 0, st
        if ordered:
            assert st["unordered_draws"] == 0, st
        elif staged:
            assert st["staged_draws"] >= r["frames"] - r["lanes"] - 2 and st["staged_draws"] > 0, st
        else:
            assert st["staged_draws"] == 0 and st["unordered_draws"] > 0, st


def culled_entries(off, shard=None):
    """tiles of the records the cull drops, from the device's projected records of the knob-off context"""
    return int(cc.tiles_per_record(off["proj"], shard)[cc.invisible(off["proj"])].sum())


def both(gs4d, monkeypatch, rec, knob, **kw):
    return render(gs4d, monkeypatch, rec, knobs={}, **kw), render(gs4d, monkeypatch, rec, knobs={knob: "0"}, **kw)


CLEAR = np.array([0.18431373, 0.20784314, 0.25882353, 1.0], np.float32)


# ---- A: records of alpha 0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [True, False], ids=["staged", "exact"])
@pytest.mark.parametrize("variant", ["colour", "aux", "ids", "ztest", "stats"])
def test_half_of_a_4d_set_is_invisible(gs4d, monkeypatch, variant, staged):
    rec = cc.records_4d(gs4d)
    kw = dict(t=cc.T_HALF, staged=staged, outputs=variant if variant in ("aux", "ids") else "colour", ztest=variant == "ztest", stats=variant == "stats")
    on, off = both(gs4d, monkeypatch, rec, "GS4D_CULL_ALPHA0", **kw)
    assert_paths(on, off, staged)
    assert_same_results(on, off, variant)
    dropped = culled_entries(off)
    zero = cc.invisible(off["proj"])
    assert 0.3 * N < zero.sum() < 0.7 * N and dropped > 0
    assert off["st"]["entries"] == int(cc.tiles_per_record(off["proj"]).sum())
    assert on["st"]["entries"] == off["st"]["entries"] - dropped, (on["st"], off["st"], dropped)
    assert np.abs(on["img"] - CLEAR).max() > 0.05                    # the kept records show
    if variant == "stats":
        assert (on["stats"]["pixels"][zero] == 0).all() and on["stats"]["pixels"].sum() > 0


@pytest.mark.parametrize("staged", [True, False], ids=["staged", "exact"])
def test_every_record_invisible(gs4d, monkeypatch, staged):
    """no entry at all: the image is the clear colour, every other plane holds its clear value, nothing is re-run — and the draws after the
    first empty one are still staged: the compositor reported its verdict for a frame whose launch box is empty"""
    rec = cc.records_4d(gs4d)
    on, off = both(gs4d, monkeypatch, rec, "GS4D_CULL_ALPHA0", t=cc.T_NONE, staged=staged, outputs="ids")
    assert_paths(on, off, staged)
    assert_same_results(on, off, "all invisible")
    zero = cc.invisible(off["proj"])
    assert zero.sum() > N // 2 and np.array_equal(zero, off["proj"][:, 14] != 0)
    assert on["st"]["entries"] == 0 and off["st"]["entries"] == culled_entries(off) > 0
    assert np.array_equal(on["img"], np.broadcast_to(CLEAR, (H, W, 4)))
    assert not on["aux"].any()
    assert (on["ids"][0] == gs4d.Context.ID_NONE).all() and (on["ids"][1] == gs4d.Context.ID_NONE).all() and not on["ids"][2].any()


@pytest.mark.parametrize("staged", [True, False], ids=["staged", "exact"])
@pytest.mark.parametrize("case", ["segment_and_wave", "negative_zero", "big_footprints"])
def test_static_sets_with_zero_alpha_records(gs4d, monkeypatch, case, staged):
    """a whole segment and a whole wave of consecutive records invisible; col.w = -0.0f; a culled and a kept record of more than 16 tiles"""
    rec, idx = getattr(cc, case)(gs4d)
    on, off = both(gs4d, monkeypatch, rec, "GS4D_CULL_ALPHA0", staged=staged)
    assert_paths(on, off, staged)
    assert_same_results(on, off, case)
    zero = cc.invisible(off["proj"])
    want = np.zeros(N, bool)
    want[idx] = True
    assert np.array_equal(zero, want & (off["proj"][:, 14] != 0)) and zero.any()
    if case == "negative_zero":
        assert np.signbit(off["proj"][zero, 6]).all()
    if case == "big_footprints":
        assert (cc.tiles_per_record(off["proj"])[5:7] > 16).all(), cc.tiles_per_record(off["proj"])[5:7]
    dropped = culled_entries(off)
    assert dropped > 0 and on["st"]["entries"] == off["st"]["entries"] - dropped, (on["st"], off["st"], dropped)


def test_a_minimum_opacity_leaves_nothing_to_cull(gs4d, monkeypatch):
    rec = cc.records_4d(gs4d)
    on, off = both(gs4d, monkeypatch, rec, "GS4D_CULL_ALPHA0", t=cc.T_HALF, min_opacity=0.25)
    assert_paths(on, off, True)
    assert_same_results(on, off, "min_opacity")
    assert not cc.invisible(off["proj"]).any()
    assert on["st"]["entries"] == off["st"]["entries"] > 0


def test_the_ordered_path_with_the_callers_sort_index(gs4d, monkeypatch):
    rec = cc.records_4d(gs4d)
    on, off = both(gs4d, monkeypatch, rec, "GS4D_CULL_ALPHA0", t=cc.T_HALF, ordered=True)
    assert_paths(on, off, False, ordered=True)
    assert_same_results(on, off, "ordered")
    dropped = culled_entries(off)
    assert dropped > 0 and on["st"]["entries"] == off["st"]["entries"] - dropped, (on["st"], off["st"], dropped)


@pytest.mark.parametrize("rank", [0, 1])
def test_two_tile_shards(gs4d, monkeypatch, rank):
    rec = cc.records_4d(gs4d)
    on, off = both(gs4d, monkeypatch, rec, "GS4D_CULL_ALPHA0", t=cc.T_HALF, shard=(rank, 2))
    assert_paths(on, off, True)
    assert_same_results(on, off, f"shard {rank}")
    dropped = culled_entries(off, (rank, 2))
    assert off["st"]["entries"] == int(cc.tiles_per_record(off["proj"], (rank, 2)).sum())
    assert dropped > 0 and on["st"]["entries"] == off["st"]["entries"] - dropped, (on["st"], off["st"], dropped)


def test_one_zero_blending_is_left_alone(gs4d, monkeypatch):
    """under (ONE, ZERO) a fragment of alpha 0 replaces the pixel: the cull does not apply — same picture and entry count as with the knob off, and
    another picture than the set without its alpha-0 records gives"""
    rec, idx = cc.segment_and_wave(gs4d)
    kw = dict(blend=(gs4d.ONE, gs4d.ZERO), ordered=False)
    on, off = both(gs4d, monkeypatch, rec, "GS4D_CULL_ALPHA0", **kw)
    assert_same_results(on, off, "(ONE, ZERO)")
    assert on["st"]["entries"] == off["st"]["entries"] == int(cc.tiles_per_record(off["proj"]).sum())
    assert culled_entries(off) > 0
    keep = np.ones(N, bool)
    keep[idx] = False
    without = render(gs4d, monkeypatch, np.ascontiguousarray(rec[keep]), knobs={}, **kw)
    assert not np.array_equal(bits(without["img"]), bits(on["img"])), "the alpha-0 records left no trace under (ONE, ZERO): the cull was applied"


def test_a_contexts_first_draw_builds_every_entry(gs4d, monkeypatch):
    """the first splat draw of a context is the measuring draw: every entry of every quad's box, whatever the knobs say (its picture is the same)"""
    rec = cc.records_4d(gs4d)
    first = render(gs4d, monkeypatch, rec, knobs={}, t=cc.T_HALF, frames=1)
    off = render(gs4d, monkeypatch, rec, knobs={"GS4D_CULL_ALPHA0": "0", "GS4D_TIGHT_RECT": "0"}, t=cc.T_HALF, frames=1)
    later = render(gs4d, monkeypatch, rec, knobs={}, t=cc.T_HALF)                # (every frame lane has drawn since: stats() reports the draw validated last)
    assert_same_results(first, off, "first draw")
    assert first["st"]["entries"] == off["st"]["entries"] == int(cc.tiles_per_record(off["proj"]).sum())
    assert np.array_equal(bits(later["img"]), bits(first["img"])) and later["st"]["entries"] < first["st"]["entries"]


# ---- B: the tightened rectangle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [True, False], ids=["staged", "exact"])
@pytest.mark.parametrize("scale,variant", [(8.0, "colour"), (8.0, "ids"), (8.0, "stats"), (8.0, "ztest"), (60.0, "colour"), (60.0, "aux")])
def test_the_tight_rectangle_changes_no_pixel(gs4d, monkeypatch, scale, variant, staged):
    """randomly rotated anisotropic splats, footprints of 2-6 pixels (scale 8) and of 10-40 (scale 60)"""
    rec = cc.rotated_splats(gs4d, scale)
    kw = dict(staged=staged, outputs=variant if variant in ("aux", "ids") else "colour", ztest=variant == "ztest", stats=variant == "stats")
    on = render(gs4d, monkeypatch, rec, knobs={}, **kw)
    off = render(gs4d, monkeypatch, rec, knobs={"GS4D_TIGHT_RECT": "0"}, **kw)
    if scale <= 8.0:
        assert_paths(on, off, staged)
    for k in ("img", "keys", "perm", "aux", "stats"):
        if k in off:
            assert np.array_equal(bits(on[k]), bits(off[k])), f"{variant}: {k} differs between the tight rectangle and the quad's box"
    if "ids" in off:
        for a, b in zip(on["ids"], off["ids"]):
            assert np.array_equal(bits(a), bits(b))
    # the records differ in their rectangles only, and the new one lies inside the old one
    same = np.ones(16, bool)
    same[10:12] = False
    assert np.array_equal(bits(on["proj"][:, same]), bits(off["proj"][:, same]))
    a, b = cc.rects(on["proj"]), cc.rects(off["proj"])
    some = (a[0] <= a[2]) & (a[1] <= a[3])
    assert (a[0][some] >= b[0][some]).all() and (a[1][some] >= b[1][some]).all() and (a[2][some] <= b[2][some]).all() and (a[3][some] <= b[3][some]).all()
    for r in (on, off):
        assert r["st"]["entries"] == int(cc.tiles_per_record(r["proj"]).sum())
    assert on["st"]["entries"] <= off["st"]["entries"]
    if scale <= 8.0:
        assert on["st"]["entries"] < off["st"]["entries"], (on["st"]["entries"], off["st"]["entries"])
    print(f"scale {scale}: entries {off['st']['entries']} -> {on['st']['entries']}")
    assert np.abs(on["img"] - CLEAR).max() > 0.05
