"""GPU: per-record contribution statistics (gs4d_set_record_stats).

Contract: within a draw every fragment that enters the colour with a weight w = T * al > 0 at a pixel inside the image adds (1, w, q(w)) to its
record's (pixels, wmax, wsum), q(w) = rint(w * 2^24); integers accumulated with atomics, so they add up across tiles, draws, frames, lanes and
shards, and a draw the library runs again counts once.  Oracles: the ID outputs of the same draw (disjoint splats: exact) and the numpy
restatement tests/stats_cases.py (layered splats: the bar of stats_cases.check).  Every test runs on both draw paths."""
import numpy as np
import pytest

import capacity_cases as cc
import id_cases
import staged_cases
import stats_cases as sc

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(autouse=True, params=["auto", "ordered"])
def draw_path(request, monkeypatch):
    """Every test runs on both draw paths, as tests/test_gpu_depth_test.py does."""
    if request.param == "ordered":
        monkeypatch.setenv("GS4D_DRAW_PATH", "ordered")
    else:
        monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    return request.param


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_stats(a, b):
    return np.array_equal(a["pixels"], b["pixels"]) and np.array_equal(bits(a["wmax"]), bits(b["wmax"])) and np.array_equal(a["wsum"], b["wsum"])


class Direct:
    """one context drawing `rec` (96-byte records) with GS4D_MODE_4D_DIRECT: instance k is record k"""

    def __init__(self, gs4d, W, H, rec, nstat=None):
        self.gs4d, self.W, self.H, self.n = gs4d, W, H, rec.shape[0]
        self.ctx = gs4d.Context(W, H)
        self.ctx.set_clear_color(gs4d.CLEAR_COLOR)
        self.db = self.ctx.buffer(rec)
        view, proj = sc.mats(gs4d, W, H)
        self.ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
        self.ctx.set_mode(gs4d.MODE_4D_DIRECT)
        self.ctx.bind(1, self.db)
        self.nstat = self.n if nstat is None else nstat
        self.sb = self.ctx.record_stats(self.nstat)

    def on(self):
        self.ctx.set_record_stats(self.sb, self.nstat)

    def off(self):
        self.ctx.set_record_stats(None)

    def frame(self, draws=1):
        self.ctx.clear()
        for _ in range(draws):
            self.ctx.draw_instanced(self.n)

    def stats(self):
        return self.ctx.read_record_stats(self.sb, self.nstat)

    def zero(self):
        self.ctx.subdata(self.sb, np.zeros(self.nstat, self.gs4d.Context.RECORD_STAT))

    def reference(self, nrecords=None):
        return sc.restate(id_cases.from_device(self.ctx.debug_projected(self.n)), None, self.W, self.H, nrecords=nrecords)

    def close(self):
        self.ctx.close()


def from_id_planes(rec_plane, w_plane, n):
    """what the ID planes of a frame of disjoint records say about every record: pixels that name it with weight > 0, the largest weight, sum of q"""
    st = np.zeros(n, sc.STAT)
    m = (rec_plane != id_cases.ID_NONE) & (w_plane > 0)
    r = rec_plane[m].astype(np.int64)
    st["pixels"] = np.bincount(r, minlength=n)
    st["wsum"] = np.bincount(r, weights=sc.quantise(w_plane[m]).astype(np.float64), minlength=n).astype(np.uint64)     # (< 2^53: exact)
    np.maximum.at(st["wmax"], r, w_plane[m])
    return st


# ---- 1. disjoint splats: bit for bit against the ID outputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small", "large", "mixed"])
def test_disjoint_splats_equal_the_id_outputs(gs4d, kind):
    W = H = 96
    rec = sc.records(gs4d, W, H, *sc.disjoint(kind, W, H))
    d = Direct(gs4d, W, H, rec)
    d.ctx.set_id_outputs(True)
    d.frame()
    img_a = d.ctx.read_pixels()
    rid, _, wt = d.ctx.read_ids()
    d.ctx.set_id_outputs(False)
    d.on()
    d.frame()
    img_b = d.ctx.read_pixels()
    got = d.stats()
    ref = d.reference()
    d.close()
    assert ref["layers"].max() == 1                                  # the premise: no pixel has two fragments
    want = from_id_planes(rid, wt, d.n)
    assert (want["pixels"] > 0).all()
    assert np.array_equal(got["pixels"], want["pixels"])
    assert np.array_equal(bits(got["wmax"]), bits(want["wmax"]))
    assert np.array_equal(got["wsum"], want["wsum"])
    assert np.array_equal(bits(img_a), bits(img_b))


# ---- 2., 4. layered splats against the restatement; an image that is no multiple of the tile -------------------------------------------------
@pytest.mark.parametrize("name", list(sc.LAYERED))
def test_layered_splats_equal_the_restatement(gs4d, name, draw_path):
    W, H, params = sc.layered(name)
    d = Direct(gs4d, W, H, sc.records(gs4d, W, H, *params))
    d.on()
    d.frame()
    got = d.stats()
    ref = d.reference()
    longest = d.ctx.stats()["longest_list"]
    d.close()
    cluster = sc.LAYERED[name][4]
    if draw_path == "auto" and cluster:
        assert longest > (256 if cluster >= 300 else 64), longest     # several chunks; a larger PER
    assert ref["fragile"].sum() <= 0.01 * ref["covered"] and not ref["subnormal"]
    sc.check(got, ref)


# ---- 3. a pixel whose T reaches exactly 0 ----------------------------------------------------------------------------------------------------
def test_nothing_counts_behind_a_pixel_whose_T_is_zero(gs4d):
    """65 x 65: the image's centre is the centre of pixel (32, 32).  In front a record of alpha 1 centred there (cg = 1, al = 1, T = 0 exactly);
    behind it two records over the same pixels.  Alone they count that pixel; behind the opaque centre they do not."""
    W = H = 65
    px, py = np.full(3, 32.5), np.full(3, 32.5)
    z = np.array([-4.0, -2.0, 3.0])                                   # instance order is the blend order: the last record is in front
    rgba = np.array([[1, 0, 0, 0.6], [0, 1, 0, 0.9], [0, 0, 1, 1.0]], np.float32)
    rec = sc.records(gs4d, W, H, px, py, z, [sc.S_LARGE, sc.S_SMALL, sc.S_SMALL], rgba)
    d = Direct(gs4d, W, H, rec)
    d.on()
    d.frame()
    got = d.stats()
    ref = d.reference()
    pj = d.ctx.debug_projected(3)
    d.close()
    assert pj[2, 0] == F(32.5) and pj[2, 1] == F(32.5) and ref["T"][32, 32] == 0.0 and (ref["T"] == 0).sum() == 1      # the premise
    sc.check(got, ref)
    assert got["wmax"][2] == F(1.0)
    solo = Direct(gs4d, W, H, rec[:2])                                 # the two records behind, without the opaque one
    solo.on()
    solo.frame()
    alone = solo.stats()
    solo_ref = solo.reference()
    solo.close()
    assert solo_ref["layers"][32, 32] == 2 and ref["layers"][32, 32] == 1
    assert got["pixels"][1] < alone["pixels"][1] and got["pixels"][0] < alone["pixels"][0]
    assert np.array_equal(got["pixels"], ref["stats"]["pixels"]) and np.array_equal(alone["pixels"], solo_ref["stats"]["pixels"])


# ---- 5. accumulation -------------------------------------------------------------------------------------------------------------------------
def test_accumulation_over_draws_and_frames(gs4d):
    W, H, params = sc.layered("chunks")
    d = Direct(gs4d, W, H, sc.records(gs4d, W, H, *params))
    d.on()
    d.frame()
    one = d.stats()
    assert one["pixels"].sum() > 0
    # two draws in one frame: the second draw starts from T = 1 again (T is draw-local), so it adds the same
    d.zero()
    d.frame(draws=2)
    two = d.stats()
    assert np.array_equal(two["pixels"], 2 * one["pixels"]) and np.array_equal(two["wsum"], 2 * one["wsum"]) and np.array_equal(bits(two["wmax"]), bits(one["wmax"]))
    # N frames back to back, no read-back in between, more frames than lanes
    d.zero()
    N = d.ctx.stats()["lanes"] + 2
    for _ in range(N):
        d.frame()
    many = d.stats()
    assert np.array_equal(many["pixels"], N * one["pixels"]) and np.array_equal(many["wsum"], np.uint64(N) * one["wsum"]) and np.array_equal(bits(many["wmax"]), bits(one["wmax"]))
    # statistics off: the buffer is untouched
    d.off()
    d.frame()
    d.ctx.finish()
    assert same_stats(d.stats(), many)
    # zeros uploaded between frames start a new count
    d.on()
    d.frame()
    d.zero()
    d.frame()
    assert same_stats(d.stats(), one)
    d.close()


# ---- 6. re-runs count once --------------------------------------------------------------------------------------------------------------------
def fresh_stats_4d(gs4d, W, H, rec, cam, t, key_mode=None):
    ctx = gs4d.Context(W, H)
    out = sorted_frame(gs4d, ctx, rec, cam, t, W, H, key_mode)
    ctx.close()
    return out


def sorted_frame(gs4d, ctx, rec, cam, t, W, H, key_mode=None, bufs=None, sb=None, view_proj=None):
    """Clear -> key loop -> sort -> Draw of `rec` with statistics on; returns the statistics"""
    n = rec.shape[0]
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    db, kb, ib = bufs or (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    own = sb is None
    sb = ctx.record_stats(n) if own else sb
    view, proj = view_proj or (gs4d.look_at(cam[0], cam[1]), gs4d.perspective(staged_cases.scenes.FOV, W, H, staged_cases.scenes.ZNEAR, staged_cases.scenes.ZFAR))
    ctx.set_record_stats(sb, n)
    ctx.clear()
    ctx.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
    ctx.keygen(db, t, cam[0], kb, ib, n, **({} if key_mode is None else {"key_mode": key_mode}))
    ctx.sort_pairs(kb, ib, n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.draw_instanced(n)
    return ctx.read_record_stats(sb, n)


def test_a_staged_miss_counts_once(gs4d, monkeypatch, draw_path):
    """staged_cases' case a: frames at T0 teach the guesses, the frame at T1 outgrows a segment block and is re-run with exact lists"""
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    rec, times = staged_cases.build(gs4d, "a")
    W, H, n = staged_cases.W, staged_cases.H, rec.shape[0]
    want = fresh_stats_4d(gs4d, W, H, rec, staged_cases.CAM, staged_cases.T1)
    ctx = gs4d.Context(W, H)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    sb = ctx.record_stats(n)
    lanes = ctx.stats()["lanes"]
    for _ in range(2 * lanes + 8):
        ctx.set_record_stats(None)
        warm_frame(gs4d, ctx, bufs, n, staged_cases.T0, W, H)
    ctx.finish()
    s0 = ctx.stats()
    got = sorted_frame(gs4d, ctx, rec, staged_cases.CAM, staged_cases.T1, W, H, bufs=bufs, sb=sb)
    s1 = ctx.stats()
    ctx.close()
    if draw_path == "auto":
        assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
        assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened
    assert want["pixels"].sum() > 0
    assert same_stats(got, want)


def warm_frame(gs4d, ctx, bufs, n, t, W, H):
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


def test_a_list_length_rerun_counts_once(gs4d, draw_path):
    """capacity_cases' c384 as quads: a new context launches the compositor for lists of 256, the long tile holds 330 entries — the draw aborts on
    the device (VF_LIST) and is re-run with a larger capacity.  The same draw again on the same context (no re-run) must give the same."""
    s = cc.Scene("c384")
    verts, _ = s.quads(gs4d)
    W, H = cc.W, cc.H
    view, proj = cc.mats(gs4d)
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    vb = ctx.buffer(verts)
    sb = ctx.record_stats(s.n)
    ctx.set_mode(gs4d.MODE_3D_FULL)
    ctx.set_uniforms(view=view, proj=proj)
    ctx.set_record_stats(sb, s.n)
    ctx.clear()
    ctx.draw_quads(vb, s.n)
    first = ctx.read_record_stats(sb, s.n)
    s1 = ctx.stats()
    ctx.subdata(sb, np.zeros(s.n, gs4d.Context.RECORD_STAT))
    ctx.clear()
    ctx.draw_quads(vb, s.n)
    second = ctx.read_record_stats(sb, s.n)
    s2 = ctx.stats()
    pj = ctx.debug_projected(s.n)
    ctx.close()
    if draw_path == "auto":
        assert s1["reruns"] == 1 and s2["reruns"] == 1 and s1["longest_list"] > 256, (s1, s2)      # the first draw was re-run, the second was not
    assert first["pixels"].sum() > 0
    assert same_stats(first, second)
    ref = sc.restate(id_cases.from_device(pj), None, W, H)
    assert np.array_equal(first["pixels"][ref["fragile_cover"] == 0], ref["stats"]["pixels"][ref["fragile_cover"] == 0])


# ---- 7. tile shards --------------------------------------------------------------------------------------------------------------------------
def test_tile_shards_add_up(gs4d):
    W, H, params = sc.layered("overlap")
    rec = sc.records(gs4d, W, H, *params)
    whole = Direct(gs4d, W, H, rec)
    whole.on()
    whole.frame()
    want = whole.stats()
    whole.close()
    parts = []
    shards = [Direct(gs4d, W, H, rec) for _ in range(2)]              # two contexts alive at once in one process
    for rank, d in enumerate(shards):
        d.ctx.set_tile_shard(rank, 2)
        d.on()
        d.frame()
    for d in shards:
        parts.append(d.stats())
        d.close()
    assert parts[0]["pixels"].sum() > 0 and parts[1]["pixels"].sum() > 0
    assert np.array_equal(parts[0]["pixels"] + parts[1]["pixels"], want["pixels"])
    assert np.array_equal(parts[0]["wsum"] + parts[1]["wsum"], want["wsum"])
    assert np.array_equal(bits(np.maximum(parts[0]["wmax"], parts[1]["wmax"])), bits(want["wmax"]))


# ---- 8. modes --------------------------------------------------------------------------------------------------------------------------------
def test_quads_count_by_quad(gs4d):
    W, H, params = sc.layered("edges")
    verts = sc.quads(gs4d, W, H, *params)
    n = verts.shape[0]
    view, proj = sc.mats(gs4d, W, H)
    ctx = gs4d.Context(W, H)
    vb, sb = ctx.buffer(verts), ctx.record_stats(n)
    ctx.set_mode(gs4d.MODE_3D_FULL)
    ctx.set_uniforms(view=view, proj=proj)
    ctx.set_record_stats(sb, n)
    ctx.clear()
    ctx.draw_quads(vb, n)
    got = ctx.read_record_stats(sb, n)
    ref = sc.restate(id_cases.from_device(ctx.debug_projected(n)), None, W, H)
    ctx.close()
    assert got["pixels"].sum() > 0
    sc.check(got, ref)


def test_sorted_mode_counts_by_the_sort_index_entry_and_skips_what_lies_beyond_the_table(gs4d):
    """GS4D_MODE_4D_SORTED with an index the caller wrote: a permutation (the index is the entry, not the instance); then the same index with
    some entries pointing beyond nrecords — beyond the table, and beyond the data: skipped, no error, every other record as before."""
    W, H, params = sc.layered("edges")
    rec = sc.records(gs4d, W, H, *params)
    n = rec.shape[0]
    perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
    view, proj = sc.mats(gs4d, W, H)
    ctx = gs4d.Context(W, H)
    db, ib, sb = ctx.buffer(rec), ctx.buffer(perm), ctx.record_stats(n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.set_record_stats(sb, n)
    ctx.clear()
    ctx.draw_instanced(n)
    got = ctx.read_record_stats(sb, n)
    proj_dev = id_cases.from_device(ctx.debug_projected(n))
    ref = sc.restate(proj_dev, perm, W, H)
    assert got["pixels"].sum() > 0 and not np.array_equal(ref["stats"]["pixels"], ref["stats"]["pixels"][perm])      # (keyed by instance it would differ)
    sc.check(got, ref)
    # a table shorter than the data: entries >= nrecords are drawn and not counted; the buffer behind the table is not touched
    short = n - 40
    ctx.subdata(sb, np.zeros(n, gs4d.Context.RECORD_STAT))
    ctx.set_record_stats(sb, short)
    ctx.clear()
    ctx.draw_instanced(n)
    got2 = ctx.read_record_stats(sb, n)
    assert same_stats(got2[:short], got[:short]) and not got2["pixels"][short:].any() and not got2["wsum"][short:].any()
    # a hostile index: some entries beyond the data — not drawn, not counted, no error
    hostile = perm.copy()
    bad = np.arange(0, n, 7)
    hostile[bad] = np.uint32(n) + np.arange(bad.size, dtype=np.uint32) * np.uint32(1000003)
    ctx.subdata(ib, hostile)
    ctx.subdata(sb, np.zeros(n, gs4d.Context.RECORD_STAT))
    ctx.set_record_stats(sb, n)
    ctx.clear()
    ctx.draw_instanced(n)
    got3 = ctx.read_record_stats(sb, n)
    ctx.finish()
    ctx.close()
    ref3 = sc.restate(proj_dev, hostile, W, H)
    assert not got3["pixels"][perm[bad]].any()
    sc.check(got3, ref3)


# ---- 9. state and errors -----------------------------------------------------------------------------------------------------------------------
def test_state_and_errors(gs4d):
    W, H, params = sc.layered("edges")
    d = Direct(gs4d, W, H, sc.records(gs4d, W, H, *params))
    c, lib = d.ctx, gs4d._lib
    d.on()
    d.frame()
    one = d.stats()
    assert one["pixels"].sum() > 0
    # a dead or short buffer: GS4D_E_INVALID, the state is kept
    small = c.buffer(nbytes=16 * (d.n - 1))
    dead = c.buffer(nbytes=16 * d.n)
    c.delete(dead)
    assert lib.gs4d_set_record_stats(c._h, dead, d.n) == -1
    assert lib.gs4d_set_record_stats(c._h, small, d.n) == -1
    assert lib.gs4d_set_record_stats(c._h, 9999, 1) == -1
    d.frame()
    two = d.stats()
    assert np.array_equal(two["pixels"], 2 * one["pixels"])            # still on, still the same buffer
    # the three combinations that are out of scope: GS4D_E_UNSUPPORTED, nothing drawn, nothing added
    def refused():
        c.clear()
        rc = lib.gs4d_draw_instanced(c._h, d.n)
        img = c.read_pixels()
        assert rc == -3, rc
        assert np.array_equal(bits(img), bits(np.broadcast_to(np.array(gs4d.CLEAR_COLOR, np.float32), img.shape)))
        assert same_stats(d.stats(), two)
    c.set_blend(gs4d.ONE, gs4d.ONE)
    refused()
    c.set_blend(gs4d.SRC_ALPHA, gs4d.ONE_MINUS_SRC_ALPHA)
    for setter in (c.set_aux_outputs, c.set_id_outputs):
        setter(True)
        refused()
        setter(False)
    plane = c.depth_plane(np.full((H, W), np.inf, np.float32))
    c.set_depth_test(plane)
    refused()
    c.set_depth_test(None)
    # lines never count
    c.clear()
    d.off()
    c.draw_instanced(d.n)
    d.on()
    c.draw_lines(np.array([[-0.9, -0.9], [0.9, 0.9]], np.float32), (1.0, 1.0, 0.0, 1.0), width=3.0)
    c.finish()
    assert same_stats(d.stats(), two)
    # destroying the buffer turns the statistics off: the next draw is an ordinary draw
    c.delete(d.sb)
    c.clear()
    c.draw_instanced(d.n)
    assert c.read_pixels()[..., :3].std() > 0
    d.close()
