"""GPU: the depth test against a caller's depth plane (gs4d_set_depth_test) — splats among opaque geometry.

Contract: a fragment of record i at pixel p is blended only if d_i < Z[p] (float32, GL_LESS), d_i the record depth of the aux outputs (slot 15
of the projected record).  A fragment that fails is treated like a discarded one (al = 0), so colour, aux and ID planes all follow the test.

Oracle: the TWIN (tests/ztest_cases.py) — the same frame without the test in which every record hidden at a pixel has alpha 0 in its data.
It has the test run's own lists, paths and blend order, so the match is bit for bit.  A plane with several values is checked pixel by pixel
against one twin per distinct value.  d_i comes from slot 15 of an aux frame of the same records and camera.  Every test runs on both draw
paths."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
import ztest_cases as zc

pytestmark = pytest.mark.gpu
ALPHA = 7                      # col.w of a 96-byte record
INF = np.float32(np.inf)


@pytest.fixture(autouse=True, params=["auto", "ordered"])
def draw_path(request, monkeypatch):
    """Every test runs on both draw paths, as tests/test_gpu_aux.py does."""
    if request.param == "ordered":
        monkeypatch.setenv("GS4D_DRAW_PATH", "ordered")
    else:
        monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    return request.param


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mats(gs4d, cam, W, H):
    return gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)


class Scene:
    """One context with a record set uploaded; frame() replays Clear -> (key loop -> sort) -> Draw and reads back what the frame has."""

    def __init__(self, gs4d, W, H, rec, outputs="colour", sort=True):
        self.gs4d, self.W, self.H, self.n, self.sort = gs4d, W, H, rec.shape[0], sort
        self.ctx = gs4d.Context(W, H)
        self.ctx.set_clear_color(gs4d.CLEAR_COLOR)
        self.db, self.kb, self.ib = self.ctx.buffer(rec), self.ctx.buffer(nbytes=4 * self.n), self.ctx.buffer(nbytes=4 * self.n)
        self.outputs(outputs)

    def outputs(self, which):
        self.which = which
        self.ctx.set_aux_outputs(which == "aux")
        self.ctx.set_id_outputs(which == "ids")

    def draw(self, cam, t=0.0):
        g, c = self.gs4d, self.ctx
        view, proj = mats(g, cam, self.W, self.H)
        c.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
        if self.sort:
            c.keygen(self.db, t, cam[0], self.kb, self.ib, self.n)
            c.sort_pairs(self.kb, self.ib, self.n)
            c.set_mode(g.MODE_4D_SORTED)
            c.bind(1, self.ib)
            c.bind(2, self.db)
        else:
            c.set_mode(g.MODE_4D_DIRECT)
            c.bind(1, self.db)
        c.draw_instanced(self.n)

    def frame(self, cam, t=0.0):
        self.ctx.clear()
        self.draw(cam, t)
        return self.read()

    def read(self):
        out = {"rgba": self.ctx.read_pixels()}
        if self.which in ("aux", "ids"):
            out["aux"] = self.ctx.read_aux()
        if self.which == "ids":
            out["ids"] = self.ctx.read_ids()
        return out

    def close(self):
        self.ctx.close()


def record_depths(gs4d, W, H, rec, cam, t=0.0, sort=True):
    """slot 15 of an aux frame of the same records and camera, and the validity flags"""
    sc = Scene(gs4d, W, H, rec, "aux", sort=sort)
    sc.frame(cam, t)
    pj = sc.ctx.debug_projected(sc.n)
    sc.close()
    return pj[:, 15].copy(), pj[:, 14] != 0


def assert_same(got, want, where=None):
    """bit-equal colour, aux and ID planes (optionally only where the boolean (H, W) mask holds)"""
    sel = (lambda a: a) if where is None else (lambda a: a[where])
    assert np.array_equal(bits(sel(got["rgba"])), bits(sel(want["rgba"])))
    if "aux" in want:
        assert np.array_equal(bits(sel(got["aux"])), bits(sel(want["aux"])))
    if "ids" in want:
        for a, b in zip(got["ids"], want["ids"]):
            assert np.array_equal(bits(sel(a)), bits(sel(b)))


def merged(twins, Z):
    """the image put together pixel by pixel from the twin of each pixel's plane value"""
    first = twins[next(iter(twins))]
    out = {"rgba": first["rgba"].copy()}
    if "aux" in first:
        out["aux"] = first["aux"].copy()
    if "ids" in first:
        out["ids"] = tuple(x.copy() for x in first["ids"])
    assert np.isin(Z, np.array(list(twins), np.float32)).all()        # every pixel has its twin
    for z, tw in twins.items():
        m = Z == z
        out["rgba"][m] = tw["rgba"][m]
        if "aux" in out:
            out["aux"][m] = tw["aux"][m]
        if "ids" in out:
            for a, b in zip(out["ids"], tw["ids"]):
                a[m] = b[m]
    return out


def cube_3d(gs4d, n, seed=None, grow=1.0):
    pos, q, scale, rgba = scenes.cube_params(n) if seed is None else scenes.cube_params(n, seed=seed)
    return gs4d.build_records_3d(pos, q, scale * grow, rgba)


def cube_4d(gs4d, n, seed=None, grow=1.0):
    args = scenes.cube_params_4d(n) if seed is None else scenes.cube_params_4d(n, seed=seed)
    pos4, q, scale, life, fade, vel, rgba = args
    return gs4d.build_records_4d(pos4, q, scale * grow, life, fade, vel, rgba)


# ---- 1. +inf everywhere ---------------------------------------------------------------------------------------------------------------
def test_inf_plane_changes_nothing_and_slot15_is_written(gs4d):
    """configs[1]'s 10^6 cube set at 1080p: colour, aux and IDs with a +inf plane are bit-equal to the frame without the test; a draw with the
    test and no aux outputs writes slot 15 exactly as an aux frame does."""
    n, W, H = 1_000_000, 1920, 1080
    rec = cube_3d(gs4d, n)
    cam = scenes.CAM_CUBE
    sc = Scene(gs4d, W, H, rec, "ids")
    want = sc.frame(cam)
    plane = sc.ctx.depth_plane(np.full((H, W), INF))
    sc.ctx.set_depth_test(plane)
    got = sc.frame(cam)
    assert_same(got, want)
    assert want["aux"][..., 1].max() > 0.5
    sc.outputs("colour")
    got_c = sc.frame(cam)
    slot15_test = sc.ctx.debug_projected(n)[:, 15].copy()
    sc.ctx.set_depth_test(None)
    want_c = sc.frame(cam)
    assert not sc.ctx.debug_projected(n)[:, 15].any()                # no test, no aux: slot 15 stays 0
    sc.close()
    assert_same(got_c, want_c)
    d, valid = record_depths(gs4d, W, H, rec, cam)
    assert valid.mean() > 0.99
    assert np.array_equal(bits(slot15_test), bits(d))


# ---- 2. constant thresholds near the quartiles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["c2", "c4_t25"])
def test_constant_thresholds_equal_the_twin(gs4d, which):
    """configs[1]'s 10^6 cube set, and configs[3]'s 10^6 4D set at t = 25, 1080p: a constant plane near each quartile of the record depths gives
    the twin's bits, in frames with no extra outputs, with aux outputs and with ID outputs."""
    n, W, H = 1_000_000, 1920, 1080
    rec, t = (cube_3d(gs4d, n), 0.0) if which == "c2" else (cube_4d(gs4d, n), 25.0)
    cam = scenes.CAM_CUBE
    d, valid = record_depths(gs4d, W, H, rec, cam, t)
    zs = zc.pick_thresholds(d[valid])
    sc = Scene(gs4d, W, H, rec)
    tw = Scene(gs4d, W, H, rec)
    plane = sc.ctx.depth_plane(np.zeros((H, W), np.float32))
    sc.ctx.set_depth_test(plane)
    for z in zs:
        sc.ctx.subdata(plane, np.full((H, W), z, np.float32))
        tw.ctx.subdata(tw.db, zc.hide_alpha(rec, d, z, ALPHA))
        for outputs in ("colour", "aux", "ids"):
            sc.outputs(outputs)
            tw.outputs(outputs)
            got, want = sc.frame(cam, t), tw.frame(cam, t)
            assert_same(got, want)
    sc.close()
    tw.close()


# ---- 3. a per-pixel plane -----------------------------------------------------------------------------------------------------------------
def test_per_pixel_plane_equals_the_twins_pixel_by_pixel(gs4d):
    """8x8 tiles of {three thresholds, +inf, 0}, cut by a diagonal and two 3-pixel stripes; ID outputs (and so aux) on"""
    n, W, H = 1_000_000, 1920, 1080
    rec = cube_3d(gs4d, n)
    cam = scenes.CAM_CUBE
    d, valid = record_depths(gs4d, W, H, rec, cam)
    zs = zc.pick_thresholds(d[valid])
    values = [zs[0], zs[1], zs[2], INF, np.float32(0.0)]
    Z = zc.per_pixel_plane(W, H, values)
    sc = Scene(gs4d, W, H, rec, "ids")
    sc.ctx.set_depth_test(sc.ctx.depth_plane(Z))
    got = sc.frame(cam)
    sc.close()
    tw = Scene(gs4d, W, H, rec, "ids")
    twins = {}
    for z in values:
        tw.ctx.subdata(tw.db, zc.hide_alpha(rec, d, z, ALPHA))
        twins[z] = tw.frame(cam)
    tw.close()
    assert_same(got, merged(twins, Z))
    # Z = 0 is in front of every record (d > 0): those pixels keep the clear colour and values
    clear = np.array(gs4d.CLEAR_COLOR, np.float32)
    assert np.array_equal(got["rgba"][Z == 0], np.broadcast_to(clear, got["rgba"][Z == 0].shape))
    assert not got["aux"][Z == 0].any()
    assert (got["ids"][0][Z == 0] == gs4d.Context.ID_NONE).all()
    assert np.abs(got["rgba"][Z == INF] - clear).max() > 0.3         # something was drawn where nothing hides


# ---- 4. against the CPU checker ---------------------------------------------------------------------------------------------------------
def checker_case(gs4d, oracle, rec, cam, W, H, t, sort):
    """the GPU frame with a per-pixel plane against oracle.composite of the checker's projected records with alpha zeroed per plane value;
    d from depth_np (float32 formula), thresholds in gaps wider than 1e-6 d"""
    view, proj = mats(gs4d, cam, W, H)
    eproj = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H, t, 0.0)
    valid = eproj["valid"] != 0
    d = zc.depth_np(rec, view, t)
    zs = zc.pick_thresholds(d[valid], min_rel_gap=1e-6)
    values = [zs[0], zs[1], zs[2], INF, np.float32(0.0)]
    Z = zc.per_pixel_plane(W, H, values, seed=11)
    sc = Scene(gs4d, W, H, rec, sort=sort)
    sc.ctx.set_depth_test(sc.ctx.depth_plane(Z))
    img = sc.frame(cam, t)["rgba"]
    order = sc.ctx.read(sc.ib, np.uint32, sc.n) if sort else None
    sc.close()
    want = np.empty_like(img)
    for z in values:
        p = eproj.copy()
        p["alpha"][~(d < z)] = 0.0
        e = oracle.composite(p, order, oracle.MODE_4D, W, H, oracle.clear_image(W, H))
        m = Z == z
        want[m] = e[m]
    err = float(np.abs(img.astype(np.float64) - want).max())
    assert err <= 1e-4, err
    assert np.abs(img[Z == INF] - oracle.CLEAR).max() > 0.1


def test_cube_cut_against_the_checker(gs4d, oracle):
    checker_case(gs4d, oracle, cube_3d(gs4d, 4096, seed=21, grow=6.0), scenes.CAM_CUBE, 960, 540, 0.0, True)


def test_teapot_block_against_the_checker(gs4d, oracle):
    checker_case(gs4d, oracle, oracle.golden("linear_first1000"), scenes.CAM_TEAPOT, 1280, 720, 0.0, True)


# ---- 5. modes ----------------------------------------------------------------------------------------------------------------------------
def run_twins(make, Z, values):
    """make(z or None) -> frame dict; the test run with plane Z against the twins of every value"""
    got = make(None)
    twins = {z: make(z) for z in values}
    assert_same(got, merged(twins, Z))
    return got


def test_4d_direct_and_sorted_with_a_caller_index(gs4d):
    n, W, H, t = 60000, 640, 360, 20.0
    rec = cube_4d(gs4d, n, seed=5, grow=3.0)
    cam = scenes.CAM_CUBE
    view, proj = mats(gs4d, cam, W, H)
    for mode in ("direct", "sorted"):
        d, valid = record_depths(gs4d, W, H, rec, cam, t, sort=(mode == "sorted"))
        zs = zc.pick_thresholds(d[valid])
        values = [zs[0], zs[2], INF]
        Z = zc.per_pixel_plane(W, H, values, seed=3)
        idx = np.argsort(-d, kind="stable").astype(np.uint32)[::-1].copy()      # a caller-supplied order (front to back): not the library's sort

        def make(z):
            ctx = gs4d.Context(W, H)
            ctx.set_clear_color(gs4d.CLEAR_COLOR)
            ctx.set_aux_outputs(True)
            db = ctx.buffer(rec if z is None else zc.hide_alpha(rec, d, z, ALPHA))
            ctx.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
            if mode == "direct":
                ctx.set_mode(gs4d.MODE_4D_DIRECT)
                ctx.bind(1, db)
            else:
                ctx.set_mode(gs4d.MODE_4D_SORTED)
                ctx.bind(1, ctx.buffer(idx))
                ctx.bind(2, db)
            if z is None:
                ctx.set_depth_test(ctx.depth_plane(Z))
            ctx.clear()
            ctx.draw_instanced(n)
            out = {"rgba": ctx.read_pixels(), "aux": ctx.read_aux()}
            ctx.close()
            return out

        got = run_twins(make, Z, values)
        assert got["aux"][..., 1].max() > 0.3, mode


def test_quads(gs4d):
    """gs4d_draw_quads: the twin zeroes the vertex alpha of a hidden quad (all four vertices)"""
    m, W, H = 600, 512, 384
    pos, q, sc_, rgba = scenes.cube_params(m, seed=82)
    verts = np.stack([gs4d.splat3d_mesh(pos[i] * 0.05, q[i], sc_[i] * 2.0, rgba[i]) for i in range(m)])
    cam = ((150.0, 100.0, -60.0), (-0.77, -0.57, 0.27))
    view, proj = mats(gs4d, cam, W, H)

    def make(z, d=None):
        ctx = gs4d.Context(W, H)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_id_outputs(True)
        v = verts.copy()
        if z is not None:
            v[~(d < np.float32(z)), :, 8] = 0.0
        vb = ctx.buffer(v)
        ctx.set_mode(gs4d.MODE_3D_FULL)
        ctx.set_uniforms(view=view, proj=proj)
        if z is None and d is not None:
            ctx.set_depth_test(ctx.depth_plane(Z))
        ctx.clear()
        ctx.draw_quads(vb, m)
        out = {"rgba": ctx.read_pixels(), "aux": ctx.read_aux(), "ids": ctx.read_ids()}
        pj = ctx.debug_projected(m)
        ctx.close()
        return out, pj

    _, pj = make(None)
    d, valid = pj[:, 15].copy(), pj[:, 14] != 0
    zs = zc.pick_thresholds(d[valid])
    values = [zs[0], zs[1], zs[2], INF]
    Z = zc.per_pixel_plane(W, H, values, seed=4)
    got, _ = make(None, d)
    twins = {z: make(z, d)[0] for z in values}
    assert_same(got, merged(twins, Z))
    assert got["aux"][..., 1].max() > 0.3


def test_2d_records_have_depth_zero(gs4d):
    """GS4D_MODE_2D: d = 0, so any Z > 0 shows everything and Z = 0 hides everything"""
    m, W, H = 40, 640, 360
    rng = np.random.default_rng(2)
    rec2 = np.zeros((m, 12), np.float32)
    rec2[:, 0:2] = rng.uniform(-2.0, 2.0, (m, 2))
    rec2[:, 4:8] = rng.uniform(0.2, 1.0, (m, 4))
    for i in range(m):
        ang, s0, s1 = rng.uniform(0, np.pi), rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4)
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        S = R @ np.diag([s0 * s0, s1 * s1]) @ R.T
        rec2[i, 8:12] = [S[0, 0], S[1, 0], S[0, 1], S[1, 1]]
    view, proj = mats(gs4d, scenes.CAM_CUBE, W, H)
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.set_id_outputs(True)
    ctx.set_mode(gs4d.MODE_2D)
    ctx.set_uniforms(view=view, proj=proj)
    ctx.bind(1, ctx.buffer(rec2))

    def one():
        ctx.clear()
        ctx.draw_instanced(m)
        return {"rgba": ctx.read_pixels(), "aux": ctx.read_aux(), "ids": ctx.read_ids()}

    want = one()
    Z = np.where(np.arange(W)[None, :] < W // 2 + 3, np.float32(1e-30), np.float32(0.0)) * np.ones((H, 1), np.float32)
    ctx.set_depth_test(ctx.depth_plane(Z.astype(np.float32)))
    got = one()
    ctx.close()
    show = Z > 0
    assert_same(got, want, show)
    assert np.abs(want["rgba"][show] - np.array(gs4d.CLEAR_COLOR, np.float32)).max() > 0.1
    assert np.array_equal(got["rgba"][~show], np.broadcast_to(np.array(gs4d.CLEAR_COLOR, np.float32), got["rgba"][~show].shape))
    assert not got["aux"][~show].any()
    assert (got["ids"][0][~show] == gs4d.Context.ID_NONE).all()


# ---- 6. knobs and paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [("GS4D_STAGED", "0"), ("GS4D_STAGED_BOX", "0"), ("GS4D_LANES", "1")])
def test_knobs(gs4d, monkeypatch, knob):
    monkeypatch.setenv(*knob)
    n, W, H = 200_000, 800, 448
    rec = cube_3d(gs4d, n, seed=7, grow=2.0)
    cam = scenes.CAM_CUBE
    d, valid = record_depths(gs4d, W, H, rec, cam)
    zs = zc.pick_thresholds(d[valid])
    values = [zs[0], zs[1], zs[2], INF, np.float32(0.0)]
    Z = zc.per_pixel_plane(W, H, values, seed=5)
    sc = Scene(gs4d, W, H, rec, "ids")
    sc.ctx.set_depth_test(sc.ctx.depth_plane(Z))
    for _ in range(4):                                                # steady state: staged draws where the knobs allow them
        got = sc.frame(cam)
    sc.close()
    tw = Scene(gs4d, W, H, rec, "ids")
    twins = {}
    for z in values:
        tw.ctx.subdata(tw.db, zc.hide_alpha(rec, d, z, ALPHA))
        for _ in range(4):
            twins[z] = tw.frame(cam)
    tw.close()
    assert_same(got, merged(twins, Z))


def test_staged_miss_after_a_camera_jump(gs4d, monkeypatch):
    """far frames, then a jump into the cube: the staged guess does not fit and the draw is re-run exactly, plane and all"""
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    n, W, H = 150_000, 800, 448
    rec = cube_3d(gs4d, n, seed=7, grow=2.0)
    far = ((1400.0, 900.0, -500.0), scenes.CAM_CUBE[1])
    near = ((330.0, 210.0, -110.0), scenes.CAM_CUBE[1])
    d, valid = record_depths(gs4d, W, H, rec, near)
    zs = zc.pick_thresholds(d[valid])
    values = [zs[0], zs[2], INF]
    Z = zc.per_pixel_plane(W, H, values, seed=6)

    def run(data, plane):
        sc = Scene(gs4d, W, H, data, "ids")
        if plane is not None:
            sc.ctx.set_depth_test(sc.ctx.depth_plane(plane))
        for _ in range(8):
            sc.frame(far)
        out = sc.frame(near)
        st = sc.ctx.stats()
        sc.close()
        return out, st

    got, st = run(rec, Z)
    if st["unordered_draws"]:
        assert st["staged_misses"] >= 1, st
    twins = {z: run(zc.hide_alpha(rec, d, z, ALPHA), None)[0] for z in values}
    assert_same(got, merged(twins, Z))


def test_tile_shard_world_2(gs4d):
    n, W, H = 50000, 800, 448
    rec = cube_3d(gs4d, n, seed=3, grow=2.0)
    cam = scenes.CAM_CUBE
    d, valid = record_depths(gs4d, W, H, rec, cam)
    zs = zc.pick_thresholds(d[valid])
    values = [zs[0], zs[1], INF]
    Z = zc.per_pixel_plane(W, H, values, seed=8)
    rows = np.arange(H) // 8
    for rank in (0, 1):
        def run(data, plane):
            sc = Scene(gs4d, W, H, data, "aux")
            sc.ctx.set_tile_shard(rank, 2)
            if plane is not None:
                sc.ctx.set_depth_test(sc.ctx.depth_plane(plane))
            out = sc.frame(cam)
            sc.close()
            return out
        got = run(rec, Z)
        twins = {z: run(zc.hide_alpha(rec, d, z, ALPHA), None) for z in values}
        assert_same(got, merged(twins, Z))
        mine = rows % 2 == rank
        assert got["aux"][mine][..., 1].max() > 0.3 and not got["aux"][~mine].any()


# ---- 7. several draws in one frame --------------------------------------------------------------------------------------------------------
def test_several_draws_and_lines_in_one_frame(gs4d):
    """draw A with plane P1, draw B without a test, lines, draw C with plane P2 — against the same frame of twins"""
    n, W, H = 30000, 640, 360
    rec = cube_3d(gs4d, 3 * n, seed=11, grow=3.0)
    parts = [np.ascontiguousarray(rec[k * n:(k + 1) * n]) for k in range(3)]
    cam = scenes.CAM_CUBE
    view, proj = mats(gs4d, cam, W, H)
    d, valid = record_depths(gs4d, W, H, rec, cam, sort=False)
    zs = zc.pick_thresholds(d[valid])
    dp = [d[k * n:(k + 1) * n] for k in range(3)]
    lines = np.array([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, -1.0]], np.float32)

    def run(twin):
        ctx = gs4d.Context(W, H)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_id_outputs(True)
        ctx.set_mode(gs4d.MODE_4D_DIRECT)
        ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
        a = ctx.buffer(zc.hide_alpha(parts[0], dp[0], zs[0], ALPHA) if twin else parts[0])
        b = ctx.buffer(parts[1])
        c = ctx.buffer(zc.hide_alpha(parts[2], dp[2], zs[2], ALPHA) if twin else parts[2])
        p1, p2 = ctx.depth_plane(np.full((H, W), zs[0], np.float32)), ctx.depth_plane(np.full((H, W), zs[2], np.float32))
        ctx.clear()
        ctx.set_depth_test(None if twin else p1)
        ctx.bind(1, a)
        ctx.draw_instanced(n)
        ctx.set_depth_test(None)
        ctx.bind(1, b)
        ctx.draw_instanced(n)
        ctx.draw_lines(lines, (1.0, 0.0, 0.0, 1.0), width=3.0)
        ctx.set_depth_test(None if twin else p2)
        ctx.bind(1, c)
        ctx.draw_instanced(n)
        out = {"rgba": ctx.read_pixels(), "aux": ctx.read_aux(), "ids": ctx.read_ids()}
        ctx.close()
        return out

    got, want = run(False), run(True)
    assert_same(got, want)
    drw = got["ids"][1]
    assert set(np.unique(drw).tolist()) <= {0, 1, 2, gs4d.Context.ID_NONE}
    assert all((drw == k).sum() > 100 for k in (0, 1, 2))


# ---- 8. ordering -------------------------------------------------------------------------------------------------------------------------
def test_plane_rewritten_before_every_frame(gs4d):
    """eight frames in the four-lane pipeline; the plane is rewritten by gs4d_buffer_subdata before each frame's draw, and each frame is read
    after the next rewrite: every frame equals its own twin"""
    n, W, H = 200_000, 640, 360
    rec = cube_3d(gs4d, n, seed=13, grow=2.0)
    cam = scenes.CAM_CUBE
    d, valid = record_depths(gs4d, W, H, rec, cam)
    zs = zc.pick_thresholds(d[valid])
    seq = [zs[0], zs[1], zs[2], INF, zs[1], zs[0], INF, zs[2]]
    sc = Scene(gs4d, W, H, rec, "aux")
    plane = sc.ctx.depth_plane(np.full((H, W), seq[0], np.float32))
    sc.ctx.set_depth_test(plane)
    got = []
    for k, z in enumerate(seq):
        sc.ctx.subdata(plane, np.full((H, W), z, np.float32))
        if k:
            got.append(sc.read())                                     # frame k-1, read after the plane was rewritten for frame k
        sc.ctx.clear()
        sc.draw(cam)
    got.append(sc.read())
    sc.close()
    tw = Scene(gs4d, W, H, rec, "aux")
    twins = {}
    for z in set(seq):
        tw.ctx.subdata(tw.db, zc.hide_alpha(rec, d, z, ALPHA))
        twins[z] = tw.frame(cam)
    tw.close()
    for k, z in enumerate(seq):
        assert_same(got[k], twins[z])


def test_plane_written_on_the_callers_stream():
    """gs4d_buffer_device_ptr + gs4d_buffer_invalidate on the caller's stream (tests/gpu_depth_plane_handoff.py, a program of its own:
    torch initialises its HIP runtime before libgs4d.so is loaded)"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_depth_plane_handoff.py")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "depth plane hand-off ok" in r.stdout


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_and_turning_the_test_off(gs4d, oracle):
    n, W, H = 20000, 320, 192
    rec = cube_3d(gs4d, n, seed=17, grow=3.0)
    cam = scenes.CAM_CUBE
    d, valid = record_depths(gs4d, W, H, rec, cam)
    z = zc.pick_thresholds(d[valid])[1]
    sc = Scene(gs4d, W, H, rec, "ids")
    want = sc.frame(cam)                                              # no test
    plane = sc.ctx.depth_plane(np.full((H, W), z, np.float32))
    # an unknown name: INVALID, the state stays as it was (off)
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        sc.ctx.set_depth_test(9999)
    assert_same(sc.frame(cam), want)
    sc.ctx.set_depth_test(plane)
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        sc.ctx.set_depth_test(9999)
    hidden = sc.frame(cam)                                            # ... and on
    assert not np.array_equal(bits(hidden["rgba"]), bits(want["rgba"]))
    # a plane that is too small: INVALID, nothing drawn
    small = sc.ctx.buffer(np.full(W * H - 1, z, np.float32))
    sc.ctx.set_depth_test(small)
    sc.ctx.clear()
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        sc.draw(cam)
    img = sc.read()
    assert np.array_equal(img["rgba"], oracle.clear_image(W, H)) and not img["aux"].any()
    # ... also after a resize that outgrows the plane
    sc.ctx.set_depth_test(plane)
    sc.ctx.resize(W + 8, H)
    sc.W = W + 8
    sc.ctx.clear()
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        sc.draw(cam)
    img = sc.read()
    assert np.array_equal(img["rgba"], oracle.clear_image(W + 8, H)) and not img["aux"].any()
    sc.ctx.resize(W, H)
    sc.W = W
    # another blend function with the test on: UNSUPPORTED, nothing drawn (a frame without aux outputs, so only the test refuses it)
    sc.outputs("colour")
    sc.ctx.set_blend(gs4d.ONE, gs4d.ONE)
    sc.ctx.clear()
    with pytest.raises(gs4d.Gs4dError, match="error -3"):
        sc.draw(cam)
    assert np.array_equal(sc.ctx.read_pixels(), oracle.clear_image(W, H))
    sc.ctx.set_depth_test(None)
    sc.ctx.clear()
    sc.draw(cam)                                                      # without the test the function draws again
    sc.ctx.set_blend(gs4d.SRC_ALPHA, gs4d.ONE_MINUS_SRC_ALPHA)
    sc.outputs("ids")
    # setting 0 turns the test off: the next draw equals a draw without it; so does destroying the plane
    sc.ctx.set_depth_test(plane)
    assert_same(sc.frame(cam), hidden)
    sc.ctx.set_depth_test(0)
    assert_same(sc.frame(cam), want)
    sc.ctx.set_depth_test(plane)
    assert_same(sc.frame(cam), hidden)                                # the state survives clear()
    sc.ctx.delete(plane)
    assert_same(sc.frame(cam), want)
    sc.close()
