"""GPU: aux outputs — per-pixel depth D and opacity O beside the colour (gs4d_set_aux_outputs / gs4d_read_aux*).

Contract: a draw with the default blend function accumulates, with the weights w_i = T_i * al_i of its colour, D_draw = sum w_i d_i
(d_i = -z_view of record i's centre, slot 15 of the projected record) and O_draw = 1 - T_final, composed over the frame's planes with the
colour's "over"; a clear gives (0, 0); overlay lines do not touch them.  Checked against the CPU checker by colour substitution — a record
coloured (d_i / s, 1, 0) composited onto black gives s * R = D and G = O — and against the GPU's own colour path at full size.
"""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu
BLACK = (0.0, 0.0, 0.0, 0.0)


@pytest.fixture(autouse=True, params=["auto", "ordered"])
def draw_path(request, monkeypatch):
    """Every test runs on both draw paths, as tests/test_gpu_render.py does."""
    if request.param == "ordered":
        monkeypatch.setenv("GS4D_DRAW_PATH", "ordered")
    else:
        monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    return request.param


def mats(gs4d, cam, W, H):
    return gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)


class Scene:
    """One context with a record set uploaded; frame() replays Clear -> key loop -> sort -> Draw."""

    def __init__(self, gs4d, W, H, rec, clear=None):
        self.gs4d, self.W, self.H, self.n = gs4d, W, H, rec.shape[0]
        self.ctx = gs4d.Context(W, H)
        self.ctx.set_clear_color(clear if clear is not None else gs4d.CLEAR_COLOR)
        self.db, self.kb, self.ib = self.ctx.buffer(rec), self.ctx.buffer(nbytes=4 * self.n), self.ctx.buffer(nbytes=4 * self.n)

    def frame(self, cam, t=0.0, sort=True, aux=None):
        g, c = self.gs4d, self.ctx
        if aux is not None:
            c.set_aux_outputs(aux)
        view, proj = mats(g, cam, self.W, self.H)
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
        if sort:
            c.keygen(self.db, t, cam[0], self.kb, self.ib, self.n)
            c.sort_pairs(self.kb, self.ib, self.n)
            c.set_mode(g.MODE_4D_SORTED)
            c.bind(1, self.ib)
            c.bind(2, self.db)
        else:
            c.set_mode(g.MODE_4D_DIRECT)
            c.bind(1, self.db)
        c.draw_instanced(self.n)
        return view, proj

    def close(self):
        self.ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def depth_np(rec, view, t):
    """-z_view of the time-conditioned centre, float32 in the projection kernel's order (preprocess.hip project_4d / project3d)"""
    r = rec.astype(np.float32)
    V = np.asarray(view, np.float32)
    dt = np.float32(t) - r[:, 3]
    k = (np.float32(1.0) / r[:, 23]) * dt
    mx, my, mz = r[:, 0] + k * r[:, 11], r[:, 1] + k * r[:, 15], r[:, 2] + k * r[:, 19]
    pcz = ((V[2] * mx + V[6] * my) + V[10] * mz) + V[14] * np.float32(1.0)
    return -pcz


def substituted(eproj, d):
    """the checker's projected records with colour (d / s, 1, 0): s * R = D and G = O after compositing onto black"""
    s = float(d.max())
    p = eproj.copy()
    p["r"], p["g"], p["b"] = (d / np.float32(s)).astype(np.float32), np.float32(1.0), np.float32(0.0)
    return p, s


def check_against_checker(oracle, aux, eproj, d, order, frag_mode, W, H):
    p, s = substituted(eproj, d)
    e = oracle.composite(p, order, frag_mode, W, H, np.zeros((H, W, 4), np.float32))
    assert np.abs(aux[..., 0].astype(np.float64) - s * e[..., 0].astype(np.float64)).max() <= 1e-4 * s
    assert np.abs(aux[..., 1].astype(np.float64) - e[..., 1]).max() <= 1e-4
    assert aux[..., 1].max() > 0.3                                  # something was drawn


def recolour_3d(gs4d, pos, q, scale, rgba, d):
    s = float(d.max())
    c = np.stack([d / np.float32(s), np.ones_like(d), np.zeros_like(d), rgba[:, 3]], axis=1).astype(np.float32)
    return gs4d.build_records_3d(pos, q, scale, c), s


def test_c2_full_size_colour_unchanged_and_aux_equals_the_gpus_own_colour(gs4d):
    """10^6 splats (configs[1]) at 1080p: the colour with aux on is bit-equal to aux off; slot 15 is 0 with aux off and -z_view with it on;
    D and O equal the GPU's own colour image of the same records recoloured (d / s, 1, 0) over black."""
    n, W, H = 1_000_000, 1920, 1080
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    cam = scenes.CAM_CUBE
    sc = Scene(gs4d, W, H, rec)
    view, _ = sc.frame(cam, aux=False)
    img_off = sc.ctx.read_pixels()
    pj = sc.ctx.debug_projected(n)
    assert np.all(pj[:, 15] == 0.0)
    with pytest.raises(gs4d.Gs4dError):
        sc.ctx.read_aux()                                            # the frame was cleared with aux outputs off
    sc.frame(cam, aux=True)
    img_on = sc.ctx.read_pixels()
    aux = sc.ctx.read_aux()
    pj = sc.ctx.debug_projected(n)
    sc.close()
    assert np.array_equal(bits(img_on), bits(img_off))
    valid = pj[:, 14] != 0
    assert valid.mean() > 0.99
    np.testing.assert_allclose(pj[valid, 15], depth_np(rec, view, 0.0)[valid], rtol=1e-6)
    d = np.where(valid, pj[:, 15], 0.0).astype(np.float32)
    rec2, s = recolour_3d(gs4d, pos, q, scale, rgba, d)
    sc2 = Scene(gs4d, W, H, rec2, clear=BLACK)
    sc2.frame(cam, aux=False)
    e = sc2.ctx.read_pixels()
    sc2.close()
    assert np.abs(aux[..., 0].astype(np.float64) - s * e[..., 0].astype(np.float64)).max() <= 1e-5 * s
    assert np.abs(aux[..., 1].astype(np.float64) - e[..., 1]).max() <= 1e-5
    assert aux[..., 1].max() > 0.5


def test_configs3_set_colour_unchanged_depth_slot_and_full_size_aux(gs4d):
    """configs[3]'s 10^6 true 4D splats at t in {0, 12.5, 25}: colour bit-equal with aux on and off, slot 15 = -z_view of the conditioned
    centre; at t = 25 also D and O against the GPU's colour of the recoloured records."""
    n, W, H = 1_000_000, 1920, 1080
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)
    rec = gs4d.build_records_4d(pos4, q, scale, life, fade, vel, rgba)
    cam = scenes.CAM_CUBE
    sc = Scene(gs4d, W, H, rec)
    for t in (0.0, 12.5, 25.0):
        sc.frame(cam, t=t, aux=False)
        img_off = sc.ctx.read_pixels()
        assert np.all(sc.ctx.debug_projected(n)[:, 15] == 0.0)
        view, _ = sc.frame(cam, t=t, aux=True)
        img_on = sc.ctx.read_pixels()
        aux = sc.ctx.read_aux()
        pj = sc.ctx.debug_projected(n)
        assert np.array_equal(bits(img_on), bits(img_off)), t
        valid = pj[:, 14] != 0
        np.testing.assert_allclose(pj[valid, 15], depth_np(rec, view, t)[valid], rtol=1e-6)
    sc.close()
    d = np.where(valid, pj[:, 15], 0.0).astype(np.float32)
    s = float(d.max())
    c = np.stack([d / np.float32(s), np.ones_like(d), np.zeros_like(d), rgba[:, 3]], axis=1).astype(np.float32)
    sc2 = Scene(gs4d, W, H, gs4d.build_records_4d(pos4, q, scale, life, fade, vel, c), clear=BLACK)
    sc2.frame(cam, t=25.0, aux=False)
    e = sc2.ctx.read_pixels()
    sc2.close()
    assert np.abs(aux[..., 0].astype(np.float64) - s * e[..., 0].astype(np.float64)).max() <= 1e-5 * s
    assert np.abs(aux[..., 1].astype(np.float64) - e[..., 1]).max() <= 1e-5


def test_teapot_colour_unchanged_and_parity_with_the_checker(gs4d, oracle):
    """the reference-generated teapot records (LinearMotion, first 1000), sorted, 1080p"""
    rec = oracle.golden("linear_first1000")
    n, W, H = rec.shape[0], 1920, 1080
    sc = Scene(gs4d, W, H, rec)
    sc.frame(scenes.CAM_TEAPOT, aux=False)
    img_off = sc.ctx.read_pixels()
    view, proj = sc.frame(scenes.CAM_TEAPOT, aux=True)
    img_on = sc.ctx.read_pixels()
    aux = sc.ctx.read_aux()
    pj = sc.ctx.debug_projected(n)
    perm = sc.ctx.read(sc.ib, np.uint32, n)
    sc.close()
    assert np.array_equal(bits(img_on), bits(img_off))
    eproj = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H)
    valid = eproj["valid"] != 0
    np.testing.assert_allclose(pj[valid, 15], depth_np(rec, view, 0.0)[valid], rtol=1e-6)
    check_against_checker(oracle, aux, eproj, pj[:, 15].copy(), perm, oracle.MODE_4D, W, H)


@pytest.mark.parametrize("t", [0.0, 12.5, 25.0])
def test_4d_cube_cut_parity_with_the_checker(gs4d, oracle, t):
    n, W, H = 30000, 960, 540
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n, seed=5)
    rec = gs4d.build_records_4d(pos4, q, scale * 4.0, life, fade, vel, rgba)
    sc = Scene(gs4d, W, H, rec)
    view, proj = sc.frame(scenes.CAM_CUBE, t=t, aux=True)
    aux = sc.ctx.read_aux()
    pj = sc.ctx.debug_projected(n)
    perm = sc.ctx.read(sc.ib, np.uint32, n)
    sc.close()
    eproj = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H, t, 0.0)
    check_against_checker(oracle, aux, eproj, pj[:, 15].copy(), perm, oracle.MODE_4D, W, H)


def test_nonlinear_block_parity_with_the_checker(gs4d, oracle):
    rec = np.ascontiguousarray(gs4d.scene_nonlinear(oracle.golden("teapot_vdata"))[:40000])
    n, W, H, t = rec.shape[0], 1280, 720, 10.0
    sc = Scene(gs4d, W, H, rec)
    view, proj = sc.frame(scenes.CAM_NONLINEAR, t=t, aux=True)
    aux = sc.ctx.read_aux()
    pj = sc.ctx.debug_projected(n)
    perm = sc.ctx.read(sc.ib, np.uint32, n)
    sc.close()
    eproj = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H, t, 0.0)
    check_against_checker(oracle, aux, eproj, pj[:, 15].copy(), perm, oracle.MODE_4D, W, H)


def test_3d_full_quads_parity_with_the_checker(gs4d, oracle):
    """MODE_3D_FULL premultiplies its colour per fragment; the weights do not depend on it: the checker composites in MODE_4D fragment mode"""
    m, W, H = 400, 512, 384
    pos, q, sc_, rgba = scenes.cube_params(m, seed=82)
    verts = np.stack([gs4d.splat3d_mesh(pos[i] * 0.05, q[i], sc_[i] * 2.0, rgba[i]) for i in range(m)])
    cam = ((150.0, 100.0, -60.0), (-0.77, -0.57, 0.27))
    view, proj = mats(gs4d, cam, W, H)
    ctx = gs4d.Context(W, H)
    vb = ctx.buffer(verts)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.set_mode(gs4d.MODE_3D_FULL)
    ctx.set_uniforms(view=view, proj=proj)
    ctx.clear()
    ctx.draw_quads(vb, m)
    img_off = ctx.read_pixels()
    ctx.set_aux_outputs(True)
    ctx.clear()
    ctx.draw_quads(vb, m)
    img_on = ctx.read_pixels()
    aux = ctx.read_aux()
    pj = ctx.debug_projected(m)
    ctx.close()
    assert np.array_equal(bits(img_on), bits(img_off))
    eproj = oracle.preprocess(oracle.MODE_3D, verts, view, proj, W, H)
    assert (pj[eproj["valid"] != 0, 15] > 0).all()
    check_against_checker(oracle, aux, eproj, pj[:, 15].copy(), None, oracle.MODE_4D, W, H)


def test_frames_over_rule_clear_lines_blend_and_2d(gs4d, oracle):
    n, W, H = 20000, 640, 360
    pos, q, scale, rgba = scenes.cube_params(n, seed=11)
    rec = gs4d.build_records_3d(pos, q, scale * 3.0, rgba)
    cam = scenes.CAM_CUBE
    view, proj = mats(gs4d, cam, W, H)
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.set_aux_outputs(True)
    a, b = ctx.buffer(np.ascontiguousarray(rec[: n // 2])), ctx.buffer(np.ascontiguousarray(rec[n // 2:]))
    ctx.set_mode(gs4d.MODE_4D_DIRECT)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)

    def one(*bufs):
        ctx.clear()
        for buf in bufs:
            ctx.bind(1, buf)
            ctx.draw_instanced(n // 2)
        return ctx.read_aux()

    # a clear alone: (0, 0) everywhere
    ctx.clear()
    assert not ctx.read_aux().any()
    da, db_ = one(a), one(b)
    both = one(a, b)
    tb = 1.0 - db_[..., 1].astype(np.float64)
    s = float(np.abs(da[..., 0]).max())
    assert np.abs(both[..., 0] - (db_[..., 0] + tb * da[..., 0])).max() <= 1e-5 * s
    assert np.abs(both[..., 1] - (db_[..., 1] + tb * da[..., 1])).max() <= 1e-5
    assert da[..., 1].max() > 0.3 and db_[..., 1].max() > 0.3
    # overlay lines change the colour, not D or O
    img0 = ctx.read_pixels()
    ctx.draw_lines(np.array([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, -1.0]], np.float32), (1.0, 0.0, 0.0, 1.0), width=3.0)
    assert np.abs(ctx.read_pixels() - img0).max() > 0.1
    assert np.array_equal(bits(ctx.read_aux()), bits(both))
    # lines first (every tile goes into memory with (0, 0)), then a draw over them: the same planes as without the lines
    ctx.clear()
    ctx.draw_lines(np.array([[-1.0, 0.0], [1.0, 0.0]], np.float32), (0.0, 1.0, 0.0, 1.0), width=2.0)
    ctx.bind(1, a)
    ctx.draw_instanced(n // 2)
    assert np.array_equal(bits(ctx.read_aux()), bits(da))
    # another blend function with aux outputs on: refused, nothing drawn
    ctx.clear()
    ctx.set_blend(gs4d.ONE, gs4d.ONE)
    with pytest.raises(gs4d.Gs4dError, match="error -3"):
        ctx.draw_instanced(n // 2)
    assert not ctx.read_aux().any()
    assert np.array_equal(ctx.read_pixels(), oracle.clear_image(W, H))
    ctx.set_blend(gs4d.SRC_ALPHA, gs4d.ONE_MINUS_SRC_ALPHA)
    # aux outputs off: draws as before, the frame has no aux planes to read; other blend functions draw again
    ctx.set_aux_outputs(False)
    ctx.clear()
    ctx.set_blend(gs4d.ONE, gs4d.ONE)
    ctx.draw_instanced(n // 2)
    ctx.set_blend(gs4d.SRC_ALPHA, gs4d.ONE_MINUS_SRC_ALPHA)
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        ctx.read_aux()
    # MODE_2D: O as the checker has it, D = 0
    m = 40
    rng = np.random.default_rng(2)
    rec2 = np.zeros((m, 12), np.float32)
    rec2[:, 0:2] = rng.uniform(-2.0, 2.0, (m, 2))
    rec2[:, 4:8] = rng.uniform(0.2, 1.0, (m, 4))
    for i in range(m):
        ang, s0, s1 = rng.uniform(0, np.pi), rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4)
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        S = R @ np.diag([s0 * s0, s1 * s1]) @ R.T
        rec2[i, 8:12] = [S[0, 0], S[1, 0], S[0, 1], S[1, 1]]
    b2 = ctx.buffer(rec2)
    ctx.set_aux_outputs(True)
    ctx.set_mode(gs4d.MODE_2D)
    ctx.bind(1, b2)
    ctx.clear()
    ctx.draw_instanced(m)
    aux = ctx.read_aux()
    ctx.close()
    eproj = oracle.preprocess(oracle.MODE_2D, rec2, view, proj, W, H)
    eproj["g"] = 1.0
    e = oracle.composite(eproj, None, oracle.MODE_2D, W, H, np.zeros((H, W, 4), np.float32))
    assert not aux[..., 0].any()
    assert np.abs(aux[..., 1] - e[..., 1]).max() <= 1e-4
    assert aux[..., 1].max() > 0.3


@pytest.mark.parametrize("lanes", [None, 1])
def test_pipelined_frames_equal_single_frame_renders(gs4d, monkeypatch, lanes):
    """16 frames of a moving camera and time, aux read every frame, against each frame rendered alone in a fresh context"""
    if lanes:
        monkeypatch.setenv("GS4D_LANES", str(lanes))
    n, W, H = 60000, 640, 360
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n, seed=9)
    rec = gs4d.build_records_4d(pos4, q, scale * 3.0, life, fade, vel, rgba)
    cams = [((551.58 - 8.0 * k, 350.43, -184.33 + 5.0 * k), scenes.CAM_CUBE[1]) for k in range(16)]
    times = [3.0 * k for k in range(16)]
    sc = Scene(gs4d, W, H, rec)
    sc.ctx.set_aux_outputs(True)
    got = []
    for cam, t in zip(cams, times):
        sc.frame(cam, t=t)
        got.append(sc.ctx.read_aux())
    sc.close()
    monkeypatch.delenv("GS4D_LANES", raising=False)
    for k in (0, 5, 10, 15):
        one = Scene(gs4d, W, H, rec)
        one.frame(cams[k], t=times[k], aux=True)
        want = one.ctx.read_aux()
        one.close()
        assert np.array_equal(bits(got[k]), bits(want)), k
        assert want[..., 1].max() > 0.3


def test_tile_shard_bands(gs4d):
    n, W, H = 50000, 800, 448
    pos, q, scale, rgba = scenes.cube_params(n, seed=3)
    rec = gs4d.build_records_3d(pos, q, scale * 2.0, rgba)
    full = Scene(gs4d, W, H, rec)
    full.frame(scenes.CAM_CUBE, aux=True)
    want = full.ctx.read_aux()
    full.close()
    rows = np.arange(H) // 8
    for rank in (0, 1):
        sc = Scene(gs4d, W, H, rec)
        sc.ctx.set_tile_shard(rank, 2)
        sc.frame(scenes.CAM_CUBE, aux=True)
        got = sc.ctx.read_aux()
        sc.close()
        mine = rows % 2 == rank
        assert np.array_equal(bits(got[mine]), bits(want[mine])), rank
        assert not got[~mine].any()


def test_staged_miss_gives_the_aux_of_exact_draws(gs4d, monkeypatch):
    """the shapes of tests/test_gpu_staged.py::test_a_guess_that_does_not_fit_is_rerun_exactly: far frames, then a jump into the cube"""
    n, W, H = 150_000, 800, 448
    pos, q, scale, rgba = scenes.cube_params(n, seed=7)
    rec = gs4d.build_records_3d(pos, q, scale * 2.0, rgba)
    far = ((1400.0, 900.0, -500.0), scenes.CAM_CUBE[1])
    near = ((330.0, 210.0, -110.0), scenes.CAM_CUBE[1])
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    sc = Scene(gs4d, W, H, rec)
    sc.ctx.set_aux_outputs(True)
    for _ in range(8):
        sc.frame(far)
    sc.frame(near)
    got = sc.ctx.read_aux()
    st = sc.ctx.stats()
    sc.close()
    monkeypatch.setenv("GS4D_STAGED", "0")
    ex = Scene(gs4d, W, H, rec)
    ex.frame(near, aux=True)
    want = ex.ctx.read_aux()
    ex.close()
    if st["unordered_draws"]:
        assert st["staged_misses"] >= 1, st
    assert np.array_equal(bits(got), bits(want))


def test_picking_one_splat(gs4d):
    W, H = 640, 480
    pos = np.array([[12.0, -7.0, 3.0]], np.float32)
    q = np.array([[1.0, 0.0, 0.0, 0.0]], np.float32)
    scale = np.array([[300.0, 300.0, 300.0]], np.float32)         # ~10 px across at this distance (the quad has no focal length in J)
    rgba = np.array([[0.8, 0.4, 0.2, 0.9]], np.float32)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    cam = ((40.0, 30.0, 120.0), (-0.25, -0.3, -1.0))
    sc = Scene(gs4d, W, H, rec)
    view, proj = sc.frame(cam, aux=True)
    aux = sc.ctx.read_aux(normalized=True)
    pj = sc.ctx.debug_projected(1)
    sc.close()
    px, py = int(pj[0, 0]), int(pj[0, 1])                            # the pixel whose centre is nearest the projected centre
    d = float(aux[py, px, 0])
    assert aux[py, px, 1] > 0.5 and d > 0.0
    p = gs4d.unproject(view, proj, W, H, px, py, d)
    pixel_width = 2.0 * d * np.tan(np.radians(scenes.FOV) / 2.0) / H
    assert np.linalg.norm(p.astype(np.float64) - pos[0]) <= pixel_width, (p, pos[0], pixel_width)


def test_read_aux_device_into_a_torch_tensor():
    """gs4d_read_aux_device into a torch tensor equals gs4d_read_aux: run as a program of its own (tests/gpu_aux_device_read.py) because torch
    has to initialise its HIP runtime before libgs4d.so is loaded (the draw path of this run is passed on through the environment)."""
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_aux_device_read.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "aux device read ok" in r.stdout
