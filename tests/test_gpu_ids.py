"""GPU: ID outputs — per pixel, the splat record that contributes most to the final colour, its draw and its weight
(gs4d_set_id_outputs / gs4d_read_ids*).

Contract: within a draw, each fragment has the weight w = T * al its colour accumulates with; the draw's candidate is the largest w > 0, the
front-most on a tie.  The draw composes it over the stored {record, draw, weight} with the colour's "over": weight <- T_final * weight, and
the candidate replaces the triple when w_cand >= weight.  A clear, and every tile no draw reached, holds {0xFFFFFFFF, 0xFFFFFFFF, 0}.
Checked against tests/id_cases.py (a numpy restatement of the compositor, itself checked against the CPU checker on the CPU), against the
GPU's own colour (a record painted red over black gives its weight), and across lanes, paths, staged misses, shards and resizes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import id_cases
import scenes
import staged_cases as sc

pytestmark = pytest.mark.gpu
NONE = id_cases.ID_NONE
BLACK = (0.0, 0.0, 0.0, 0.0)


@pytest.fixture(autouse=True, params=["auto", "ordered"])
def draw_path(request, monkeypatch):
    """Every test runs on both draw paths, as tests/test_gpu_aux.py does."""
    if request.param == "ordered":
        monkeypatch.setenv("GS4D_DRAW_PATH", "ordered")
    else:
        monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    return request.param


def mats(gs4d, cam, W, H):
    return gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_ids(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


class Scene:
    """One context with a record set uploaded; frame() replays Clear -> key loop -> sort -> Draw (MODE_4D_SORTED)."""

    def __init__(self, gs4d, W, H, rec, clear=None):
        self.gs4d, self.W, self.H, self.n = gs4d, W, H, rec.shape[0]
        self.ctx = gs4d.Context(W, H)
        self.ctx.set_clear_color(clear if clear is not None else gs4d.CLEAR_COLOR)
        self.db, self.kb, self.ib = self.ctx.buffer(rec), self.ctx.buffer(nbytes=4 * self.n), self.ctx.buffer(nbytes=4 * self.n)

    def frame(self, cam, t=0.0, ids=None, aux=None):
        g, c = self.gs4d, self.ctx
        if aux is not None:
            c.set_aux_outputs(aux)
        if ids is not None:
            c.set_id_outputs(ids)
        view, proj = mats(g, cam, self.W, self.H)
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
        c.keygen(self.db, t, cam[0], self.kb, self.ib, self.n)
        c.sort_pairs(self.kb, self.ib, self.n)
        c.set_mode(g.MODE_4D_SORTED)
        c.bind(1, self.ib)
        c.bind(2, self.db)
        c.draw_instanced(self.n)
        return view, proj

    def close(self):
        self.ctx.close()


def check_parity(got, want):
    """the device's planes against the restatement of one draw: records equal off the near-tie mask and among the two best on it,
    weights within 2e-6, draw 0 wherever there is a record"""
    rec, drw, w = got
    ok = ~want["fragile"]                                            # pixels where a fragment's discard (cg >= 1e-4) is decided by the last ulp
    tie = want["tie"] & ok
    off = ~want["tie"] & ok
    assert rec.shape == want["record"].shape
    bad = off & (rec != want["record"])
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), rec[bad][:5].tolist(), want["record"][bad][:5].tolist())
    assert ((rec[tie] == want["record"][tie]) | (rec[tie] == want["second"][tie])).all()
    assert np.abs(w[ok].astype(np.float64) - want["weight"][ok]).max() <= 2e-6
    hit = (want["record"] != NONE) & ok
    miss = (want["record"] == NONE) & ok
    assert (drw[hit] == 0).all() and (drw[miss] == NONE).all() and (w[miss] == 0).all()
    assert hit.mean() > 0.001                                        # something was drawn
    assert want["tie"].mean() < 0.01 and want["fragile"].mean() < 1e-3


# ---- 1. colour and aux unchanged ------------------------------------------------------------------------------------------------------
def test_c2_full_size_colour_and_aux_unchanged(gs4d):
    """10^6 splats (configs[1]) at 1080p: colour bit-equal with IDs off and on, aux bit-equal with aux alone and with IDs"""
    n, W, H = 1_000_000, 1920, 1080
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    s = Scene(gs4d, W, H, rec)
    s.frame(scenes.CAM_CUBE)
    img_off = s.ctx.read_pixels()
    with pytest.raises(gs4d.Gs4dError):
        s.ctx.read_ids()
    s.frame(scenes.CAM_CUBE, aux=True)
    aux_only = s.ctx.read_aux()
    s.frame(scenes.CAM_CUBE, aux=False, ids=True)
    img_on = s.ctx.read_pixels()
    aux_on = s.ctx.read_aux()                                        # IDs imply aux
    rec_, drw, w = s.ctx.read_ids()
    s.close()
    assert np.array_equal(bits(img_on), bits(img_off))
    assert np.array_equal(bits(aux_on), bits(aux_only))
    hit = rec_ != NONE
    assert hit.mean() > 0.1 and (rec_[hit] < n).all() and (drw[hit] == 0).all() and (w[hit] > 0).all() and (w <= 1.0).all()


def test_configs3_set_colour_and_aux_unchanged(gs4d):
    n, W, H = 1_000_000, 1920, 1080
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)
    rec = gs4d.build_records_4d(pos4, q, scale, life, fade, vel, rgba)
    s = Scene(gs4d, W, H, rec)
    for t in (0.0, 25.0):
        s.frame(scenes.CAM_CUBE, t=t, aux=False, ids=False)
        img_off = s.ctx.read_pixels()
        s.frame(scenes.CAM_CUBE, t=t, aux=True)
        aux_only = s.ctx.read_aux()
        s.frame(scenes.CAM_CUBE, t=t, aux=False, ids=True)
        assert np.array_equal(bits(s.ctx.read_pixels()), bits(img_off)), t
        assert np.array_equal(bits(s.ctx.read_aux()), bits(aux_only)), t
        rec_, _, w = s.ctx.read_ids()
        assert (rec_ != NONE).mean() > 0.05 and (rec_[rec_ != NONE] < n).all()
        s.ctx.set_id_outputs(False)
    s.close()


# ---- 2. parity with the restatement ---------------------------------------------------------------------------------------------------
def sorted_parity(gs4d, rec, cam, W, H, t):
    s = Scene(gs4d, W, H, rec)
    s.frame(cam, t=t, ids=True)
    got = s.ctx.read_ids()
    pj = s.ctx.debug_projected(s.n)
    perm = s.ctx.read(s.ib, np.uint32, s.n)
    s.close()
    check_parity(got, id_cases.restate(id_cases.from_device(pj), perm, W, H))


def test_teapot_parity(gs4d, oracle):
    rec = oracle.golden("linear_first1000")
    sorted_parity(gs4d, rec, scenes.CAM_TEAPOT, 1920, 1080, 0.0)


@pytest.mark.parametrize("t", [0.0, 12.5, 25.0])
def test_4d_cube_cut_parity(gs4d, t):
    n, W, H = 30000, 960, 540
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n, seed=5)
    rec = gs4d.build_records_4d(pos4, q, scale * 4.0, life, fade, vel, rgba)
    sorted_parity(gs4d, rec, scenes.CAM_CUBE, W, H, t)


def test_nonlinear_block_parity(gs4d, oracle):
    rec = np.ascontiguousarray(gs4d.scene_nonlinear(oracle.golden("teapot_vdata"))[:40000])
    sorted_parity(gs4d, rec, scenes.CAM_NONLINEAR, 1280, 720, 10.0)


def test_3d_full_quads_parity(gs4d):
    m, W, H = 400, 512, 384
    pos, q, sc_, rgba = scenes.cube_params(m, seed=82)
    verts = np.stack([gs4d.splat3d_mesh(pos[i] * 0.05, q[i], sc_[i] * 2.0, rgba[i]) for i in range(m)])
    view, proj = mats(gs4d, ((150.0, 100.0, -60.0), (-0.77, -0.57, 0.27)), W, H)
    ctx = gs4d.Context(W, H)
    vb = ctx.buffer(verts)
    ctx.set_mode(gs4d.MODE_3D_FULL)
    ctx.set_uniforms(view=view, proj=proj)
    ctx.clear()
    ctx.draw_quads(vb, m)
    img_off = ctx.read_pixels()
    ctx.set_id_outputs(True)
    ctx.clear()
    ctx.draw_quads(vb, m)
    img_on = ctx.read_pixels()
    got = ctx.read_ids()
    pj = ctx.debug_projected(m)
    ctx.close()
    assert np.array_equal(bits(img_on), bits(img_off))
    check_parity(got, id_cases.restate(id_cases.from_device(pj), None, W, H, premult=True))


def records_2d(m, seed=2):
    rng = np.random.default_rng(seed)
    rec2 = np.zeros((m, 12), np.float32)
    rec2[:, 0:2] = rng.uniform(-2.0, 2.0, (m, 2))
    rec2[:, 4:8] = rng.uniform(0.2, 1.0, (m, 4))
    for i in range(m):
        ang, s0, s1 = rng.uniform(0, np.pi), rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4)
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        S = R @ np.diag([s0 * s0, s1 * s1]) @ R.T
        rec2[i, 8:12] = [S[0, 0], S[1, 0], S[0, 1], S[1, 1]]
    return rec2


def test_2d_records_parity(gs4d):
    m, W, H = 40, 640, 360
    view, proj = mats(gs4d, scenes.CAM_CUBE, W, H)
    ctx = gs4d.Context(W, H)
    b2 = ctx.buffer(records_2d(m))
    ctx.set_id_outputs(True)
    ctx.set_mode(gs4d.MODE_2D)
    ctx.set_uniforms(view=view, proj=proj)
    ctx.bind(1, b2)
    ctx.clear()
    ctx.draw_instanced(m)
    got = ctx.read_ids()
    pj = ctx.debug_projected(m)
    ctx.close()
    check_parity(got, id_cases.restate(id_cases.from_device(pj), None, W, H))


# ---- 3. frames of several draws, lines, blend, disable --------------------------------------------------------------------------------
def test_two_draws_over_rule_ordinals_lines_blend_and_disable(gs4d, oracle):
    n, W, H = 20000, 640, 360
    pos, q, scale, rgba = scenes.cube_params(n, seed=11)
    rec = gs4d.build_records_3d(pos, q, scale * 3.0, rgba)
    view, proj = mats(gs4d, scenes.CAM_CUBE, W, H)
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.set_id_outputs(True)
    a, b = ctx.buffer(np.ascontiguousarray(rec[: n // 2])), ctx.buffer(np.ascontiguousarray(rec[n // 2:]))
    ctx.set_mode(gs4d.MODE_4D_DIRECT)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)

    def one(*bufs, lines_between=False):
        ctx.clear()
        for k, buf in enumerate(bufs):
            if lines_between and k:
                ctx.draw_lines(np.array([[-1.0, -1.0], [1.0, 1.0]], np.float32), (1.0, 0.0, 0.0, 1.0), width=3.0)
            ctx.bind(1, buf)
            ctx.draw_instanced(n // 2)
        return ctx.read_ids()

    ctx.clear()
    assert same_ids(ctx.read_ids(), id_cases.sentinel(H, W))         # a clear alone
    ia = one(a)
    ib = one(b)
    tb = 1.0 - ctx.read_aux()[..., 1].astype(np.float64)              # draw b's final transmittance (to float rounding)
    both = one(a, b)
    assert (ia[0] != NONE).mean() > 0.05 and (ib[0] != NONE).mean() > 0.05
    assert {0, 1} <= set(np.unique(both[1]).tolist()) <= {0, 1, NONE}
    from_b = both[1] == 1
    from_a = both[1] == 0
    # a pixel whose triple came from draw 1 holds draw b's candidate exactly; from draw 0, draw a's record with its weight faded by b's T
    assert np.array_equal(both[0][from_b], ib[0][from_b]) and np.array_equal(bits(both[2][from_b]), bits(ib[2][from_b]))
    assert np.array_equal(both[0][from_a], ia[0][from_a])
    assert np.abs(both[2][from_a] - tb[from_a] * ia[2][from_a]).max() <= 1e-6
    # the choice: the newer draw wins where its candidate is at least the faded old weight (decided away from float rounding)
    faded = tb * ia[2]
    clear_b = (ib[0] != NONE) & (ib[2] > faded + 1e-6)
    clear_a = (ia[0] != NONE) & ((ib[0] == NONE) | (ib[2] < faded - 1e-6))
    assert from_b[clear_b].all() and from_a[clear_a].all()
    assert clear_a.sum() > 100 and clear_b.sum() > 100
    assert ((both[0] == NONE) == ((ia[0] == NONE) & (ib[0] == NONE))).all()
    # overlay lines: not a draw, and they leave the planes alone — between the draws and after them
    assert same_ids(one(a, b, lines_between=True), both)
    img0 = ctx.read_pixels()
    ctx.draw_lines(np.array([[-1.0, 1.0], [1.0, -1.0]], np.float32), (0.0, 1.0, 0.0, 1.0), width=3.0)
    assert np.abs(ctx.read_pixels() - img0).max() > 0.1
    assert same_ids(ctx.read_ids(), both)
    # another blend function with ID outputs on: refused, nothing drawn
    ctx.clear()
    ctx.set_blend(gs4d.ONE, gs4d.ONE)
    with pytest.raises(gs4d.Gs4dError, match="error -3"):
        ctx.draw_instanced(n // 2)
    assert same_ids(ctx.read_ids(), id_cases.sentinel(H, W))
    assert np.array_equal(ctx.read_pixels(), oracle.clear_image(W, H))
    ctx.set_blend(gs4d.SRC_ALPHA, gs4d.ONE_MINUS_SRC_ALPHA)
    # the refused draw took no ordinal
    ctx.bind(1, a)
    ctx.draw_instanced(n // 2)
    assert same_ids(ctx.read_ids(), ia)
    # ID outputs off: the next cleared frame has none (and no aux outputs either, since aux was never asked for)
    ctx.set_id_outputs(False)
    ctx.clear()
    ctx.draw_instanced(n // 2)
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        ctx.read_ids()
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        ctx.read_aux()
    ctx.close()


# ---- 4. lanes, paths, staged misses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_pipelined_frames_equal_single_frame_renders(gs4d, monkeypatch, lanes):
    monkeypatch.setenv("GS4D_LANES", str(lanes))
    n, W, H = 60000, 640, 360
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n, seed=9)
    rec = gs4d.build_records_4d(pos4, q, scale * 3.0, life, fade, vel, rgba)
    cams = [((551.58 - 8.0 * k, 350.43, -184.33 + 5.0 * k), scenes.CAM_CUBE[1]) for k in range(16)]
    times = [3.0 * k for k in range(16)]
    s = Scene(gs4d, W, H, rec)
    s.ctx.set_id_outputs(True)
    got = []
    for cam, t in zip(cams, times):
        s.frame(cam, t=t)
        got.append(s.ctx.read_ids())
    s.close()
    monkeypatch.delenv("GS4D_LANES", raising=False)
    for k in (0, 5, 10, 15):
        one = Scene(gs4d, W, H, rec)
        one.frame(cams[k], t=times[k], ids=True)
        want = one.ctx.read_ids()
        one.close()
        assert same_ids(got[k], want), k
        assert (want[0] != NONE).mean() > 0.05


@pytest.mark.parametrize("env", ["GS4D_STAGED", "GS4D_STAGED_BOX"])
def test_unstaged_and_unboxed_equal_the_default(gs4d, monkeypatch, env):
    n, W, H = 60000, 640, 360
    pos, q, scale, rgba = scenes.cube_params(n, seed=3)
    rec = gs4d.build_records_3d(pos, q, scale * 2.0, rgba)
    out = {}
    for val in (None, "0"):
        if val is None:
            monkeypatch.delenv(env, raising=False)
        else:
            monkeypatch.setenv(env, val)
        s = Scene(gs4d, W, H, rec)
        s.ctx.set_id_outputs(True)
        for _ in range(12):                                          # steady state: the default context stages its draws
            s.frame(scenes.CAM_CUBE)
        out[val] = s.ctx.read_ids()
        s.close()
    assert same_ids(out[None], out["0"])
    assert (out[None][0] != NONE).mean() > 0.05


def test_staged_miss_gives_the_ids_of_an_exact_draw(gs4d, monkeypatch):
    """staged_cases.py case a: frames at T0 teach the guesses, the frame at T1 overflows the last segment's block and is re-run exactly"""
    rec, times = sc.build(gs4d, "a")
    view, proj = sc.mats(gs4d)
    monkeypatch.setenv("GS4D_NB", str(sc.NB))

    def run(staged, warm):
        if staged:
            monkeypatch.delenv("GS4D_STAGED", raising=False)
        else:
            monkeypatch.setenv("GS4D_STAGED", "0")
        ctx = gs4d.Context(sc.W, sc.H)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_id_outputs(True)
        n = rec.shape[0]
        data, keys, idx = ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
        for k, t in enumerate([sc.T0] * warm + [times[0]]):
            if warm and k == warm:
                ctx.finish()                                         # as test_gpu_staged_misses.py's warm-up: validated before the miss frame
            ctx.clear()
            ctx.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
            ctx.keygen(data, t, sc.CAM[0], keys, idx, n)
            ctx.sort_pairs(keys, idx, n)
            ctx.set_mode(gs4d.MODE_4D_SORTED)
            ctx.bind(1, idx)
            ctx.bind(2, data)
            ctx.draw_instanced(n)
        ids = ctx.read_ids()
        st = ctx.stats()
        ctx.close()
        return ids, st

    want, st0 = run(False, 0)
    assert st0["staged_draws"] == 0
    got, st = run(True, 2 * 4 + 8)
    if st["unordered_draws"]:
        assert st["staged_misses"] >= 1 and st["reruns"] >= 1, st
    assert same_ids(got, want)
    assert (want[0] != NONE).any()


# ---- 5. shards and resize ---------------------------------------------------------------------------------------------------------------
def test_tile_shards_and_resize(gs4d):
    n, W, H = 50000, 800, 448
    pos, q, scale, rgba = scenes.cube_params(n, seed=3)
    rec = gs4d.build_records_3d(pos, q, scale * 2.0, rgba)
    full = Scene(gs4d, W, H, rec)
    full.frame(scenes.CAM_CUBE, ids=True)
    want = full.ctx.read_ids()
    # resize: new planes of the new size; reads of the old size are refused; the next frame renders as a fresh context of that size does
    W2, H2 = 480, 272
    full.ctx.resize(W2, H2)
    full.W, full.H = W2, H2
    full.frame(scenes.CAM_CUBE)
    got2 = full.ctx.read_ids()
    assert got2[0].shape == (H2, W2)
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        full.ctx.read_ids((W2 - 4, 0, 8, 8))
    with pytest.raises(gs4d.Gs4dError, match="error -1"):
        full.ctx.read_ids_device(1, 1, 1, W * H * 4)                  # never dereferenced: the size is refused first
    full.close()
    fresh = Scene(gs4d, W2, H2, rec)
    fresh.frame(scenes.CAM_CUBE, ids=True)
    assert same_ids(got2, fresh.ctx.read_ids())
    fresh.close()
    rows = np.arange(H) // 8
    for rank in (0, 1):
        s = Scene(gs4d, W, H, rec)
        s.ctx.set_tile_shard(rank, 2)
        s.frame(scenes.CAM_CUBE, ids=True)
        got = s.ctx.read_ids()
        s.close()
        mine = rows % 2 == rank
        assert same_ids([x[mine] for x in got], [x[mine] for x in want]), rank
        assert same_ids([x[~mine] for x in got], [x[~mine] for x in id_cases.sentinel(H, W)]), rank


# ---- 6. picking -------------------------------------------------------------------------------------------------------------------------
def test_pick_one_known_splat_under_a_permuted_sort_index(gs4d):
    """record 137 of 400 is a large, nearly opaque splat in front of the others: a pick at its projected centre returns its DATA index
    (MODE_4D_SORTED draws it at some other instance), and its weight is the red of a render in which only it is red, onto black"""
    m, K, W, H = 400, 137, 640, 480
    pos, q, scale, rgba = scenes.cube_params(m, seed=21)
    pos = (pos * 0.1).astype(np.float32)
    cam = ((0.0, 0.0, 120.0), (0.0, 0.0, -1.0))
    pos[K] = (35.0, 25.0, 60.0)                                      # in front, and away from the cluster of the others
    scale[K] = (300.0, 300.0, 300.0)
    rgba[K] = (0.8, 0.4, 0.2, 0.95)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    s = Scene(gs4d, W, H, rec)
    view, proj = s.frame(cam, ids=True)
    perm = s.ctx.read(s.ib, np.uint32, m)
    pj = s.ctx.debug_projected(m)
    px, py = int(pj[K, 0]), int(pj[K, 1])
    p = s.ctx.pick(px, py, view, proj)
    s.close()
    assert int(np.nonzero(perm == K)[0][0]) != K                      # the sort index does permute it
    assert p is not None and p["record"] == K and p["draw"] == 0 and p["weight"] > 0.5, p
    pixel_width = 2.0 * p["depth"] * np.tan(np.radians(scenes.FOV) / 2.0) / H
    assert np.linalg.norm(p["point"].astype(np.float64) - pos[K]) <= 2.0 * pixel_width, (p, pos[K])
    # the weight is the share of the final colour: paint K red, everything else black with the same alphas, over black
    c = np.zeros_like(rgba)
    c[:, 3] = rgba[:, 3]
    c[K, 0] = 1.0
    s2 = Scene(gs4d, W, H, gs4d.build_records_3d(pos, q, scale, c), clear=BLACK)
    s2.frame(cam)
    red = s2.ctx.read_pixels()[py, px, 0]
    s2.close()
    assert abs(float(red) - p["weight"]) <= 1e-6, (float(red), p["weight"])


def test_pick_returns_none_on_a_sentinel_pixel(gs4d):
    W, H = 64, 64
    ctx = gs4d.Context(W, H)
    ctx.set_id_outputs(True)
    ctx.clear()
    view, proj = mats(gs4d, scenes.CAM_CUBE, W, H)
    assert ctx.pick(10, 20, view, proj) is None
    ctx.close()


# ---- 7. rectangles and device reads -----------------------------------------------------------------------------------------------------
def test_rectangle_reads_are_slices_of_a_full_read(gs4d):
    n, W, H = 20000, 640, 360
    pos, q, scale, rgba = scenes.cube_params(n, seed=4)
    rec = gs4d.build_records_3d(pos, q, scale * 3.0, rgba)
    s = Scene(gs4d, W, H, rec)
    s.frame(scenes.CAM_CUBE, ids=True)
    full = s.ctx.read_ids()
    for x, y, w, h in ((0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (17, 203, 129, 41), (300, 0, 5, H)):
        got = s.ctx.read_ids((x, y, w, h))
        assert same_ids(got, [a[y:y + h, x:x + w] for a in full]), (x, y, w, h)
    for bad in ((-1, 0, 4, 4), (0, -1, 4, 4), (W - 3, 0, 4, 4), (0, H - 3, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0)):
        with pytest.raises(gs4d.Gs4dError, match="error -1"):
            s.ctx.read_ids(bad)
    s.close()
    assert (full[0] != NONE).mean() > 0.05


def test_read_ids_device_into_torch_tensors():
    """gs4d_read_ids_device into torch tensors equals gs4d_read_ids: a program of its own (tests/gpu_ids_device_read.py), because torch
    has to initialise its HIP runtime before libgs4d.so is loaded (the draw path of this run is passed on through the environment)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_ids_device_read.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ids device read ok" in r.stdout
