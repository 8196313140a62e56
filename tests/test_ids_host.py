"""CPU: the host half of the ID outputs — the numpy restatement the GPU tests hold the compositor to (tests/id_cases.py),
and the argument checks of the new entry points.  No GPU needed: the restatement is checked against the CPU checker, and every ID entry
point refuses a NULL context before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import id_cases
import scenes


def _mats(gs4d, cam, W, H):
    return gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)


def _restatement_matches_the_checker(oracle, rec, cam, view, proj, W, H, t, covered):
    clear = np.asarray(oracle.CLEAR, np.float32)
    img, perm, _ = oracle.render_4d(rec, True, t, 0.0, cam[0], view, proj, W, H, clear=clear)
    eproj = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H, t, 0.0)
    r = id_cases.restate(eproj, perm, W, H)
    got = r["rgb"] + r["T"][..., None] * clear[None, None, :3]
    assert np.abs(got - img[..., :3]).max() <= 1e-6
    # a pixel with a record has a positive weight and some transmittance used up; the sentinel exactly where nothing was blended
    hit = r["record"] != id_cases.ID_NONE
    assert hit.mean() > covered
    assert (r["weight"][hit] > 0).all() and not r["weight"][~hit].any()
    assert (r["T"][~hit] == 1.0).all()
    # the candidate is a record that was drawn, and no weight exceeds the alpha it was drawn with
    assert np.isin(r["record"][hit], perm).all()
    assert (r["weight"][hit] <= np.clip(eproj["alpha"][r["record"][hit]], 0.0, 1.0) + 1e-7).all()
    assert r["tie"].mean() < 0.01
    return r


def test_restatement_reproduces_the_checker_on_a_teapot_cut(gs4d, oracle):
    rec = oracle.golden("linear_first1000")
    W, H = 480, 270
    view, proj = _mats(gs4d, scenes.CAM_TEAPOT, W, H)
    _restatement_matches_the_checker(oracle, rec, scenes.CAM_TEAPOT, view, proj, W, H, 0.0, 0.005)


@pytest.mark.parametrize("t", [0.0, 25.0])
def test_restatement_reproduces_the_checker_on_a_4d_cube_cut(gs4d, oracle, t):
    n, W, H = 6000, 320, 180
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n, seed=5)
    rec = gs4d.build_records_4d(pos4, q, scale * 4.0, life, fade, vel, rgba)
    view, proj = _mats(gs4d, scenes.CAM_CUBE, W, H)
    _restatement_matches_the_checker(oracle, rec, scenes.CAM_CUBE, view, proj, W, H, t, 0.02)


def test_over_rule():
    """DESIGN.md §4's composition: the stored weight fades with the newer draw's transmittance; the newer candidate wins ties"""
    old = (np.array([[7, 7, 7, 7]], np.uint32), np.array([[0, 0, 0, 0]], np.uint32), np.array([[0.5, 0.5, 0.5, 0.5]], np.float32))
    T = np.array([[1.0, 0.5, 0.5, 0.5]], np.float32)
    rec, drw, w = id_cases.over(T, np.array([[3, 3, 3, id_cases.ID_NONE]], np.uint32), np.array([[0.2, 0.25, 0.3, 0.0]], np.float32), 1, old)
    assert rec.tolist() == [[7, 3, 3, 7]] and drw.tolist() == [[0, 1, 1, 0]]
    np.testing.assert_array_equal(w, np.array([[0.5, 0.25, 0.3, 0.25]], np.float32))
    rec, drw, w = id_cases.over(np.ones((1, 1), np.float32), np.array([[5]], np.uint32), np.array([[0.1]], np.float32), 0, id_cases.sentinel(1, 1))
    assert (rec[0, 0], drw[0, 0], w[0, 0]) == (5, 0, np.float32(0.1))


def test_id_entry_points_are_declared_and_exported(gs4d):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs4d.h")).read()
    for name in ("gs4d_set_id_outputs", "gs4d_read_ids", "gs4d_read_ids_device"):
        assert f"GS4D_API int {name}(" in header, name
        assert name in gs4d.EXPORTS, name
        assert getattr(gs4d._lib, name) is not None
    for m in ("set_id_outputs", "read_ids", "read_ids_device", "pick"):
        assert callable(getattr(gs4d.Context, m)), m


def test_id_entry_points_refuse_a_null_context(gs4d):
    lib = gs4d._lib
    rec = (C.c_uint32 * 4)()
    drw = (C.c_uint32 * 4)()
    wt = (C.c_float * 4)()
    vp = lambda a: C.cast(a, C.c_void_p)          # noqa: E731
    assert lib.gs4d_set_id_outputs(None, 1) == -1
    assert lib.gs4d_set_id_outputs(None, 0) == -1
    assert lib.gs4d_read_ids(None, 0, 0, 2, 2, vp(rec), vp(drw), vp(wt)) == -1
    assert lib.gs4d_read_ids(None, 0, 0, 1, 1, None, None, None) == -1
    assert lib.gs4d_read_ids_device(None, vp(rec), vp(drw), vp(wt), 16) == -1
    assert lib.gs4d_read_ids_device(None, None, None, None, 0) == -1
