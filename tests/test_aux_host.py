"""CPU: the host half of the aux outputs — gs4d_host_unproject, and the argument checks of the new entry points.
No GPU needed: unproject is CPU code of libgs4d.so, and every aux entry point refuses a NULL context before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import scenes


def project(view, proj, W, H, x):
    """float64: world point -> (pixel px, py as unproject takes them, view depth -z_view)"""
    V = np.asarray(view, np.float64).reshape(4, 4).T          # column-major -> row-major
    P = np.asarray(proj, np.float64).reshape(4, 4).T
    v = V @ np.append(np.asarray(x, np.float64), 1.0)
    c = P @ v
    ndc = c[:3] / c[3]
    return (ndc[0] + 1.0) * 0.5 * W - 0.5, (ndc[1] + 1.0) * 0.5 * H - 0.5, -v[2]


@pytest.mark.parametrize("W,H,cam", [(1920, 1080, scenes.CAM_CUBE), (640, 360, scenes.CAM_TEAPOT), (3840, 2160, scenes.CAM_NONLINEAR), (333, 517, ((1.0, -2.0, 3.0), (0.3, 0.2, -1.0)))])
def test_unproject_inverts_projection(gs4d, W, H, cam):
    view = gs4d.look_at(cam[0], cam[1])
    proj = gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    rng = np.random.default_rng(W + H)
    eye = np.asarray(cam[0], np.float64)
    fwd = np.asarray(cam[1], np.float64) / np.linalg.norm(cam[1])
    checked = 0
    for _ in range(400):
        x = eye + fwd * rng.uniform(1.0, 800.0) + rng.normal(0.0, 60.0, 3)
        px, py, d = project(view, proj, W, H, x)
        if d <= scenes.ZNEAR or not (-0.5 <= px <= W - 0.5 and -0.5 <= py <= H - 0.5):
            continue
        got = gs4d.unproject(view, proj, W, H, px, py, d).astype(np.float64)
        assert np.linalg.norm(got - x) <= 1e-4 * max(1.0, np.linalg.norm(x)), (x, got)
        checked += 1
    assert checked > 100


def test_unproject_pixel_centre_convention(gs4d):
    """pixel (px, py) means window coordinates (px + 0.5, py + 0.5), row 0 at the bottom: the centre of the image lies on the view axis"""
    W, H = 64, 32
    view = gs4d.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    proj = gs4d.perspective(60.0, W, H, 0.1, 100.0)
    p = gs4d.unproject(view, proj, W, H, W / 2 - 0.5, H / 2 - 0.5, 10.0)
    np.testing.assert_allclose(p, [0.0, 0.0, -10.0], atol=1e-5)
    top = gs4d.unproject(view, proj, W, H, W / 2 - 0.5, H - 1, 10.0)
    assert top[1] > 0.0                                          # the last row is the top of the picture


def test_aux_entry_points_refuse_a_null_context(gs4d):
    lib = gs4d._lib
    buf = (C.c_float * 8)()
    assert lib.gs4d_set_aux_outputs(None, 1) == -1
    assert lib.gs4d_set_aux_outputs(None, 0) == -1
    assert lib.gs4d_read_aux(None, C.cast(buf, C.c_void_p), 8 * 4) == -1
    assert lib.gs4d_read_aux(None, None, 0) == -1
    assert lib.gs4d_read_aux_device(None, C.cast(buf, C.c_void_p), 8 * 4) == -1
    assert lib.gs4d_read_aux_device(None, None, 0) == -1
