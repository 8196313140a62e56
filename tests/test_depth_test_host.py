"""CPU: the depth test's entry points (gs4d_set_depth_test, Context.set_depth_test / depth_plane) and the premises the GPU tests
(tests/test_gpu_depth_test.py) build on: thresholds strictly between consecutive record depths exist near every quartile, and the per-pixel
plane cuts through tiles."""
import os
import re

import numpy as np

import scenes
import ztest_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_depth_test(gs4d):
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert re.search(r"^GS4D_API int gs4d_set_depth_test\(gs4d_ctx\* ctx, gs4d_buf plane\);", hdr, flags=re.M)
    assert "gs4d_set_depth_test" in gs4d.EXPORTS
    assert callable(gs4d.Context.set_depth_test) and callable(gs4d.Context.depth_plane)


def test_cube_set_has_threshold_gaps_near_every_quartile(gs4d, oracle):
    """configs[1]'s 10^6-record cube set from CAM_CUBE at 1080p: within +-10 % of each quartile of the valid records' depths there is a relative
    gap of at least 6e-6 between consecutive distinct depths (50 to 100 float32 ulps), so thresholds that no rounding can move exist."""
    n, W, H = 1_000_000, 1920, 1080
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    view = gs4d.look_at(*scenes.CAM_CUBE)
    proj = gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    valid = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H)["valid"] != 0
    assert valid.mean() > 0.99
    d = zc.depth_np(rec, view, 0.0)[valid]
    assert (d > 0).all()
    z = zc.pick_thresholds(d, min_rel_gap=6e-6)
    assert z[0] < z[1] < z[2]


def test_per_pixel_plane_cuts_through_tiles():
    W, H = 1920, 1080
    vals = [10.0, 20.0, 30.0, np.inf, 0.0]
    Z = zc.per_pixel_plane(W, H, vals)
    assert Z.shape == (H, W) and Z.dtype == np.float32
    assert set(np.unique(Z).tolist()) == set(vals)
    t = Z[: H // 8 * 8, : W // 8 * 8].reshape(H // 8, 8, W // 8, 8)
    mixed = (t.max(axis=(1, 3)) != t.min(axis=(1, 3))).sum()
    assert mixed > 200                                                # the diagonal and both stripes split tiles


def test_twin_hides_exactly_the_records_that_fail():
    rec = np.ones((6, 24), np.float32)
    d = np.array([1.0, 2.0, 3.0, np.nan, 0.0, 2.5], np.float32)
    tw = zc.hide_alpha(rec, d, 2.5, 7)
    assert tw[:, 7].tolist() == [1.0, 1.0, 0.0, 0.0, 1.0, 0.0]        # d < z shows; d >= z and NaN hide
    assert np.array_equal(np.delete(tw, 7, axis=1), np.delete(rec, 7, axis=1))
