"""CPU: the host side of gs4d_transform_records (include/gs4d.h) — gs4d_host_transform_records against the header's text restated in
numpy float32, the per-record text the kernel and the host function share (csrc/transform_record.h) compiled stand-alone with g++ against the host
function, the float64 bounds, what a
transformed record means to a draw (the conditional mean and covariance), one picture with the CPU checker, gs4d_host_affine4 and the ABI."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import build_cases as bc
import scenes
import transform_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N = 400


def assert_same(got, want, what):
    ok = tc.same_bits(got, want)
    assert ok.all(), f"{what}: {int((~ok).sum())} words differ, first at {np.argwhere(~ok)[0].tolist()}"


def every_set(gs4d, n=N):
    return [(which, tc.records(gs4d, which, n)) for which in tc.SETS]


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.NAMES)
def test_the_host_function_is_the_headers_text(gs4d, name):
    xf = tc.transforms()[name]
    for which, rec in every_set(gs4d):
        got = gs4d.transform_records_host(rec, xf)
        assert got.shape == rec.shape and got.dtype == f32
        assert_same(got, tc.by_the_text(rec, xf), f"{name}, {which}")
        assert np.array_equal(tc.bits(got[:, 4:8]), tc.bits(rec[:, 4:8])), "rgba is copied"
    hostile = gs4d.transform_records_host(tc.records(gs4d, "hostile", N), xf)
    assert np.isnan(hostile).any() and np.isinf(hostile).any()                       # the block reaches the non-finite paths under every row


def test_several_rows_give_instance_after_instance(gs4d):
    rec = tc.records(gs4d, "4d_vel", 37)
    names = ("rigid", "zero", "retime")
    got = gs4d.transform_records_host(rec, tc.rows(names))
    assert got.shape == (3, 37, 24)
    for j, name in enumerate(names):
        assert_same(got[j], tc.by_the_text(rec, tc.transforms()[name]), name)
    assert gs4d.transform_records_host(rec[:0], tc.rows(names)).shape == (3, 0, 24)
    a = gs4d.Affine4.from_buffer_copy(tc.transforms()["rigid"].tobytes())
    assert_same(gs4d.transform_records_host(rec, a), got[0], "an Affine4 structure")


def test_the_identity_copies_finite_non_zero_records(gs4d):
    """x * 1 and x + 0 are exact, and so is x + y * 0 for finite y and x != 0 (a zero x could change its sign: such words are kept out)"""
    for form in bc.FORMS:
        rec = tc.records(gs4d, form, N).copy()
        rec[~np.isfinite(rec) | (rec == 0.0)] = f32(0.375)
        got = gs4d.transform_records_host(rec, tc.transforms()["identity"])
        assert np.array_equal(tc.bits(got), tc.bits(rec)), form


def test_the_zero_matrix_gives_the_offset_and_a_zero_covariance(gs4d):
    rec = tc.records(gs4d, "4d_2q", N)
    got = gs4d.transform_records_host(rec, tc.transforms()["zero"])
    assert np.array_equal(got[:, :4], np.tile(tc.transforms()["zero"][16:], (N, 1))) and (got[:, 8:] == 0.0).all()


# ---- the kernel's per-record text on the CPU ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("transform_record_check") / "transform_record_check"
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "transform_record_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return str(exe)


@pytest.mark.parametrize("which", tc.SETS)
def test_the_kernels_record_text_gives_the_host_functions_bits_on_the_cpu(gs4d, check_program, tmp_path, which):
    rows = tc.rows(tc.NAMES)
    for n in tc.SIZES:
        rec = tc.records(gs4d, which, n)
        src, xf, out = tmp_path / "records.bin", tmp_path / "xf.bin", tmp_path / "out.bin"
        rec.tofile(src)
        rows.tofile(xf)
        r = subprocess.run([check_program, str(n), str(rows.shape[0]), str(src), str(xf), str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.fromfile(out, f32).reshape(-1, 24)
        # the NaN rule of gs4d.h, as in tests/test_build_host.py: the library's host code and this program come from two compilers, and x86 gives a sum
        # of two NaNs the sign and payload of its first operand
        assert_same(got, tc.expected(gs4d, rec, rows), f"{which}, n = {n}")


# ---- against float64 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.FINITE)
@pytest.mark.parametrize("form", bc.FORMS)
def test_records_are_within_the_rounding_bounds_of_float64(gs4d, form, name):
    """two nested four-term dot products: (1 + u)^8 - 1 < 9 u on the sum of absolute products; the mean: a four-term dot product and a sum, < 6 u"""
    rec, xf = tc.records(gs4d, form, N), tc.transforms()[name]
    got = gs4d.transform_records_host(rec, xf)
    assert np.isfinite(got).all()
    L, o = tc.matrices(xf)
    p, S = tc.mean_cov(rec)
    p1, S1 = tc.mean_cov(got)
    err_S, bound_S = np.abs(S1 - L @ S @ L.T), 9.0 * tc.U * (np.abs(L) @ np.abs(S) @ np.abs(L).T)
    err_p, bound_p = np.abs(p1 - (p @ L.T + o)), 6.0 * tc.U * (np.abs(p) @ np.abs(L).T + np.abs(o))
    assert (err_S <= bound_S).all(), f"Sigma: worst error / bound = {np.nanmax(err_S / bound_S):.3f}"
    assert (err_p <= bound_p).all(), f"mean: worst error / bound = {np.nanmax(err_p / bound_p):.3f}"


# ---- what the transformed record means to a draw ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.TIME_BLOCK)
@pytest.mark.parametrize("form", bc.FORMS)
def test_the_conditional_gaussian_is_the_mapped_conditional_gaussian(gs4d, form, name):
    """With the time row (0, 0, 0, a) and x' = A x + v t + b: the transformed set conditioned on a t + c is A (the source conditioned on t) + v t + b,
    with covariance A C A^T.  Evaluated in float64 from the float32 records; the bound is the first-order effect of the rounding bounds of the test
    above on the conditional (tc.conditional_bound), doubled for the terms of higher order."""
    rec, xf = tc.records(gs4d, form, N), tc.transforms()[name]
    L, o = tc.matrices(xf)
    A, v, a, b, c = L[:3, :3], L[:3, 3], L[3, 3], o[:3], o[3]
    assert (L[3, :3] == 0.0).all() and a != 0.0
    p, S = tc.mean_cov(rec)
    p1, S1 = tc.mean_cov(gs4d.transform_records_host(rec, xf))
    dS, dp = 9.0 * tc.U * (np.abs(L) @ np.abs(S) @ np.abs(L).T), 6.0 * tc.U * (np.abs(p) @ np.abs(L).T + np.abs(o))
    for dt in (0.0, 0.3, -0.7):
        t = p[:, 3] + dt                                             # per record: a time near its own, where it shows
        mean, cov = tc.conditional(p, S, t)
        mean1, cov1 = tc.conditional(p1, S1, a * t + c)
        want_mean, want_cov = mean @ A.T + t[:, None] * v + b, A @ cov @ A.T
        bound_mean, bound_cov = tc.conditional_bound(p1, S1, a * t + c, dp, dS)
        assert (np.abs(mean1 - want_mean) <= 2.0 * bound_mean).all(), f"mean, dt = {dt}: worst error / bound = {np.max(np.abs(mean1 - want_mean) / bound_mean):.3f}"
        assert (np.abs(cov1 - want_cov) <= 2.0 * bound_cov).all(), f"covariance, dt = {dt}: worst error / bound = {np.max(np.abs(cov1 - want_cov) / bound_cov):.3f}"


def test_a_velocity_column_moves_the_conditional_mean_by_v_t(gs4d):
    """a static 3D set (mu_t = 0, no time column): under the velocity row its centre at time t is p + v t, and its shape does not change"""
    rec, xf = tc.records(gs4d, "3d", N), tc.transforms()["velocity"]
    v = np.asarray(tc.VELOCITY)
    p, S = tc.mean_cov(rec)
    p1, S1 = tc.mean_cov(gs4d.transform_records_host(rec, xf))
    assert np.array_equal(p1, p)                                      # mu_t = 0: v * 0 moves nothing
    for t in (0.0, 1.0, -2.5, 40.0):
        mean1, cov1 = tc.conditional(p1, S1, np.full(N, t))
        # Sigma' has v in its time column and Sigma44 = 1, exactly (products with 0 and 1): the mean is exact in float64 up to its own rounding
        assert np.allclose(mean1, p[:, :3] + v * t, rtol=1e-15, atol=0.0)
        bound = 9.0 * tc.U * (np.abs(S[:, :3, :3]) + np.abs(np.outer(v, v)))
        assert (np.abs(cov1 - S[:, :3, :3]) <= 2.0 * bound).all()


# ---- one picture --------------------------------------------------------------------------------------------------------------------------------
W, H = 64, 48
CAM, CAM_DIR = (0.0, 0.0, 150.0), (0.0, 0.0, -1.0)
# Measured with the CPU checker on this scene (the roundings of the transform, of the mapped view matrix and of the projection of other numbers), as
# L-infinity differences between the two pictures:
#     blended in record order, rigid map with time_scale 0.5 and offset 3.25      5.96e-07
#     blended in the order of the depth keys, the same map with time_scale 1      5.36e-07
# The bar is four times the measured value, because the roundings move with scene and camera.
# A FINDING, not a rounding: in the order of the depth keys the map with time_scale 0.5 gives 1.92e-01 (293 of 300 places of the blend order differ).
# Every splat is where it belongs — the picture in record order shows that — but the depth key (Scenes.h:28-36, oracle/gs4d_oracle.cpp gs4do_keygen) moves
# the centre by sig[3].xyz * (t - mu_t) WITHOUT the division by Sigma44 that the draw's conditioning has.  Under a time scale a, sig[3].xyz and t - mu_t both
# take a factor a: the key's displacement takes a^2 where the conditional centre's takes none, so a retimed set is blended in another order than its
# source unless a is 1 or -1.  The last test of this section pins that.  gs4d.h says so where it describes the call.
PICTURE_MEASURED = {"record order, retimed": 5.96e-07, "key order, time offset only": 5.36e-07}
PICTURE_MAPS = {"record order, retimed": (False, tc.RETIME[0], tc.RETIME[1]), "key order, time offset only": (True, 1.0, tc.RETIME[1])}


def picture_pair(gs4d, oracle, do_sort, a, c):
    """(checker image of the source under V at t, of the set under the rigid map with time scale a and offset c under V M^-1 at a t + c, the two orders)"""
    src = bc.host_records(gs4d, "4d_vel", bc.picture_set(gs4d, "4d_vel", 300))
    xf = tc.row(tc.block4(tc.rotation(tc.RIGID_AXIS, tc.RIGID_ANGLE), a=a), tc.RIGID_SHIFT + (c,))
    L, o = tc.matrices(xf)                                               # the map as the float32 row holds it
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = L[:3, :3], o[:3]
    view = gs4d.look_at(CAM, CAM_DIR)
    proj = gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    V = view.astype(np.float64).reshape(4, 4).T
    view1 = (V @ np.linalg.inv(M)).T.reshape(16).astype(f32)
    cam1 = (M @ np.array(CAM + (1.0,)))[:3].astype(f32)
    t = bc.T
    want, order, _ = oracle.render_4d(src, do_sort, t, 0.0, CAM, view, proj, W, H, nthreads=4)
    got, order1, _ = oracle.render_4d(gs4d.transform_records_host(src, xf), do_sort, a * t + c, 0.0, cam1, view1, proj, W, H, nthreads=4)
    assert int((np.abs(want - oracle.CLEAR).max(-1) > 1.0 / 255.0).sum()) > 100, "an empty frame"
    return want, got, order, order1


@pytest.mark.parametrize("what", sorted(PICTURE_MAPS))
def test_the_picture_of_a_placed_set_under_the_mapped_camera_is_the_picture_of_the_source(gs4d, oracle, what):
    want, got, order, order1 = picture_pair(gs4d, oracle, *PICTURE_MAPS[what])
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"picture, {what}: Linf = {err:.3e}")
    assert np.array_equal(order, order1)
    assert err <= 4.0 * PICTURE_MEASURED[what], f"Linf = {err:.3e} against a bar of {4.0 * PICTURE_MEASURED[what]:.3e}"


def test_a_time_scale_changes_the_order_of_the_depth_keys(gs4d, oracle):
    """the finding above: the reference's key is the conditional centre only where Sigma44 = 1, so time_scale 0.5 reorders the blend"""
    want, got, order, order1 = picture_pair(gs4d, oracle, True, *tc.RETIME)
    assert not np.array_equal(order, order1)
    assert sorted(order) == sorted(order1)


# ---- gs4d_host_affine4, the structure, the ABI -----------------------------------------------------------------------------------------------------
def test_affine4_is_its_expression(gs4d):
    rng = np.random.default_rng(0x5453)
    for q in (np.array([1.0, 0.0, 0.0, 0.0], f32), tc.quaternion((1.0, 2.0, -0.5), 0.7), (3.0 * rng.standard_normal(4)).astype(f32)):      # unit and not
        s, tr, v, a, c = f32(1.75), rng.uniform(-9, 9, 3).astype(f32), rng.uniform(-2, 2, 3).astype(f32), f32(0.5), f32(3.25)
        w, x, y, z = q
        two, one = f32(2.0), f32(1.0)
        R = np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],                     # [row, column]: rot_of of gs4d_host.cpp
                      [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                      [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], f32)
        want = np.zeros(20, f32)
        for col in range(3):
            want[4 * col:4 * col + 3] = s * R[:, col]
        want[12:15], want[15], want[16:19], want[19] = v, a, tr, c
        got = gs4d.affine4(q, s, tr, v, a, c)
        assert got.dtype == f32 and np.array_equal(tc.bits(got), tc.bits(want)), (q, got, want)
    assert np.array_equal(gs4d.affine4(), tc.transforms()["identity"])
    # the upper 3 x 3 is scale * the R of gs4d_host_splat3d_cov: with unit scales that function gives R R^T
    q = tc.quaternion((0.0, 0.0, 1.0), np.pi / 2.0)
    R = gs4d.affine4(q)[:16].reshape(4, 4).T[:3, :3]
    assert np.allclose(R, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-6)
    assert np.allclose(gs4d.splat3d_cov(q, (1.0, 2.0, 3.0)).reshape(3, 3).T, R.astype(np.float64) @ np.diag([1.0, 4.0, 9.0]) @ R.T, atol=1e-5)


def test_the_structure_is_80_bytes(gs4d):
    assert ctypes.sizeof(gs4d.Affine4) == 80
    assert [n for n, _ in gs4d.Affine4._fields_] == ["l", "o"] and gs4d.Affine4.o.offset == 64
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert "gs4d_transform_records(gs4d_ctx* ctx, gs4d_buf src, size_t n, gs4d_buf xf, size_t m, gs4d_buf dst, size_t dst_first)" in hdr
    assert "typedef struct gs4d_affine4" in hdr and "float l[16];" in hdr and "float o[4];" in hdr


def test_the_call_refuses_what_it_can_without_a_device(gs4d):
    """every other argument error needs a context, and a context needs a device: tests/test_gpu_transform.py"""
    lib = gs4d._lib
    assert lib.gs4d_transform_records(None, 1, 1, 2, 1, 3, 0) == -1                  # GS4D_E_INVALID: no context
    assert lib.gs4d_transform_records(None, 0, 0, 0, 0, 0, 0) == -1
    assert lib.gs4d_transform_records(None, 1, 1 << 32, 2, 1, 3, 0) == -1
    assert {"gs4d_transform_records", "gs4d_host_transform_records", "gs4d_host_affine4"} <= set(gs4d.EXPORTS)
