"""CPU: the host side of gs4d_slice_records (include/gs4d.h) — gs4d_host_slice_records against the header's text restated in numpy
float32 (word 7 with libm's expf through ctypes), the fixed point on the CPU checker (a 4D set projected at t and its slice projected at mu_t_out give
the same projected records), the two depth keys of a set and of its slice, the structure and the ABI."""
import ctypes
import os

import numpy as np
import pytest

import slice_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N = 400
W, H = 64, 48
CAM, CAM_DIR = (0.0, 0.0, 150.0), (0.0, 0.0, -1.0)
FOV, ZNEAR, ZFAR = 60.0, 0.1, 5000.0


def assert_same(got, want, what):
    ok = sc.same_bits(got, want)
    assert ok.all(), f"{what}: {int((~ok).sum())} words differ, first at {np.argwhere(~ok)[0].tolist()}"


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sc.SETS)
def test_the_host_function_is_the_headers_text(gs4d, which):
    rec = sc.records(gs4d, which, N)
    dead = 0
    for q in sc.queries():
        got = gs4d.slice_records_host(rec, *q)
        assert got.shape == rec.shape and got.dtype == f32
        want = sc.by_the_text(rec, *q)
        assert_same(got, want, f"{which}, {q}")
        # word 7 with libm's expf is bit-equal also where it is a NaN-free word; the fixed words are exact
        assert np.array_equal(sc.bits(got[:, 4:7]), sc.bits(rec[:, 4:7])), "rgb is copied"
        assert (sc.bits(got[:, sc.COLUMN + sc.ROW]) == 0x80000000).all(), "the time row and column are -0"
        assert (sc.bits(got[:, 3]) == sc.bits(f32(q[2]))).all() and (sc.bits(got[:, 23]) == sc.bits(f32(q[3]))).all()
        dead += int((got[:, 7] == 0.0).sum())
    if which != "hostile":
        assert dead > 0, "no query gave an alpha of exactly 0"


def test_the_default_mu_t_out_is_t_and_nothing_is_a_no_op(gs4d):
    rec = sc.records(gs4d, "4d_vel", 37)
    assert_same(gs4d.slice_records_host(rec, 25.0), gs4d.slice_records_host(rec, 25.0, 0.0, 25.0, 1.0), "defaults")
    assert gs4d.slice_records_host(rec[:0], 1.0).shape == (0, 24)
    q = gs4d.slice_query(3.0, 0.25, None, 0.5)
    assert (q.t, q.min_opacity, q.mu_t_out, q.s44_out) == (3.0, 0.25, 3.0, 0.5)


def test_the_neg_zero_set_reaches_the_signed_zero_cases(gs4d):
    rec = sc.records(gs4d, "neg_zero", N)
    got = gs4d.slice_records_host(rec, 25.0)
    assert (sc.bits(got[:, :3]) == 0x80000000).any(), "no centre coordinate of the slice is -0"
    assert (sc.bits(got[:, [9, 12, 18]]) == 0x80000000).any(), "no covariance element of the slice is -0"
    assert set(np.unique(rec[:, 23]).tolist()) == {0.25, 1.0, 3.0}
    sym = sc.symmetric(rec)
    assert sym.any() and (~sym).any()


# ---- the fixed point on the CPU checker -----------------------------------------------------------------------------------------------------------
def cam_mats(gs4d):
    return gs4d.look_at(CAM, CAM_DIR), gs4d.perspective(FOV, W, H, ZNEAR, ZFAR)


def projected_words(p):
    return np.ascontiguousarray(p).view(np.uint32).reshape(p.shape[0], -1)


@pytest.mark.parametrize("which", sc.SETS)
def test_a_slice_projects_to_the_bits_of_its_source(gs4d, oracle, which):
    """oracle.preprocess of the source at t and of the slice at mu_t_out: bit-equal projected records, NaN words by NaN-ness.  If a word differs,
    the definition is wrong, not the test."""
    view, proj = cam_mats(gs4d)
    rec = sc.records(gs4d, which, N)
    if which != "hostile":                                       # in front of the camera: the conditioned covariance reaches the conic
        rec = rec.copy()
        rec[:, :3] *= f32(0.2)
    for q in sc.queries():
        t, m, mu_t_out, _ = q
        want = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H, t, m)
        got = oracle.preprocess(oracle.MODE_4D, gs4d.slice_records_host(rec, *q), view, proj, W, H, mu_t_out, m)
        g, w = projected_words(got), projected_words(want)
        ok = (g == w) | (np.isnan(g.view(f32)) & np.isnan(w.view(f32)))
        assert ok.all(), f"{which}, {q}: {int((~ok).any(1).sum())} records differ, first word at {np.argwhere(~ok)[0].tolist()}"
        if which != "hostile" and t == 25.0:
            assert int(want["valid"].sum()) > N // 4, "hardly a record is projected: the test shows nothing"


def test_positive_zeros_would_not_be_a_fixed_point(gs4d, oracle):
    """the reason for the -0 words: the same slice with +0 in the time row and column turns a -0 centre coordinate into +0"""
    rec = sc.records(gs4d, "neg_zero", N)
    s = gs4d.slice_records_host(rec, 25.0)
    assert (sc.bits(s[:, :3]) == 0x80000000).any()
    plus = s.copy()
    plus[:, sc.COLUMN + sc.ROW] = 0.0
    again, again_plus = gs4d.slice_records_host(s, 25.0), gs4d.slice_records_host(plus, 25.0)
    assert np.array_equal(sc.bits(again[:, :3]), sc.bits(s[:, :3])) and np.array_equal(sc.bits(again[:, 8:19]), sc.bits(s[:, 8:19]))
    assert not np.array_equal(sc.bits(again_plus[:, :3]), sc.bits(s[:, :3]))


# ---- the keys -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sc.SETS)
def test_the_keys_of_a_slice(gs4d, oracle, which):
    """VIEW_Z: equal for records with a bit-symmetric time row / column; REF_INV_EUCLID: equal where, besides, Sigma44 == 1"""
    view, _ = cam_mats(gs4d)
    rec = sc.records(gs4d, which, N)
    sym = sc.symmetric(rec)
    one = sym & (rec[:, 23] == 1.0)
    if which in ("3d", "4d_vel"):
        assert sym.all(), "the host builders mirror the time column"
    if which == "3d":
        assert one.all()
    for q in sc.queries():
        t, _, mu_t_out, _ = q
        s = gs4d.slice_records_host(rec, *q)
        _, kz = oracle.keygen_viewz(rec, t, view)
        _, kz1 = oracle.keygen_viewz(s, mu_t_out, view)
        assert sc.same_bits(kz1, kz)[sym].all(), f"{which}, {q}: view-z keys of symmetric records differ"
        _, kr = oracle.keygen(rec, t, CAM)
        _, kr1 = oracle.keygen(s, mu_t_out, CAM)
        assert sc.same_bits(kr1, kr)[one].all(), f"{which}, {q}: reference keys of records with Sigma44 == 1 differ"


def test_the_reference_key_of_a_source_is_not_that_of_its_drawn_centre(gs4d, oracle):
    """Sigma44 = 0.25, velocity (2, 0, 0), mu_t = 0, drawn at t = 1: the draw puts the centre at x = 0 + (1 / 0.25) * 1 * 2 = 8, the reference's key
    of the source takes x = 0 + 2 * 1 = 2.  The slice's key is that of the drawn centre."""
    rec = np.zeros((1, 24), f32)
    rec[0, 4:8] = 1.0
    rec[0, [8, 13, 18]] = 1.0
    rec[0, 11], rec[0, 20], rec[0, 23] = 2.0, 2.0, 0.25
    s = gs4d.slice_records_host(rec, 1.0)
    assert s[0, 0] == 8.0
    cam = (0.0, 0.0, 10.0)
    _, k_src = oracle.keygen(rec, 1.0, cam)
    _, k_slice = oracle.keygen(s, 1.0, cam)
    assert k_src[0] == f32(1.0) / np.sqrt(f32(2.0 * 2.0 + 10.0 * 10.0), dtype=f32)
    assert k_slice[0] == f32(1.0) / np.sqrt(f32(8.0 * 8.0 + 10.0 * 10.0), dtype=f32)
    assert k_src[0] != k_slice[0]
    view = gs4d.look_at(cam, (0.0, 0.0, -1.0))
    assert sc.same_bits(oracle.keygen_viewz(rec, 1.0, view)[1], oracle.keygen_viewz(s, 1.0, view)[1]).all()      # the view-z key divides, as the draw does


# ---- the structure, the ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_structure_is_16_bytes(gs4d):
    assert ctypes.sizeof(gs4d.Slice) == 16
    assert [n for n, _ in gs4d.Slice._fields_] == ["t", "min_opacity", "mu_t_out", "s44_out"]
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert "gs4d_slice_records(gs4d_ctx* ctx, gs4d_buf src, size_t n, const gs4d_slice* q, gs4d_buf dst, size_t dst_first)" in hdr
    assert "gs4d_host_slice_records(size_t n, const float* records24, const gs4d_slice* q, float* out24)" in hdr
    assert "typedef struct gs4d_slice" in hdr


def test_refused_queries_change_nothing(gs4d):
    """without a context every call is refused, whatever the query; the query and the records it names are read at most (every other argument error
    needs a context, and a context needs a device: tests/test_gpu_slice.py)"""
    lib = gs4d._lib
    assert {"gs4d_slice_records", "gs4d_host_slice_records"} <= set(gs4d.EXPORTS)
    for t, m, mu, s in ((1.0, 0.0, 1.0, 1.0), (np.nan, 0.0, 1.0, 1.0), (1.0, np.nan, 1.0, 1.0), (1.0, 0.0, np.inf, 1.0), (1.0, 0.0, 1.0, 0.0), (1.0, 0.0, 1.0, -1.0)):
        q = gs4d.Slice(t, m, mu, s)
        before = bytes(q)
        assert lib.gs4d_slice_records(None, 1, 1, ctypes.byref(q), 2, 0) == -1
        assert bytes(q) == before
    assert lib.gs4d_slice_records(None, 1, 1, None, 2, 0) == -1
    assert lib.gs4d_slice_records(None, 0, 0, None, 0, 0) == -1
    assert lib.gs4d_slice_records(None, 1, 1 << 32, None, 2, 0) == -1
    # the host function takes a query the device call refuses as data, and leaves its input alone
    rec = sc.records(gs4d, "4d_vel", 9)
    keep = rec.copy()
    out = gs4d.slice_records_host(rec, np.nan, np.nan, np.inf, -1.0)
    assert np.array_equal(sc.bits(rec), sc.bits(keep))
    assert_same(out, sc.by_the_text(rec, np.nan, np.nan, np.inf, -1.0), "a refused query on the host")
