"""gs4d_shade_sh_t and gs4d_collapse_sh (include/gs4d.h) without a GPU: the weights over every float32 of their interval (the
stand-alone program tests/sh_time_check.cpp, which compiles csrc/sh_time_record.h with g++) and at the points the header names; the host
definitions against the numpy restatement of tests/shade_t_cases.py bit for bit and against the 4DGS formula in float64; the posed 4D table
through gs4d_host_rotate_sh; sh_rows_t against an element loop; and the ABI."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sh_rotate_cases as rc
import shade_cases as sc
import shade_t_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, u32 = np.float32, np.float64, np.uint32
CAM = sc.CAM


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


# ---- the stand-alone program -------------------------------------------------------------------------------------------------------------------
def build_check(tmp_path_factory, san):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("sh_time_check") / "sh_time_check"
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", *san, os.path.join(ROOT, "tests", "sh_time_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module", params=("plain", "asan_ubsan"))
def check_program(request, tmp_path_factory):
    """the stand-alone program, built plainly and as an executable instrumented with AddressSanitizer + UndefinedBehaviorSanitizer (nothing is preloaded)"""
    return build_check(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else [])


@pytest.fixture(scope="module")
def plain_program(tmp_path_factory):
    return build_check(tmp_path_factory, [])


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_the_cosine_over_every_float32_of_its_interval(plain_program):
    """every float32 x in [0, 0.25]: |c - cos(2 pi x)| <= 1.6e-7 (measured: 1.561e-7 at x = 0.247934252), c in [0, 1], c(0) = 1, c(0.25) = 0,
    and the bits of the T_j — the program's exit status says so"""
    r = subprocess.run([plain_program, "cosine"], capture_output=True, text=True, timeout=900)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    m = re.search(r"floats (\d+)\s+worst ([0-9.e+-]+)", r.stdout)
    assert m and int(m.group(1)) == 0x3E800000 + 1 and 1.0e-7 < float(m.group(2)) <= 1.6e-7


def test_the_calls_checks_on_the_cpu(check_program):
    r = subprocess.run([check_program, "args"], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([check_program, "rows", "4", "560", "3", "2", "0", "0", "0", "0", "0", "192", "a", "b", "c", "d"], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 3, "a stride the call refuses must end the program before it opens a file"


def hex32(v):
    return f"{int(np.array([v], f32).view(u32)[0]):08x}"


def test_the_kernels_text_gives_the_host_functions_bits_on_the_cpu(gs4d, check_program, tmp_path):
    paths = [str(tmp_path / f) for f in ("rec.bin", "sh.bin", "rows.bin", "out.bin")]
    n = 257
    rec = tc.hostile_mu_t(n)
    for k, (degree, degree_t) in enumerate(tc.PAIRS):
        stride, dst_stride = tc.strides_t(degree, degree_t)[k % 3], tc.dst_strides(degree)[(k + 1) % 3]
        tab = tc.table_t(n, degree, degree_t, stride, hostile=True)
        for name, t, ip in (("plain", sc.T, 0.25),) + tc.HOSTILE_TIMES[k % 3::3]:
            rec.tofile(paths[0])
            tab.tofile(paths[1])
            r = subprocess.run([check_program, "rows", str(n), str(stride), str(degree), str(degree_t), hex32(t), hex32(ip), *(hex32(v) for v in CAM), str(dst_stride),
                                *paths], capture_output=True, text=True, timeout=120, env=ENV)
            what = f"degree {degree}, degree_t {degree_t}, {name}"
            assert r.returncode == 0, what + "\n" + r.stderr[-3000:]
            want = gs4d.collapse_sh_host(rec, tab, degree, degree_t, t, ip, stride, dst_stride)
            got = np.fromfile(paths[2], f32).reshape(want.shape)
            assert tc.same_rows(got, want).all(), what             # (the library's host code and this program come from two compilers)
            assert np.array_equal(np.fromfile(paths[3], u32).reshape(n, 24), bits(gs4d.shade_sh_t_host(rec, tab, degree, degree_t, t, ip, CAM, stride))), what


# ---- the weights -------------------------------------------------------------------------------------------------------------------------------
def w_of(gs4d, v, degree_t=1):
    """(w_1, mask) at u = v: t = v, mu_t = 0, inv_period = 1 — the subtraction and the product are exact"""
    w, mask = gs4d.sh_time_weights(degree_t, v, 1.0, 0.0)
    return w[0], mask


def test_the_weights_at_the_points_the_header_names(gs4d):
    assert [int(b) for b in np.array(tc.T_SERIES, f32).view(u32)] == list(tc.T_BITS)
    one, minus = f32(1.0), f32(-1.0)
    for v in (0.0, -0.0, 1.0, -1.0, 2.0, 7.0, -300.0):
        assert w_of(gs4d, v) == (one, 1), v
    for v in (0.5, -0.5, 1.5, -2.5, 100.5):
        assert w_of(gs4d, v) == (minus, 1), v
    for v in (0.25, -0.25, 0.75, 3.25):
        assert bits(w_of(gs4d, v)[0]) in (0, 0x80000000) and w_of(gs4d, v)[1] == 1, v
    # |v| >= 2^23: every float is an integer, r = 0, w = 1
    for v in (2.0 ** 23, -(2.0 ** 23), 2.0 ** 23 + 1, 2.0 ** 24 + 2, 1e10, -1e30, 3.4e38):
        assert w_of(gs4d, v) == (one, 1), v
    # even, and within [-1, 1]
    rng = np.random.default_rng(0x5356)
    v = np.concatenate([rng.uniform(-2, 2, 2000), rng.uniform(-1000, 1000, 500), rng.standard_normal(500) * 1e6]).astype(f32)
    w = tc.cos_turns(v)
    assert np.array_equal(bits(w), bits(tc.cos_turns(-v))) and (np.abs(w) <= 1).all()
    for x in v[:300]:
        assert bits(w_of(gs4d, x)[0]) == bits(w_of(gs4d, -x)[0])
    # ... and it is the cosine: 1.561e-7 is the whole error against cos(2 pi v) of the float32 v
    assert float(np.abs(w.astype(f64) - np.cos(2 * np.pi * v.astype(f64))).max()) <= 1.6e-7
    # degree_t says how many blocks there are; block 2 runs at twice the rate
    assert gs4d.sh_time_weights(0, 0.3, 1.0, 0.0)[1] == 0 and not gs4d.sh_time_weights(0, 0.3, 1.0, 0.0)[0].any()
    w, mask = gs4d.sh_time_weights(2, 0.25, 1.0, 0.0)
    assert mask == 3 and bits(w[0]) in (0, 0x80000000) and w[1] == minus
    w, mask = gs4d.sh_time_weights(1, 0.25, 1.0, 0.0)
    assert mask == 1 and w[1] == 0


def test_who_takes_part(gs4d):
    nan, inf = float("nan"), float("inf")
    none = lambda *a: gs4d.sh_time_weights(2, *a)[1] == 0 and not gs4d.sh_time_weights(2, *a)[0].any()
    for t in (nan, inf, -inf):
        assert none(t, 0.25, 1.0), t                             # (t, inv_period, mu_t)
    for mu in (nan, inf, -inf):
        assert none(1.0, 0.25, mu), mu
    for ip in (nan, inf, -inf):
        assert none(1.0, ip, 0.5), ip
    assert none(inf, 0.0, 0.0)                                    # inf * 0
    # inv_period 0: u = 0, every weight 1; 1e30: u is huge but finite, every weight 1
    for ip in (0.0, 1e30):
        w, mask = gs4d.sh_time_weights(2, 1.0, ip, 0.5)
        assert mask == 3 and np.array_equal(w, np.ones(2, f32)), ip
    # u finite with 2 u overflowing: block 1 in (w = 1), block 2 out
    w, mask = gs4d.sh_time_weights(2, 1.5, 1.5e38, 0.0)
    assert np.isfinite(f32(1.5) * f32(1.5e38)) and mask == 1 and np.array_equal(w, np.array([1.0, 0.0], f32))
    # t - mu_t overflowing while each is finite
    assert none(3e38, 0.25, -3e38)
    # a query the binding cannot build: a degree_t outside 0 .. 2 gives no block
    q = gs4d.sh_time_query(3, 2, 1.0, 0.25)
    q.degree_t = 3
    w, mask = np.ones(2, f32), ctypes.c_int(7)
    gs4d._lib.gs4d_host_sh_time_weights(ctypes.byref(q), ctypes.c_float(0.0), w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(mask))
    assert mask.value == 0 and not w.any()


def test_the_restatement_of_the_weights_equals_the_host_function_bit_for_bit(gs4d):
    rng = np.random.default_rng(0x5357)
    u = np.concatenate([rng.uniform(-0.75, 0.75, 60000), rng.uniform(-4, 4, 20000), rng.uniform(-200, 200, 10000), rng.standard_normal(5000) * 1e5,
                        rng.standard_normal(5000) * 1e-4,
                        [0.0, -0.0, 0.25, -0.25, 0.5, -0.5, 0.125, 0.375, 1.0, 2.0 ** 23, -(2.0 ** 23), 2.0 ** 22 + 0.5, 1e30, 2.25e38, 3.4e38, np.inf, -np.inf, np.nan,
                         1e-40, 0.24999999, 0.25000003, 0.49999997, 0.50000006]]).astype(f32)
    assert u.size >= 100000
    w, part = tc.weights(2, 0.0, -1.0, u)                          # u = (0 - mu_t) * -1 = mu_t, exactly
    got_w, got_mask = np.empty((2, u.size), f32), np.empty(u.size, np.int64)
    for i, x in enumerate(u):
        ww, got_mask[i] = gs4d.sh_time_weights(2, 0.0, -1.0, x)
        got_w[:, i] = ww
    assert np.array_equal(bits(got_w), bits(w)), f"{int((bits(got_w) != bits(w)).any(0).sum())} weights differ"
    assert np.array_equal(got_mask, part[0] + 2 * part[1])
    assert (part[0] & ~part[1]).any() and (~part[0]).any() and part[1].mean() > 0.99
    # with a subtraction and a product that round: random (t, inv_period, mu_t)
    t, ip = f32(sc.T + 0.3), f32(1.0 / 50.0)
    mu = (sc.T + rng.uniform(-20, 20, 4000)).astype(f32)
    w, part = tc.weights(2, t, ip, mu)
    for i in range(mu.size):
        ww, mask = gs4d.sh_time_weights(2, t, ip, mu[i])
        assert np.array_equal(bits(ww), bits(w[:, i])) and mask == 3


# ---- collapse_sh_host ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,degree_t", tc.PAIRS)
def test_collapse_sh_host_equals_the_restatement(gs4d, degree, degree_t):
    n = 300
    rec = tc.hostile_mu_t(n, seed=0x5358 + degree)
    W = tc.row_words(degree)
    for stride in tc.strides_t(degree, degree_t):
        for dst_stride in tc.dst_strides(degree):
            tab = tc.table_t(n, degree, degree_t, stride, seed=0x5359 + stride, hostile=dst_stride != 1024)
            for name, t, ip in (("period 4", sc.T, 0.25), ("period 50", sc.T + 0.7, 1.0 / 50.0)) + tc.HOSTILE_TIMES:
                got = gs4d.collapse_sh_host(rec, tab, degree, degree_t, t, ip, stride, dst_stride)
                want = tc.collapse(rec, tab, degree, degree_t, t, ip, dst_stride)
                what = f"stride {stride} -> {dst_stride}, {name}"
                assert got.shape == want.shape == (n, dst_stride // 4)
                assert tc.same_rows(got, want).all(), what
                assert not bits(got[:, W:]).any(), what + ": the padding is not zero"
                if degree_t == 0:
                    assert np.array_equal(bits(got[:, :W]), bits(tab[:, :W])), what + ": degree_t 0 is the prefix"
    # the blocks matter, and so does the time
    tab = tc.table_t(n, degree, degree_t, tc.row_bytes_t(degree, degree_t))
    a, b = gs4d.collapse_sh_host(rec, tab, degree, degree_t, sc.T, 0.25), gs4d.collapse_sh_host(rec, tab, degree, degree_t, sc.T + 0.5, 0.25)
    assert (degree_t == 0) == np.array_equal(bits(a), bits(b))
    # a lower degree_t reads a prefix of the same row
    if degree_t:
        assert np.array_equal(bits(gs4d.collapse_sh_host(rec, tab, degree, degree_t - 1, sc.T, 0.25, tab.shape[1] * 4)),
                              bits(tc.collapse(rec, tab[:, :W * degree_t], degree, degree_t - 1, sc.T, 0.25)))


def test_calls_the_device_would_refuse_write_nothing(gs4d):
    n = 4
    rec, tab = sc.records(n), tc.table_t(n, 1, 1, 96)
    lib, p = gs4d._lib, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(n=n, stride=96, dst_stride=48, degree=1, degree_t=1, reserved=0)
    bad = [dict(degree=-1), dict(degree=4), dict(degree_t=-1), dict(degree_t=3), dict(reserved=1), dict(stride=80), dict(stride=100), dict(stride=0), dict(stride=1040),
           dict(dst_stride=32), dict(dst_stride=0), dict(dst_stride=56), dict(dst_stride=1040), dict(n=1 << 32)]
    for kw in bad:
        a = dict(good, **kw)
        q = gs4d.sh_time_query(a["degree"], a["degree_t"], sc.T, 0.25, CAM)
        q.reserved = a["reserved"]
        out, shaded = np.zeros((n, 256), f32), rec.copy()
        lib.gs4d_host_collapse_sh(a["n"], p(rec), p(tab), a["stride"], ctypes.byref(q), p(out), a["dst_stride"])
        assert not out.any(), kw
        if "dst_stride" not in kw:
            lib.gs4d_host_shade_sh_t(a["n"], p(shaded), p(tab), a["stride"], ctypes.byref(q))
            assert np.array_equal(bits(shaded), bits(rec)), kw
    out, shaded = np.zeros((n, 12), f32), rec.copy()
    lib.gs4d_host_collapse_sh(n, p(rec), p(tab), 96, None, p(out), 48)
    lib.gs4d_host_shade_sh_t(n, p(shaded), p(tab), 96, None)
    assert not out.any() and np.array_equal(bits(shaded), bits(rec))
    q = gs4d.sh_time_query(1, 1, sc.T, 0.25, CAM)
    lib.gs4d_host_collapse_sh(n, p(rec), p(tab), 96, ctypes.byref(q), p(out), 48)
    lib.gs4d_host_shade_sh_t(n, p(shaded), p(tab), 96, ctypes.byref(q))
    assert out.any() and not np.array_equal(bits(shaded), bits(rec))
    with pytest.raises(ValueError):
        gs4d.collapse_sh_host(rec, tab[:3], 1, 1, sc.T, 0.25)      # fewer rows than records


# ---- shade_sh_t_host -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,degree_t", tc.PAIRS)
def test_shade_sh_t_host_is_shade_sh_of_the_collapsed_rows(gs4d, degree, degree_t):
    cases = [("records", sc.records(sc.TILE + 37), sc.T, CAM)] + list(sc.hostile())
    for k, (name, rec, t, cam) in enumerate(cases):
        n = rec.shape[0]
        stride = tc.strides_t(degree, degree_t)[k % 3]
        tab = tc.table_t(n, degree, degree_t, stride, seed=0x535A + k, hostile=k % 2 == 1)
        for ip in (0.25, 1.0 / 50.0):
            got = gs4d.shade_sh_t_host(rec, tab, degree, degree_t, t, ip, cam, stride)
            rows = gs4d.collapse_sh_host(rec, tab, degree, degree_t, t, ip, stride)
            want = rec.copy()
            want[:, 4:7] = sc.shade(rec, rows, degree, t, cam)
            assert np.array_equal(bits(got), bits(want)), f"{name}, period {1 / ip:g}"
            assert np.array_equal(bits(got), bits(tc.shaded_records(rec, tab, degree, degree_t, t, ip, cam))), name      # (the restatement all the way)
            if degree_t == 0:
                assert np.array_equal(bits(got), bits(sc.shaded_records(rec, tab, degree, t, cam))), name + ": degree_t 0 is gs4d_shade_sh on the table itself"
    # no block taking part gives the bits of gs4d_shade_sh on the same table
    rec = sc.records(100)
    tab = tc.table_t(100, degree, degree_t, tc.row_bytes_t(degree, degree_t))
    assert np.array_equal(bits(gs4d.shade_sh_t_host(rec, tab, degree, degree_t, sc.T, np.nan, CAM)), bits(sc.shaded_records(rec, tab, degree, sc.T, CAM)))


def test_against_the_4dgs_formula_in_float64(gs4d):
    """0.5 + sum_n cos(2 pi n u) sum_k Y_k c_(n,k) in float64, normalised by 0.5 + sum_n |w_n| sum_k |b_k c_(n,k)|: 20 000 records, periods 4 and 50,
    blocks scaled 1, 1/2, 1/4, a positive DC shift so that nothing is clamped.  The bar is that of tests/test_shade_host.py, 4 x 2.9e-7.
    Measured (period 4 / period 50) for degree_t 0, 1, 2 — degree 0: 7.3e-8 / 7.3e-8, 1.6e-7 / 1.5e-7, 1.7e-7 / 1.8e-7; degree 1: 1.8e-7 / 1.8e-7,
    2.0e-7 / 2.1e-7, 2.2e-7 / 2.1e-7; degree 2: 2.8e-7 / 2.8e-7, 2.5e-7 / 2.4e-7, 2.8e-7 / 2.7e-7; degree 3: 3.5e-7 / 3.5e-7, 3.5e-7 / 3.0e-7,
    3.5e-7 / 3.1e-7 (degree_t 0 is gs4d_shade_sh itself over these 20 000 records)."""
    n = 20000
    rec = sc.records(n)
    worst = 0.0
    for degree, degree_t in tc.PAIRS:
        c = tc.coefficients_t(n, degree, degree_t)
        c[:, 0:3] = np.abs(c[:, 0:3]) + f32(4.0)
        for period in tc.PERIODS:
            ip = f32(1.0 / period)
            got = gs4d.shade_sh_t_host(rec, sc.table(c, tc.row_bytes_t(degree, degree_t)), degree, degree_t, sc.T, ip, CAM)[:, 4:7].astype(f64)
            val, scale = tc.shade64_t(rec, c, degree, degree_t, sc.T, ip, CAM)
            assert (val > 0).all()
            err = float((np.abs(got - val) / scale).max())
            print(f"degree {degree}, degree_t {degree_t}, period {period:g}: largest error relative to 0.5 + sum |w_n| sum |b_k c_nk| = {err:.3e}")
            worst = max(worst, err)
            assert err <= 4 * 2.9e-7, (degree, degree_t, period)
    # a flipped sign of one time block misses the bar by more than 10^4 x
    for degree, degree_t, block in ((1, 1, 1), (3, 2, 1), (3, 2, 2), (0, 2, 2)):
        c = tc.coefficients_t(n, degree, degree_t)
        c[:, 0:3] = np.abs(c[:, 0:3]) + f32(4.0)
        W = tc.row_words(degree)
        flipped = c.copy()
        flipped[:, block * W:(block + 1) * W] *= f32(-1.0)
        got = gs4d.shade_sh_t_host(rec, sc.table(flipped, tc.row_bytes_t(degree, degree_t)), degree, degree_t, sc.T, 0.25, CAM)[:, 4:7].astype(f64)
        val, scale = tc.shade64_t(rec, c, degree, degree_t, sc.T, 0.25, CAM)
        miss = float((np.abs(got - val) / scale).max())
        assert miss > 1e4 * 4 * 2.9e-7, (degree, degree_t, block, miss)


# ---- a posed 4D table through gs4d_rotate_sh --------------------------------------------------------------------------------------------------------
def test_a_posed_4d_table_through_rotate_sh_by_the_host_definitions(gs4d):
    """degree 3, degree_t 2, rows of 576 bytes taken as 3 n rows of 192: every block turns with the same band matrices.  Measured: 7.7e-8 of
    sum |c| over all blocks (the bar is sh_rotate_cases.PICTURE_BAR, 6.7e-7); the unrotated table misses by more than 1000 x the bar."""
    rec, tab = tc.posed_set()
    assert tab.shape == (rc.PICTURE_N, 144)
    l = rc.picture_maps(gs4d)["rigid"]
    a, b, stale = tc.posed_routes_host(gs4d, rec, tab, l, rc.PICTURE_CAM, rc.PICTURE_T)
    ratio, off = tc.colour_ratio_t(a, b, tab), tc.colour_ratio_t(a, stale, tab)
    print(f"posed 4D table: the two routes differ by {ratio:.3g} sum |c| (the unrotated table: {off:.3g})")
    assert ratio <= rc.PICTURE_BAR
    assert off > 1000 * rc.PICTURE_BAR
    # the time blocks are in the picture: without them the colours are others
    assert tc.colour_ratio_t(a, gs4d.shade_sh_t_host(rec, tab, 3, 0, rc.PICTURE_T, tc.POSED_INV_PERIOD, rc.inverse_camera(l, rc.PICTURE_CAM), 576)[:, 4:7], tab) > 1000 * rc.PICTURE_BAR
    # GS4D_POSE_INDEX with every bind word repeated degree_t + 1 times turns the same rows
    n = rec.shape[0]
    each = gs4d.rotate_sh_host(tab.reshape(3 * n, 48), l.reshape(1, 20), 3)
    index = gs4d.rotate_sh_host(tab.reshape(3 * n, 48), l.reshape(1, 20), 3, np.repeat(np.zeros(n, u32), 3))
    assert np.array_equal(bits(each), bits(index))


# ---- a frozen frame ---------------------------------------------------------------------------------------------------------------------------------
def test_a_frozen_frame_keeps_its_view_dependence_by_the_host_definitions(gs4d):
    """slice_records at t, collapse_sh at t, shade_sh of the slice at t == mu_t_out: the colours shade_sh_t gives the source, bit for bit, for records
    whose time column (the slice's) and time row (the shade's) hold the same bits"""
    n, t = 700, sc.T + 0.25
    rec = sc.records(n, seed=0x5366)
    rec[:, [11, 15, 19]] = rec[:, 20:23]
    for degree, degree_t in ((3, 2), (1, 1)):
        tab = tc.table_t(n, degree, degree_t, tc.row_bytes_t(degree, degree_t))
        sliced = gs4d.slice_records_host(rec, t)
        rows = gs4d.collapse_sh_host(rec, tab, degree, degree_t, t, 0.25)
        for cam in (CAM, (-40.0, 22.0, -95.0)):
            assert np.array_equal(bits(sc.shade(sliced, rows, degree, t, cam)), bits(gs4d.shade_sh_t_host(rec, tab, degree, degree_t, t, 0.25, cam)[:, 4:7]))


# ---- the layout helpers and the ABI -----------------------------------------------------------------------------------------------------------------
def test_sh_rows_t_against_an_element_loop(gs4d):
    rng = np.random.default_rng(11)
    n = 23
    for src_degree in (1, 3):
        KS = (src_degree + 1) ** 2
        for B in (1, 3):
            feat = rng.standard_normal((n, KS * B, 3)).astype(f32)
            for degree in range(src_degree + 1):
                for degree_t in range(B):
                    for stride in (None, 1024):
                        rows = gs4d.sh_rows_t(feat, degree, degree_t, src_degree, stride)
                        nbytes = gs4d.sh_row_bytes_t(degree, degree_t) if stride is None else stride
                        assert rows.dtype == np.uint8 and rows.shape == (n, nbytes) and gs4d.sh_row_bytes_t(degree, degree_t) == tc.row_bytes_t(degree, degree_t)
                        K = (degree + 1) ** 2
                        want = np.zeros((n, nbytes // 4), f32)
                        for i in range(n):
                            for b in range(degree_t + 1):
                                for k in range(K):
                                    for ch in range(3):
                                        want[i, 3 * (b * K + k) + ch] = feat[i, b * KS + k, ch]
                        assert np.array_equal(rows.view(u32), want.view(u32)), (src_degree, B, degree, degree_t, stride)
    # at degree 3 the 4DGS tensor [N, 16 (degree_t + 1), 3] is the row as it stands
    feat = rng.standard_normal((n, 48, 3)).astype(f32)
    assert np.array_equal(gs4d.sh_rows_t(feat, 3, 2).view(f32), feat.reshape(n, 144))
    assert [gs4d.sh_row_bytes_t(3, dt) for dt in range(3)] == [192, 384, 576] and gs4d.sh_row_bytes_t(2, 2) == 336 and gs4d.sh_row_bytes_t(0, 2) == 48
    for bad in (dict(degree=4, degree_t=0), dict(degree=3, degree_t=3), dict(degree=3, degree_t=2, stride=560), dict(degree=3, degree_t=2, stride=2048),
                dict(degree=3, degree_t=2, src_degree=2)):
        with pytest.raises(ValueError):
            gs4d.sh_rows_t(feat, **bad)
    with pytest.raises(ValueError):
        gs4d.sh_rows_t(feat[:, :32], 3, 2)                         # two blocks cannot give degree_t 2


def test_the_structure_and_the_abi(gs4d, tmp_path):
    S = gs4d.ShTime
    assert ctypes.sizeof(S) == 32
    assert [(getattr(S, f).offset, getattr(S, f).size) for f in ("degree", "degree_t", "t", "inv_period", "cam_pos", "reserved")] == \
        [(0, 4), (4, 4), (8, 4), (12, 4), (16, 12), (28, 4)]
    q = gs4d.sh_time_query(3, 2, 1.5, 0.25, (1.0, 2.0, 3.0))
    assert (q.degree, q.degree_t, q.t, q.inv_period, tuple(q.cam_pos), q.reserved) == (3, 2, 1.5, 0.25, (1.0, 2.0, 3.0), 0)
    names = {"gs4d_shade_sh_t": 6, "gs4d_collapse_sh": 8, "gs4d_host_sh_time_weights": 4, "gs4d_host_collapse_sh": 7, "gs4d_host_shade_sh_t": 5}
    lib = ctypes.CDLL(gs4d.LIB_PATH)
    for name, nargs in names.items():
        assert hasattr(lib, name) and name in gs4d.EXPORTS and len(getattr(gs4d._lib, name).argtypes) == nargs, name
    for name in ("shade_sh_t", "collapse_sh"):
        assert callable(getattr(gs4d.Context, name))
    for name in ("sh_time_query", "sh_row_bytes_t", "sh_rows_t", "shade_sh_t_host", "collapse_sh_host", "sh_time_weights"):
        assert callable(getattr(gs4d, name))
    assert "collapse_sh" in gs4d.Context.freeze.__doc__ and "kept_index" in gs4d.Context.freeze.__doc__
    q = gs4d.sh_time_query(3, 2, 0.0, 0.25)
    assert gs4d._lib.gs4d_shade_sh_t(None, 1, 1, 2, 576, ctypes.byref(q)) == -1 and gs4d._lib.gs4d_collapse_sh(None, 1, 1, 2, 576, ctypes.byref(q), 3, 192) == -1
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    for text in ("-19.739208802178716", "7.903536371318465", "c19de9e6 4281e0f8 c2aae9e4 4270fa83 c1d368f9 40fce9c5", "the pitch of the blocks is K", "REST mean"):
        assert text in hdr, text
    internal = open(os.path.join(ROOT, "4dgaussiansplatrendering_amd", "csrc", "gs4d_internal.h")).read()
    assert f"constexpr uint32_t SHADE_T_TILE = {tc.TILE};" in internal, "tests/shade_t_cases.py TILE must follow SHADE_T_TILE"
    assert {tc.TILE - 1, tc.TILE, tc.TILE + 1, 3 * tc.TILE + 1, 1, 63, 64, 65, 769} <= set(tc.SIZES)
    # the structure as C sees it
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    compiler = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert compiler, "no C compiler: neither gcc, cc, clang nor the ROCm clang the library is built with"
    src = tmp_path / "sh_time_abi.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdint.h>
#include "gs4d.h"
typedef char size_is_32[sizeof(gs4d_sh_time) == 32 ? 1 : -1];
typedef char offsets[offsetof(gs4d_sh_time, degree_t) == 4 && offsetof(gs4d_sh_time, t) == 8 && offsetof(gs4d_sh_time, inv_period) == 12 &&
                     offsetof(gs4d_sh_time, cam_pos) == 16 && offsetof(gs4d_sh_time, reserved) == 28 ? 1 : -1];
int main(void) {
    int (*shade)(gs4d_ctx*, gs4d_buf, size_t, gs4d_buf, size_t, const gs4d_sh_time*) = gs4d_shade_sh_t;
    int (*collapse)(gs4d_ctx*, gs4d_buf, size_t, gs4d_buf, size_t, const gs4d_sh_time*, gs4d_buf, size_t) = gs4d_collapse_sh;
    gs4d_sh_time q = { 3, 2, 0.5f, 1.0f, { 0.0f, 0.0f, 0.0f }, 0 };
    float w[2];
    int mask = 0;
    gs4d_host_sh_time_weights(&q, 0.0f, w, &mask);
    if (mask != 3 || w[0] != -1.0f || w[1] != 1.0f) return 3;
    /* a NULL context is refused, not dereferenced */
    if (shade(NULL, 1, 1, 2, 576, &q) != GS4D_E_INVALID || collapse(NULL, 1, 1, 2, 576, &q, 3, 192) != GS4D_E_INVALID) return 2;
    return 0;
}
''')
    exe = tmp_path / "sh_time_abi"
    libdir = os.path.dirname(gs4d.LIB_PATH)
    cc_ = subprocess.run([compiler, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                          "-L", libdir, "-lgs4d", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-500:])
