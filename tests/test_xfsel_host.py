"""CPU: the host side of gs4d_transform_selected (include/gs4d.h) — gs4d_host_transform_selected against the header's text restated in
numpy float32 (tests/xfsel_cases.py), the per-record text and the measurement centre that the kernel and the host functions share
(csrc/transform_record.h) compiled stand-alone with g++ against the host functions, what stays untouched, what a rotation about the measured pivot means to a draw, the structure and the ABI."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import build_cases as bc
import transform_cases as tc
import xfsel_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def host_call(gs4d, rec, xf, n, table, pivot, measure):
    return gs4d.transform_selected_host(rec, xf, pivot=pivot, measure=measure, n=n, **xc.keywords(table))


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", xc.SETS)
@pytest.mark.parametrize("name", tc.NAMES)
def test_the_host_function_is_the_headers_text(gs4d, name, which):
    """every size and table; the pivot forms taken round and round, so that every form meets every kind of table at some size"""
    xf, k, forms = tc.transforms()[name], 0, set()
    for n in xc.SIZES:
        rec = tc.records(gs4d, which, n + xc.EXTRA)
        for tname, table in xc.tables(n).items():
            form = xc.PIVOT_FORMS[k % len(xc.PIVOT_FORMS)]
            k += 1
            forms.add(form)
            pivot, measure = xc.pivot_case(gs4d, form, rec, n, table, k)
            got = host_call(gs4d, rec, xf, n, table, pivot, measure)
            assert got.shape == rec.shape and got.dtype == f32
            want = xc.expected(gs4d, rec, xf, n, table, pivot, measure)
            xc.assert_records(got, want, rec, xc.selected(n, table), n, f"{name}, {which}, n = {n}, {tname}, pivot {form}")
    assert forms == set(xc.PIVOT_FORMS)


@pytest.mark.parametrize("form", xc.PIVOT_FORMS)
def test_every_pivot_form_on_every_table(gs4d, form):
    """the three-tiles-plus-one size under the rigid row: every table with every pivot form, every hostile measurement"""
    n, xf = xc.SIZES[-1], tc.transforms()["rigid"]
    rec = tc.records(gs4d, "4d_vel", n + xc.EXTRA)
    for k, (tname, table) in enumerate(xc.tables(n).items()):
        for j in range(len(xc.hostile_measures(gs4d)) if form == "hostile" else 1):
            pivot, measure = xc.pivot_case(gs4d, form, rec, n, table, k + j)
            got = host_call(gs4d, rec, xf, n, table, pivot, measure)
            xc.assert_records(got, xc.expected(gs4d, rec, xf, n, table, pivot, measure), rec, xc.selected(n, table), n, f"{tname}, pivot {form} {j}")


def test_without_pivot_and_table_it_is_transform_records(gs4d):
    for which in xc.SETS:
        rec = tc.records(gs4d, which, 300)
        for name in tc.NAMES:
            got, want = gs4d.transform_selected_host(rec, tc.transforms()[name]), gs4d.transform_records_host(rec, tc.transforms()[name])
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{which}, {name}"         # byte-equal: the same code on the same machine


def test_a_zero_pivot_still_costs_its_two_operations(gs4d):
    """signed zeros through the identity: the header's lines decide what a -0 coordinate becomes — with a pivot flag the subtraction and the addition
    are performed also for c = 0 and c = -0 — and the restatement and the host function agree on them"""
    rec = tc.records(gs4d, "3d", 8).copy()
    rec[:, :3] = f32(-0.0)
    ident = tc.transforms()["identity"]
    for pivot in (None, (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0)):
        got = gs4d.transform_selected_host(rec, ident, pivot=pivot)
        want = xc.by_the_text(rec, ident, np.ones(8, bool), pivot)
        assert np.array_equal(xc.bits(got), xc.bits(want)), pivot
    assert np.array_equal(xc.bits(gs4d.transform_selected_host(rec, ident, pivot=(0.0, 0.0, 0.0))[:, :3]), np.zeros((8, 3), np.uint32))


def test_unselected_records_and_records_behind_n_are_byte_equal(gs4d):
    n = 257
    rec = tc.records(gs4d, "hostile", n + xc.EXTRA)                                   # NaN payloads and signed zeros must survive a record that is skipped
    for tname, table in xc.tables(n).items():
        got = gs4d.transform_selected_host(rec, tc.transforms()["full"], pivot=xc.PIVOT, n=n, **xc.keywords(table))
        keep = np.ones(n + xc.EXTRA, bool)
        keep[:n] = ~xc.selected(n, table)
        assert np.array_equal(got[keep].view(np.uint8), rec[keep].view(np.uint8)), tname
        moved = (xc.bits(got[~keep]) != xc.bits(rec[~keep])).any(1)
        assert moved.all(), f"{tname}: a selected record kept its bits under a full map"


def test_calls_the_device_would_refuse_change_nothing(gs4d):
    rec = tc.records(gs4d, "4d_vel", 9)
    x = gs4d.selection_xf(tc.transforms()["rigid"], pivot=xc.PIVOT)
    for flags in (3, 4, 0x80000000):
        x.flags = flags
        assert np.array_equal(gs4d.transform_selected_host(rec, x).view(np.uint8), rec.view(np.uint8)), flags
    out = rec.copy()
    x.flags = gs4d.XS_PIVOT_MEASURE
    gs4d._lib.gs4d_host_transform_selected(9, out.ctypes.data_as(ctypes.c_void_p), None, None, ctypes.byref(x), None)      # no measure
    gs4d._lib.gs4d_host_transform_selected(9, out.ctypes.data_as(ctypes.c_void_p), None, None, None, None)                 # no xf
    assert np.array_equal(out.view(np.uint8), rec.view(np.uint8))
    with pytest.raises(TypeError):
        gs4d.selection_xf(tc.transforms()["rigid"], pivot=xc.PIVOT, measure=True)
    with pytest.raises(TypeError):
        gs4d.transform_selected_host(rec, tc.transforms()["rigid"], pivot=xc.PIVOT, measure=gs4d.Measure())


# ---- the measurement centre ---------------------------------------------------------------------------------------------------------------------
def measures(gs4d):
    out = xc.hostile_measures(gs4d) + [xc.count0_measure(gs4d)]
    for which in xc.SETS:
        rec = tc.records(gs4d, which, 300)
        for table in xc.tables(300).values():
            out.append(gs4d.measure_records_host(rec, t=0.25, **xc.keywords(table)))
    return out


def test_the_restated_centre_is_gs4d_host_measure_centre(gs4d):
    some = 0
    for m in measures(gs4d):
        c = m.as_dict()["centre"]
        want = np.zeros(3, f32) if c is None else c
        assert xc.same_bits(xc.centre_by_the_text(m), want).all(), (m.count, m.lo[:], m.hi[:], m.cell_sum[:])
        some += c is not None and bool(np.isfinite(c).all())
    assert some > 20


# ---- the kernel's text on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=("plain", "asan_ubsan"))
def check_program(request, tmp_path_factory):
    """the stand-alone program, built plainly and as an executable instrumented with AddressSanitizer + UndefinedBehaviorSanitizer (nothing is preloaded)"""
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("transform_selected_check") / "transform_selected_check"
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *san, os.path.join(ROOT, "tests", "transform_selected_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return str(exe)


def test_the_kernels_text_gives_the_host_functions_bits_on_the_cpu(gs4d, check_program, tmp_path):
    """every transform row under each pivot flag, on every set and a table per size; the centre of every measurement"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ms = measures(gs4d)
    k = 0
    for which in xc.SETS:
        for n in xc.SIZES:
            rec = tc.records(gs4d, which, n)
            tables = list(xc.tables(n).items())
            tname, table = tables[k % len(tables)]
            measure = ms[k % len(ms)]
            k += 1
            sel = xc.selected(n, table)
            rows = []
            for name in tc.NAMES:
                rows += [gs4d.selection_xf(tc.transforms()[name]), gs4d.selection_xf(tc.transforms()[name], pivot=xc.PIVOT),
                         gs4d.selection_xf(tc.transforms()[name], measure=True)]
            paths = [tmp_path / f for f in ("records.bin", "sel.bin", "xf.bin", "measure.bin", "out.bin")]
            rec.tofile(paths[0])
            sel.astype(np.uint8).tofile(paths[1])
            paths[2].write_bytes(b"".join(bytes(x) for x in rows))
            paths[3].write_bytes(bytes(measure))
            r = subprocess.run([check_program, str(n), str(len(rows)), *map(str, paths)], capture_output=True, text=True, timeout=120, env=env)
            assert r.returncode == 0, r.stderr[-3000:]
            out = np.fromfile(paths[4], f32)
            c = measure.as_dict()["centre"]
            assert xc.same_bits(out[:3], np.zeros(3, f32) if c is None else c).all(), f"the centre of measurement {k - 1}"
            got = out[3:].reshape(len(rows), n, 24)
            for j, x in enumerate(rows):
                want = gs4d.transform_selected_host(rec, x, measure=measure if x.flags == gs4d.XS_PIVOT_MEASURE else None, **xc.keywords(table))
                # the NaN rule of gs4d.h, as in tests/test_transform_host.py: the library's host code and this program come from two compilers
                ok = xc.same_bits(got[j], want)
                assert ok.all(), f"{which}, n = {n}, {tname}, row {j}: first word at {np.argwhere(~ok)[0].tolist()}"


# ---- what the moved records mean to a draw ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("4d_vel", "4d_2q"))
def test_a_rotation_about_the_measured_pivot_keeps_the_selections_centroid(gs4d, form):
    """A spatial rotation R about c (time row (0, 0, 0, 1), no offset) maps a record's conditional mean m at time t to R (m - c) + c: the centroid g of
    the selection's conditional means moves by (R - I)(g - c).  c is the centre of gs4d_measure_records at t, which gs4d.h places within
    (hi - lo) * 2^-19 of the centroid of its float32 centres; those centres are within 4 u (|p| + |k sig3|) of the float64 conditional means (three
    roundings and a product).  The records' own roundings: q = p - c (u |q|, carried through |L|), the mean's dot product and sum (6 u on the absolute
    products, as tests/test_transform_host.py), p' = u + c (u |p'|), and 9 u on the absolute products of Sigma' — through tc.conditional_bound,
    doubled for the terms of higher order.  Records that are not selected keep their bytes, so their conditional means are untouched exactly."""
    n, t, u = 400, bc.T, tc.U
    rec = tc.records(gs4d, form, n)
    table = xc.tables(n)["alternating"]
    sel = xc.selected(n, table)
    measure = gs4d.measure_records_host(rec, t=t, **xc.keywords(table))
    assert measure.count == int(sel.sum())
    xf = tc.row(tc.block4(tc.rotation(tc.RIGID_AXIS, tc.RIGID_ANGLE)), (0.0, 0.0, 0.0, 0.0))
    got = gs4d.transform_selected_host(rec, xf, measure=measure, **xc.keywords(table))
    L, o = tc.matrices(xf)
    R = L[:3, :3]
    c = measure.as_dict()["centre"].astype(np.float64)
    p, S = tc.mean_cov(rec)
    p1, S1 = tc.mean_cov(got)
    mean, _ = tc.conditional(p, S, np.full(n, t))
    mean1, _ = tc.conditional(p1, S1, np.full(n, t))
    assert np.array_equal(mean1[~sel], mean[~sel]) and np.array_equal(got[~sel].view(np.uint8), rec[~sel].view(np.uint8))
    q = p.copy()
    q[:, :3] -= c
    dq = u * np.abs(q)
    dq[:, 3] = 0.0                                                                    # (q[3] = p[3]: no rounding)
    dp = dq @ np.abs(L).T + 6.0 * u * (np.abs(q) @ np.abs(L).T)
    dp[:, :3] += u * np.abs(p1[:, :3])                                                # (p' = u + c)
    dS = 9.0 * u * (np.abs(L) @ np.abs(S) @ np.abs(L).T)
    bound_mean, _ = tc.conditional_bound(p1, S1, np.full(n, t), dp, dS)
    k = np.abs((t - p[:, 3]) / S[:, 3, 3])
    centres = 4.0 * u * (np.abs(p[:, :3]) + k[:, None] * np.abs(S[:, :3, 3]))
    extent = np.array(measure.hi[:], np.float64) - np.array(measure.lo[:], np.float64)
    pivot_off = extent * 2.0 ** -19 + centres[sel].mean(0) + u * np.abs(c)
    bound = 2.0 * bound_mean[sel].mean(0) + np.abs(R - np.eye(3)) @ pivot_off
    moved = np.abs(mean1[sel].mean(0) - mean[sel].mean(0))
    print(f"{form}: centroid moved by {moved}, bound {bound}")
    assert (moved <= bound).all(), f"worst moved / bound = {np.max(moved / bound):.3f}"
    assert np.abs(mean1[sel] - mean[sel]).max() > 1.0, "nothing moved: the test shows nothing"
    # and every selected record's conditional mean is the rotated one, to the same per-record bound
    want = (mean[sel] - c) @ R.T + c
    assert (np.abs(mean1[sel] - want) <= 2.0 * bound_mean[sel] + np.abs(R) @ (u * np.abs(c))).all()


# ---- the structure, the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_structure_is_96_bytes(gs4d):
    assert ctypes.sizeof(gs4d.SelectionXf) == 96 and xc.sizeof_selection_xf(gs4d) == 96
    assert [n for n, _ in gs4d.SelectionXf._fields_] == ["xf", "pivot", "flags"]
    assert gs4d.SelectionXf.pivot.offset == 80 and gs4d.SelectionXf.flags.offset == 92
    assert (gs4d.XS_PIVOT, gs4d.XS_PIVOT_MEASURE) == (1, 2)
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert "enum { GS4D_XS_PIVOT = 1, GS4D_XS_PIVOT_MEASURE = 2 };" in hdr and "typedef struct gs4d_selection_xf" in hdr
    assert "gs4d_transform_selected(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_selection_xf* xf," in hdr
    x = gs4d.selection_xf(tc.transforms()["full"], pivot=xc.PIVOT)
    raw = np.frombuffer(bytes(x), f32)
    assert np.array_equal(raw[:20], tc.transforms()["full"]) and np.array_equal(raw[20:23], np.array(xc.PIVOT, f32)) and x.flags == 1


def test_the_call_refuses_what_it_can_without_a_device(gs4d):
    """every other argument error needs a context, and a context needs a device: tests/test_gpu_transform_selected.py"""
    lib = gs4d._lib
    x = gs4d.selection_xf(tc.transforms()["rigid"])
    assert lib.gs4d_transform_selected(None, 1, 1, ctypes.byref(x), 0, None, 0) == -1          # GS4D_E_INVALID: no context
    assert lib.gs4d_transform_selected(None, 0, 0, None, 0, None, 0) == -1
    assert {"gs4d_transform_selected", "gs4d_host_transform_selected"} <= set(gs4d.EXPORTS)
