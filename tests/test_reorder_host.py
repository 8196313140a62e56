"""gs4d_spatial_order / gs4d_gather_records without a GPU: the numpy restatement of tests/reorder_cases.py against an independent
record-by-record reference and against bench.py's --spatial-order permutation, the hostile classes by hand, and the ABI: the exports, the
declarations, the prototypes as C sees them."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np

import reorder_cases as rc
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def test_the_restatement_equals_a_record_by_record_reference():
    for name, n in (("uniform", 3000), ("clusters", 2000), ("hostile/mixed", 2000), ("hostile/overflow", 500), ("hostile/zeros", 500), ("hostile/flat1", 500)):
        pos = rc.positions(name, n)
        want_order, want_keys = rc.loop_order(pos)
        assert np.array_equal(rc.keys(pos), want_keys), name
        assert np.array_equal(rc.order(pos), want_order), name
    pos = rc.positions("uniform", 3000)
    k = rc.keys(pos)
    assert k.max() < 1 << 30 and np.unique(k).size > 2500 and np.unique(rc.cells(pos)[0]).size > 900       # the cases say something


def test_the_order_is_the_one_bench_uploads():
    """bench.py --spatial-order on the benchmark's own positions: the same permutation, so a device-reordered set is the host-permuted upload"""
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    for n in (1000, 50_000):
        pos = scenes.cube_params(n)[0]
        assert pos.dtype == np.float32 and pos.shape == (n, 3)
        assert np.array_equal(rc.order(pos), bench.morton_order(pos).astype(np.uint32)), n


def test_unplaced_records_go_last_in_their_order():
    pos = rc.f32([[0, 0, 0], [NAN, 0, 0], [1, 1, 1], [0, INF, 0], [0.5, 0.5, 0.5], [0, 0, -INF], [1e30, 0, 0]])
    k = rc.keys(pos)
    assert list(rc.placed(pos)) == [True, False, True, False, True, False, True]
    assert (k[[1, 3, 5]] == rc.UNPLACED).all() and (k[[0, 2, 4, 6]] < rc.UNPLACED).all()
    assert list(rc.order(pos)[-3:]) == [1, 3, 5]
    # 1e30 is a position like any other: it stretches the box
    cell, _ = rc.cells(pos)
    assert list(cell[6]) == [1023, 0, 0] and list(cell[0]) == [0, 0, 0] and cell[2, 0] == 0 and cell[2, 1] == 1023


def test_all_records_unplaced_is_the_identity():
    pos = rc.positions("hostile/unplaced_all", 300)
    assert not rc.placed(pos).any() and (rc.keys(pos) == rc.UNPLACED).all()
    assert np.array_equal(rc.order(pos), np.arange(300, dtype=np.uint32))


def test_the_sign_of_a_zero_cannot_change_a_cell():
    a = rc.f32([[0.0, -0.0, 0.0], [-0.0, 0.0, 1.0], [2.0, 0.0, -0.0], [1.0, -0.0, 0.5]])
    for perm in ([0, 1, 2, 3], [1, 0, 3, 2], [3, 2, 1, 0]):                 # whichever zero the minimum picks
        cell, ok = rc.cells(a[perm])
        assert ok.all() and np.array_equal(cell, rc.cells(np.abs(a[perm]))[0])
    # by hand: lo = -0 and lo = +0 give the same d / e * 1023 up to the sign of a zero, which g >= 0 accepts
    for lo in (np.float32(0.0), np.float32(-0.0)):
        for p in (np.float32(0.0), np.float32(-0.0)):
            g = (p - lo) / (np.float32(2.0) - lo) * np.float32(1023.0)
            assert g == 0 and g >= 0


def test_degenerate_axes_and_an_overflowing_box():
    one = rc.positions("hostile/flat1", 400)
    cell, ok = rc.cells(one)
    assert ok.all() and (cell[:, 1] == 0).all() and cell[:, 0].max() == 1023 and cell[:, 2].max() == 1023      # 0 / 0 on the flat axis only
    three = rc.f32(np.tile([[1.5, -2.0, 3.0]], (50, 1)))
    assert (rc.keys(three) == 0).all() and np.array_equal(rc.order(three), np.arange(50, dtype=np.uint32))
    # hi - lo overflows on x: finite / inf = 0 for the ordinary records, inf / inf = NaN -> 0 for the one whose own distance overflows
    over = rc.f32([[-3.0e38, 0, 0], [3.0e38, 1, 0], [0.0, 0.5, 0], [1.0, 0.25, 0]])
    cell, ok = rc.cells(over)
    assert ok.all() and (cell[:, 0] == 0).all() and list(cell[:, 1]) == [0, 1023, 511, 255] and (cell[:, 2] == 0).all()
    assert np.array_equal(rc.order(rc.positions("hostile/overflow", 500)), rc.loop_order(rc.positions("hostile/overflow", 500))[0])


def test_the_gather_reference_and_the_lists():
    src = rc.cc.records(100, 48)
    lists = rc.index_lists(100)
    assert set(lists) == {"identity", "reversed", "repeated", "longer", "shorter", "out_of_range"}
    assert lists["longer"].size > 100 > lists["shorter"].size and np.unique(lists["repeated"]).size < lists["repeated"].size
    bad = lists["out_of_range"]
    assert (bad == 0xFFFFFFFF).any() and (bad == 100).any() and (bad < 100).any()
    dst = np.full((bad.size, 12), 0xA5A5A5A5, np.uint32)
    out = rc.gather_reference(bad, src, dst)
    for j in range(bad.size):
        assert np.array_equal(out[j], src[bad[j]] if bad[j] < 100 else dst[j])


def test_library_exports_the_entry_points_and_the_binding_binds_them(gs4d):
    lib = ctypes.CDLL(gs4d.LIB_PATH)
    for name, nargs in (("gs4d_spatial_order", 6), ("gs4d_gather_records", 7)):
        assert hasattr(lib, name) and name in gs4d.EXPORTS
        assert len(getattr(gs4d._lib, name).argtypes) == nargs
    for name in ("spatial_order", "gather_records", "reorder_spatial"):
        assert callable(getattr(gs4d.Context, name))


def test_header_declares_the_calls_in_c(gs4d, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert re.search(r"GS4D_API\s+int\s+gs4d_spatial_order\s*\(", hdr) and re.search(r"GS4D_API\s+int\s+gs4d_gather_records\s*\(", hdr)
    assert "0x40000000" in hdr and "The guarantee" in hdr
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    compiler = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert compiler, "no C compiler: neither gcc, cc, clang nor the ROCm clang the library is built with"
    src = tmp_path / "reorder_abi.c"
    src.write_text(r'''
#include <stddef.h>
#include "gs4d.h"
int main(void) {
    int (*order)(gs4d_ctx*, gs4d_buf, size_t, size_t, size_t, gs4d_buf) = gs4d_spatial_order;
    int (*gather)(gs4d_ctx*, gs4d_buf, size_t, gs4d_buf, size_t, size_t, gs4d_buf) = gs4d_gather_records;
    /* a NULL context is refused, not dereferenced */
    if (order(NULL, 1, 1, 96, 0, 2) != GS4D_E_INVALID || gather(NULL, 1, 1, 2, 1, 96, 3) != GS4D_E_INVALID) return 2;
    return 0;
}
''')
    exe = tmp_path / "reorder_abi"
    libdir = os.path.dirname(gs4d.LIB_PATH)
    cc_ = subprocess.run([compiler, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                          "-L", libdir, "-lgs4d", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-500:])
