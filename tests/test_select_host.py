"""gs4d_count_ids without a GPU: the numpy restatement of tests/select_cases.py against a plain Python loop, the shared cases
pinned to what they document and to the kernel's constants, and the ABI — the export, the declaration, the size of the structure, the binding."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

import compact_cases as cc
import select_cases as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loop_restate(record, draw, weight, reg, mask, table_in, nrecords):
    """the contract of gs4d.h as a plain Python loop over the rectangle's pixels"""
    x, y, w, h, d0, d1, mw = reg
    rows = [[int(t["pixels"]), int(t["wmax"]), int(t["wsum"])] for t in table_in]
    wbits = np.ascontiguousarray(weight).view(np.uint32)
    for r in range(h):
        for c in range(w):
            rec, drw, wb = int(record[y + r, x + c]), int(draw[y + r, x + c]), int(wbits[y + r, x + c])
            if rec == 0xFFFFFFFF or rec >= nrecords or not (d0 <= drw <= d1) or wb < mw:
                continue
            if mask is not None and int(mask[r, c]) == 0:
                continue
            q = int(np.rint(np.float32(weight[y + r, x + c]) * np.float32(16777216.0)))      # float32 product, round to nearest even
            row = rows[rec]
            row[0] = (row[0] + 1) & 0xFFFFFFFF
            row[1] = max(row[1], wb)
            row[2] = (row[2] + q) & 0xFFFFFFFFFFFFFFFF
    out = np.zeros(len(rows), sel.STAT)
    for i, row in enumerate(rows):
        out[i] = tuple(row)
    return out


def random_planes(rng, w, h, n):
    """records up to 2n (half of them >= n), a fifth of the pixels the sentinel, draws 0 .. 3, weights in (0, 1] with exact ties"""
    rec = rng.integers(0, 2 * n, (h, w)).astype(np.uint32)
    drw = rng.integers(0, 4, (h, w)).astype(np.uint32)
    wt = rng.choice(np.array([1.0, 0.5, 0.25, 3e-8], np.float32), (h, w))
    loose = rng.uniform(size=(h, w)) < 0.6
    wt[loose] = rng.uniform(1e-6, 1.0, int(loose.sum())).astype(np.float32)
    none = rng.uniform(size=(h, w)) < 0.2
    rec[none], drw[none], wt[none] = sel.ID_NONE, sel.ID_NONE, 0.0
    return rec, drw, wt


def test_restatement_equals_a_plain_loop_on_random_planes():
    rng = np.random.default_rng(cc.seed("select/host/random"))
    counted = 0
    for trial in range(300):
        w, h, n = int(rng.integers(1, 14)), int(rng.integers(1, 11)), int(rng.integers(1, 9))
        rec, drw, wt = random_planes(rng, w, h, n)
        rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        rx, ry = int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))
        d0 = int(rng.integers(0, 4))
        draws = sel.EVERY_DRAW if trial % 3 == 0 else (d0, int(rng.integers(d0, 4)))
        mw = 0 if trial % 2 == 0 else sel.weight_bits(rng.choice([0.25, 0.5, 0.7]))
        mask = None if trial % 4 < 2 else rng.choice(np.array([0, 1, 0x80], np.uint8), (rh, rw))
        nrec = n if trial % 5 else max(0, n // 2)
        reg = sel.region(rx, ry, rw, rh, draws, mw)
        for kind in sel.TABLES:
            tin = sel.table(kind, n, f"host{trial}")
            got = sel.restate(rec, drw, wt, reg, mask, tin, nrec)
            want = loop_restate(rec, drw, wt, reg, mask, tin, nrec)
            assert got.tobytes() == want.tobytes(), (trial, kind)
            assert np.array_equal(got[nrec:], tin[nrec:])                # the tail is skipped
            counted += int(got["pixels"].astype(np.int64).sum() - tin["pixels"].astype(np.int64).sum())
    assert counted > 500


def test_restatement_on_hand_made_planes():
    rec = np.array([[0, 0, 1], [sel.ID_NONE, 1, 5]], np.uint32)
    drw = np.array([[0, 1, 1], [sel.ID_NONE, 0, 0]], np.uint32)
    wt = np.array([[1.0, 0.5, 0.25], [0.0, 0.75, 0.5]], np.float32)
    zero = sel.table("zero", 2)
    full = sel.restate(rec, drw, wt, sel.region(0, 0, 3, 2), None, zero, 2)              # record 5 >= nrecords, the sentinel: skipped
    assert full["pixels"].tolist() == [2, 2] and full["wmax"].tolist() == [sel.weight_bits(1.0), sel.weight_bits(0.75)]
    assert full["wsum"].tolist() == [(1 << 24) + (1 << 23), (1 << 22) + 3 * (1 << 22)]
    assert sel.restate(rec, drw, wt, sel.region(0, 0, 3, 2, draws=(1, 1)), None, zero, 2)["pixels"].tolist() == [1, 1]
    assert sel.restate(rec, drw, wt, sel.region(0, 0, 3, 2, min_weight=sel.weight_bits(0.5)), None, zero, 2)["pixels"].tolist() == [2, 1]      # inclusive
    assert sel.restate(rec, drw, wt, sel.region(1, 0, 2, 2), None, zero, 2)["pixels"].tolist() == [1, 2]
    assert sel.restate(rec, drw, wt, sel.region(0, 0, 3, 2), np.array([[0, 0x80, 0], [1, 1, 1]], np.uint8), zero, 2)["pixels"].tolist() == [1, 1]
    assert sel.restate(rec, drw, wt, sel.region(0, 0, 3, 2), None, zero, 1)["pixels"].tolist() == [2, 0]
    twice = sel.restate(rec, drw, wt, sel.region(0, 0, 3, 2), None, full, 2)
    assert twice.tobytes() == sel.add_tables(full, full).tobytes() and twice["wmax"].tolist() == full["wmax"].tolist()
    # a wmax above every weight stays; the halves of a split rectangle add up to the whole
    high = sel.table("filled", 3, "hand")
    assert sel.restate(rec, drw, wt, sel.region(0, 0, 3, 2), None, high, 2)["wmax"][0] == sel.weight_bits(1.5)
    halves = sel.restate(rec, drw, wt, sel.region(2, 0, 1, 2), None, sel.restate(rec, drw, wt, sel.region(0, 0, 2, 2), None, zero, 2), 2)
    assert halves.tobytes() == full.tobytes()


def test_the_cases_match_the_kernel_constants_and_what_they_document():
    src = open(os.path.join(ROOT, "4dgaussiansplatrendering_amd", "csrc", "select.hip")).read()
    m = re.search(r"SEL_WAVES\s*=\s*(\d+),\s*SEL_BATCH\s*=\s*(\d+),\s*SEL_BATCHES\s*=\s*(\d+)", src)
    assert m, "SEL_WAVES, SEL_BATCH, SEL_BATCHES"
    waves, batch, batches = (int(g) for g in m.groups())
    assert batch * batches == sel.WAVE_ROWS and waves * sel.WAVE_ROWS == sel.GROUP_ROWS
    for w, h in ((sel.W, sel.H), (96, 96)):
        assert w % sel.WAVE_COLS and h % sel.GROUP_ROWS and w > sel.WAVE_COLS and h > sel.GROUP_ROWS      # partial waves, more than one workgroup each way
        rects = sel.rectangles(w, h)
        assert len(rects) == 8
        for x, y, rw, rh in rects.values():
            assert 0 <= x and 0 <= y and rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h
        x, y, rw, rh = rects["straddle"]
        assert x % 2 and y % 2 and rw % 2 and rh % 2 and rw > sel.WAVE_COLS and rh > 2 * sel.WAVE_ROWS and rh % batch
    assert sel.H % batch                                                                # the last batch of the image is a partial one
    t = sel.table("filled", 300, "pin")
    assert (t["pixels"] > 0).all() and (t["wsum"] > 0).all() and (t["wmax"] > 0).all()
    assert (t["wmax"] > sel.weight_bits(1.0)).sum() == 100 and (t["wsum"] > 1 << 32).any()
    assert sel.table_bytes(t).size == (300 + sel.TAIL_ROWS) * 16
    assert not sel.mask("zeros", 7, 5).any() and (sel.mask("ones", 7, 5) == 0xFF).all()
    assert sel.mask("checker", 7, 5).sum() == 17 and set(np.unique(sel.mask("random", 31, 17)).tolist()) == {0, 1, 0x80}


def test_the_scenes_are_what_they_document(gs4d, oracle):
    """the premises tests/test_gpu_select.py asserts on the device's planes, here on the CPU: the checker's projection and id_cases.restate"""
    import id_cases
    import stats_cases as sc
    shown = {}
    for name in ("one", "grid", "layered"):
        w, h, rec = sel.scene(gs4d, name)
        view, proj = sc.mats(gs4d, w, h)
        plane = id_cases.restate(oracle.preprocess(oracle.MODE_4D_DIRECT, rec, view, proj, w, h), None, w, h)["record"]
        on = plane != sel.ID_NONE
        shown[name] = (float(on.mean()), np.unique(plane[on]).size, rec.shape[0], float((plane[:, 1:] != plane[:, :-1]).mean()))
    assert shown["one"][:2] == (1.0, 1)
    frac, records, n, differ = shown["grid"]
    assert 0.2 < frac < 0.8 and records == n > 300 and differ > 0.2, shown["grid"]
    assert shown["layered"][0] > 0.6 and shown["layered"][1] > 1000, shown["layered"]


def test_library_exports_the_entry_point_and_the_binding_binds_it(gs4d):
    lib = ctypes.CDLL(gs4d.LIB_PATH)
    assert hasattr(lib, "gs4d_count_ids")
    assert "gs4d_count_ids" in gs4d.EXPORTS
    assert len(gs4d._lib.gs4d_count_ids.argtypes) == 5
    assert ctypes.sizeof(gs4d.IdRegion) == 32
    assert [f[0] for f in gs4d.IdRegion._fields_] == ["x", "y", "w", "h", "draw_first", "draw_last", "min_weight", "reserved"]
    assert gs4d.Context.ID_NONE == sel.ID_NONE
    for name in ("count_ids", "select"):
        assert callable(getattr(gs4d.Context, name))


def test_header_declares_the_call_and_its_structure_in_c(gs4d, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert re.search(r"GS4D_API\s+int\s+gs4d_count_ids\s*\(", hdr) and re.search(r"typedef\s+struct\s+gs4d_id_region\s*\{", hdr)
    assert re.search(r"#define\s+GS4D_ID_NONE\s+0xFFFFFFFFu", hdr)
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    compiler = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert compiler, "no C compiler: neither gcc, cc, clang nor the ROCm clang the library is built with"
    src = tmp_path / "select_abi.c"
    src.write_text(r'''
#include <stddef.h>
#include "gs4d.h"
_Static_assert(sizeof(gs4d_id_region) == 32, "gs4d_id_region is 32 bytes");
_Static_assert(offsetof(gs4d_id_region, x) == 0 && offsetof(gs4d_id_region, h) == 12 && offsetof(gs4d_id_region, draw_first) == 16 &&
               offsetof(gs4d_id_region, draw_last) == 20 && offsetof(gs4d_id_region, min_weight) == 24 && offsetof(gs4d_id_region, reserved) == 28, "the fields");
_Static_assert(GS4D_ID_NONE == 0xFFFFFFFFu, "the sentinel");
int main(void) {
    int (*fn)(gs4d_ctx*, const gs4d_id_region*, gs4d_buf, gs4d_buf, size_t) = gs4d_count_ids;
    return fn == 0;
}
''')
    exe = tmp_path / "select_abi"
    libdir = os.path.dirname(gs4d.LIB_PATH)
    cc_ = subprocess.run([compiler, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                          "-L", libdir, "-lgs4d", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-500:])
