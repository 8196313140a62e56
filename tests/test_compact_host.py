"""gs4d_compact_records without a GPU: the case table of tests/compact_cases.py pinned, its numpy reference against a plain Python
loop, and the ABI — the export, the declarations and the sizes of the two structures."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import compact_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_table_is_the_documented_one():
    assert cc.SIZES == (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 12289, 135165) and cc.LARGE == 1048581
    assert cc.STRIDES == (16, 48, 96, 288, 1024) and all(s % 16 == 0 for s in cc.STRIDES)
    assert set(cc.STRIDE_SIZES) <= set(cc.SIZES)
    assert cc.BITS_1_255 == 0x3B808081 and cc.WSUM_MIN > 1 << 32
    for tile in (256, 512, 1024, 2048, 4096):                  # every power-of-two tile has a size on, one below and one above a multiple of it
        assert any(n % tile == 0 and n for n in cc.SIZES) and any(n % tile == 1 for n in cc.SIZES) and any(n % tile == tile - 1 for n in cc.SIZES)
        assert -(-cc.LARGE // tile) >= 256
    assert any(n % 64 == 63 for n in cc.SIZES) and any(n % 64 == 1 for n in cc.SIZES)


@pytest.mark.parametrize("n", cc.SIZES)
def test_every_pattern_keeps_what_it_documents(n):
    for pattern in cc.PATTERNS:
        m = cc.pattern_mask(pattern, n)
        assert m.shape == (n,) and int(m.sum()) == cc.pattern_kept(pattern, n), pattern
        for rule in ("prune", "all_fields"):
            st = cc.pattern_table(pattern, n, cc.RULES[rule])
            assert np.array_equal(cc.keeps(st, cc.RULES[rule]), m), (pattern, rule)
            assert np.array_equal(st, cc.pattern_table(pattern, n, cc.RULES[rule]))          # deterministic
            # a dropped row fails on exactly one field
            mp, mw, ms = cc.RULES[rule]
            fails = (st["pixels"] < mp).astype(int) + (st["wmax"] < mw) + (st["wsum"] < np.uint64(ms))
            assert np.array_equal(fails == 1, ~m) and np.array_equal(fails == 0, m), (pattern, rule)
    assert cc.pattern_kept("tile", n) == (0 if n <= 4096 else min(n, 8192) - 4096)
    if n >= 255:                                                 # (p = 0.03 / 0.97 leave room on both sides from here on)
        assert 0 < cc.pattern_kept("p03", n) < cc.pattern_kept("p50", n) < cc.pattern_kept("p97", n) < n


def test_the_threshold_table_straddles_every_field():
    st = cc.threshold_table()
    mp, mw, ms = cc.RULES["all_fields"]
    assert st.size > 64
    assert {int(v) - mp for v in np.unique(st["pixels"])} == {-1, 0, 1}
    assert {0, mw - 1, mw, mw + 1, 0x3F800000} == {int(v) for v in np.unique(st["wmax"])}
    assert {0, ms - 1, ms, ms + 1, ms - (1 << 32), 0xFFFFFFFF} == {int(v) for v in np.unique(st["wsum"])}
    k = cc.keeps(st, cc.RULES["all_fields"])
    assert k.sum() == 3 * 2 * 3 * 2                             # pixels in {min, min + 1}, wmax in {min, min + 1, 1.0f}, wsum in {min, min + 1}
    # a 32-bit compare of the low words would keep these two
    low = (st["wsum"] & np.uint64(0xFFFFFFFF)) >= np.uint64(ms & 0xFFFFFFFF)
    assert (low & (st["wsum"] < np.uint64(ms))).any()
    big = cc.threshold_table(3 * 4096 + 1)                      # the same rows across tiles: every one of the 90 on both sides of a tile edge
    assert big.size == 12289 and np.array_equal(big[:90], st[:90]) and np.array_equal(big[90:180], st[:90])
    assert int(cc.keeps(big, cc.RULES["all_fields"]).sum()) == 12 * (12289 // 90) + int(cc.keeps(st[:12289 % 90], cc.RULES["all_fields"]).sum())
    # every field alone drops rows whose other two fields pass
    others = [(st["wmax"] >= mw) & (st["wsum"] >= np.uint64(ms)), (st["pixels"] >= mp) & (st["wsum"] >= np.uint64(ms)), (st["pixels"] >= mp) & (st["wmax"] >= mw)]
    alone = [st["pixels"] < mp, st["wmax"] < mw, st["wsum"] < np.uint64(ms)]
    for o, a in zip(others, alone):
        assert (o & a).any()


@pytest.mark.parametrize("n", [n for n in cc.SIZES if n <= 4097])
def test_reference_equals_a_plain_loop_and_respects_the_capacities(n):
    for pattern in ("none", "all", "first", "last", "alternating", "p50"):
        st = cc.pattern_table(pattern, n)
        src = cc.records(n, 48)
        kept = cc.pattern_kept(pattern, n)
        for invert in (False, True):
            for cap_dst, cap_idx in ((None, None), (n, n), (kept // 2, n), (n, max(kept - 1, 0)), (0, None), (None, 0)):
                dst, idx, k, w = cc.reference(st, cc.RULES["prune"], src, 48, cap_dst, cap_idx, invert)
                lidx, lk, lw = cc.loop_reference(st, cc.RULES["prune"], cap_dst, cap_idx, invert)
                assert (k, w) == (lk, lw) and idx.tolist() == lidx and idx.dtype == np.uint32
                assert k == (n - kept if invert else kept) and w == min([k] + [c for c in (cap_dst, cap_idx) if c is not None])
                assert np.all(np.diff(idx.astype(np.int64)) > 0)                                # stable: ascending
                assert dst.shape == (w, 48) and np.array_equal(dst.view(np.uint32), src[idx])
    a = cc.reference(cc.pattern_table("p50", n), cc.RULES["prune"], None, 96, None, None)
    b = cc.reference(cc.pattern_table("p50", n), cc.RULES["prune"], None, 96, None, None, invert=True)
    assert a[0] is None and np.array_equal(np.sort(np.concatenate([a[1], b[1]])), np.arange(n))   # the two lists partition 0..n-1


def test_records_are_a_function_of_record_and_offset():
    r = cc.records(300, 288)
    assert r.shape == (300, 72) and r.dtype == np.uint32
    pieces = r.reshape(-1, 4)
    assert np.unique(pieces, axis=0).shape[0] == pieces.shape[0]                                 # no two 16-byte pieces alike


def test_library_exports_the_entry_point_and_the_binding_binds_it(gs4d):
    lib = ctypes.CDLL(gs4d.LIB_PATH)
    assert hasattr(lib, "gs4d_compact_records")
    assert "gs4d_compact_records" in gs4d.EXPORTS
    assert gs4d._lib.gs4d_compact_records.argtypes is not None and len(gs4d._lib.gs4d_compact_records.argtypes) == 9
    assert gs4d.KEEP_INVERT == 1
    assert gs4d.Context.KEEP_RULE.itemsize == 24 and gs4d.Context.COMPACT_COUNT.itemsize == 8
    assert gs4d.Context.KEEP_RULE.fields["min_wsum"][1] == 8 and gs4d.Context.KEEP_RULE.fields["flags"][1] == 16
    for name in ("compact_records", "prune"):
        assert callable(getattr(gs4d.Context, name))


def test_header_declares_the_call_and_its_structures_in_c(gs4d, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert re.search(r"GS4D_API\s+int\s+gs4d_compact_records\s*\(", hdr)
    assert re.search(r"typedef\s+struct\s+gs4d_keep_rule\s*\{", hdr) and re.search(r"typedef\s+struct\s+gs4d_compact_count\s*\{", hdr)
    # any C compiler will do: the system's, or the clang that builds the library
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    compiler = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert compiler, "no C compiler: neither gcc, cc, clang nor the ROCm clang the library is built with"
    src = tmp_path / "compact_abi.c"
    src.write_text(r'''
#include <stddef.h>
#include "gs4d.h"
_Static_assert(sizeof(gs4d_keep_rule) == 24, "gs4d_keep_rule is 24 bytes");
_Static_assert(offsetof(gs4d_keep_rule, min_pixels) == 0 && offsetof(gs4d_keep_rule, min_wmax) == 4 && offsetof(gs4d_keep_rule, min_wsum) == 8, "thresholds");
_Static_assert(offsetof(gs4d_keep_rule, flags) == 16 && offsetof(gs4d_keep_rule, reserved) == 20, "flags, reserved");
_Static_assert(sizeof(gs4d_compact_count) == 8 && offsetof(gs4d_compact_count, written) == 4, "gs4d_compact_count is 8 bytes");
_Static_assert(GS4D_KEEP_INVERT == 1, "the flag");
int main(void) {
    int (*fn)(gs4d_ctx*, gs4d_buf, size_t, const gs4d_keep_rule*, gs4d_buf, size_t, gs4d_buf, gs4d_buf, gs4d_buf) = gs4d_compact_records;
    return fn == 0;
}
''')
    exe = tmp_path / "compact_abi"
    libdir = os.path.dirname(gs4d.LIB_PATH)
    cc_ = subprocess.run([compiler, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                          "-L", libdir, "-lgs4d", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-500:])
