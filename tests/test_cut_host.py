"""gs4d_stat_cut without a GPU: the numpy restatement of tests/cut_cases.py against a plain Python loop, the generators pinned to
what they document, and the ABI — the export, the declaration, the size of the structure, the binding."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import compact_cases as cc
import cut_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_table_matches_the_kernel_constants():
    src = open(os.path.join(ROOT, "4dgaussiansplatrendering_amd", "csrc", "gs4d_internal.h")).read()
    for name, want in (("CUT_DIGIT_BITS", kc.DIGIT_BITS), ("CUT_TILE", kc.TILE), ("CUT_GROUPS", kc.GROUPS)):
        m = re.search(r"constexpr\s+uint32_t\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*(\d+)", src)
        assert m and int(m.group(1)) == want, name
    assert kc.SIZES == (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 6145)
    tiles = -(-kc.STRIDE_SIZE // kc.TILE)
    assert tiles // kc.GROUPS >= 2 and tiles > 2 * kc.GROUPS       # every workgroup of the capped grid takes a second tile, the first a third
    assert kc.CUT.itemsize == 16 and kc.CUT.fields["above"][1] == 8 and kc.CUT.fields["equal"][1] == 12


def test_restatement_equals_a_plain_loop_on_random_tables():
    rng = np.random.default_rng(cc.seed("cut/host/random"))
    tables = 0
    for field in kc.FIELDS:
        top = (1 << kc.FIELD_BITS[field]) - 1
        for trial in range(1000):
            n = int(rng.integers(0, 25))
            kind = trial % 4
            if kind == 0:                                    # the whole width
                f = rng.integers(0, top, n, dtype=np.uint64, endpoint=True)
            elif kind == 1:                                  # many ties
                f = rng.integers(0, 4, n).astype(np.uint64) << np.uint64(kc.FIELD_BITS[field] - 3)
            elif kind == 2:                                  # the ends of the field
                f = rng.choice(np.array([0, 1, top - 1, top], np.uint64), n)
            else:                                            # neighbours around a digit boundary
                f = np.uint64(1 << (kc.FIELD_BITS[field] - kc.DIGIT_BITS)) + rng.integers(0, 5, n).astype(np.uint64) - np.uint64(2)
            for budget in {1, 2, max(1, n // 2), max(1, n - 1), max(1, n), n + 7}:
                got = kc.restate(f, budget)
                assert got == kc.loop_restate(f, budget), (field, f.tolist(), budget)
                check_contract(f, budget, got)
            tables += 1
    assert tables == 3000


def check_contract(f, budget, got):
    """the inequalities gs4d.h states"""
    value, above, equal = got
    n = len(f)
    if n == 0:
        assert got == (0, 0, 0)
        return
    k = min(budget, n)
    assert above < k <= above + equal and equal >= 1
    assert above == int((f > np.uint64(value)).sum()) and above + equal == int((f >= np.uint64(value)).sum())


def test_restatement_on_hand_made_tables():
    u = lambda *v: np.array(v, np.uint64)
    assert kc.restate(u(), 3) == (0, 0, 0)
    assert kc.restate(u(5), 1) == (5, 0, 1) and kc.restate(u(5), 9) == (5, 0, 1)
    assert kc.restate(u(1, 2, 3, 4), 1) == (4, 0, 1) and kc.restate(u(1, 2, 3, 4), 4) == (1, 3, 1) and kc.restate(u(1, 2, 3, 4), 11) == (1, 3, 1)
    assert kc.restate(u(7, 7, 7), 1) == (7, 0, 3) and kc.restate(u(7, 7, 7), 3) == (7, 0, 3)
    assert kc.restate(u(9, 5, 5, 5, 2, 2), 2) == (5, 1, 3) and kc.restate(u(9, 5, 5, 5, 2, 2), 4) == (5, 1, 3) and kc.restate(u(9, 5, 5, 5, 2, 2), 5) == (2, 4, 2)
    top = (1 << 64) - 1
    assert kc.restate(u(top, 0, top), 2) == (top, 0, 2) and kc.restate(u(top, 0, top), 3) == (0, 2, 1)
    # equal low words, different high words: a 32-bit compare would call them a tie
    assert kc.restate(u((3 << 32) | 9, (1 << 32) | 9, (2 << 32) | 9), 2) == ((2 << 32) | 9, 1, 1)
    for f, b in ((u(9, 5, 5, 5, 2, 2), 4), (u(top, 0, top), 3)):
        assert kc.restate(f, b) == kc.loop_restate(f, b)


@pytest.mark.parametrize("n", [n for n in kc.SIZES if n <= 257])
def test_generators_on_small_sizes_against_the_loop(n):
    for gen in kc.GENERATORS:
        st = kc.table(gen, n)
        assert st.dtype == kc.STAT and st.shape == (n,) and np.array_equal(st, kc.table(gen, n))      # deterministic
        for field in kc.FIELDS:
            f = kc.field_u64(st, field)
            for budget in kc.budgets(n):
                got = kc.restate(f, budget)
                assert got == kc.loop_restate(f, budget), (gen, field, budget)
                check_contract(f, budget, got)
                e = kc.expected_bytes(st, field, budget)
                assert e.shape == (16,) and int(e[:8].view(np.uint64)[0]) == got[0] and tuple(int(x) for x in e[8:].view(np.uint32)) == got[1:]


@pytest.mark.parametrize("n", [257, kc.TILE + 1, 3 * kc.TILE + 1])
def test_generators_are_what_they_document(n):
    bits, d = kc.FIELD_BITS, kc.DIGIT_BITS
    for field in kc.FIELDS:
        f = lambda gen: kc.field_u64(kc.table(gen, n), field)
        assert np.unique(f("equal")).size == 1 and kc.restate(f("equal"), n // 2) == (int(f("equal")[0]), 0, n)
        assert np.unique(f("distinct")).size == n
        for k in kc.budgets(n):
            assert kc.restate(f("distinct"), k)[1:] == (min(k, n) - 1, 1)
        top, low = f("top_digit"), f("bottom_digit")
        assert np.unique(top & np.uint64((1 << (bits[field] - d)) - 1)).size == 1 and np.unique(top >> np.uint64(bits[field] - d)).size > 100
        assert np.unique(low >> np.uint64(d)).size == 1 and np.unique(low & np.uint64((1 << d) - 1)).size > 100
        zero = f("mostly_zero")
        assert 0 < (zero != 0).sum() <= n // 50 + 1 and kc.restate(zero, n)[0] == 0
        # the two tie groups and the budgets on their boundary
        t, a, b = kc.tie_layout(n)
        ties = f("ties")
        k1, k2 = kc.tie_budgets(n)
        v1, above1, equal1 = kc.restate(ties, k1)
        v2, above2, equal2 = kc.restate(ties, k2)
        assert (above1, equal1) == (t, a) and above1 + equal1 == k1              # the last member of the upper group: exactly k kept at min = value
        assert (above2, equal2) == (t + a, b) and v2 < v1 and above2 + equal2 == n > k2      # the first member of the lower group: the tie does not fit
    hh = kc.table("high_half", n)["wsum"]
    assert np.unique(hh & np.uint64(0xFFFFFFFF)).size == 1 and np.unique(hh >> np.uint64(32)).size > 200 and int(hh.max()) >= 1 << 40
    w = kc.table("weights", n)["wmax"].view(np.float32)
    assert (w > 0).all() and (w <= 1).all() and np.unique(w).size > n // 2
    # wmax bit patterns are in float order: the cut of the bit patterns is the cut of the weights
    v, above, _ = kc.restate(kc.field_u64(kc.table("weights", n), "wmax"), n // 3)
    assert above == int((w > np.array([v], np.uint32).view(np.float32)[0]).sum())


def test_library_exports_the_entry_point_and_the_binding_binds_it(gs4d):
    lib = ctypes.CDLL(gs4d.LIB_PATH)
    assert hasattr(lib, "gs4d_stat_cut")
    assert "gs4d_stat_cut" in gs4d.EXPORTS
    assert len(gs4d._lib.gs4d_stat_cut.argtypes) == 6
    assert (gs4d.STAT_PIXELS, gs4d.STAT_WMAX, gs4d.STAT_WSUM) == (0, 1, 2)
    assert gs4d.Context.CUT == kc.CUT and gs4d.Context.STAT_FIELDS == {"pixels": 0, "wmax": 1, "wsum": 2}
    for name in ("stat_cut", "read_stat_cut", "prune_to_budget"):
        assert callable(getattr(gs4d.Context, name))


def test_header_declares_the_call_and_its_structure_in_c(gs4d, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert re.search(r"GS4D_API\s+int\s+gs4d_stat_cut\s*\(", hdr) and re.search(r"typedef\s+struct\s+gs4d_cut\s*\{", hdr)
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    compiler = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert compiler, "no C compiler: neither gcc, cc, clang nor the ROCm clang the library is built with"
    src = tmp_path / "cut_abi.c"
    src.write_text(r'''
#include <stddef.h>
#include "gs4d.h"
_Static_assert(sizeof(gs4d_cut) == 16, "gs4d_cut is 16 bytes");
_Static_assert(offsetof(gs4d_cut, value) == 0 && offsetof(gs4d_cut, above) == 8 && offsetof(gs4d_cut, equal) == 12, "value, above, equal");
_Static_assert(GS4D_STAT_PIXELS == 0 && GS4D_STAT_WMAX == 1 && GS4D_STAT_WSUM == 2, "the fields");
int main(void) {
    int (*fn)(gs4d_ctx*, gs4d_buf, size_t, int, size_t, gs4d_buf) = gs4d_stat_cut;
    return fn == 0;
}
''')
    exe = tmp_path / "cut_abi"
    libdir = os.path.dirname(gs4d.LIB_PATH)
    cc_ = subprocess.run([compiler, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                          "-L", libdir, "-lgs4d", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-500:])
