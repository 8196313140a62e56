"""gs4d_record_time_spans / gs4d_compact_time_window without a GPU: the numpy restatement of tests/time_window_cases.py checked
against its own definition — threshold exactness, monotonicity, a brute-force neighbourhood, the three classes on a hand-written table — the
window rule against a plain loop, and the ABI: the exports, the declarations, the structure and the constant."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import scenes
import time_window_cases as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SYNTH, N_EXTREME = 200_000, 1000


@pytest.fixture(scope="module")
def synth():
    mu, s44 = tw.synthetic(N_SYNTH, N_EXTREME)
    table = tw.spans_of(mu, np.ones_like(mu), s44, 0.0)
    for a in (mu, s44, table):
        a.setflags(write=False)
    return mu, np.float32(1.0) / s44, table


def test_the_cases_cover_what_they_claim():
    mu, s44 = tw.synthetic(N_SYNTH, N_EXTREME)
    ext = s44[N_SYNTH:]
    assert ext.min() < 1e-11 and ext.max() > 1e11 and np.abs(mu[N_SYNTH:]).max() > 9e5 and (mu[N_SYNTH:] == 0).any()
    assert tw.SPAN.itemsize == 8 and tw.DEAD_ARG == np.float32(-106.0)
    assert np.exp(np.float64(tw.DEAD_ARG)) < 0.5 * 2.0 ** -149              # the premise on the constant: below half the smallest denormal
    t = tw.f32([-np.inf, -tw.FLT_MAX, -1.0, -2.0 ** -149, -0.0, 0.0, 2.0 ** -149, 1.0, tw.FLT_MAX, np.inf])
    k = tw.key(t)
    assert (np.diff(k) > 0).all() and k[5] - k[4] == 1 and np.array_equal(tw.unkey(k).view(np.uint32), t.view(np.uint32))


def test_the_ends_sit_exactly_on_the_threshold(synth):
    mu, inv, table = synth
    first, last = table["t_first"], table["t_last"]
    assert np.isfinite(first).all() and np.isfinite(last).all() and (first <= mu).all() and (mu <= last).all()
    assert (tw.arg(last, mu, inv) >= tw.DEAD_ARG).all() and (tw.arg(first, mu, inv) >= tw.DEAD_ARG).all()
    assert (tw.arg(np.nextafter(last, tw.INF), mu, inv) < tw.DEAD_ARG).all()
    assert (tw.arg(np.nextafter(first, -tw.INF), mu, inv) < tw.DEAD_ARG).all()
    # where float32 resolves the lifetime, the ends are where the real-valued expression puts them: |t - mu| = sqrt(212 * s44)
    half = np.sqrt(212.0 / inv.astype(np.float64))
    fine = half > 1e4 * np.spacing(np.abs(mu) + half.astype(np.float32))
    assert fine[:N_SYNTH].all() and fine[N_SYNTH:].any() and not fine[N_SYNTH:].all()
    assert np.allclose((last - mu)[fine], half[fine], rtol=1e-3) and np.allclose((mu - first)[fine], half[fine], rtol=1e-3)


def test_times_inside_are_alive_and_times_beyond_are_dead(synth):
    mu, inv, table = synth
    rng = np.random.default_rng(tw.seed("time_window/inside"))
    kf, kl = tw.key(table["t_first"]), tw.key(table["t_last"])
    for _ in range(4):
        inside = tw.unkey(kf + (rng.uniform(size=mu.size) * (kl - kf + 1)).astype(np.int64).clip(0, kl - kf))
        assert (tw.arg(inside, mu, inv) >= tw.DEAD_ARG).all()
        # beyond: any float between the end and +-FLT_MAX, log-uniform in the distance of the bit patterns
        up = tw.unkey(kl + 1 + (np.exp(rng.uniform(0.0, 1.0, mu.size) * np.log((tw.key(tw.FLT_MAX) - kl).clip(1))) - 1).astype(np.int64))
        down = tw.unkey(kf - 1 - (np.exp(rng.uniform(0.0, 1.0, mu.size) * np.log((kf - tw.key(-tw.FLT_MAX)).clip(1))) - 1).astype(np.int64))
        assert (up > table["t_last"]).all() and (down < table["t_first"]).all()
        assert (tw.arg(up, mu, inv) < tw.DEAD_ARG).all() and (tw.arg(down, mu, inv) < tw.DEAD_ARG).all()


def test_arg_is_monotone_in_the_distance_from_mu(synth):
    mu, inv, _ = synth
    rng = np.random.default_rng(tw.seed("time_window/monotone"))
    for side in (1.0, -1.0):
        d = np.sort(np.abs(rng.normal(size=(mu.size, 8))) * np.sqrt(212.0 / inv.astype(np.float64))[:, None], axis=1)
        t = (mu[:, None].astype(np.float64) + side * d).astype(np.float32)                      # ascending distance, a few per record, around the ends
        a = tw.arg(t, mu[:, None], inv[:, None])
        assert (np.diff(a, axis=1) <= 0).all()


def test_a_brute_force_neighbourhood_agrees(synth):
    """every float32 within 4096 bit patterns of both ends, on the extreme records and as many ordinary ones: alive exactly between the ends — the
    scan walks past the other end on records whose whole span is shorter than the scan, and says so"""
    mu, inv, table = synth
    sel = np.r_[0:N_EXTREME, N_SYNTH:N_SYNTH + N_EXTREME]
    kf, kl = tw.key(table["t_first"][sel]), tw.key(table["t_last"][sel])
    short = 0
    for end in ("t_first", "t_last"):
        k, alive = tw.brute_alive(mu[sel], inv[sel], table[end][sel], 4096)
        assert np.array_equal(alive, (k >= kf[:, None]) & (k <= kl[:, None]))
        short += int(((k < kf[:, None]).any(1) & (k > kl[:, None]).any(1)).sum())
    assert short > 0, "no record whose span is shorter than the scan"


def test_the_three_classes_on_the_hand_written_table():
    seen = set()
    for floor in tw.CLASS_FLOORS:
        rec, want = tw.class_records(floor)
        table = tw.spans(rec, floor)
        for i, w in enumerate(want):
            got = (table["t_first"][i], table["t_last"][i])
            if w == "span":
                assert np.isfinite(got[0]) and np.isfinite(got[1]) and got[0] <= rec[i, 3] <= got[1], (floor, i, got)
            else:
                assert got == w, (floor, i, got)
            seen.add(w if w == "span" else ("never" if w == tw.NEVER else "always"))
    assert sum(len(tw.class_records(f)[1]) for f in tw.CLASS_FLOORS) == len(tw.CLASS_TABLE) and seen == {"span", "never", "always"}
    names = " ".join(r[0] for r in tw.CLASS_TABLE)
    for what in ("alpha 0", "alpha -0", "alpha negative", "alpha NaN", "s44 0", "s44 negative", "s44 inf", "s44 NaN", "mu inf", "a floor", "a NaN floor"):
        assert what in names
    # the ends of the plain row by hand: sqrt(212 * 0.25) = 7.2801
    rec, _ = tw.class_records(0.0)
    plain = tw.spans(rec)[0]
    assert abs(plain["t_last"] - (25.0 + 7.2801)) < 1e-3 and abs(plain["t_first"] - (25.0 - 7.2801)) < 1e-3
    # a span at FLT_MAX: one float (the next one down is 2e31 away); and the longest-lived record there is (s44 = FLT_MAX, a subnormal reciprocal) still dies
    big = tw.spans_of([tw.FLT_MAX, 0.0], [1.0, 1.0], [1.0, tw.FLT_MAX], 0.0)
    assert big["t_last"][0] == tw.FLT_MAX and big["t_first"][0] == tw.FLT_MAX
    assert np.isclose(big["t_last"][1], np.sqrt(212.0 * float(tw.FLT_MAX)), rtol=1e-6) and big["t_first"][1] == -big["t_last"][1]


def test_cube_params_4d_spans_and_the_window_shares(gs4d):
    rec = gs4d.build_records_4d(*scenes.cube_params_4d(4096))
    table = tw.spans(rec)
    assert np.isfinite(table["t_first"]).all() and np.isfinite(table["t_last"]).all()
    half = np.sqrt(212.0 * rec[:, 23].astype(np.float64))
    assert np.allclose(table["t_last"] - rec[:, 3], half, rtol=1e-4) and np.allclose(rec[:, 3] - table["t_first"], half, rtol=1e-4)
    shares = [float(tw.keeps(table, *w).mean()) for w in ((25.0, 25.0), (24.0, 26.0), (20.0, 30.0), (-1e9, 1e9), (200.0, 300.0))]
    assert 0.1 < shares[0] < shares[1] < shares[2] < 0.9 and shares[3] == 1.0 and shares[4] == 0.0, shares
    assert tw.keeps(tw.spans(rec, 0.05), 200.0, 300.0).all()                                     # a floor: every record always


@pytest.mark.parametrize("n", tw.COMPACT_SIZES)
def test_the_window_reference_equals_a_plain_loop(n):
    table = tw.window_table(n)
    src = np.arange(n * 4, dtype=np.uint32).reshape(n, 4)
    for t0, t1 in ((24.0, 26.0), (-np.inf, np.inf), (1e9, 2e9), (25.0, 25.0)):
        want = [i for i in range(n) if float(table["t_first"][i]) <= t1 and float(table["t_last"][i]) >= t0]
        for cap_dst, cap_idx in ((None, None), (n, n), (len(want) // 2, n), (n, max(len(want) - 1, 0)), (0, None)):
            dst, idx, kept, written = tw.reference(table, t0, t1, src, 16, cap_dst, cap_idx)
            assert kept == len(want) and written == min([kept] + [c for c in (cap_dst, cap_idx) if c is not None])
            assert idx.tolist() == want[:written] and idx.dtype == np.uint32 and np.array_equal(dst.view(np.uint32), src[idx])
    if n >= 2047:                                            # every kind of row is there, on both sides of the rule
        k = tw.keeps(table, 24.0, 26.0)
        assert 0.3 * n < k.sum() < 0.7 * n
        assert np.isnan(table["t_first"]).any() and not k[np.isnan(table["t_first"]) | np.isnan(table["t_last"])].any()
        assert k[(table["t_last"] == np.float32(24.0))].all() and not k[table["t_last"] == np.nextafter(np.float32(24.0), -tw.INF)].any()
        assert k[(table["t_first"] == np.float32(26.0))].all() and not k[table["t_first"] == np.nextafter(np.float32(26.0), tw.INF)].any()


def test_library_exports_the_entry_points_and_the_binding_binds_them(gs4d):
    lib = ctypes.CDLL(gs4d.LIB_PATH)
    for name, nargs in (("gs4d_record_time_spans", 5), ("gs4d_compact_time_window", 10)):
        assert hasattr(lib, name) and name in gs4d.EXPORTS
        assert len(getattr(gs4d._lib, name).argtypes) == nargs
    assert gs4d.TIME_DEAD_ARG == -106.0 and gs4d.Context.TIME_SPAN == tw.SPAN
    for name in ("record_time_spans", "compact_time_window", "time_window"):
        assert callable(getattr(gs4d.Context, name))


def test_header_declares_the_calls_and_the_structure_in_c(gs4d, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert re.search(r"GS4D_API\s+int\s+gs4d_record_time_spans\s*\(", hdr) and re.search(r"GS4D_API\s+int\s+gs4d_compact_time_window\s*\(", hdr)
    assert re.search(r"typedef\s+struct\s+gs4d_time_span\s*\{", hdr) and re.search(r"#define\s+GS4D_TIME_DEAD_ARG\s+\(-106\.0f\)", hdr)
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    compiler = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert compiler, "no C compiler: neither gcc, cc, clang nor the ROCm clang the library is built with"
    src = tmp_path / "time_window_abi.c"
    src.write_text(r'''
#include <stddef.h>
#include "gs4d.h"
_Static_assert(sizeof(gs4d_time_span) == 8 && offsetof(gs4d_time_span, t_first) == 0 && offsetof(gs4d_time_span, t_last) == 4, "gs4d_time_span is two floats");
int main(void) {
    int (*spans)(gs4d_ctx*, gs4d_buf, size_t, float, gs4d_buf) = gs4d_record_time_spans;
    int (*window)(gs4d_ctx*, gs4d_buf, size_t, float, float, gs4d_buf, size_t, gs4d_buf, gs4d_buf, gs4d_buf) = gs4d_compact_time_window;
    const float dead = GS4D_TIME_DEAD_ARG;
    /* a NULL context is refused, not dereferenced */
    if (spans(NULL, 1, 1, 0.0f, 2) != GS4D_E_INVALID || window(NULL, 1, 1, 0.0f, 1.0f, 0, 96, 0, 0, 2) != GS4D_E_INVALID) return 2;
    return dead == -106.0f ? 0 : 3;
}
''')
    exe = tmp_path / "time_window_abi"
    libdir = os.path.dirname(gs4d.LIB_PATH)
    cc_ = subprocess.run([compiler, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                          "-L", libdir, "-lgs4d", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-500:])
