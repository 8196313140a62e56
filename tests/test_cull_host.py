"""CPU: the premises of tests/test_gpu_cull.py and the containment proof of the tightened pixel rectangle.

* The alpha-0 share of BASELINE.json configs[3]'s 4D set at the five times of its sweep, recomputed with the checker, and that every cut the GPU
  tests draw holds both records the cull drops and records it keeps (or none, or all, where the case says so).
* tests/footprint_rect_check.cpp, a stand-alone program, built with -ffp-contract=off, plainly and with AddressSanitizer +
  UndefinedBehaviorSanitizer (an executable of its own: nothing is preloaded): on more than 10^6 seeded records no pixel the compositor's
  predicate accepts lies outside the new rectangle; on a cut of the benchmark's static cube it prints the share of entries and candidate pixels saved.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cull_cases as cc
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alpha0(oracle, gs4d, rec, t, min_opacity=0.0, w=cc.W, h=cc.H):
    view, proj = cc.mats(gs4d, w, h)
    p = oracle.preprocess(oracle.MODE_4D, rec, view, proj, w, h, t, min_opacity)
    valid = p["valid"] != 0
    return valid, valid & (p["alpha"] == 0.0), p


def test_the_alpha0_share_of_the_4d_set(gs4d, oracle):
    """ot * col.w == 0.0f for 39 % of the records in the middle of the sweep and 69 % at its ends (the first 200 000 records of the set at 1080p)"""
    rec = cc.records_4d(gs4d, 200_000, scale=1.0)
    for t, share in zip(cc.TIMES, cc.SHARES):
        view, proj = cc.mats(gs4d, 1920, 1080)
        p = oracle.preprocess(oracle.MODE_4D, rec, view, proj, 1920, 1080, t, 0.0)
        valid = p["valid"] != 0                              # (an invalid record's alpha is stored as 0: the share is taken among the valid ones, nearly all)
        got = float((p["alpha"][valid] == 0.0).mean())
        print(f"t = {t}: alpha == 0 for {100 * got:.1f} % of {int(valid.sum())} valid records")
        assert abs(got - share) <= 0.01, (t, got, share)


def test_every_cut_of_the_gpu_tests_holds_what_its_case_needs(gs4d, oracle):
    rec = cc.records_4d(gs4d)
    valid, zero, _ = alpha0(oracle, gs4d, rec, cc.T_HALF)
    assert 0.3 * valid.sum() < zero.sum() < 0.7 * valid.sum() and valid.sum() > cc.N // 2, (int(valid.sum()), int(zero.sum()))
    for seg in range(4):                                     # every segment of the projection kernel holds both kinds
        s = slice(seg * cc.SEG, min(cc.N, (seg + 1) * cc.SEG))
        assert zero[s].any() and (valid[s] & ~zero[s]).any(), seg
    valid, zero, _ = alpha0(oracle, gs4d, rec, cc.T_NONE)
    assert valid.sum() > cc.N // 2 and np.array_equal(valid, zero)
    valid, zero, _ = alpha0(oracle, gs4d, rec, cc.T_HALF, min_opacity=0.25)
    assert valid.sum() > cc.N // 2 and not zero.any()
    for make in (cc.segment_and_wave, cc.negative_zero, cc.big_footprints):
        rec3, idx = make(gs4d)
        valid, zero, p = alpha0(oracle, gs4d, rec3, 0.0)
        want = np.zeros(cc.N, bool)
        want[idx] = True
        assert np.array_equal(zero, valid & want), make.__name__
        assert zero.any() and (valid & ~zero).any(), make.__name__
    rec3, idx = cc.big_footprints(gs4d)
    _, _, p = alpha0(oracle, gs4d, rec3, 0.0)
    hx, hy = p["hx"][5:7], p["hy"][5:7]
    assert (p["valid"][5:7] != 0).all() and ((1.5 * hx // cc.TILE) * (1.5 * hy // cc.TILE) > 16).all(), (hx, hy)      # (three quarters of the quad's box: what the tightened rectangle keeps at least)


# ---- the containment check ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=("plain", "asan_ubsan"))
def check_program(request, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("footprint_rect_check") / "footprint_rect_check"
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    cc_ = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *san, os.path.join(ROOT, "tests", "footprint_rect_check.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-3000:]
    return str(exe)


def benchmark_quads(gs4d, oracle, n=60_000, w=1920, h=1080):
    """a cut of the benchmark's static cube as the checker projects it: e0 e1 s0 s1 sx sy cx cy of every valid record"""
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    view, proj = cc.mats(gs4d, w, h)
    p = oracle.preprocess(oracle.MODE_4D, rec, view, proj, w, h, 0.0, 0.0)
    p = p[p["valid"] != 0]
    pr = np.asarray(proj, np.float32).reshape(-1)
    sx, sy = np.float32(pr[0]) * np.float32(w * 0.5), np.float32(pr[5]) * np.float32(h * 0.5)
    out = np.stack([p["e0x"], p["e0y"], p["e1x"], p["e1y"], p["s0"], p["s1"], np.full(p.size, sx, np.float32), np.full(p.size, sy, np.float32), p["cx"], p["cy"]], 1)
    return np.ascontiguousarray(out, np.float32)


def test_no_accepted_pixel_lies_outside_the_new_rectangle(gs4d, oracle, check_program, tmp_path):
    quads = benchmark_quads(gs4d, oracle)
    assert quads.shape[0] > 50_000
    path = tmp_path / "quads.bin"
    quads.tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([check_program, str(path)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = {ln.split(":")[0]: ln for ln in r.stdout.splitlines()}
    assert set(lines) == {"benchmark", "seeded, 0.01 .. 16 px", "seeded, 16 .. 2000 px"}
    records = 0
    for name, ln in lines.items():
        m = re.search(r"(\d+) records \((\d+) tightened\), entries (\d+) -> (\d+) .* candidate pixels (\d+) -> (\d+) .* (\d+) accepted pixels, (\d+) violations", ln)
        assert m, ln
        nrec, tight, e0, e1, p0, p1, acc, bad = map(int, m.groups())
        assert bad == 0 and acc > 0 and tight > 0 and e1 <= e0 and p1 <= p0, ln
        records += nrec
        if name == "benchmark":
            assert nrec == quads.shape[0] and e1 < e0 and p1 < p0, ln           # the rectangle saves entries and candidate pixels on the benchmark's own set
    assert records >= 1_000_000 + quads.shape[0]
