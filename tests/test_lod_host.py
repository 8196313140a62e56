"""CPU: the host side of gs4d_lod_append and gs4d_lod_cut (include/gs4d.h) — gs4d_host_lod_cut against the header's text restated in
numpy (tests/lod_cases.py: float32, one numpy call per operation; every word as uint32), the property that every chain of parent links draws exactly
one node, the text that the kernel and the host function share (csrc/lod_query.h) compiled stand-alone with g++ against the host function, every
refusal of the two calls through the checks the library makes before it queues anything (csrc/lod_operands.h under csrc/operands.h), and the ABI."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import lod_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


def forests(gs4d):
    """(what, rec, parent, level_first) of every forest the tests of the call use: the sets over leaf counts and level counts around the tiles, the
    skipped waves, the hostile parent words"""
    for call, leaves in enumerate(lc.LEAVES):
        which, levels = lc.SETS[call % 4], lc.LEVELS[call % 4]
        yield (f"{which}, {leaves} leaves, {levels} levels",) + lc.random_forest(gs4d, which, leaves, levels, call)
    for which in lc.SETS:
        yield (f"{which}, 300 leaves, 16 levels",) + lc.random_forest(gs4d, which, 300, 16, 77, fan=2)
        yield (f"{which}, 2049 leaves, 5 levels",) + lc.random_forest(gs4d, which, 2049, 5, 78)
    yield ("skipped waves",) + lc.skipped_wave_forest(gs4d)[:3]
    yield ("a skipped wave next to a tested one",) + lc.skipped_wave_forest(gs4d, fill=True)[:3]
    yield ("hostile parents",) + lc.hostile_parent_forest(gs4d)


def queries(rec):
    """(ratio, near) of a forest: 0, +inf and a middle value; no near distance and one above every distance"""
    mid = lc.middle_ratio(rec, lc.EYE, lc.T)
    return ((0.0, 0.0), (np.inf, 0.0), (mid, 0.0), (mid, 1e30), (1.0, 0.0))


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------
def test_the_host_function_is_the_headers_text(gs4d):
    drawn = stopped = descended = inner = 0
    for what, rec, parent, first in forests(gs4d):
        n = rec.shape[0]
        stats = lc.stats_table(gs4d, n, n)
        for call, (ratio, near) in enumerate(queries(rec)):
            cap = (None, 7, 0)[call % 3]
            q = gs4d.lod_query(first, lc.EYE, lc.T, ratio, near)
            dst, index, table, count = gs4d.lod_cut_host(rec, parent, q, capacity=cap, stats=stats)
            wdst, windex, wtable, wcount, state = lc.cut_by_the_text(rec, parent, first, lc.EYE, lc.T, ratio, near, cap, stats)
            where = f"{what}, ratio {ratio}, near {near}, capacity {cap}"
            assert tuple(int(v) for v in count) == wcount, where
            w = wcount[1]
            assert np.array_equal(lc.bits(dst[:w]), lc.bits(wdst)) and np.array_equal(index[:w], windex), where
            assert not dst[w:].any() and not index[w:].any(), f"{where}: slots at or beyond `written` were written"
            assert np.array_equal(table.view(u32), wtable.view(u32)), f"{where}: stats"
            assert lc.chains_draw_once(parent, first, state) == first[1]
            if ratio == 0.0 and len(first) > 2:
                assert wcount[3] <= wcount[0]
            drawn, stopped, descended = drawn + wcount[0], stopped + int((state == lc.STOP).sum()), descended + int((state == lc.DESCEND).sum())
            inner += wcount[0] - wcount[3]
    assert drawn > 10000 and stopped > 10000 and descended > 1000 and inner > 1000


def test_the_extremes_of_the_ratio_and_the_near_distance(gs4d):
    rec, parent, first = lc.random_forest(gs4d, "4d_vel", 769, 5, 3)
    n = first[-1]
    level = np.searchsorted(np.asarray(first[1:]), np.arange(n), side="right")
    child = (parent.astype(np.int64) >= np.asarray(first)[level + 1]) & (parent.astype(np.int64) < n)
    # ratio 0: nothing with a positive extent is fine, so every chain ends at its leaf — and a root above the leaves is never drawn
    _, index, _, count = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, lc.EYE, lc.T, 0.0))
    assert (rec[:, [8, 13, 18]].max(1) > 0).all()
    assert tuple(int(v) for v in count) == (first[1], first[1], n, first[1]) and np.array_equal(index[:first[1]], np.arange(first[1]))
    # ratio +inf: everything is fine, the cut is the roots
    _, index, _, count = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, lc.EYE, lc.T, np.inf))
    roots = np.flatnonzero(~child)
    assert int(count["drawn"]) == roots.size == int(count["tested"]) and np.array_equal(index[:roots.size], roots)
    # a near distance above every distance: the cut no longer depends on the eye
    mid = lc.middle_ratio(rec, lc.EYE, lc.T)
    a = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, lc.EYE, lc.T, mid * 1e-3, 1e3))
    b = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, (-7.0, 9.0, -2.0), lc.T, mid * 1e-3, 1e3))
    assert np.array_equal(a[1], b[1]) and a[3] == b[3] and 0 < int(a[3]["drawn"])
    # a single level: the cut is the set itself, whatever the parent words say
    one = [0, n]
    dst, index, _, count = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(one, lc.EYE, lc.T, np.inf))
    assert tuple(int(v) for v in count) == (n, n, n, n) and np.array_equal(lc.bits(dst), lc.bits(rec)) and np.array_equal(index, np.arange(n))


def test_extents_that_do_not_grow_towards_the_root(gs4d):
    """leaf -> parent -> grandparent, one chain per case: the topmost fine node is drawn"""
    first = lc.firsts([4, 4, 4])
    rec = lc.sized_record(gs4d, 12, lc.LARGE)
    parent = np.r_[np.arange(4, 8), np.arange(8, 12), [lc.ID_NONE] * 4].astype(u32)
    # chain 0: only the grandparent is fine; 1: the parent is fine, the grandparent is not, the leaf is; 2: grandparent fine and parent not; 3: none
    rec[8, [8, 13, 18]] = lc.SMALL
    rec[[5, 1], 8:19:5] = lc.SMALL
    rec[10, [8, 13, 18]] = lc.SMALL
    _, index, _, count = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, lc.EYE, lc.T, 1.0))
    assert index[:4].tolist() == [3, 5, 8, 10] and tuple(int(v) for v in count) == (4, 4, 4 + 2 + 1, 1)
    # one variance alone decides: the largest of the three
    rec[8, 13] = lc.LARGE
    assert gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, lc.EYE, lc.T, 1.0))[1][:4].tolist() == [0, 3, 5, 10]


def test_hostile_parent_words_are_data(gs4d):
    rec, parent, first = lc.hostile_parent_forest(gs4d)
    n = first[-1]
    _, index, _, count = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, lc.EYE, lc.T, 1.0))
    # nothing is fine: every valid link is followed, every leaf is drawn and every node tested
    assert tuple(int(v) for v in count) == (300, 300, n, 300) and np.array_equal(index[:300], np.arange(300))
    # everything is fine: the roots — the whole top level, the six hostile words of level 1, five of the seven of level 0
    _, index, _, count = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, lc.EYE, lc.T, np.inf))
    want = [0, 1, 2, 4, 6] + [first[1], first[1] + 1, first[1] + 2, first[1] + 3, first[1] + 5] + list(range(first[2], n))
    assert index[:int(count["drawn"])].tolist() == want


def test_calls_the_device_would_refuse_write_nothing(gs4d):
    rec, parent, first = lc.random_forest(gs4d, "3d", 65, 2, 1)
    good = gs4d.lod_query(first, lc.EYE, lc.T, 1.0)
    assert int(gs4d.lod_cut_host(rec, parent, good)[3]["drawn"]) > 0
    bad = []
    for field, value in (("levels", 0), ("levels", 17), ("flags", 1), ("ratio", np.nan), ("ratio", -1.0), ("near_dist", np.inf), ("near_dist", np.nan),
                         ("near_dist", -0.5)):
        q = gs4d.lod_query(first, lc.EYE, lc.T, 1.0)
        setattr(q, field, value)
        bad.append((f"{field} = {value}", q))
    for k, v in ((0, 1), (1, first[2] + 1), (2, first[2] - 1), (2, first[2] + 1)):
        q = gs4d.lod_query(first, lc.EYE, lc.T, 1.0)
        q.level_first[k] = v
        bad.append((f"level_first[{k}] = {v}", q))
    for r in range(3):
        q = gs4d.lod_query(first, lc.EYE, lc.T, 1.0)
        q.reserved[r] = 1
        bad.append((f"reserved[{r}]", q))
    for what, q in bad:
        dst, index, table, count = gs4d.lod_cut_host(rec, parent, q)
        assert not dst.any() and not index.any() and not table.view(u32).any() and tuple(count) == (0, 0, 0, 0), what
    count = np.full(4, 7, u32)
    gs4d._lib.gs4d_host_lod_cut(first[-1], gs4d._ptr(rec), gs4d._ptr(parent), None, None, None, None, gs4d._ptr(count), 5)
    assert count.tolist() == [7, 7, 7, 7]                                             # q == NULL
    gs4d._lib.gs4d_host_lod_cut(first[-1], gs4d._ptr(rec), gs4d._ptr(parent), ctypes.byref(good), None, None, None, gs4d._ptr(count), 5)
    assert count[0] > 0 and count[1] == min(count[0], 5)                              # dst, cut_index and stats are optional
    empty = gs4d.lod_cut_host(np.zeros((0, 24), f32), np.zeros(0, u32), gs4d.lod_query([0, 0, 0], lc.EYE, lc.T, 1.0))
    assert tuple(empty[3]) == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        gs4d.lod_cut_host(rec, parent[:5], good)
    with pytest.raises(ValueError):
        gs4d.lod_query([0] * 18, lc.EYE, lc.T, 1.0)


def test_lod_ratio(gs4d):
    # 3 standard deviations of a node of variance 4 at distance 100 under a 90 degree field of view, 1000 pixels high: 3 * 2 / 100 * 500 = 30 pixels
    r = gs4d.lod_ratio(90.0, 1000, 30.0)
    assert abs(r - 2.0 / 100.0) < 1e-12
    assert abs(gs4d.lod_ratio(90.0, 1000, 30.0, sigmas=1.0) - 3 * r) < 1e-12 and gs4d.lod_ratio(60.0, 1080, 0.0) == 0.0


# ---- the kernel's text on the CPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=("plain", "asan_ubsan"))
def check_program(request, tmp_path_factory):
    """the stand-alone program, built plainly and as an executable instrumented with AddressSanitizer + UndefinedBehaviorSanitizer (nothing is preloaded)"""
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("lod_query_check") / "lod_query_check"
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", *san, os.path.join(ROOT, "tests", "lod_query_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return str(exe)


ENV = dict(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_the_kernels_text_gives_the_host_functions_words_on_the_cpu(gs4d, check_program, tmp_path):
    env = dict(os.environ, **ENV)
    paths = [tmp_path / f for f in ("query.bin", "nodes.bin", "parent.bin", "dst.bin", "index.bin", "state.bin", "count.bin")]
    hostile = 0
    for what, rec, parent, first in forests(gs4d):
        if not (what.startswith("hostile") or "hostile parents" in what or "skipped" in what or "2049" in what):
            continue
        n = rec.shape[0]
        rec.tofile(paths[1])
        parent.tofile(paths[2])
        for call, (ratio, near) in enumerate(queries(rec)):
            cap = (n, 7)[call % 2]
            q = gs4d.lod_query(first, lc.EYE, lc.T, ratio, near)
            paths[0].write_bytes(bytes(q))
            r = subprocess.run([check_program, str(n), *map(str, paths[:3]), str(cap), *map(str, paths[3:])], capture_output=True, text=True, timeout=120, env=env)
            assert r.returncode == 0, what + "\n" + r.stderr[-3000:]
            dst, index, _, count = gs4d.lod_cut_host(rec, parent, q, capacity=cap)
            w = int(count["written"])
            assert np.array_equal(np.fromfile(paths[6], u32), np.array(tuple(count), u32)), what
            assert np.array_equal(np.fromfile(paths[3], u32), lc.bits(dst[:w]).reshape(-1)) and np.array_equal(np.fromfile(paths[4], u32), index[:w]), what
            state = lc.states_by_the_text(rec, parent, first, lc.EYE, lc.T, ratio, near)[0]
            assert np.array_equal(np.fromfile(paths[5], np.uint8), state), what
        hostile += what.startswith("hostile")
    assert hostile >= 3


def test_every_refusal_through_the_cpu_operand_check(check_program):
    r = subprocess.run([check_program, "refusals"], capture_output=True, text=True, timeout=120, env=dict(os.environ, **ENV))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " cases, 0 failed" in r.stdout


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_the_structures_and_the_abi(gs4d):
    assert ctypes.sizeof(gs4d.LodQuery) == 112 and gs4d.LodQuery.level_first.offset == 32 and gs4d.LodQuery.reserved.offset == 100
    assert gs4d.LOD_COUNT.itemsize == 16 and gs4d.LOD_COUNT.names == ("drawn", "written", "tested", "drawn_leaves")
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert "gs4d_lod_append(gs4d_ctx* ctx, gs4d_buf level, size_t m," in hdr and "gs4d_buf nodes, gs4d_buf parent, size_t first);" in hdr
    assert "gs4d_lod_cut(gs4d_ctx* ctx, gs4d_buf nodes, gs4d_buf parent, size_t n, const gs4d_lod_query* q," in hdr
    assert "gs4d_host_lod_cut(size_t n, const float* records24, const uint32_t* parent, const gs4d_lod_query* q," in hdr
    assert "} gs4d_lod_query;             /* 112 bytes */" in hdr
    internal = open(os.path.join(ROOT, "4dgaussiansplatrendering_amd", "csrc", "gs4d_internal.h")).read()
    assert f"constexpr uint32_t LOD_TILE = {lc.LOD_TILE};" in internal and f"constexpr uint32_t COMPACT_TILE = {lc.COMPACT_TILE};" in internal
    text = open(os.path.join(ROOT, "4dgaussiansplatrendering_amd", "csrc", "lod_query.h")).read()
    assert f"enum : uint8_t {{ STOP = {lc.STOP}, DESCEND = {lc.DESCEND}, DRAW = {lc.DRAW} }};" in text
    assert {"gs4d_lod_append", "gs4d_lod_cut", "gs4d_host_lod_cut"} <= set(gs4d.EXPORTS)
    assert gs4d._lib.gs4d_lod_append(None, 1, 1, 0, 0, 0, 2, 3, 0) == -1              # GS4D_E_INVALID: no context
    assert gs4d._lib.gs4d_lod_cut(None, 1, 2, 1, None, 0, 0, 0, 3) == -1
