"""The segment-fed depth sort of a staged, fused frame (csrc/preprocess.hip: k_project_count<SRC, Stage, SegmentFed> writes every segment's (key, index)
pairs grouped by top digit; csrc/sort.hip: k_os_tail<LB, true> gathers its bucket from the segments' runs, no k_os_pass launch), through the C ABI.

Every case draws frames as the reference's loop does — Clear -> key loop -> sort -> Draw, the draw executing the key generation and the sort — on
contexts with GS4D_SORT_HYBRID=1 GS4D_SORT_SEGFEED=1 (small sets qualify) and on contexts with GS4D_SORT_SEGFEED=0, the two-launch hybrid.

Bar: keys, permutation and image of every frame equal those of GS4D_SORT_SEGFEED=0 bit for bit; keys and permutation equal the stable sort
(sort_cases.reference) of the keys oracle.keygen computes, element for element; the image is the CPU renderer's (oracle.render_4d) within 1e-4.
Proof of path: the statistics' change over a frame — staged_draws + 1, fused_keygen_draws + 1, hybrid_sorts + 1, sort_launches + 1 — names it a
staged, fused, segment-fed frame; a case none of whose judged frames is one fails.
"""
import numpy as np
import pytest

import scenes
import sort_cases
import staged_cases as stc
from hybrid_cases import KEY_LO, _uniform
from test_gpu_paths import _ctx
from test_gpu_staged_misses import Run, reference as unstaged_reference, premise, same

pytestmark = pytest.mark.gpu

TOL = 1e-4
SEG = 2048                                                   # records of a staged segment (tile_lists_plan), pairs of a segment block
ON = {"GS4D_SORT_HYBRID": 1, "GS4D_SORT_SEGFEED": 1}
OFF = {"GS4D_SORT_HYBRID": 1, "GS4D_SORT_SEGFEED": 0}
# The cube scene's splats pile up on the tiles at the cube's centre (9192 records: a list of 1300 entries, 30000: 4427): more than the 1024 entries a
# tile list holds, and such a frame is drawn in instance order, never staged.  64 depth slabs per tile keep every sub-list short enough.
SLABS = {"GS4D_SLABS": 64}
CLEARED = ("GS4D_SLABS", "GS4D_SORT_TAILCAP", "GS4D_STAGED", "GS4D_NB", "GS4D_LANES", "GS4D_SORT_SEGFEED", "GS4D_SORT_HYBRID")


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------------
class Scene:
    """records, camera, image size, time — and what the checkers expect of a frame (computed once per scene)"""

    def __init__(self, gs4d, oracle, rec, cam, w, h, t):
        self.rec, self.cam, self.w, self.h, self.t, self.n = rec, cam, w, h, t, rec.shape[0]
        self.view, self.proj = gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, w, h, scenes.ZNEAR, scenes.ZFAR)
        _, ek = oracle.keygen(rec, t, np.array(cam[0], np.float32))
        self.keys = ek.view(np.uint32)
        self.want = sort_cases.reference(self.keys, np.arange(self.n, dtype=np.uint32))
        self.eimg, eperm, _ = oracle.render_4d(rec, True, t, 0.0, cam[0], self.view, self.proj, w, h)
        assert np.array_equal(eperm, self.want[1])           # the two checkers agree
        assert float(np.abs(self.eimg - np.array(gs4d.CLEAR_COLOR, np.float32)).max()) > 0.05, "empty frame"


def cube_scene(gs4d, oracle, n):
    """test_gpu_sort_hybrid.py::test_fused_frame_path's: cube_params_4d seen from three times CAM_CUBE's distance at t = 25 (a proven span of 24 bits),
    320 x 180, the splats 30 times their size"""
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)
    rec = gs4d.build_records_4d(pos4, q, scale * 30.0, life, fade, vel, rgba)
    cam = (tuple(3.0 * v for v in scenes.CAM_CUBE[0]), scenes.CAM_CUBE[1])
    return Scene(gs4d, oracle, rec, cam, 320, 180, 25.0)


SHELL_W, SHELL_H = 640, 360
SHELL_CAM = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))


def shell_scene(gs4d, oracle, key_bits, seed):
    """Static records whose keys are (about) the float bit patterns key_bits, as hybrid_cases._records builds them — record i at distance
    1 / key_i from a camera at the origin — but dealt over the image instead of along one axis: record i lies on the ray through a pixel
    of its own, so that the set can be drawn with short tile lists.  Footprints of about two pixels whatever the distance."""
    n = len(key_bits)
    rng = np.random.default_rng(seed)
    proj = gs4d.perspective(scenes.FOV, SHELL_W, SHELL_H, scenes.ZNEAR, scenes.ZFAR)
    d = (np.float32(1.0) / np.asarray(key_bits, np.uint32).view(np.float32)).astype(np.float64)
    cell = (np.arange(n) * 1031) % (SHELL_W * SHELL_H // 4)                  # a pixel pair of its own per record while n allows, round the image
    px = (cell % (SHELL_W // 2)) * 2.0 + 1.0 + rng.uniform(-0.4, 0.4, n)
    py = (cell // (SHELL_W // 2)) * 2.0 + 1.0 + rng.uniform(-0.4, 0.4, n)
    ray = np.stack([(px * 2.0 / SHELL_W - 1.0) / proj[0], (py * 2.0 / SHELL_H - 1.0) / proj[5], -np.ones(n)], 1)
    pos = ray / np.linalg.norm(ray, axis=1)[:, None] * d[:, None]
    pos4 = np.concatenate([pos, np.zeros((n, 1))], 1).astype(np.float32)
    q = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1))
    s = (0.004 * d).astype(np.float32)
    rgba = np.concatenate([rng.uniform(0.0, 1.0, (n, 3)), rng.uniform(0.3, 0.9, (n, 1))], 1).astype(np.float32)
    rec = gs4d.build_records_4d(pos4, q, np.stack([s, s, s], 1), np.ones(n, np.float32), np.full(n, 0.5, np.float32), np.zeros((n, 3), np.float32), rgba)
    return Scene(gs4d, oracle, rec, SHELL_CAM, SHELL_W, SHELL_H, 0.0)


def proven(gs4d, sc):
    """(bias, key bits) the library proves for the scene's buffer: from the box of its positions (shell scenes: static, mu_t = 0, no velocity)"""
    lo7, hi7 = np.zeros(7, np.float32), np.zeros(7, np.float32)
    lo7[:3], hi7[:3] = sc.rec[:, :3].min(0), sc.rec[:, :3].max(0)
    bias, span = gs4d.key_bounds(lo7, hi7, sc.t, sc.cam[0])
    return bias, max(1, int(span).bit_length())


def top_counts(gs4d, sc):
    bias, bits = proven(gs4d, sc)
    assert 19 <= bits <= 27 and sc.keys.min() >= bias, (bias, bits)
    return np.bincount((sc.keys - np.uint32(bias)) >> np.uint32(bits - 9), minlength=512)


# ---- frames -------------------------------------------------------------------------------------------------------------------------------------------
PATH_KEYS = ("staged_draws", "fused_keygen_draws", "reruns", "staged_misses")


def path_stats(ctx):
    st, ss = ctx.stats(), ctx.sort_stats()
    return {**{k: st[k] for k in PATH_KEYS}, "hybrid_sorts": ss["hybrid_sorts"], "sort_launches": ss["sort_launches"]}, ss


def segment_fed(d):
    return d["staged_draws"] == 1 and d["fused_keygen_draws"] == 1 and d["hybrid_sorts"] == 1 and d["sort_launches"] == 1


class Frames:
    """one context; frame(scene) -> (keys, permutation, image, change of the path statistics, the sort report)"""

    def __init__(self, gs4d, monkeypatch, w, h, env, **more):
        for k in CLEARED:
            monkeypatch.delenv(k, raising=False)
        self.gs4d = gs4d
        self.ctx = _ctx(gs4d, w, h, monkeypatch, **{k: v for k, v in {**env, **more}.items() if v is not None})
        self.ctx.set_clear_color(gs4d.CLEAR_COLOR)
        self.lanes = self.ctx.stats()["lanes"]
        self.bufs = {}

    def frame(self, sc):
        c, n = self.ctx, sc.n
        if id(sc) not in self.bufs:
            self.bufs[id(sc)] = (c.buffer(sc.rec), c.buffer(nbytes=4 * n), c.buffer(nbytes=4 * n))
        db, kb, ib = self.bufs[id(sc)]
        before, _ = path_stats(c)
        c.clear()
        c.set_uniforms(time=sc.t, min_opacity=0.0, view=sc.view, proj=sc.proj)
        c.keygen(db, sc.t, sc.cam[0], kb, ib, n)
        c.sort_pairs(kb, ib, n)
        c.set_mode(self.gs4d.MODE_4D_SORTED)
        c.bind(1, ib)
        c.bind(2, db)
        c.draw_instanced(n)
        img = c.read_pixels()
        k, p = c.read(kb, np.uint32, n), c.read(ib, np.uint32, n)
        after, report = path_stats(c)
        return k, p, img, {key: after[key] - before[key] for key in after}, report

    def close(self):
        self.ctx.finish()
        self.ctx.close()


def judge(sc, new, old, what):
    """one frame of both settings against the checkers and against each other"""
    (k, p, img, d, _), (k0, p0, img0, d0, _) = new, old
    for name, got, want in (("keys", k, sc.want[0]), ("permutation", p, sc.want[1])):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}, {name}: {bad.size} of {sc.n} slots differ from the stable sort, the first at {int(bad[0])}: got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x} ({d})"
    err = float(np.abs(img.astype(np.float64) - sc.eimg).max())
    assert err <= TOL, f"{what}: Linf against the CPU renderer = {err:.3e}"
    assert np.array_equal(k, k0) and np.array_equal(p, p0) and same(img, img0), f"{what}: differs from the frame of GS4D_SORT_SEGFEED=0"
    assert d0["sort_launches"] == 2 * d0["hybrid_sorts"] or d0["hybrid_sorts"] == 0, d0      # never segment-fed


def run_both(gs4d, monkeypatch, sc, frames=None, **more):
    """`frames` frames (default 2 * lanes + 4: both histogram slots, every frame lane) of the scene under both settings, each judged; -> the changes
    of the path statistics of the segment-fed context's frames, its last sort report (the largest bucket of any lane's latest report, the slow buckets of
    every lane's latest report added up) and the number of frame lanes"""
    out = []
    for env in (ON, OFF):
        f = Frames(gs4d, monkeypatch, sc.w, sc.h, env, **more)
        try:
            out.append([f.frame(sc) for _ in range(frames or 2 * f.lanes + 4)])
        finally:
            f.close()
    for j, (new, old) in enumerate(zip(*out)):
        judge(sc, new, old, f"frame {j}")
    deltas = [fr[3] for fr in out[0]]
    print("path statistics per frame:", deltas)
    assert any(segment_fed(d) for d in deltas), f"no frame was a staged, fused, segment-fed frame: {deltas}"
    return deltas, out[0][-1][4], f.lanes


# ---- 1. segment counts and ragged ends ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SEG, SEG + 1, 4 * SEG + 1000, 30000])
def test_segment_counts_and_ragged_ends(gs4d, oracle, monkeypatch, n):
    """one full segment; a last segment of one record; a last segment of 1000; test_fused_frame_path's 30000 (15 segments, the last of 1328)"""
    deltas, report, _ = run_both(gs4d, monkeypatch, cube_scene(gs4d, oracle, n), **(SLABS if n > SEG + 1 else {}))
    assert report["slow_buckets"] == 0
    assert all(d["hybrid_sorts"] >= 1 for d in deltas)       # a 24-bit span: every sort the hybrid, segment-fed or not


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------------------------------------
def test_ties_across_and_inside_segments(gs4d, oracle, monkeypatch):
    """3000 records ten times each: four copies 3000 records apart (always in different segments), three 300 apart (different waves of a segment: a
    wave owns 256 consecutive records), three next to one another (one wave, but for the pairs a wave's end cuts)"""
    first = cube_scene(gs4d, oracle, 3000)
    base = first.rec
    a = np.tile(np.arange(3000), 4)
    b = np.tile(np.arange(3000).reshape(10, 300), (1, 3)).ravel()
    c = np.repeat(np.arange(3000), 3)
    order = np.concatenate([a, b, c])
    assert order.size == 30000 and (np.bincount(order) == 10).all()
    sc = Scene(gs4d, oracle, np.ascontiguousarray(base[order]), first.cam, first.w, first.h, first.t)
    assert (np.bincount(np.unique(sc.keys, return_inverse=True)[1]) % 10 == 0).all()      # every key occurs (a multiple of) 10 times
    seg, wave = np.arange(30000) // SEG, np.arange(30000) // 256
    by = np.argsort(order, kind="stable").reshape(3000, 10)                                # the ten places of every base record
    assert (np.diff(seg[by[:, :4]], axis=1) > 0).all()
    assert ((np.diff(seg[by[:, 4:7]], axis=1) == 0) & (np.diff(wave[by[:, 4:7]], axis=1) > 0)).all(axis=1).sum() > 1500      # (the rest: a segment's end between them)
    assert (np.diff(wave[by[:, 7:]], axis=1) == 0).all(axis=1).sum() > 2000
    run_both(gs4d, monkeypatch, sc, **SLABS)


# ---- 3. top digits partly used ----------------------------------------------------------------------------------------------------------------------------
def test_top_digits_partly_used_and_empty_runs(gs4d, oracle, monkeypatch):
    """test_top_digits_partly_used's keys (a span of 66 % of 2^24), drawn: most top digits hold nothing, and in the used ones the 35 segments' runs are
    a few pairs each, some empty"""
    n, span = 70001, int(0.66 * (1 << 24))
    sc = shell_scene(gs4d, oracle, _uniform(n, span, 66), 66)
    tc = top_counts(gs4d, sc)
    assert 20 < np.count_nonzero(tc) < 400 and tc.max() <= 8192, (np.count_nonzero(tc), tc.max())
    deltas, report, _ = run_both(gs4d, monkeypatch, sc, frames=6)
    assert report["slow_buckets"] == 0 and report["largest_bucket"] == tc.max()


# ---- 4. a bucket above the capacity ----------------------------------------------------------------------------------------------------------------------
def crowded_keys(n, share, seed):
    """`share` of the keys within 2^10 bit patterns of one another, the rest uniform over a 24-bit span"""
    keys = _uniform(n, (1 << 24) - (1 << 19), seed)
    rng = np.random.default_rng(seed + 1)
    m = int(n * share)
    keys[rng.choice(n, m, replace=False)] = (KEY_LO + (200 << 15) + (1 << 13) + rng.integers(0, 1 << 10, m, dtype=np.int64)).astype(np.uint32)
    return keys, m


def test_a_bucket_above_the_capacity(gs4d, oracle, monkeypatch):
    """GS4D_SORT_TAILCAP=2048 and 40 % of 20000 records at nearly one depth: that bucket is gathered into its range of scratch 1 and sorted by the
    slow path, in 8192-key chunks"""
    keys, m = crowded_keys(20000, 0.4, 3)
    sc = shell_scene(gs4d, oracle, keys, 4)
    tc = top_counts(gs4d, sc)
    assert tc.max() >= m > 2048 and np.count_nonzero(tc > 2048) == 1, (tc.max(), m)
    deltas, report, lanes = run_both(gs4d, monkeypatch, sc, frames=6, GS4D_SORT_TAILCAP=2048)
    assert report["slow_buckets"] == min(6, lanes) and report["largest_bucket"] == tc.max()      # one slow bucket in the latest report of every lane that sorted


def test_every_bucket_above_a_capacity_of_one(gs4d, oracle, monkeypatch):
    """GS4D_SORT_TAILCAP=1 at n = 2049: every bucket of two keys or more takes the slow path behind the gather"""
    sc = cube_scene(gs4d, oracle, SEG + 1)
    deltas, report, _ = run_both(gs4d, monkeypatch, sc, frames=6, GS4D_SORT_TAILCAP=1)
    assert report["slow_buckets"] >= 1


# ---- 5. a staged miss in a segment-fed frame --------------------------------------------------------------------------------------------------------------
def knobs(monkeypatch, env):
    for k in CLEARED:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def test_a_staged_miss_in_a_segment_fed_frame(gs4d, oracle, monkeypatch):
    """case a of test_gpu_staged_misses.py: the last segment outgrows its block.  Its depth block and its row of the run table are written all the
    same, the sort behind the aborted draw sorts the caller's buffers, the draw is re-run with exact lists (which read no key from those buffers)"""
    rec, times = stc.build(gs4d, "a")
    knobs(monkeypatch, ON)
    warm, loads, eimgs, _ = unstaged_reference(gs4d, rec, times, monkeypatch, None)
    premise("a", warm, loads, times)
    got = {}
    for name, env in (("on", ON), ("off", OFF)):
        knobs(monkeypatch, env)
        run = Run(gs4d, rec, monkeypatch, staged=True, lanes=None)
        try:
            s0 = run.warm_up()
            b, _ = path_stats(run.ctx)
            run.frame(stc.T1)
            img = run.ctx.read_pixels()
            keys, perm = run.ctx.read(run.keys, np.uint32, run.n), run.ctx.read(run.idx, np.uint32, run.n)
            a, _ = path_stats(run.ctx)
            got[name] = (keys, perm, img, {k: a[k] - b[k] for k in a})
        finally:
            run.close()
    keys, perm, img, d = got["on"]
    print("the miss frame:", d, "without segment blocks:", got["off"][3])
    # the staged run (segment-fed: one launch) and its exact re-run, which finds the keys written and the sort queued: no second sort
    assert d == {"staged_draws": 1, "fused_keygen_draws": 1, "reruns": 1, "staged_misses": 1, "hybrid_sorts": 1, "sort_launches": 1}, d
    assert got["off"][3] == {**d, "sort_launches": 2}, got["off"][3]
    assert same(img, eimgs[0]), "the miss frame differs from the frame without staged lists"
    eimg, eperm, ekeys = oracle.render_4d(rec, True, stc.T1, 0.0, stc.CAM[0], run.view, run.proj, stc.W, stc.H)
    _, ek = oracle.keygen(rec, stc.T1, np.array(stc.CAM[0], np.float32))
    want = sort_cases.reference(ek.view(np.uint32), np.arange(run.n, dtype=np.uint32))
    assert np.array_equal(perm, eperm) and np.array_equal(perm, want[1]) and np.array_equal(keys, want[0])
    assert np.abs(img.astype(np.float64) - eimg).max() <= TOL
    assert np.array_equal(keys, got["off"][0]) and np.array_equal(perm, got["off"][1]) and same(img, got["off"][2])


def test_frames_queued_behind_a_miss(gs4d, oracle, monkeypatch):
    """case f: the miss frame and the frames behind it are queued before anything is read — every one staged with the old guesses, segment-fed, aborted
    and re-run.  The last frame read must be the frame without staged lists, its buffers sorted."""
    rec, times = stc.build(gs4d, "f")
    knobs(monkeypatch, ON)
    run = Run(gs4d, rec, monkeypatch, staged=True, lanes=None)
    lanes = run.lanes
    run.close()
    j = max(1, min(lanes - 1, len(times) - 1))
    knobs(monkeypatch, ON)
    warm, loads, eimgs, _ = unstaged_reference(gs4d, rec, times[:j + 1], monkeypatch, None)
    premise("f", warm, loads, times[:j + 1])
    got = {}
    for name, env in (("on", ON), ("off", OFF)):
        knobs(monkeypatch, env)
        run = Run(gs4d, rec, monkeypatch, staged=True, lanes=None)
        try:
            run.warm_up()
            b, _ = path_stats(run.ctx)
            for t in times[:j + 1]:
                run.frame(t)
            img = run.ctx.read_pixels()
            keys, perm = run.ctx.read(run.keys, np.uint32, run.n), run.ctx.read(run.idx, np.uint32, run.n)
            a, _ = path_stats(run.ctx)
            got[name] = (keys, perm, img, {k: a[k] - b[k] for k in a})
        finally:
            run.close()
    keys, perm, img, d = got["on"]
    print(f"{lanes} lanes, {j + 1} frames queued:", d)
    assert d["hybrid_sorts"] == d["sort_launches"] == d["fused_keygen_draws"] == j + 1 and d["staged_misses"] >= 1, d
    assert got["off"][3]["sort_launches"] == 2 * (j + 1), got["off"][3]
    assert same(img, eimgs[j]), f"frame {j} differs from the frame without staged lists"
    _, ek = oracle.keygen(rec, times[j], np.array(stc.CAM[0], np.float32))
    want = sort_cases.reference(ek.view(np.uint32), np.arange(run.n, dtype=np.uint32))
    assert np.array_equal(keys, want[0]) and np.array_equal(perm, want[1])
    eimg, _, _ = oracle.render_4d(rec, True, times[j], 0.0, stc.CAM[0], run.view, run.proj, stc.W, stc.H)
    assert np.abs(img.astype(np.float64) - eimg).max() <= TOL
    assert np.array_equal(keys, got["off"][0]) and np.array_equal(perm, got["off"][1]) and same(img, got["off"][2])


# ---- 6. fallback and return -----------------------------------------------------------------------------------------------------------------------------
def test_fallback_to_lsd_passes_and_return(gs4d, oracle, monkeypatch):
    """As test_feedback_falls_back_and_returns, in frames: a crowded set (a bucket above the 8192-key tile) is segment-fed with a slow bucket until its
    report reaches the host, then sorted by LSD passes; a spread set brings the segment-fed sort back.  Every sort exact."""
    n = 30000
    keys, m = crowded_keys(n, 0.4, 7)
    crowded, spread = shell_scene(gs4d, oracle, keys, 8), shell_scene(gs4d, oracle, _uniform(n, (1 << 24) - (1 << 19), 9), 10)
    assert top_counts(gs4d, crowded).max() >= m > 8192 and top_counts(gs4d, spread).max() <= 8192
    out = {}
    for name, env in (("on", ON), ("off", OFF)):
        f = Frames(gs4d, monkeypatch, SHELL_W, SHELL_H, env)
        try:
            k = 2 * f.lanes + 4
            out[name] = [f.frame(crowded) for _ in range(k)] + [f.frame(spread) for _ in range(k)]
        finally:
            f.close()
    for j, (new, old) in enumerate(zip(out["on"], out["off"])):
        judge(crowded if j < k else spread, new, old, f"frame {j}")
    deltas = [fr[3] for fr in out["on"]]
    print("crowded:", deltas[:k], "\nspread:", deltas[k:])
    assert any(segment_fed(d) for d in deltas[:k]), "the crowded set was never segment-fed"
    assert deltas[k - 1]["hybrid_sorts"] == 0 and deltas[k - 1]["sort_launches"] == 3 + 1, "the plan did not fall back to the LSD passes"      # three passes and the report
    assert all(segment_fed(d) for d in deltas[-2:]), "the plan did not return to the segment-fed sort"


# ---- 7. the knob --------------------------------------------------------------------------------------------------------------------------------------------
def test_an_explicit_hybrid_knob_alone_keeps_the_two_launch_hybrid(gs4d, oracle, monkeypatch):
    """GS4D_SORT_SEGFEED unset with GS4D_SORT_HYBRID=1: the plans exactly as they were — hybrid sorts of two launches, staged or not"""
    sc = cube_scene(gs4d, oracle, 30000)
    f = Frames(gs4d, monkeypatch, sc.w, sc.h, {"GS4D_SORT_HYBRID": 1}, **SLABS)
    try:
        frames = [f.frame(sc) for _ in range(4)]
    finally:
        f.close()
    for j, (k, p, img, d, _) in enumerate(frames):
        assert np.array_equal(k, sc.want[0]) and np.array_equal(p, sc.want[1]), f"frame {j}"
        assert float(np.abs(img.astype(np.float64) - sc.eimg).max()) <= TOL
        # (a draw that overflows its tile lists and is re-run in instance order regenerates its order with a sort of its own, of the same kind)
        assert d["hybrid_sorts"] >= 1 and d["sort_launches"] == 2 * d["hybrid_sorts"] and (d["hybrid_sorts"] == 1 or d["reruns"]), (j, d)
    assert any(d["staged_draws"] == 1 for *_, d, _ in frames), "no frame was staged"
