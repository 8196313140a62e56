"""The staged projection loads round it + 1's record while it computes round it (csrc/preprocess.hip: k_project_count<SRC, Stage, KEYS>,
load_record / project_record / arrived), through the C ABI, at the ends of segments — where a look-ahead reaches past what a wave or a workgroup
owns.

The static layout's instances are the ones that look ahead (load_ahead); the 96-byte and the symmetric layout run the same loop with the load inside the
round, and are held to the same bar here, so that a look-ahead given to them later meets these cases as they are.

A look-ahead can go wrong in two ways: it reads past the end of the draw (the last plane of a buffer as long as the draw ends exactly there), or a
record that was only looked at is projected, counted or keyed.  EVERY case but the last uploads exactly the n records it draws, so that a look-ahead
without its bound would leave the last plane; the last case draws n records of a longer buffer, where such a read would find live records.

Bar (that of test_gpu_sort_segfeed.py, whose harness this file uses): keys, permutation and image of every frame are bit-identical between the staged
and the unstaged (GS4D_STAGED=0) way of building the lists, and between the segment-fed and the two-launch hybrid frame; keys and permutation equal
the stable sort of the checker's keys; the image is the CPU renderer's within 1e-4.  Proof of path: the statistics' change over a frame names at least
one judged frame of every context a staged frame of the form the case is about, and record_read_bytes names the record layout the projection read.
"""
import copy

import numpy as np
import pytest

import scenes
import staged_cases as stc
from hybrid_cases import _uniform
from test_gpu_paths import _ctx
from test_gpu_sort_segfeed import CLEARED, OFF, ON, SLABS, TOL, Frames, Scene, cube_scene, judge, path_stats, segment_fed, shell_scene
from test_gpu_staged_misses import same

pytestmark = pytest.mark.gpu

FRAMES = 6                                                   # the first frames of a context teach the guesses; test_gpu_sort_segfeed.py's short cases use 6 too
LAYOUT_BYTES = {"full": 96, "static3d": 64, "symmetric": 72}
UNSTAGED = {**ON, "GS4D_STAGED": 0}

_scenes = {}


def scene(gs4d, oracle, layout, n):
    """one scene per (layout, n), its CPU reference computed once: cube_scene's records are the 96-byte layout (sig is not bit-symmetric), the same
    records with the upper triangle of sig mirrored into the lower are the 72-byte symmetric layout, shell_scene's are static 3D (64 bytes)"""
    if (layout, n) not in _scenes:
        if layout == "full":
            sc = cube_scene(gs4d, oracle, n)
        elif layout == "symmetric":
            pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)                 # cube_scene's records, camera, size and time
            rec = gs4d.build_records_4d(pos4, q, scale * 30.0, life, fade, vel, rgba)
            sig = rec[:, 8:].reshape(-1, 4, 4)
            iu = np.triu_indices(4, 1)
            sig[:, iu[0], iu[1]] = sig[:, iu[1], iu[0]]
            assert (sig == sig.transpose(0, 2, 1)).all()
            sc = Scene(gs4d, oracle, rec, (tuple(3.0 * v for v in scenes.CAM_CUBE[0]), scenes.CAM_CUBE[1]), 320, 180, 25.0)
        else:
            sc = shell_scene(gs4d, oracle, _uniform(n, (1 << 24) - (1 << 19), n), n + 1)
        _scenes[(layout, n)] = sc
    return _scenes[(layout, n)]


def knobs_for(layout, lanes):
    return {**(SLABS if layout != "static3d" else {}), **({"GS4D_LANES": lanes} if lanes else {})}


def staged_fused(d):
    return d["staged_draws"] == 1 and d["fused_keygen_draws"] == 1


def sorted_frames(gs4d, monkeypatch, sc, env, more, frames=FRAMES):
    """`frames` frames of one context -> the frames (Frames.frame), the entries statistic after each, the layout the projection read"""
    f = Frames(gs4d, monkeypatch, sc.w, sc.h, env, **more)
    try:
        out, entries = [], []
        for _ in range(frames):
            out.append(f.frame(sc))
            entries.append(f.ctx.stats()["entries"])
        return out, entries, f.ctx.stats()["record_read_bytes"]
    finally:
        f.close()


def run_three(gs4d, monkeypatch, sc, layout, lanes=None):
    """the scene's frames segment-fed, as the two-launch hybrid and with exact (unstaged) lists: each judged, all three equal bit for bit"""
    more = knobs_for(layout, lanes)
    (new, _, b_new), (old, _, b_old), (exact, _, b_exact) = (sorted_frames(gs4d, monkeypatch, sc, env, more) for env in (ON, OFF, UNSTAGED))
    assert b_new == b_old == b_exact == LAYOUT_BYTES[layout], (b_new, b_old, b_exact)
    for j, (a, b, c) in enumerate(zip(new, old, exact)):
        judge(sc, a, b, f"frame {j}")
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and same(a[2], c[2]), f"frame {j}: differs from the frame of GS4D_STAGED=0"
        assert c[3]["staged_draws"] == 0, c[3]
    d_new, d_old = [fr[3] for fr in new], [fr[3] for fr in old]
    print("segment-fed:", d_new, "\ntwo-launch:", d_old)
    assert any(segment_fed(d) for d in d_new), f"no frame was a staged, fused, segment-fed frame: {d_new}"
    assert any(staged_fused(d) and d["sort_launches"] == 2 for d in d_old), f"no two-launch frame was a staged, fused frame: {d_old}"
    return new


# ---- 1. ragged ends at wave granularity ---------------------------------------------------------------------------------------------------------------
# Segment-fed, a wave owns 256 consecutive records in four rounds of 64.  n = 4096 + r is three segments of 1536 (staged_cases.plan): the last holds
# 1024 + r records — waves 0..3 full, wave 4 with r records, wave 5 and the rest with none.  r = 64 exactly: a round that exists and the next that does
# not.  (The same n under GS4D_SORT_SEGFEED=0: round it is records i0 + 512 it + t, the last segment ends r records into its third round.)
# The static layout's instances are the ones that look ahead: they get every r, at the default lane count and (the ends of a round) at one lane.
WAVE_CASES = [("static3d", r, None) for r in (1, 63, 64, 65, 128, 255)] + [("static3d", r, 1) for r in (63, 64, 65)] \
    + [("full", r, None) for r in (1, 64, 65, 255)] + [("full", 64, 1)] \
    + [("symmetric", r, None) for r in (63, 64, 128)] + [("symmetric", 65, 1)]


@pytest.mark.parametrize("layout, r, lanes", WAVE_CASES)
def test_a_wave_of_the_last_segment_holds_r_records(gs4d, oracle, monkeypatch, layout, r, lanes):
    n = 4096 + r
    rows, seg = stc.plan(n)
    last = n - (rows - 1) * seg
    assert (rows, seg) == (3, 1536) and last // 256 == 4 and last % 256 == r and last < 5 * 256, (rows, seg, last)      # wave 4 holds r records, wave 5 none
    run_three(gs4d, monkeypatch, scene(gs4d, oracle, layout, n), layout, lanes)


# ---- 2. ragged ends at workgroup granularity ----------------------------------------------------------------------------------------------------------
def n_with_last_segment(last):
    """the smallest n above one segment whose last segment (staged_cases.plan) holds `last` records"""
    for n in range(2049, 4 * 2048 + 1):
        rows, seg = stc.plan(n)
        if rows > 1 and n - (rows - 1) * seg == last:
            return n, rows, seg
    raise AssertionError(last)


def direct_frames(gs4d, monkeypatch, sc, env, rec=None, frames=FRAMES):
    """MODE_4D_DIRECT draws of the scene's n records (instance k is record k: no key generation to fuse) -> images, changes of the path statistics,
    the entries statistic after each frame, the layout read"""
    for k in CLEARED:
        monkeypatch.delenv(k, raising=False)
    c = _ctx(gs4d, sc.w, sc.h, monkeypatch, **env)
    try:
        c.set_clear_color(gs4d.CLEAR_COLOR)
        db = c.buffer(sc.rec if rec is None else rec)
        imgs, deltas, entries = [], [], []
        for _ in range(frames):
            before, _ = path_stats(c)
            c.clear()
            c.set_uniforms(time=sc.t, min_opacity=0.0, view=sc.view, proj=sc.proj)
            c.set_mode(gs4d.MODE_4D_DIRECT)
            c.bind(1, db)
            c.draw_instanced(sc.n)
            imgs.append(c.read_pixels())
            after, _ = path_stats(c)
            deltas.append({k: after[k] - before[k] for k in after})
            entries.append(c.stats()["entries"])
        return imgs, deltas, entries, c.stats()["record_read_bytes"]
    finally:
        c.finish()
        c.close()


_direct_want = {}


def run_direct(gs4d, oracle, monkeypatch, sc, layout, lanes=None):
    """staged and exact lists of an instance-ordered draw: bit-identical, and the CPU renderer's image without a sort"""
    if id(sc) not in _direct_want:
        _direct_want[id(sc)] = oracle.render_4d(sc.rec, False, sc.t, 0.0, sc.cam[0], sc.view, sc.proj, sc.w, sc.h)[0]
    want, more = _direct_want[id(sc)], knobs_for(layout, lanes)
    imgs, deltas, _, b = direct_frames(gs4d, monkeypatch, sc, more)
    imgs0, deltas0, _, b0 = direct_frames(gs4d, monkeypatch, sc, {**more, "GS4D_STAGED": 0})
    assert b == b0 == LAYOUT_BYTES[layout], (b, b0)
    print("direct:", deltas)
    for j, (img, img0) in enumerate(zip(imgs, imgs0)):
        err = float(np.abs(img.astype(np.float64) - want).max())
        assert err <= TOL, f"frame {j}: Linf against the CPU renderer = {err:.3e}"
        assert same(img, img0), f"frame {j}: differs from the frame of GS4D_STAGED=0"
    assert all(d["staged_draws"] == 0 for d in deltas0), deltas0
    assert any(d["staged_draws"] == 1 and d["fused_keygen_draws"] == 0 and d["reruns"] == 0 for d in deltas), f"no frame was staged without fused keys: {deltas}"


@pytest.mark.parametrize("layout, last, lanes", [("static3d", v, None) for v in (1, 511, 512, 513, 1025)] + [("static3d", 513, 1), ("full", 513, None), ("symmetric", 511, None)])
def test_a_last_segment_of_so_many_records(gs4d, oracle, monkeypatch, layout, last, lanes):
    """the staged forms whose round it is records i0 + 512 it + t: the two-launch hybrid frame (run_three's second context) and an instance-ordered
    draw with no keys to fuse"""
    n, rows, seg = n_with_last_segment(last)
    assert stc.plan(n) == (rows, seg) and n - (rows - 1) * seg == last and n % seg == last % seg, (n, rows, seg)
    sc = scene(gs4d, oracle, layout, n)
    run_three(gs4d, monkeypatch, sc, layout, lanes)
    run_direct(gs4d, oracle, monkeypatch, sc, layout, lanes)


# ---- 3. a buffer longer than the draw -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["static3d", "full"])
def test_the_look_ahead_takes_nothing_past_the_draw(gs4d, oracle, monkeypatch, layout):
    """n records drawn from a buffer of n + 5000: the records behind the draw are live ones (copies of the scene's, all of them visible), and the last
    wave's look-ahead would find them.  Entries, keys, permutation and image equal those of the buffer of n records."""
    n = 4096 + 64
    sc = scene(gs4d, oracle, layout, n)
    longer = copy.copy(sc)                                   # Frames.frame uploads .rec and draws .n records
    longer.rec = np.ascontiguousarray(np.concatenate([sc.rec, sc.rec[(np.arange(5000) * 7) % n]]))
    assert longer.rec.shape[0] == n + 5000 and longer.n == n
    more = knobs_for(layout, None)
    for env in (ON, OFF):
        short, e_short, b_short = sorted_frames(gs4d, monkeypatch, sc, env, more)
        long_, e_long, b_long = sorted_frames(gs4d, monkeypatch, longer, env, more)
        assert b_short == b_long == LAYOUT_BYTES[layout]
        assert e_short == e_long, (e_short, e_long)
        for j, (a, b) in enumerate(zip(long_, short)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and same(a[2], b[2]), f"frame {j}: differs from the frame of the {n}-record buffer"
            assert np.array_equal(a[0], sc.want[0]) and np.array_equal(a[1], sc.want[1])
            assert float(np.abs(a[2].astype(np.float64) - sc.eimg).max()) <= TOL
        # (a draw of part of a buffer executes no queued key generation — draw_common fuses only the keygen of the whole buffer — so which lists the
        # frames of the longer buffer get is the host's choice; the staged look-ahead into a longer buffer is proven by the instance-ordered draws below)
        print("longer buffer:", [fr[3] for fr in long_])
        assert all(fr[3]["fused_keygen_draws"] == 0 for fr in long_) and any(staged_fused(fr[3]) for fr in short), ([fr[3] for fr in long_], [fr[3] for fr in short])
    imgs, deltas, e_direct, b_direct = direct_frames(gs4d, monkeypatch, sc, more)
    imgs_l, deltas_l, e_direct_l, b_direct_l = direct_frames(gs4d, monkeypatch, sc, more, rec=longer.rec)
    assert b_direct == b_direct_l == LAYOUT_BYTES[layout], (b_direct, b_direct_l)
    assert e_direct == e_direct_l, (e_direct, e_direct_l)
    assert all(same(a, b) for a, b in zip(imgs_l, imgs)), f"an instance-ordered frame differs from the frame of the {n}-record buffer"
    assert any(d["staged_draws"] == 1 and d["reruns"] == 0 for d in deltas_l), f"no frame of the longer buffer was staged: {deltas_l}"
