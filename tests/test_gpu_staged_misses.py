"""Staged tile lists: each guess missed on its own, at one, the default and eight frame lanes.

A staged draw runs on guesses (tests/staged_cases.py lists them); the device checks each one, and a draw that misses is re-run
(csrc/gs4d_api.hip, resolve_lane).  tests/test_gpu_staged.py shows draws that never miss, a jump that misses every guess at once and a box
miss.  Here one frame misses exactly what its case names, and proves it (the premise, from the projected records of a context without
staging, before anything is staged):

a  the last segment outgrows its block (k_bucket_tiles_staged must not read its runs: they would lie past the end of the blocks)
b  a middle segment outgrows its block (its runs would be read out of the next segment's block)
c  one bucket outgrows bcap while every segment fits
d  one tile list outgrows the compositor's list capacity after it has shrunk: re-run staged, with a larger capacity (no staged miss)
e  a segment overflow and entries outside the launch box in the same frame
f  the miss frame of a, followed by more frames queued before anything is read: all of them staged with the old guesses

Bar: the miss frame equals the same frame of a context without staging (GS4D_STAGED=0) bit for bit, its permutation the checker's bit for
bit, its image the checker's (oracle.render_4d) within 1e-4; it counts one re-run (and, but for d, one staged miss); the frames after it are
staged again and do not miss.
"""
import numpy as np
import pytest

import staged_cases as sc

TOL = 1e-4
LANES = [pytest.param(1, id="lanes1"), pytest.param(None, id="lanes_default"), pytest.param(8, id="lanes8")]
NPIX = sc.W * sc.H


class Run:
    """one context over one scene, frames as the reference's loop draws them: Clear -> key loop -> sort -> Draw"""

    def __init__(self, gs4d, rec, monkeypatch, staged, lanes):
        monkeypatch.setenv("GS4D_NB", str(sc.NB))
        if lanes:
            monkeypatch.setenv("GS4D_LANES", str(lanes))
        if staged:
            monkeypatch.delenv("GS4D_STAGED", raising=False)
        else:
            monkeypatch.setenv("GS4D_STAGED", "0")
        self.gs4d, self.n = gs4d, rec.shape[0]
        self.ctx = gs4d.Context(sc.W, sc.H)
        self.ctx.set_clear_color(gs4d.CLEAR_COLOR)
        self.data, self.keys, self.idx = self.ctx.buffer(rec), self.ctx.buffer(nbytes=4 * self.n), self.ctx.buffer(nbytes=4 * self.n)
        self.view, self.proj = sc.mats(gs4d)
        self.lanes = self.ctx.stats()["lanes"]

    def frame(self, t):
        c = self.ctx
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=self.view, proj=self.proj)
        c.keygen(self.data, t, sc.CAM[0], self.keys, self.idx, self.n)
        c.sort_pairs(self.keys, self.idx, self.n)
        c.set_mode(self.gs4d.MODE_4D_SORTED)
        c.bind(1, self.idx)
        c.bind(2, self.data)
        c.draw_instanced(self.n)

    def warm_up(self):
        """2 * lanes + 8 frames at T0.  A draw is issued once its lane's previous draw (`lanes` frames earlier) has been validated
        (gs4d_draw_instanced -> resolve_lane): the first statistics arrive with frame `lanes`, every frame from there on is staged; more than
        8 draws validated with short lists let the list capacity shrink"""
        k = 2 * self.lanes + 8
        for _ in range(k):
            self.frame(sc.T0)
        self.ctx.finish()
        s = self.ctx.stats()
        assert s["staged_draws"] == k - self.lanes and s["staged_misses"] == 0 and s["reruns"] == 0 and s["aborted_discarded"] == 0, s
        return s

    def close(self):
        self.ctx.close()


def reference(gs4d, rec, times, monkeypatch, lanes, rgba8=False):
    """a context without staging: the load of the warm-up frame and of the frames at `times` from the device's own pixel rectangles, and
    those frames' images (float; rgba8: also packed to RGBA8 on the device)"""
    ex = Run(gs4d, rec, monkeypatch, staged=False, lanes=lanes)
    ex.frame(sc.T0)
    warm = sc.Load(sc.rects_from_device(ex.ctx.debug_projected(ex.n)))
    out = ex.ctx.buffer(nbytes=NPIX * 4) if rgba8 else None
    loads, imgs, packed = [], [], []
    for t in times:
        ex.frame(t)
        imgs.append(ex.ctx.read_pixels())
        loads.append(sc.Load(sc.rects_from_device(ex.ctx.debug_projected(ex.n))))
        if rgba8:
            ex.ctx.read_pixels_rgba8_device(ex.ctx.device_ptr(out)[0], NPIX * 4)
            ex.ctx.finish()
            packed.append(ex.ctx.read(out, np.uint8, NPIX * 4))
    st = ex.ctx.stats()
    ex.close()
    assert st["staged_draws"] == 0, st
    return warm, loads, imgs, packed


def premise(case, warm, loads, times):
    for t, ld in zip(times, loads):
        got = sc.crossed(warm, ld)
        assert got == sc.TARGETS[case], f"case {case}, t = {t}: the frame crosses {sorted(got)}, not {sorted(sc.TARGETS[case])}\n  warm-up {warm}\n  frame {ld}"
    print(f"case {case}: the miss frame crosses {sorted(sc.TARGETS[case])} only")


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", list("abcdef"))
def test_the_checker_sees_each_case_cross_its_guesses(gs4d, oracle, case):
    """the premise of every case from the checker's projection (no GPU): the scenes and the capacity arithmetic mirrored from the host"""
    rec, times = sc.build(gs4d, case)
    view, proj = sc.mats(gs4d)
    load = lambda t: sc.Load(sc.rects_from_checker(oracle.preprocess(oracle.MODE_4D, rec, view, proj, sc.W, sc.H, t=t)))
    premise(case, load(sc.T0), [load(t) for t in times], times)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("case", list("abcde"))
def test_one_frame_misses_one_guess(gs4d, oracle, monkeypatch, case, lanes):
    rec, times = sc.build(gs4d, case)
    warm, loads, eimgs, _ = reference(gs4d, rec, times, monkeypatch, lanes)
    premise(case, warm, loads, times)
    run = Run(gs4d, rec, monkeypatch, staged=True, lanes=lanes)
    s0 = run.warm_up()
    run.frame(sc.T1)
    img = run.ctx.read_pixels()
    perm = run.ctx.read(run.idx, np.uint32, run.n)
    s1 = run.ctx.stats()
    # a capacity or the box: flags & 4, a staged miss, re-run with exact lists; the list capacity alone: flags & 2, re-run staged with a larger one
    list_only = sc.TARGETS[case] == {"list"}
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + (0 if list_only else 1), (s0, s1)
    assert s1["staged_draws"] == s0["staged_draws"] + (2 if list_only else 1) and s1["aborted_discarded"] == s0["aborted_discarded"], (s0, s1)
    assert same(img, eimgs[0]), "the miss frame differs from the frame without staged lists"
    eimg, eperm, _ = oracle.render_4d(rec, True, sc.T1, 0.0, sc.CAM[0], run.view, run.proj, sc.W, sc.H)
    assert np.array_equal(perm, eperm)
    assert np.abs(img.astype(np.float64) - eimg).max() <= TOL
    assert np.abs(eimg - oracle.CLEAR).max() > 0.05
    # the frames after it: the miss frame was validated (read) before they were issued, so they start from what it taught — staged, no miss
    k = 2 * run.lanes + 8
    for _ in range(k):
        run.frame(sc.T1)
    img2 = run.ctx.read_pixels()
    s2 = run.ctx.stats()
    run.close()
    assert s2["staged_draws"] == s1["staged_draws"] + k, (s1, s2)
    assert (s2["staged_misses"], s2["reruns"], s2["aborted_discarded"]) == (s1["staged_misses"], s1["reruns"], s1["aborted_discarded"]), (s1, s2)
    assert same(img2, img)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", LANES)
def test_a_miss_with_frames_in_flight(gs4d, oracle, monkeypatch, lanes):
    """case f: the miss frame (last segment over its block) and j more frames at later times are queued without reading — each of them is
    staged with the guesses of the warm-up and misses too.  Then frame j is read (read_pixels) and frame j - 1 packed from the swap chain
    (gs4d_read_frame_rgba8_device(1)): both must be the frames of a context without staging, bit for bit.  For every j a lane count allows
    (1 .. lanes - 1: the swap chain reaches one frame back); one lane has no previous image: its frame 1 is issued after frame 0 was cleared
    away unread (counted as aborted_discarded, learnt from), and must be right and staged without a miss."""
    rec, times = sc.build(gs4d, "f")
    warm, loads, eimgs, epacked = reference(gs4d, rec, times, monkeypatch, lanes, rgba8=True)
    premise("f", warm, loads, times)
    view, proj = sc.mats(gs4d)
    lanes_now = None
    for j in range(1, len(times)):
        run = Run(gs4d, rec, monkeypatch, staged=True, lanes=lanes)
        L = lanes_now = run.lanes
        if L > 1 and j >= L:
            run.close()
            break
        out = run.ctx.buffer(nbytes=NPIX * 4)
        s0 = run.warm_up()
        for t in times[:j + 1]:
            run.frame(t)
        img = run.ctx.read_pixels()
        if L > 1:
            run.ctx.read_frame_rgba8_device(1, run.ctx.device_ptr(out)[0], NPIX * 4)
        perm = run.ctx.read(run.idx, np.uint32, run.n)
        s = run.ctx.stats()
        run.ctx.finish()
        prev = run.ctx.read(out, np.uint8, NPIX * 4) if L > 1 else None
        run.close()
        d = {k: s[k] - s0[k] for k in ("staged_draws", "staged_misses", "reruns", "aborted_discarded")}
        if L > 1:
            # frames 0 .. j all on lanes whose previous draw was validated in the warm-up: all staged with its guesses, all missed, all re-run
            assert d == {"staged_draws": j + 1, "staged_misses": j + 1, "reruns": j + 1, "aborted_discarded": 0}, (j, d)
            assert np.array_equal(prev, epacked[j - 1]), f"frame {j - 1} packed from the swap chain differs from the frame without staged lists"
        else:
            assert d == {"staged_draws": 2, "staged_misses": 1, "reruns": 0, "aborted_discarded": 1}, (j, d)
        assert same(img, eimgs[j]), f"frame {j} differs from the frame without staged lists"
        eimg, eperm, _ = oracle.render_4d(rec, True, times[j], 0.0, sc.CAM[0], view, proj, sc.W, sc.H)
        assert np.array_equal(perm, eperm)
        assert np.abs(img.astype(np.float64) - eimg).max() <= TOL
        if L == 1:
            break
    assert lanes_now is not None
