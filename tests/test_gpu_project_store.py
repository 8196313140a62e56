"""The projection kernel's record stores (csrc/preprocess.hip, csrc/proj_tile.h): a wave of k_project_count puts its 64 projected records into LDS and
writes them as whole 64-byte lines (sources with WAVE_STORE; the others store a record per thread), through the C ABI, where a wave holds fewer than 64
records, exactly 64, none at all, and where the last segment ends inside a wave.

Bar: Context.debug_projected(n), all 16 words of every record as uint32 bit patterns, equals — bit for bit, no word excepted — what a
GS4D_DRAW_PATH=ordered context leaves that draws the same records with MODE_4D_DIRECT and the same uniforms: k_preprocess, one record per thread, which
keeps its per-thread stores on purpose.  (debug_projected reorders six words of a record on the host the same way on both sides.)

Forms (the records are read after a frame whose statistics name the form; a context's first frames are exact-list frames):
  segment-fed     staged, fused, one sort launch                          k_project_count<SRC, Stage, SegmentFed>
  two-launch      GS4D_SORT_SEGFEED=0: staged, fused, two sort launches   k_project_count<SRC, Stage, Write>
  exact           GS4D_STAGED=0: fused, never staged                      k_project_count<SRC, Count, Write>
  direct          MODE_4D_DIRECT draws, staged, no keys                   k_project_count<SRC, Stage, None>
  ordered-sorted  GS4D_DRAW_PATH=ordered, the draw runs its keygen        k_project_count<SRC, None, Write>
n = 1 has only the fourth of them: gs4d_sort_pairs returns at once for one pair, so the queued key generation never becomes a sorted one, no draw
executes it (fused_keygen_draws stays 0) and the library draws the record on the ordered path.  The four sorted contexts still run at n = 1 and their
records are held to the same bar — whatever kernel projected them — but no form is asked of their frames; the direct context's frame is a staged one.

Harness and scenes of test_gpu_sort_segfeed.py / test_gpu_project_prefetch.py (320 x 180 and the shell scene's 640 x 360, 6 frames a context).
"""
import numpy as np
import pytest

import blend_cases as bc
import hostile_cases as hc
import staged_cases as stc
from test_gpu_paths import _ctx
from test_gpu_project_forms import N as N_FORMS, scene as scene_nokeys
from test_gpu_project_prefetch import FRAMES, LAYOUT_BYTES, UNSTAGED, knobs_for, scene
from test_gpu_sort_segfeed import CLEARED, OFF, ON, Frames, path_stats, segment_fed

pytestmark = pytest.mark.gpu

ORDERED = {"GS4D_DRAW_PATH": "ordered"}
STATS = ("unordered_draws", "staged_draws", "fused_keygen_draws", "reruns", "staged_misses")


def staged_fused(d):
    return d["staged_draws"] == 1 and d["fused_keygen_draws"] == 1 and d["reruns"] == 0


def bits(ctx, n):
    return ctx.debug_projected(n).view(np.uint32).copy()


def direct_records(gs4d, monkeypatch, sc, env, named, frames=FRAMES):
    """MODE_4D_DIRECT draws of the scene's records in one context -> the projected records after the last frame whose statistics `named` accepts (None:
    no such frame), and the layout the projection read"""
    for k in CLEARED:
        monkeypatch.delenv(k, raising=False)
    c = _ctx(gs4d, sc.w, sc.h, monkeypatch, **env)
    try:
        c.set_clear_color(gs4d.CLEAR_COLOR)
        db = c.buffer(sc.rec)
        got, deltas = None, []
        for _ in range(frames):
            before = c.stats()
            c.clear()
            c.set_uniforms(time=sc.t, min_opacity=getattr(sc, "min_opacity", 0.0), view=sc.view, proj=sc.proj)
            c.set_mode(gs4d.MODE_4D_DIRECT)
            c.bind(1, db)
            c.draw_instanced(sc.n)
            c.finish()
            after = c.stats()
            deltas.append({k: after[k] - before[k] for k in STATS})
            if named(deltas[-1]):
                got = bits(c, sc.n)
        return got, deltas, c.stats()["record_read_bytes"]
    finally:
        c.finish()
        c.close()


def sorted_records(gs4d, monkeypatch, sc, env, named, frames=FRAMES):
    """keygen, sort, MODE_4D_SORTED draw (Frames.frame) -> as direct_records"""
    f = Frames(gs4d, monkeypatch, sc.w, sc.h, env)
    try:
        got, deltas = None, []
        for _ in range(frames):
            before = f.ctx.stats()["unordered_draws"]
            d = f.frame(sc)[3]
            d["unordered_draws"] = f.ctx.stats()["unordered_draws"] - before
            deltas.append(d)
            if named(d):
                got = bits(f.ctx, sc.n)
        return got, deltas, f.ctx.stats()["record_read_bytes"]
    finally:
        f.close()


_reference = {}


def reference(gs4d, monkeypatch, sc, layout):
    """k_preprocess' records of the scene, once per scene"""
    if id(sc) not in _reference:
        want, deltas, b = direct_records(gs4d, monkeypatch, sc, {**knobs_for(layout, None), **ORDERED}, lambda d: d["unordered_draws"] == 0 and d["staged_draws"] == 0, frames=2)
        assert want is not None and b == LAYOUT_BYTES[layout], (deltas, b)
        assert (want[:, 14] == np.float32(1.0).view(np.uint32)).sum() >= (sc.n + 1) // 2, "most records of the scene are valid ones"
        _reference[id(sc)] = (sc, want)                          # (the scene is kept with it: its id stays its own)
    return _reference[id(sc)][1]


def equal_records(got, want, what):
    assert got is not None, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ from k_preprocess' records, the first: record {int(bad[0][0])} word {int(bad[0][1])}: " \
                          f"{int(got[tuple(bad[0])]):#010x} for {int(want[tuple(bad[0])]):#010x}"


def forms(n):
    """(name, sorted frames?, environment, the frame that names the form) of the five forms at n records"""
    out = [
        ("segment-fed", True, ON, segment_fed),
        ("two-launch", True, OFF, lambda d: staged_fused(d) and d["sort_launches"] == 2),
        ("exact", True, UNSTAGED, lambda d: d["staged_draws"] == 0 and d["fused_keygen_draws"] == 1 and d["unordered_draws"] == 1),
        ("direct", False, {}, lambda d: d["staged_draws"] == 1 and d["fused_keygen_draws"] == 0 and d["reruns"] == 0),
        ("ordered-sorted", True, {**ON, **ORDERED}, lambda d: d["unordered_draws"] == 0 and d["staged_draws"] == 0 and d["fused_keygen_draws"] == 1),
    ]
    if n == 1:                                                   # one pair is never sorted, so no draw is fused (the module's docstring): any frame of a sorted context
        out = [(name, is_sorted, env, (lambda d: d["fused_keygen_draws"] == 0) if is_sorted else named) for name, is_sorted, env, named in out]
    return out


def run_forms(gs4d, oracle, monkeypatch, layout, n):
    sc = scene(gs4d, oracle, layout, n)
    want = reference(gs4d, monkeypatch, sc, layout)
    more = knobs_for(layout, None)
    for name, is_sorted, env, named in forms(n):
        got, deltas, b = (sorted_records if is_sorted else direct_records)(gs4d, monkeypatch, sc, {**more, **env}, named)
        print(f"{layout} n = {n}, {name}:", deltas)
        assert b == LAYOUT_BYTES[layout], (name, b)
        assert got is not None, f"{name}: no frame of the context was a frame of that form: {deltas}"
        equal_records(got, want, f"{layout} n = {n}, {name}")


# n = 1 .. 513: one segment, whose last wave holds n % 64 records (or 64) and the waves behind it none; 4096 + r: three segments of 1536
# (staged_cases.plan), the last with wave 4 holding r records and wave 5 none
SMALL = (1, 63, 64, 65, 511, 513)
RAGGED = tuple(4096 + r for r in (1, 63, 64, 65))


@pytest.mark.parametrize("n", SMALL + RAGGED)
def test_static_records_leave_through_the_wave(gs4d, oracle, monkeypatch, n):
    if n > 4096:
        rows, seg = stc.plan(n)
        last = n - (rows - 1) * seg
        assert (rows, seg) == (3, 1536) and last // 256 == 4 and last % 256 == n - 4096, (rows, seg, last)
    run_forms(gs4d, oracle, monkeypatch, "static3d", n)


@pytest.mark.parametrize("layout, n", [("full", 4096 + 63), ("full", 4096 + 64), ("symmetric", 4096 + 1), ("symmetric", 4096 + 64)])
def test_the_other_4d_layouts(gs4d, oracle, monkeypatch, layout, n):
    """a partial-wave and a full-wave n (their instances may store a record per thread: the bar is the same)"""
    run_forms(gs4d, oracle, monkeypatch, layout, n)


@pytest.mark.parametrize("source", ["quads", "2d"])
def test_quads_and_2d_records_staged(gs4d, oracle, monkeypatch, source):
    """k_project_count<Src3D | Src2D, Stage, None> against k_preprocess<Src3D | Src2D>: test_gpu_project_forms.py's scene, 4096 + 65 records"""
    data, _ = scene_nokeys(gs4d, oracle, source)
    view, proj = bc.mats(gs4d, 320, 180)

    def records(env, named):
        for k in CLEARED:
            monkeypatch.delenv(k, raising=False)
        c = _ctx(gs4d, 320, 180, monkeypatch, **env)
        try:
            c.set_clear_color(gs4d.CLEAR_COLOR)
            buf = c.buffer(data)
            got, deltas = None, []
            for _ in range(FRAMES):
                before = c.stats()
                c.clear()
                c.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
                if source == "quads":
                    c.set_mode(gs4d.MODE_3D_FULL)
                    c.draw_quads(buf, N_FORMS)
                else:
                    c.set_mode(gs4d.MODE_2D)
                    c.bind(1, buf)
                    c.draw_instanced(N_FORMS)
                c.finish()
                after = c.stats()
                deltas.append({k: after[k] - before[k] for k in STATS})
                if named(deltas[-1]):
                    got = bits(c, N_FORMS)
            return got, deltas
        finally:
            c.finish()
            c.close()

    want, d_want = records(ORDERED, lambda d: d["unordered_draws"] == 0 and d["staged_draws"] == 0)
    got, d_got = records({}, lambda d: d["unordered_draws"] == 1 and d["staged_draws"] == 1 and d["reruns"] == 0 and d["staged_misses"] == 0)
    print("ordered:", d_want, "\nstaged:", d_got)
    assert want is not None, d_want
    assert got is not None, f"no frame was staged: {d_got}"
    equal_records(got, want, source)


class Hostile:
    """records of tests/hostile_cases.py as a static 3D set (the 64-byte layout, whose instances store through the wave): the implants of the colour and
    non-finite families that keep a finite time term — NaN and infinite colours and alphas, negative colours and alphas, a NaN position — with mu_t, sig's
    time row and its time column set to one value in every record"""

    def __init__(self, gs4d):
        names = ("nan_inf_colour", "nan_inf_alpha", "negative_colour", "negative_alpha", "colour_above_one", "alpha_above_one", "x_nan", "sig00_ninf", "sub_pixel_scale")
        rec = np.concatenate([hc.get(k).rec for k in names]).copy()
        rec[:, hc.F_MUT] = hc.T0
        rec[:, list(hc.F_TIMECOL + hc.F_VEL)] = 0.0
        rec[:, hc.F_S44] = 1.0
        c = hc.get(names[0])
        self.rec, self.n, self.t, self.cam, self.view, self.proj, self.w, self.h, self.min_opacity = rec, rec.shape[0], c.t, c.cam, c.view, c.proj, hc.W, hc.H, 0.0


def test_hostile_payloads_go_through_the_stage_unchanged(gs4d, monkeypatch):
    sc = Hostile(gs4d)
    want, d_want, b_want = direct_records(gs4d, monkeypatch, sc, ORDERED, lambda d: d["unordered_draws"] == 0, frames=2)
    assert want is not None and b_want == 64, (d_want, b_want)
    valid = want[:, 14] == np.float32(1.0).view(np.uint32)
    assert 0 < int((~valid).sum()) < sc.n and (want[~valid][:, :7] == 0).all(), "the set holds records that project to nothing: centre, rows and alpha 0"
    neg = (want[valid][:, [2, 3, 4, 5]] >> 31).astype(bool)
    assert neg.any() and (~neg).any(), "affine rows of both signs"
    # whichever lists the library builds for these records, their projection is a k_project_count instance of the static source
    got, deltas, b = direct_records(gs4d, monkeypatch, sc, {}, lambda d: d["unordered_draws"] == 1)
    print("direct:", deltas)
    assert b == 64, b
    equal_records(got, want, "hostile records, instance-ordered draws")
    got, deltas, b = sorted_records(gs4d, monkeypatch, sc, {}, lambda d: d["unordered_draws"] == 1 and d["fused_keygen_draws"] == 1)
    print("sorted:", deltas)
    assert b == 64, b
    equal_records(got, want, "hostile records, sorted frames")
