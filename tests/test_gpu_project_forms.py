"""The forms of the projection kernel (csrc/preprocess.hip; TileCount::lists, TileCount::keys) that no other file proves run, through the C ABI:
k_preprocess<SRC> and k_project_count<SRC, Count | Stage, None> for SRC = Src3D, Src2D — what a quad draw and a 2D draw can reach: no draw of these two
sources is ever fused (draw_common), so their instances with keys do not exist, and no case here asks for one — and the two ordered forms of the three 4D
layouts, k_preprocess<SRC> and k_project_count<SRC, None, Write> (test_gpu_project_prefetch.py proves the five others of each layout).

Harness and shapes of test_gpu_project_prefetch.py: n = 4096 + 65 records — three segments of 1536 (staged_cases.plan), the last ending one record
into a wave's second round — at 320 x 180, 6 frames of one context so that the guesses of a staged draw are learnt; the GS4D_STAGED=0 context is the
exact-lists twin, the GS4D_DRAW_PATH=ordered context the one-thread-per-record kernel.

Bar: every staged frame equals the exact-lists frame bit for bit; every frame of all three contexts is the CPU renderer's image within TOL (1e-4,
test_gpu_sort_segfeed.py's).  Proof of path, from the statistics' change over a frame: at least one judged frame of the staged context is a staged,
unordered draw without fused keys and without a re-run (Stage); every frame of the twin is an unordered draw that is not staged (Count); no frame of
the ordered context is an unordered draw (k_preprocess).
"""
import numpy as np
import pytest

import blend_cases as bc
import staged_cases as stc
from test_gpu_paths import _ctx
from test_gpu_project_prefetch import LAYOUT_BYTES, knobs_for, scene as scene_4d
from test_gpu_sort_segfeed import CLEARED, ON, TOL, Frames
from test_gpu_staged_misses import same

pytestmark = pytest.mark.gpu

N, W, H, FRAMES = 4096 + 65, 320, 180, 6
PATH_KEYS = ("unordered_draws", "staged_draws", "fused_keygen_draws", "reruns", "staged_misses")

_scenes = {}


def scene(gs4d, oracle, source):
    """(records, the checker's mode, the CPU renderer's image), once per source: N small splats dealt over the image — quads of 6 pixels, about two
    tiles each, so that a segment's entries fit a staged block and every tile's list is short"""
    if source not in _scenes:
        assert stc.plan(N) == (3, 1536) and (N - 2 * 1536) % 64 == 1
        rng = np.random.default_rng(0x7072)
        px, py = rng.uniform(4.0, W - 4.0, N), rng.uniform(4.0, H - 4.0, N)
        rgba = np.concatenate([rng.uniform(0.0, 1.0, (N, 3)), rng.uniform(0.3, 0.9, (N, 1))], 1).astype(np.float32)
        if source == "quads":
            data, mode = bc.quads(gs4d, oracle, W, H, px, py, rng.uniform(-20.0, 20.0, N), np.full(N, 0.6), rgba), oracle.MODE_3D
        else:
            data, mode = bc.records_2d(gs4d, oracle, W, H, px, py, np.full(N, 3.0), rgba, rng.uniform(0.0, np.pi, N)), oracle.MODE_2D
        data = np.ascontiguousarray(data, np.float32)
        view, proj = bc.mats(gs4d, W, H)
        eproj = oracle.preprocess(mode, data, view, proj, W, H)
        assert int((eproj["valid"] != 0).sum()) == N
        want = oracle.composite(eproj, None, mode, W, H, oracle.clear_image(W, H))
        assert float(np.abs(want - oracle.clear_image(W, H)).max()) > 0.05, "empty frame"
        _scenes[source] = (data, want)
    return _scenes[source]


def frames(gs4d, monkeypatch, source, data, env):
    """FRAMES draws of the scene in one context -> images, changes of the path statistics"""
    for k in CLEARED:
        monkeypatch.delenv(k, raising=False)
    c = _ctx(gs4d, W, H, monkeypatch, **env)
    try:
        view, proj = bc.mats(gs4d, W, H)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        buf = c.buffer(data)
        imgs, deltas = [], []
        for _ in range(FRAMES):
            before = c.stats()
            c.clear()
            c.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
            if source == "quads":
                c.set_mode(gs4d.MODE_3D_FULL)
                c.draw_quads(buf, N)
            else:
                c.set_mode(gs4d.MODE_2D)
                c.bind(1, buf)
                c.draw_instanced(N)
            imgs.append(c.read_pixels())
            after = c.stats()
            deltas.append({k: after[k] - before[k] for k in PATH_KEYS})
        return imgs, deltas
    finally:
        c.finish()
        c.close()


@pytest.mark.parametrize("source", ["quads", "2d"])
def test_the_forms_a_source_without_keys_can_reach(gs4d, oracle, monkeypatch, source):
    data, want = scene(gs4d, oracle, source)
    staged, d_staged = frames(gs4d, monkeypatch, source, data, {})
    exact, d_exact = frames(gs4d, monkeypatch, source, data, {"GS4D_STAGED": 0})
    ordered, d_ordered = frames(gs4d, monkeypatch, source, data, {"GS4D_DRAW_PATH": "ordered"})
    print("staged:", d_staged, "\nexact:", d_exact, "\nordered:", d_ordered)
    for j in range(FRAMES):
        for name, img in (("staged", staged[j]), ("exact lists", exact[j]), ("ordered", ordered[j])):
            err = float(np.abs(img.astype(np.float64) - want).max())
            print(f"frame {j} {name}: Linf against the CPU renderer = {err:.3e}")
            assert err <= TOL, f"frame {j}, {name}: Linf against the CPU renderer = {err:.3e}"
        assert same(staged[j], exact[j]), f"frame {j}: differs from the frame of GS4D_STAGED=0"
    assert all(d["fused_keygen_draws"] == 0 for d in d_staged + d_exact + d_ordered), (d_staged, d_exact, d_ordered)
    assert any(d["unordered_draws"] == 1 and d["staged_draws"] == 1 and d["reruns"] == 0 and d["staged_misses"] == 0 for d in d_staged), f"no frame was staged: {d_staged}"
    assert all(d["unordered_draws"] == 1 and d["staged_draws"] == 0 and d["reruns"] == 0 for d in d_exact), f"not every frame of the twin built exact lists: {d_exact}"
    assert all(d["unordered_draws"] == 0 and d["staged_draws"] == 0 for d in d_ordered), f"a frame of the ordered context took the unordered path: {d_ordered}"


@pytest.mark.parametrize("layout", tuple(LAYOUT_BYTES))
def test_the_ordered_forms_of_a_4d_layout(gs4d, oracle, monkeypatch, layout):
    """on the ordered path (GS4D_DRAW_PATH=ordered): a draw that executes its queued key generation — keys Write without lists: keys and permutation are
    the stable sort of the checker's keys — and an instance-ordered draw, one thread per record; record_read_bytes names the layout either read"""
    sc = scene_4d(gs4d, oracle, layout, N)
    env = {**ON, **knobs_for(layout, None), "GS4D_DRAW_PATH": "ordered"}
    f = Frames(gs4d, monkeypatch, sc.w, sc.h, env)
    try:
        got = [f.frame(sc) for _ in range(FRAMES)]
        st = f.ctx.stats()
    finally:
        f.close()
    assert st["unordered_draws"] == 0 and st["staged_draws"] == 0 and st["fused_keygen_draws"] == FRAMES and st["record_read_bytes"] == LAYOUT_BYTES[layout], st
    for j, (k, p, img, _, _) in enumerate(got):
        assert np.array_equal(k, sc.want[0]) and np.array_equal(p, sc.want[1]), f"frame {j}: keys or permutation"
        assert float(np.abs(img.astype(np.float64) - sc.eimg).max()) <= TOL, f"frame {j}"
    want = oracle.render_4d(sc.rec, False, sc.t, 0.0, sc.cam[0], sc.view, sc.proj, sc.w, sc.h)[0]
    for k in CLEARED:
        monkeypatch.delenv(k, raising=False)
    c = _ctx(gs4d, sc.w, sc.h, monkeypatch, **{k: v for k, v in env.items() if k not in ON})
    try:
        c.set_clear_color(gs4d.CLEAR_COLOR)
        db = c.buffer(sc.rec)
        for j in range(FRAMES):
            c.clear()
            c.set_uniforms(time=sc.t, min_opacity=0.0, view=sc.view, proj=sc.proj)
            c.set_mode(gs4d.MODE_4D_DIRECT)
            c.bind(1, db)
            c.draw_instanced(sc.n)
            err = float(np.abs(c.read_pixels().astype(np.float64) - want).max())
            assert err <= TOL, f"frame {j}: Linf against the CPU renderer = {err:.3e}"
        st = c.stats()
    finally:
        c.finish()
        c.close()
    assert st["unordered_draws"] == 0 and st["staged_draws"] == 0 and st["fused_keygen_draws"] == 0 and st["record_read_bytes"] == LAYOUT_BYTES[layout], st
