"""GPU: gs4d_build_records — the 96-byte records of a splat set built on the device from its parameters (include/gs4d.h).

The records are compared word for word with the host builders (tests/build_cases.py: equal as uint32, a word that is a NaN on both sides counting as
equal), with the rest of dst, guard buffers and the parameter buffers compared against what was uploaded; pictures drawn from built records are compared
bit for bit with those of a fresh context that uploaded the host-built records; gs4d_debug_shadow_builds shows the one repack a build costs.  All calls
go through the Python binding over the C ABI."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import build_cases as bc
import scenes
import staged_cases

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


def upload(ctx, p, guards=None):
    """the parameter buffers of a set, each followed by a guard buffer when `guards` (a list) is given"""
    bufs = {}
    for name, a in p.items():
        bufs[name] = ctx.buffer(a)
        if guards is not None:
            guards.append(fill(ctx, GUARD))
    return bufs


def params_unchanged(ctx, bufs, p):
    return all(np.array_equal(ctx.read(bufs[k], np.uint32, p[k].size), bits(p[k]).reshape(-1)) for k in p)


# ---- 1. the records ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", bc.FORMS)
def test_records_equal_the_host_builder(gs4d, form):
    ctx = gs4d.Context(64, 64)
    extra = 3                                                   # records >= n that must stay as they are
    for n in bc.SIZES:
        for kind, p in bc.cases(gs4d, form, n):
            what = f"{form}, {kind}, n = {n}"
            guards = [fill(ctx, GUARD)]
            bufs = upload(ctx, p, guards)
            host = np.full((n + extra) * 96 + GUARD, SENTINEL, np.uint8)
            dst = ctx.buffer(host)
            guards.append(fill(ctx, GUARD))
            assert ctx.build_records(bc.form_id(gs4d, form), n, dst=dst, **bufs) == dst
            got = ctx.read(dst, np.uint8, host.size)
            want = bc.host_records(gs4d, form, p)
            ok = bc.same_bits(got[:n * 96].view(f32).reshape(n, 24), want)
            assert ok.all(), f"{what}: {int((~ok).any(1).sum())} of {n} records differ from the host builder, first word at {np.argwhere(~ok)[0].tolist()}"
            assert (got[n * 96:] == SENTINEL).all(), f"{what}: bytes of dst behind record n - 1 changed"
            assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
            assert params_unchanged(ctx, bufs, p), f"{what}: a parameter buffer changed"
            for b in guards + list(bufs.values()) + [dst]:
                ctx.delete(b)
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    p = bc.clean(gs4d, "4d_2q", 4)
    bufs, dst = upload(ctx, p), fill(ctx, 96 * 4)
    ctx.build_records(gs4d.PARAMS_4D_2Q, 0, dst=dst, **bufs)
    ctx.finish()
    assert untouched(ctx, dst, 96 * 4) and params_unchanged(ctx, bufs, p) and ctx.shadow_builds(dst) == 0
    ctx.close()


# ---- 2. pictures, 3. the repack ----------------------------------------------------------------------------------------------------------------
W, H, N = 64, 48, 300
CAM, CAM_DIR = (0.0, 0.0, 150.0), (0.0, 0.0, -1.0)


class Scene:
    """a context with a record buffer (uploaded, or None: to be built), key buffers and the camera of the picture sets"""

    def __init__(self, gs4d, n, rec=None, outputs=False, w=W, h=H):
        self.gs4d, self.n, self.outputs = gs4d, n, outputs
        self.ctx = c = gs4d.Context(w, h)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        if outputs:
            c.set_id_outputs(True)                              # (a frame with ID outputs has aux outputs too)
        self.db = c.buffer(rec) if rec is not None else c.buffer(nbytes=96 * n)
        self.kb, self.ib = c.buffer(nbytes=4 * n), c.buffer(nbytes=4 * n)
        self.view, self.proj = gs4d.look_at(CAM, CAM_DIR), gs4d.perspective(scenes.FOV, w, h, scenes.ZNEAR, scenes.ZFAR)

    def frame(self, mode, t, build=None):
        """one frame; build: (form, parameter buffers) — built first, the documented order"""
        c, gs4d = self.ctx, self.gs4d
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=self.view, proj=self.proj)
        if build is not None:
            c.build_records(bc.form_id(gs4d, build[0]), self.n, dst=self.db, **build[1])
        if mode == gs4d.MODE_4D_SORTED:
            c.keygen(self.db, t, CAM, self.kb, self.ib, self.n)
            c.sort_pairs(self.kb, self.ib, self.n)
        c.set_mode(mode)
        if mode == gs4d.MODE_4D_SORTED:
            c.bind(1, self.ib)
            c.bind(2, self.db)
        else:
            c.bind(1, self.db)                                  # (instance k is record k)
        c.draw_instanced(self.n)

    def read(self):
        c = self.ctx
        out = [c.read_pixels()]
        if self.outputs:
            out += [c.read_aux(), *c.read_ids()]
        return out


def host_frame(gs4d, rec, mode, t, outputs=False):
    """the frame of a fresh context that uploaded the host-built records"""
    s = Scene(gs4d, rec.shape[0], rec, outputs)
    s.frame(mode, t)
    out = s.read()
    s.ctx.close()
    return out


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w)), f"{int((bits(g) != bits(w)).sum())} words differ"


def modes(gs4d):
    return {"sorted": gs4d.MODE_4D_SORTED, "direct": gs4d.MODE_4D_DIRECT}


@pytest.mark.parametrize("mode", ("sorted", "direct"))
@pytest.mark.parametrize("form", bc.FORMS)
def test_pictures_from_built_records_equal_those_from_uploaded_records(gs4d, form, mode):
    mode, t = modes(gs4d)[mode], bc.picture_time(form)
    p = bc.picture_set(gs4d, form, N)
    want = host_frame(gs4d, bc.host_records(gs4d, form, p), mode, t, outputs=True)
    s = Scene(gs4d, N, outputs=True)
    bufs = upload(s.ctx, p)
    assert s.ctx.shadow_builds(s.db) == 0
    s.frame(mode, t, build=(form, bufs))
    got = s.read()
    same(got, want)
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert int((np.abs(got[0] - clear).max(-1) > 1.0 / 255.0).sum()) > 100, "an empty frame"
    # the repack: one for the build followed by a draw, none for a second draw, one more for the next build
    assert s.ctx.shadow_builds(s.db) == 1
    s.frame(mode, t)
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 1, "a second draw repacked"
    s.frame(mode, t, build=(form, bufs))
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 2, "a build must make the next draw repack exactly once"
    s.ctx.finish()
    s.ctx.close()


# ---- 4. ordering without a finish ----------------------------------------------------------------------------------------------------------------
def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch):
    """a build into the buffer that the previous lane's draw still reads: that frame keeps the old set; a host write into a parameter buffer right
    behind the call does not change its result; build, keygen, sort and draw are queued back to back"""
    monkeypatch.setenv("GS4D_LANES", "4")
    mode, form = gs4d.MODE_4D_SORTED, "4d_2q"
    t = bc.picture_time(form)
    old, new = bc.picture_set(gs4d, form, N, seed=0x4256), bc.picture_set(gs4d, form, N, seed=0x4257)
    old_rec, new_rec = bc.host_records(gs4d, form, old), bc.host_records(gs4d, form, new)
    ref = Scene(gs4d, N, old_rec)
    ref.frame(mode, t)
    ref_rgba8 = ref.ctx.buffer(nbytes=W * H * 4)
    ref.ctx.read_frame_rgba8_device(0, ref.ctx.device_ptr(ref_rgba8)[0], W * H * 4)
    ref.ctx.finish()
    want_prev = ref.ctx.read(ref_rgba8, np.uint8, W * H * 4)
    ref.ctx.close()
    want = host_frame(gs4d, new_rec, mode, t)
    s = Scene(gs4d, N, old_rec)
    assert s.ctx.stats()["lanes"] == 4
    bufs, out = upload(s.ctx, new), s.ctx.buffer(nbytes=W * H * 4)
    for _ in range(3):
        s.frame(mode, t)                                        # frames in flight that read the old records and their shadow
    s.frame(mode, t, build=(form, bufs))                        # the build is the first call of the next lane's frame
    for k in new:
        s.ctx.subdata(bufs[k], np.zeros_like(new[k]))           # directly behind: the call must not see the zeros
    s.ctx.read_frame_rgba8_device(1, s.ctx.device_ptr(out)[0], W * H * 4)
    got = s.read()
    s.ctx.finish()
    assert np.array_equal(s.ctx.read(out, np.uint8, W * H * 4), want_prev), "the frame before the build shows another set than it was drawn with"
    same(got, want)
    assert not np.array_equal(bits(got[0]), bits(host_frame(gs4d, old_rec, mode, t)[0])), "the two sets give the same picture: the test shows nothing"
    assert bc.same_bits(s.ctx.read(s.db, f32, N * 24).reshape(N, 24), new_rec).all(), "the records are not those of the parameters as they were at the call"
    assert s.ctx.shadow_builds(s.db) == 2
    s.ctx.close()


def sorted_frame(gs4d, ctx, bufs, n, t):
    db, kb, ib = bufs
    view, proj = staged_cases.mats(gs4d)
    ctx.clear()
    ctx.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
    ctx.keygen(db, t, staged_cases.CAM[0], kb, ib, n)
    ctx.sort_pairs(kb, ib, n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.draw_instanced(n)


def test_a_build_waits_for_a_rerun(gs4d, monkeypatch):
    """staged_cases' case a (as tests/test_gpu_shade.py; its scene fixes the 640 x 360 context): frames at T0 teach the guesses, the frame at T1
    outgrows a segment block; the build into its record buffer settles the draw first — the re-run uses the old records"""
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    rec, _ = staged_cases.build(gs4d, "a")
    Wb, Hb, n = staged_cases.W, staged_cases.H, rec.shape[0]
    p = bc.clean(gs4d, "3d", n)
    fresh = gs4d.Context(Wb, Hb)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    sorted_frame(gs4d, fresh, (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n)), n, staged_cases.T1)
    want = fresh.read_pixels()
    fresh.close()
    ctx = gs4d.Context(Wb, Hb)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    params = upload(ctx, p)
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    ctx.build_records(gs4d.PARAMS_3D, n, dst=bufs[0], **params)                # no read-back in between
    s1 = ctx.stats()
    assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    got = ctx.read_pixels()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"
    assert bc.same_bits(ctx.read(bufs[0], f32, n * 24).reshape(n, 24), bc.host_records(gs4d, "3d", p)).all()
    ctx.close()


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", bc.FORMS)
def test_argument_errors_leave_everything_as_it_was(gs4d, form):
    n = 300
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    p = bc.clean(gs4d, form, n)
    bufs, dst = upload(ctx, p), fill(ctx, 96 * n)
    short = {k: ctx.buffer(a.reshape(-1)[:-1]) for k, a in p.items()}           # one float short of n rows
    short_dst, spare, dead = fill(ctx, 96 * n - 16), fill(ctx, 96 * n), fill(ctx, 64)
    ctx.delete(dead)
    names = gs4d.Context.PARAM_BUFFERS
    unused = [k for k in names if k not in p]

    def build(n=n, dst=dst, form=bc.form_id(gs4d, form), flags=0, reserved=0, null=False, **over):
        use = {k: bufs.get(k, 0) for k in names}
        use.update(over)
        params = gs4d.SplatParams(form, flags, *(use[k] for k in names), reserved)
        return lib.gs4d_build_records(ctx._h, None if null else ctypes.byref(params), ctypes.c_size_t(n), dst)

    bad = {"params == NULL": dict(null=True), "form 3": dict(form=3), "form 0xFFFFFFFF": dict(form=0xFFFFFFFF), "flags": dict(flags=1), "reserved": dict(reserved=1),
           "n > 0xFFFFFFFF": dict(n=1 << 32), "dead dst": dict(dst=dead), "no dst": dict(dst=0), "unknown dst": dict(dst=9999), "dst too small": dict(dst=short_dst)}
    for k in p:
        bad.update({f"dead {k}": {k: dead}, f"no {k}": {k: 0}, f"unknown {k}": {k: 9999}, f"{k} too small": {k: short[k]}, f"{k} == dst": {k: dst}})
    for k in unused:
        bad[f"{k} given though the form does not use it"] = {k: spare}
    for a, b in itertools.combinations(p, 2):
        bad[f"{a} == {b}"] = {a: bufs[b]}
    for what, kw in bad.items():
        assert build(**kw) == -1, what
        assert b"build_records" in lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    assert untouched(ctx, dst, 96 * n) and untouched(ctx, short_dst, 96 * n - 16) and untouched(ctx, spare, 96 * n), "a refused call wrote something"
    assert params_unchanged(ctx, bufs, p)
    assert build(n=0) == 0
    ctx.finish()
    assert untouched(ctx, dst, 96 * n) and ctx.shadow_builds(dst) == 0
    # the call works after the refusals
    assert build() == 0
    assert bc.same_bits(ctx.read(dst, f32, n * 24).reshape(n, 24), bc.host_records(gs4d, form, p)).all()
    assert params_unchanged(ctx, bufs, p)
    ctx.close()


# ---- 6. parameters that live in torch tensors ----------------------------------------------------------------------------------------------------
def test_build_from_torch_tensors():
    """Context.write_tensor + build + draw from device tensors on a torch side stream: a program of its own (tests/gpu_build_from_torch.py) because
    torch has to initialise its HIP runtime before libgs4d.so is loaded."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_build_from_torch.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "build from torch ok" in r.stdout
