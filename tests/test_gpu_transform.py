"""GPU: gs4d_transform_records — the 96-byte records of a set under 4D affine maps, placed and instanced on the device (include/gs4d.h).

The records are compared word for word with the host definition (tests/transform_cases.py: equal as uint32, a word that is a NaN on both sides counting
as equal), with the rest of dst, guard buffers, src and xf compared against what was uploaded; pictures drawn from transformed records are compared bit
for bit with those of a fresh context that uploaded the host-transformed records; gs4d_debug_shadow_builds shows the one repack a call costs.  All calls
go through the Python binding over the C ABI."""
import os
import subprocess
import sys

import numpy as np
import pytest

import build_cases as bc
import scenes
import staged_cases
import transform_cases as tc

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


def unchanged(ctx, buf, a):
    return np.array_equal(ctx.read(buf, np.uint32, a.size), bits(a).reshape(-1))


# ---- 1. the records ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", tc.SETS)
def test_records_equal_the_host_definition(gs4d, which):
    ctx = gs4d.Context(64, 64)
    extra, call = 3, 0                                          # records behind the last one that must stay as they are
    for n in tc.SIZES:
        rec = tc.records(gs4d, which, n)
        for m in tc.INSTANCES:
            for first in (0, 7):
                rows = tc.rows_for(call, m)
                call += 1
                what = f"{which}, n = {n}, m = {m}, dst_first = {first}"
                guards = [fill(ctx, GUARD)]
                src = ctx.buffer(rec)
                guards.append(fill(ctx, GUARD))
                xf = ctx.buffer(rows)
                guards.append(fill(ctx, GUARD))
                host = np.full((first + m * n + extra) * 96 + 32, SENTINEL, np.uint8)
                dst = ctx.buffer(host)
                guards.append(fill(ctx, GUARD))
                assert ctx.transform_records(src, n, xf, m, dst=dst, dst_first=first) == dst
                got = ctx.read(dst, np.uint8, host.size)
                want = tc.expected(gs4d, rec, rows)
                ok = tc.same_bits(got[first * 96:(first + m * n) * 96].view(f32).reshape(m * n, 24), want)
                assert ok.all(), f"{what}: {int((~ok).any(1).sum())} of {m * n} records differ from the host definition, first word at {np.argwhere(~ok)[0].tolist()}"
                assert (got[:first * 96] == SENTINEL).all(), f"{what}: bytes of dst in front of record dst_first changed"
                assert (got[(first + m * n) * 96:] == SENTINEL).all(), f"{what}: bytes of dst behind the last record changed"
                assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
                assert unchanged(ctx, src, rec) and unchanged(ctx, xf, rows), f"{what}: src or xf changed"
                for b in guards + [src, xf, dst]:
                    ctx.delete(b)
    assert call >= len(tc.NAMES)                                # every transform was used
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_an_array_of_rows_allocates_and_gives_the_same_records(gs4d):
    ctx = gs4d.Context(64, 64)
    n, rec, rows = 300, tc.records(gs4d, "4d_vel", 300), tc.rows(("rigid", "retime", "velocity"))
    src = ctx.buffer(rec)
    dst = ctx.transform_records(src, n, rows, dst_first=2)
    assert ctx.device_ptr(dst)[1] >= (2 + 3 * n) * 96
    assert tc.same_bits(ctx.read(dst, f32, 3 * n * 24, offset=2 * 96).reshape(3 * n, 24), tc.expected(gs4d, rec, rows)).all()
    one = ctx.transform_records(src, n, gs4d.affine4(tc.quaternion(tc.RIGID_AXIS, tc.RIGID_ANGLE), 2.0, tc.RIGID_SHIFT))
    want = gs4d.transform_records_host(rec, gs4d.affine4(tc.quaternion(tc.RIGID_AXIS, tc.RIGID_ANGLE), 2.0, tc.RIGID_SHIFT))
    assert tc.same_bits(ctx.read(one, f32, n * 24).reshape(n, 24), want).all()
    ctx.close()


def test_no_records_or_no_rows_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    rec, rows = tc.records(gs4d, "4d_2q", 4), tc.rows(("rigid",))
    src, xf, dst = ctx.buffer(rec), ctx.buffer(rows), fill(ctx, 96 * 8)
    ctx.transform_records(src, 0, xf, 1, dst=dst)
    ctx.transform_records(src, 4, xf, 0, dst=dst, dst_first=8)
    ctx.finish()
    assert untouched(ctx, dst, 96 * 8) and unchanged(ctx, src, rec) and unchanged(ctx, xf, rows) and ctx.shadow_builds(dst) == 0
    ctx.close()


# ---- 2. pictures, 3. the repack ----------------------------------------------------------------------------------------------------------------
W, H, N = 64, 48, 300
CAM, CAM_DIR = (0.0, 0.0, 150.0), (0.0, 0.0, -1.0)
A, C = tc.RETIME
# two instances in front of the camera: the rigid map of the other tests and a second pose, both retimed alike so that they show at the same time
PLACES = np.stack([tc.row(tc.block4(tc.rotation(tc.RIGID_AXIS, tc.RIGID_ANGLE), a=A), (30.0, -7.5, 20.0, C)),
                   tc.row(tc.block4(0.75 * tc.rotation((0.0, 1.0, 0.3), -1.1), v=(0.2, 0.0, 0.0), a=A), (-35.0, 10.0, -10.0, C))])


class Scene:
    """a context with a record buffer (uploaded, or None: to be written by the call), key buffers and the camera of the picture sets"""

    def __init__(self, gs4d, n, rec=None, outputs=False, w=W, h=H):
        self.gs4d, self.n, self.outputs = gs4d, n, outputs
        self.ctx = c = gs4d.Context(w, h)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        if outputs:
            c.set_id_outputs(True)                              # (a frame with ID outputs has aux outputs too)
        self.db = c.buffer(rec) if rec is not None else c.buffer(nbytes=96 * n)
        self.kb, self.ib = c.buffer(nbytes=4 * n), c.buffer(nbytes=4 * n)
        self.view, self.proj = gs4d.look_at(CAM, CAM_DIR), gs4d.perspective(scenes.FOV, w, h, scenes.ZNEAR, scenes.ZFAR)

    def frame(self, mode, t, place=None):
        """one frame; place: (src, n, xf, m) — transformed into the record buffer first, the documented order"""
        c, gs4d = self.ctx, self.gs4d
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=self.view, proj=self.proj)
        if place is not None:
            c.transform_records(*place, dst=self.db)
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
    """the frame of a fresh context that uploaded the host-transformed records"""
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


def picture_records(gs4d, form, seed=0x4254):
    return bc.host_records(gs4d, form, bc.picture_set(gs4d, form, N, seed))


@pytest.mark.parametrize("mode", ("sorted", "direct"))
@pytest.mark.parametrize("form", bc.FORMS)
def test_pictures_from_transformed_records_equal_those_from_uploaded_records(gs4d, form, mode):
    mode, t = modes(gs4d)[mode], A * bc.picture_time(form) + C
    rec = picture_records(gs4d, form)
    want = host_frame(gs4d, tc.expected(gs4d, rec, PLACES), mode, t, outputs=True)
    s = Scene(gs4d, 2 * N, outputs=True)
    place = (s.ctx.buffer(rec), N, s.ctx.buffer(PLACES), 2)
    assert s.ctx.shadow_builds(s.db) == 0
    s.frame(mode, t, place)
    got = s.read()
    same(got, want)
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert int((np.abs(got[0] - clear).max(-1) > 1.0 / 255.0).sum()) > 100, "an empty frame"
    # the repack: one for the call followed by a draw, none for a second draw, one more for the next call
    assert s.ctx.shadow_builds(s.db) == 1
    s.frame(mode, t)
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 1, "a second draw repacked"
    s.frame(mode, t, place)
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 2, "a call must make the next draw repack exactly once"
    s.ctx.finish()
    s.ctx.close()


def test_two_calls_assemble_one_buffer_from_two_sets(gs4d):
    mode, t = gs4d.MODE_4D_SORTED, A * bc.T + C
    one, two = picture_records(gs4d, "4d_vel")[:257], picture_records(gs4d, "4d_2q", seed=0x4258)
    want_rec = np.concatenate([tc.expected(gs4d, one, PLACES), tc.expected(gs4d, two, PLACES[1:])])
    n = want_rec.shape[0]
    assert n == 2 * 257 + N
    s = Scene(gs4d, n)
    c = s.ctx
    xf = c.buffer(PLACES)
    xf1 = c.buffer(PLACES[1:])
    c.transform_records(c.buffer(one), 257, xf, 2, dst=s.db)
    c.transform_records(c.buffer(two), N, xf1, 1, dst=s.db, dst_first=2 * 257)
    s.frame(mode, t)
    got = s.read()
    assert c.shadow_builds(s.db) == 1, "two calls in front of one draw: one repack"
    assert tc.same_bits(c.read(s.db, f32, n * 24).reshape(n, 24), want_rec).all()
    same(got, host_frame(gs4d, want_rec, mode, t))
    c.close()


# ---- 4. ordering without a finish ----------------------------------------------------------------------------------------------------------------
def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch):
    """a call into the buffer that the previous lane's draw still reads: that frame keeps the old set; host writes into xf and src right behind the
    call do not change its result; transform, keygen, sort and draw are queued back to back"""
    monkeypatch.setenv("GS4D_LANES", "4")
    mode, t = gs4d.MODE_4D_SORTED, A * bc.T + C
    old_rec = tc.expected(gs4d, picture_records(gs4d, "4d_vel", seed=0x4256), PLACES)
    src_rec = picture_records(gs4d, "4d_2q", seed=0x4257)
    new_rec = tc.expected(gs4d, src_rec, PLACES)
    ref = Scene(gs4d, 2 * N, old_rec)
    ref.frame(mode, t)
    ref_rgba8 = ref.ctx.buffer(nbytes=W * H * 4)
    ref.ctx.read_frame_rgba8_device(0, ref.ctx.device_ptr(ref_rgba8)[0], W * H * 4)
    ref.ctx.finish()
    want_prev = ref.ctx.read(ref_rgba8, np.uint8, W * H * 4)
    ref.ctx.close()
    want = host_frame(gs4d, new_rec, mode, t)
    s = Scene(gs4d, 2 * N, old_rec)
    assert s.ctx.stats()["lanes"] == 4
    src, xf, out = s.ctx.buffer(src_rec), s.ctx.buffer(PLACES), s.ctx.buffer(nbytes=W * H * 4)
    for _ in range(3):
        s.frame(mode, t)                                        # frames in flight that read the old records and their shadow
    s.frame(mode, t, place=(src, N, xf, 2))                     # the call is the first of the next lane's frame
    s.ctx.subdata(xf, np.zeros_like(PLACES))                    # directly behind: the call must not see the zeros
    s.ctx.subdata(src, np.zeros_like(src_rec))
    s.ctx.read_frame_rgba8_device(1, s.ctx.device_ptr(out)[0], W * H * 4)
    got = s.read()
    s.ctx.finish()
    assert np.array_equal(s.ctx.read(out, np.uint8, W * H * 4), want_prev), "the frame before the call shows another set than it was drawn with"
    same(got, want)
    assert not np.array_equal(bits(got[0]), bits(host_frame(gs4d, old_rec, mode, t)[0])), "the two sets give the same picture: the test shows nothing"
    assert tc.same_bits(s.ctx.read(s.db, f32, 2 * N * 24).reshape(2 * N, 24), new_rec).all(), "the records are not those of src and xf as they were at the call"
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


def test_a_call_waits_for_a_rerun(gs4d, monkeypatch):
    """staged_cases' case a (as tests/test_gpu_build.py; its scene fixes the 640 x 360 context): frames at T0 teach the guesses, the frame at T1
    outgrows a segment block; the call into its record buffer settles the draw first — the re-run uses the old records"""
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    rec, _ = staged_cases.build(gs4d, "a")
    Wb, Hb, n = staged_cases.W, staged_cases.H, rec.shape[0]
    src_rec, rows = tc.records(gs4d, "3d", n), tc.rows(("scale_shear",))
    fresh = gs4d.Context(Wb, Hb)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    sorted_frame(gs4d, fresh, (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n)), n, staged_cases.T1)
    want = fresh.read_pixels()
    fresh.close()
    ctx = gs4d.Context(Wb, Hb)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    src, xf = ctx.buffer(src_rec), ctx.buffer(rows)
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    ctx.transform_records(src, n, xf, 1, dst=bufs[0])                           # no read-back in between
    s1 = ctx.stats()
    assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    got = ctx.read_pixels()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"
    assert tc.same_bits(ctx.read(bufs[0], f32, n * 24).reshape(n, 24), tc.expected(gs4d, src_rec, rows)).all()
    ctx.close()


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_everything_as_it_was(gs4d):
    n, m, first = 300, 3, 5
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    rec, rows = tc.records(gs4d, "4d_vel", n), tc.rows(("rigid", "retime", "full"))
    src, xf = ctx.buffer(rec), ctx.buffer(rows)
    dst_bytes = (first + m * n) * 96
    dst, short_dst, dead = fill(ctx, dst_bytes), fill(ctx, dst_bytes - 16), fill(ctx, 64)
    short_src, short_xf = ctx.buffer(rec.reshape(-1)[:-1]), ctx.buffer(rows.reshape(-1)[:-1])      # one float short
    long_xf = fill(ctx, 80 * (m + 1))
    ctx.delete(dead)                                            # (last: a buffer made from here on could take its name)

    def call(src=src, n=n, xf=xf, m=m, dst=dst, first=first):
        return lib.gs4d_transform_records(ctx._h, src, n, xf, m, dst, first)

    big = 1 << 32
    bad = {"n > 0xFFFFFFFF": dict(n=big), "m > 0xFFFFFFFF": dict(m=big), "dst_first > 0xFFFFFFFF": dict(first=big),
           "m * n > 0xFFFFFFFF": dict(n=1 << 16, m=1 << 16), "dst_first + m * n > 0xFFFFFFFF": dict(first=big - m * n),
           "m * n near 2^64": dict(n=big - 1, m=big - 1),
           "src too small": dict(src=short_src), "xf too small": dict(xf=short_xf), "dst too small": dict(dst=short_dst),
           "dst too small for dst_first": dict(first=first + 1), "dst too small for m": dict(m=m + 1, xf=long_xf),
           "src == dst": dict(src=dst), "xf == dst": dict(xf=dst), "src == xf": dict(xf=src)}
    for k in ("src", "xf", "dst"):
        bad.update({f"dead {k}": {k: dead}, f"no {k}": {k: 0}, f"unknown {k}": {k: 9999}})
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"transform_records" in lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and untouched(ctx, short_dst, dst_bytes - 16), "a refused call wrote something"
    assert unchanged(ctx, src, rec) and unchanged(ctx, xf, rows)
    assert call(n=0) == 0 and call(m=0) == 0 and call(n=0, m=0, first=0xFFFFFFFF) == -1      # (a no-op still needs room for dst_first records)
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and ctx.shadow_builds(dst) == 0
    # the call works after the refusals
    assert call() == 0
    got = ctx.read(dst, np.uint8, dst_bytes)
    assert (got[:first * 96] == SENTINEL).all()
    assert tc.same_bits(got[first * 96:].view(f32).reshape(m * n, 24), tc.expected(gs4d, rec, rows)).all()
    assert unchanged(ctx, src, rec) and unchanged(ctx, xf, rows)
    ctx.close()


# ---- 6. transforms that live in a torch tensor ---------------------------------------------------------------------------------------------------
def test_rows_written_on_the_device():
    """Context.write_tensor + transform from a device tensor on a torch side stream: a program of its own (tests/gpu_transform_from_torch.py) because
    torch has to initialise its HIP runtime before libgs4d.so is loaded."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_transform_from_torch.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "transform from torch ok" in r.stdout
