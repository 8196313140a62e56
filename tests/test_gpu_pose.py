"""GPU: gs4d_pose_records — every record of a set under the map its bind row takes from a table, indexed or blended (include/gs4d.h).

Built to the plan of tests/test_gpu_transform.py: the records are compared word for word with the host definition (tests/pose_cases.py: equal as
uint32, a word that is a NaN on both sides of a transformed record counting as equal, copied records byte-equal), with the rest of dst, guard buffers,
src, xf and bind compared against what was uploaded; pictures drawn from posed records are compared bit for bit with those of a fresh context that
uploaded the host-posed records; gs4d_debug_shadow_builds shows the one repack a call costs.  All calls go through the Python binding over the C ABI."""
import numpy as np
import pytest

import build_cases as bc
import pose_cases as pc
import staged_cases
import test_gpu_transform as tg
import transform_cases as tc
from test_gpu_transform import GUARD, SENTINEL, Scene, bits, fill, host_frame, modes, picture_records, same, sorted_frame, untouched

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32
W, H, N, PLACES, A, C = tg.W, tg.H, tg.N, tg.PLACES, tg.A, tg.C


def same_bytes(ctx, buf, a):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return np.array_equal(ctx.read(buf, np.uint8, a.size), a)


# ---- 1. the records ----------------------------------------------------------------------------------------------------------------------------
def one_call(gs4d, ctx, rec, m, form, stride, first, call, what, extra=3):
    n = rec.shape[0]
    xf_rows, table = pc.xf_table(m, call), pc.bind_bytes(gs4d, form, n, m, stride, seed=call)
    guards = [fill(ctx, GUARD)]
    src = ctx.buffer(rec)
    guards.append(fill(ctx, GUARD))
    xf = ctx.buffer(xf_rows) if m else fill(ctx, 80)
    guards.append(fill(ctx, GUARD))
    bind = ctx.buffer(table)
    guards.append(fill(ctx, GUARD))
    host = np.full((first + n + extra) * 96 + 32, SENTINEL, np.uint8)
    dst = ctx.buffer(host)
    guards.append(fill(ctx, GUARD))
    assert ctx.pose_records(src, n, xf, bind, form, m, stride, dst=dst, dst_first=first) == dst
    got = ctx.read(dst, np.uint8, host.size)
    want = pc.expected(gs4d, rec, xf_rows, table, form, stride)
    moved = pc.by_the_text(rec, xf_rows, table, form, stride)[1]
    pc.assert_records(got[first * 96:(first + n) * 96].view(f32), want, rec, moved, what)
    assert (got[:first * 96] == SENTINEL).all(), f"{what}: bytes of dst in front of record dst_first changed"
    assert (got[(first + n) * 96:] == SENTINEL).all(), f"{what}: bytes of dst behind the last record changed"
    assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
    assert same_bytes(ctx, src, rec) and same_bytes(ctx, bind, table) and (same_bytes(ctx, xf, xf_rows) if m else untouched(ctx, xf, 80)), f"{what}: src, xf or bind changed"
    for b in guards + [src, xf, bind, dst]:
        ctx.delete(b)
    return int(moved.sum()), int((~moved).sum())


@pytest.mark.parametrize("which", pc.SETS)
def test_records_equal_the_host_definition(gs4d, which):
    ctx = gs4d.Context(64, 64)
    call = moved = copied = 0
    for n in pc.SIZES + (pc.WALK_N,):
        rec = tc.records(gs4d, which, n)
        for m in pc.TABLE_SIZES if n != pc.WALK_N else (3, pc.LDS_ROWS, pc.LDS_ROWS + 1):
            for fname, form in pc.FORMS.items():
                for first in (0, 7):
                    stride = pc.STRIDES[form][(call // 4) % 2]             # (five table sizes: every one meets both strides over the sizes)
                    a, b = one_call(gs4d, ctx, rec, m, form, stride, first, call, f"{which}, n = {n}, m = {m}, {fname}, stride {stride}, dst_first = {first}")
                    moved, copied, call = moved + a, copied + b, call + 1
    assert moved > 1000 and copied > 1000
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_arrays_allocate_and_give_the_same_records(gs4d):
    ctx = gs4d.Context(64, 64)
    n, m = 300, 3
    rec, xf = tc.records(gs4d, "4d_vel", n), pc.xf_table(m, 1)
    src = ctx.buffer(rec)
    idx = pc.index_bind(n, m)
    dst = ctx.pose_records(src, n, xf, idx, dst_first=2)
    assert ctx.device_ptr(dst)[1] >= (2 + n) * 96
    assert pc.same_bits(ctx.read(dst, f32, n * 24, offset=2 * 96).reshape(n, 24), gs4d.pose_records_host(rec, xf, idx)).all()
    rows = gs4d.bind_rows(*pc.blend_bind(n, m))
    dst = ctx.pose_records(src, n, xf, rows)
    assert pc.same_bits(ctx.read(dst, f32, n * 24).reshape(n, 24), gs4d.pose_records_host(rec, xf, rows)).all()
    with pytest.raises(TypeError):
        ctx.pose_records(src, n, ctx.buffer(xf), idx)           # a table buffer needs its m
    with pytest.raises(TypeError):
        ctx.pose_records(src, n, xf, ctx.buffer(idx))           # a bind buffer needs its form
    ctx.close()


def test_no_records_is_a_no_op_and_no_rows_is_a_copy(gs4d):
    ctx = gs4d.Context(64, 64)
    rec = tc.records(gs4d, "hostile", 4)
    src, xf, bind, dst = ctx.buffer(rec), ctx.buffer(pc.xf_table(1)), ctx.buffer(np.zeros(4, u32)), fill(ctx, 96 * 8)
    ctx.pose_records(src, 0, xf, bind, pc.INDEX, 1, dst=dst)
    ctx.finish()
    assert untouched(ctx, dst, 96 * 8) and ctx.shadow_builds(dst) == 0
    ctx.pose_records(src, 4, xf, bind, pc.INDEX, 0, dst=dst, dst_first=2)
    got = ctx.read(dst, np.uint8, 96 * 8)
    assert np.array_equal(got[2 * 96:6 * 96], rec.view(np.uint8).reshape(-1)) and (got[:2 * 96] == SENTINEL).all() and (got[6 * 96:] == SENTINEL).all()
    ctx.close()


# ---- 2. equivalences on the device ---------------------------------------------------------------------------------------------------------------
# Two device calls are compared here, and gs4d.h promises the bits of a device record only up to the sign and payload of a word that is a NaN on both
# sides: which of two NaN operands an instruction passes on depends on their order, and two kernels need not order them alike (measured: the inf row
# on the hostile set gives such words in gs4d_transform_records and in the INDEX form that differ).  So the bytes are demanded wherever no such word
# arises — the clean sets under the rows whose results stay finite, which is asserted — and everywhere else every word that is not a NaN in both.
def assert_same_device_records(a, b, which, name, finite):
    a, b = a.view(f32).reshape(-1, 24), b.view(f32).reshape(-1, 24)
    if which != "hostile" and finite:
        assert np.isfinite(a).all(), f"{which}, {name}: the clean case is not finite"
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{which}, {name}: the bytes differ"
    ok = pc.same_bits(a, b)
    assert ok.all(), f"{which}, {name}: {int((~ok).any(1).sum())} records differ, first word at {np.argwhere(~ok)[0].tolist()}"


def test_index_zero_gives_the_bytes_of_transform_records(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 769
    zeros = ctx.buffer(np.zeros(n, u32))
    for which in pc.SETS:
        rec = tc.records(gs4d, which, n)
        src, a, b = ctx.buffer(rec), fill(ctx, n * 96), fill(ctx, n * 96)
        for name in tc.NAMES:
            xf = ctx.buffer(tc.rows((name,)))
            ctx.transform_records(src, n, xf, 1, dst=a)
            ctx.pose_records(src, n, xf, zeros, pc.INDEX, 1, dst=b)
            assert_same_device_records(ctx.read(a, np.uint8, n * 96), ctx.read(b, np.uint8, n * 96), which, name, name in tc.FINITE)
    ctx.close()


def test_weight_one_rows_give_the_bytes_of_the_index_call(gs4d):
    ctx = gs4d.Context(64, 64)
    for tname, table in (("finite", pc.weight_one_table(tc.FINITE)), ("all", pc.weight_one_table())):
        m, n = table.shape[0], 769
        xf = ctx.buffer(table)
        idx, rows = pc.weight_one_binds(gs4d, n, m)
        bi, bb = ctx.buffer(idx), ctx.buffer(rows)
        for which in pc.SETS:
            rec = tc.records(gs4d, which, n)
            src, a, b = ctx.buffer(rec), fill(ctx, n * 96), fill(ctx, n * 96)
            ctx.pose_records(src, n, xf, bi, pc.INDEX, m, dst=a)
            ctx.pose_records(src, n, xf, bb, pc.BLEND4, m, dst=b)
            got = ctx.read(b, np.uint8, n * 96)
            assert_same_device_records(ctx.read(a, np.uint8, n * 96), got, which, tname, tname == "finite")
            assert pc.same_bits(got.view(f32).reshape(n, 24), gs4d.pose_records_host(rec, table, idx)).all(), which
    ctx.close()


# ---- 3. pictures, the repack ---------------------------------------------------------------------------------------------------------------------
def picture_bind(gs4d, fname):
    """half the set bound to PLACES[0], half to PLACES[1]; BLEND4: a band between them blended half and half"""
    half = (np.arange(N) >= N // 2).astype(u32)
    if fname == "index":
        return half
    j = np.stack([half, np.full(N, pc.ID_NONE, u32)], 1)
    w = np.tile(np.array([1.0, 0.0], f32), (N, 1))
    band = slice(N // 2 - 30, N // 2 + 30)
    j[band], w[band] = (0, 1), (0.5, 0.5)
    return gs4d.bind_rows(j, w)


def posed_frame(s, mode, t, pose=None):
    """Scene.frame with a pose call in the place of the transform, the documented order: (shade), pose, keygen, sort, draw"""
    c, gs4d = s.ctx, s.gs4d
    c.clear()
    c.set_uniforms(time=t, min_opacity=0.0, view=s.view, proj=s.proj)
    if pose is not None:
        src, n, xf, m, bind, form = pose
        c.pose_records(src, n, xf, bind, form, m, dst=s.db)
    if mode == gs4d.MODE_4D_SORTED:
        c.keygen(s.db, t, tg.CAM, s.kb, s.ib, s.n)
        c.sort_pairs(s.kb, s.ib, s.n)
    c.set_mode(mode)
    if mode == gs4d.MODE_4D_SORTED:
        c.bind(1, s.ib)
        c.bind(2, s.db)
    else:
        c.bind(1, s.db)                                         # (instance k is record k)
    c.draw_instanced(s.n)


@pytest.mark.parametrize("mode", ("sorted", "direct"))
@pytest.mark.parametrize("fname", tuple(pc.FORMS))
@pytest.mark.parametrize("form", bc.FORMS)
def test_pictures_from_posed_records_equal_those_from_uploaded_records(gs4d, form, fname, mode):
    mode, t = modes(gs4d)[mode], A * bc.picture_time(form) + C
    rec, table = picture_records(gs4d, form), picture_bind(gs4d, fname)
    want_rec = gs4d.pose_records_host(rec, PLACES, table)
    want = host_frame(gs4d, want_rec, mode, t, outputs=True)
    s = Scene(gs4d, N, outputs=True)
    pose = (s.ctx.buffer(rec), N, s.ctx.buffer(PLACES), 2, s.ctx.buffer(table), pc.FORMS[fname])
    assert s.ctx.shadow_builds(s.db) == 0
    posed_frame(s, mode, t, pose)
    got = s.read()
    same(got, want)
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert int((np.abs(got[0] - clear).max(-1) > 1.0 / 255.0).sum()) > 100, "an empty frame"
    # the repack: one for the call followed by a draw, none for a second draw, one more for the next call
    assert s.ctx.shadow_builds(s.db) == 1
    posed_frame(s, mode, t)
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 1, "a second draw repacked"
    posed_frame(s, mode, t, pose)
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 2, "a call must make the next draw repack exactly once"
    s.ctx.finish()
    s.ctx.close()


# ---- 4. ordering without a finish ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", tuple(pc.FORMS))
def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch, fname):
    """a call into the buffer that the previous lane's draw still reads: that frame keeps the old set; host writes into xf, bind and src right behind
    the call do not change its result; pose, keygen, sort and draw are queued back to back"""
    monkeypatch.setenv("GS4D_LANES", "4")
    mode, t = gs4d.MODE_4D_SORTED, A * bc.T + C
    table = picture_bind(gs4d, fname)
    old_rec = gs4d.pose_records_host(picture_records(gs4d, "4d_vel", seed=0x4256), PLACES, table)
    src_rec = picture_records(gs4d, "4d_2q", seed=0x4257)
    new_rec = gs4d.pose_records_host(src_rec, PLACES, table)
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
    src, xf, bind, out = s.ctx.buffer(src_rec), s.ctx.buffer(PLACES), s.ctx.buffer(table), s.ctx.buffer(nbytes=W * H * 4)
    for _ in range(3):
        s.frame(mode, t)                                        # frames in flight that read the old records and their shadow
    posed_frame(s, mode, t, (src, N, xf, 2, bind, pc.FORMS[fname]))      # the call is the first of the next lane's frame
    s.ctx.subdata(xf, np.zeros_like(PLACES))                    # directly behind: the call must not see the zeros
    s.ctx.subdata(bind, np.zeros_like(table))
    s.ctx.subdata(src, np.zeros_like(src_rec))
    s.ctx.read_frame_rgba8_device(1, s.ctx.device_ptr(out)[0], W * H * 4)
    got = s.read()
    s.ctx.finish()
    assert np.array_equal(s.ctx.read(out, np.uint8, W * H * 4), want_prev), "the frame before the call shows another set than it was drawn with"
    same(got, want)
    assert not np.array_equal(bits(got[0]), bits(host_frame(gs4d, old_rec, mode, t)[0])), "the two sets give the same picture: the test shows nothing"
    assert pc.same_bits(s.ctx.read(s.db, f32, N * 24).reshape(N, 24), new_rec).all(), "the records are not those of src, xf and bind as they were at the call"
    assert s.ctx.shadow_builds(s.db) == 2
    s.ctx.close()


def test_a_call_waits_for_a_rerun(gs4d, monkeypatch):
    """staged_cases' case a (as tests/test_gpu_transform.py): frames at T0 teach the guesses, the frame at T1 outgrows a segment block; the call into
    its record buffer settles the draw first — the re-run uses the old records"""
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    rec, _ = staged_cases.build(gs4d, "a")
    Wb, Hb, n = staged_cases.W, staged_cases.H, rec.shape[0]
    m = 3
    src_rec, rows = tc.records(gs4d, "3d", n), tc.rows(("scale_shear", "rigid", "full"))
    table = gs4d.bind_rows(*pc.blend_bind(n, m))
    fresh = gs4d.Context(Wb, Hb)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    sorted_frame(gs4d, fresh, (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n)), n, staged_cases.T1)
    want = fresh.read_pixels()
    fresh.close()
    ctx = gs4d.Context(Wb, Hb)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    src, xf, bind = ctx.buffer(src_rec), ctx.buffer(rows), ctx.buffer(table)
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    ctx.pose_records(src, n, xf, bind, pc.BLEND4, m, dst=bufs[0])                 # no read-back in between
    s1 = ctx.stats()
    assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    got = ctx.read_pixels()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"
    assert pc.same_bits(ctx.read(bufs[0], f32, n * 24).reshape(n, 24), gs4d.pose_records_host(src_rec, rows, table)).all()
    ctx.close()


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_everything_as_it_was(gs4d):
    n, m, first, stride = 300, 3, 5, 48
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    rec, rows = tc.records(gs4d, "4d_vel", n), pc.xf_table(m)
    table = pc.bind_bytes(gs4d, pc.BLEND4, n, m, stride)
    src, xf, bind = ctx.buffer(rec), ctx.buffer(rows), ctx.buffer(table)
    dst_bytes = (first + n) * 96
    dst, short_dst, dead = fill(ctx, dst_bytes), fill(ctx, dst_bytes - 16), fill(ctx, 64)
    short_src, short_xf, short_bind = ctx.buffer(rec.reshape(-1)[:-1]), ctx.buffer(rows.reshape(-1)[:-1]), ctx.buffer(table[:-16])
    ctx.delete(dead)                                            # (last: a buffer made from here on could take its name)

    def call(src=src, n=n, xf=xf, m=m, bind=bind, form=pc.BLEND4, stride=stride, dst=dst, first=first):
        return lib.gs4d_pose_records(ctx._h, src, n, xf, m, bind, form, stride, dst, first)

    big = 1 << 32
    bad = {"n > 0xFFFFFFFF": dict(n=big), "m > 0xFFFFFFFF": dict(m=big), "dst_first > 0xFFFFFFFF": dict(first=big),
           "dst_first + n > 0xFFFFFFFF": dict(first=big - n), "unknown form 2": dict(form=2), "unknown form": dict(form=0xFFFFFFFF),
           "blend stride 16": dict(stride=16), "blend stride 0": dict(stride=0), "blend stride 40": dict(stride=40),
           "index stride 0": dict(form=pc.INDEX, stride=0), "index stride 2": dict(form=pc.INDEX, stride=2), "index stride 6": dict(form=pc.INDEX, stride=6),
           "src too small": dict(src=short_src), "xf too small": dict(xf=short_xf), "bind too small": dict(bind=short_bind), "dst too small": dict(dst=short_dst),
           "dst too small for dst_first": dict(first=first + 1), "xf too small for m": dict(m=m + 1), "bind too small for the stride": dict(stride=64),
           "src == dst": dict(src=dst), "xf == dst": dict(xf=dst), "bind == dst": dict(bind=dst), "src == xf": dict(xf=src), "src == bind": dict(bind=src),
           "xf == bind": dict(bind=xf)}
    for k in ("src", "xf", "bind", "dst"):
        bad.update({f"dead {k}": {k: dead}, f"no {k}": {k: 0}, f"unknown {k}": {k: 9999}})
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"pose_records" in lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and untouched(ctx, short_dst, dst_bytes - 16), "a refused call wrote something"
    assert same_bytes(ctx, src, rec) and same_bytes(ctx, xf, rows) and same_bytes(ctx, bind, table)
    assert call(n=0) == 0 and call(n=0, first=0xFFFFFFFF) == -1          # (a no-op still needs room for dst_first records)
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and ctx.shadow_builds(dst) == 0
    # the call works after the refusals; the same bytes are a table of the INDEX form too (the word at the start of every row)
    assert call() == 0
    got = ctx.read(dst, np.uint8, dst_bytes)
    assert (got[:first * 96] == SENTINEL).all()
    assert pc.same_bits(got[first * 96:].view(f32).reshape(n, 24), pc.expected(gs4d, rec, rows, table, pc.BLEND4, stride)).all()
    assert call(form=pc.INDEX, m=0) == 0
    assert np.array_equal(ctx.read(dst, np.uint8, n * 96, offset=first * 96), rec.view(np.uint8).reshape(-1))
    assert same_bytes(ctx, src, rec) and same_bytes(ctx, xf, rows) and same_bytes(ctx, bind, table)
    ctx.close()


# ---- 6. a table updated per frame ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", tuple(pc.FORMS))
def test_a_table_updated_per_frame(gs4d, fname):
    """three frames, each a subdata of a new xf followed by pose, keygen, sort and draw with no finish in between: every frame's picture is that of
    the host-posed set"""
    mode, t = gs4d.MODE_4D_SORTED, A * bc.T + C
    rec, table = picture_records(gs4d, "4d_vel"), picture_bind(gs4d, fname)
    tables = []
    for f in range(3):
        rows = PLACES.copy()
        rows[:, 16] += f32(12.0 * f)                            # the two halves drift in x
        rows[1, 17] -= f32(9.0 * f)
        tables.append(rows)
    s = Scene(gs4d, N)
    src, xf, bind = s.ctx.buffer(rec), s.ctx.buffer(nbytes=PLACES.nbytes), s.ctx.buffer(table)
    outs = [s.ctx.buffer(nbytes=W * H * 4) for _ in tables]
    for rows, out in zip(tables, outs):
        s.ctx.subdata(xf, rows)
        posed_frame(s, mode, t, (src, N, xf, 2, bind, pc.FORMS[fname]))
        s.ctx.read_frame_rgba8_device(0, s.ctx.device_ptr(out)[0], W * H * 4)
    s.ctx.finish()
    got = [s.ctx.read(out, np.uint8, W * H * 4) for out in outs]
    assert s.ctx.shadow_builds(s.db) == 3
    s.ctx.close()
    for f, rows in enumerate(tables):
        ref = Scene(gs4d, N, gs4d.pose_records_host(rec, rows, table))
        ref.frame(mode, t)
        out = ref.ctx.buffer(nbytes=W * H * 4)
        ref.ctx.read_frame_rgba8_device(0, ref.ctx.device_ptr(out)[0], W * H * 4)
        ref.ctx.finish()
        want = ref.ctx.read(out, np.uint8, W * H * 4)
        ref.ctx.close()
        assert np.array_equal(got[f], want), f"frame {f}: {int((got[f] != want).any() and (got[f].reshape(-1, 4) != want.reshape(-1, 4)).any(1).sum())} pixels differ"
        assert f == 0 or not np.array_equal(got[f], got[f - 1]), "two frames show the same picture: the test shows nothing"
