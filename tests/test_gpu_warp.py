"""GPU: gs4d_warp_records — every record of a set pushed through the map of a 4D lattice of displacement nodes, linearised at its centre (include/gs4d.h,
DESIGN.md §4).

Built to the plan of tests/test_gpu_pose.py: the records are compared word for word with the host definition (tests/warp_cases.py: equal as uint32, a
word that is a NaN on both sides of a warped record counting as equal, copied records byte-equal), with the rest of dst, guard buffers, src and nodes
compared against what was uploaded; pictures drawn from warped records are compared bit for bit with those of a fresh context that uploaded the
host-warped records; gs4d_debug_shadow_builds shows the one repack a call costs.  All calls go through the Python binding over the C ABI."""
import ctypes

import numpy as np
import pytest

import build_cases as bc
import staged_cases
import test_gpu_transform as tg
import transform_cases as tc
import warp_cases as wc
from test_gpu_pose import assert_same_device_records, same_bytes
from test_gpu_transform import GUARD, SENTINEL, Scene, bits, fill, host_frame, modes, picture_records, same, sorted_frame, untouched

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32
W, H, N = tg.W, tg.H, tg.N
IDENTITY = tc.rows(("identity",))


# ---- 1. the records ----------------------------------------------------------------------------------------------------------------------------
def one_call(gs4d, ctx, rec, node_values, lat, first, what, extra=3):
    n = rec.shape[0]
    guards = [fill(ctx, GUARD)]
    src = ctx.buffer(rec)
    guards.append(fill(ctx, GUARD))
    nodes = ctx.buffer(node_values)
    guards.append(fill(ctx, GUARD))
    host = np.full((first + n + extra) * 96 + 32, SENTINEL, np.uint8)
    dst = ctx.buffer(host)
    guards.append(fill(ctx, GUARD))
    assert ctx.warp_records(src, n, nodes, lat, dst=dst, dst_first=first) == dst
    got = ctx.read(dst, np.uint8, host.size)
    want = gs4d.warp_records_host(rec, node_values, lat)
    warped, copied, clamped = wc.by_the_text(rec, node_values, lat)[1:]
    wc.assert_records(got[first * 96:(first + n) * 96].view(f32), want, rec, warped, what)
    assert (got[:first * 96] == SENTINEL).all(), f"{what}: bytes of dst in front of record dst_first changed"
    assert (got[(first + n) * 96:] == SENTINEL).all(), f"{what}: bytes of dst behind the last record changed"
    assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
    assert same_bytes(ctx, src, rec) and same_bytes(ctx, nodes, node_values), f"{what}: src or nodes changed"
    for b in guards + [src, nodes, dst]:
        ctx.delete(b)
    return int(warped.sum()), int(copied.sum()), int(clamped.sum())


@pytest.mark.parametrize("which", wc.SETS)
def test_records_equal_the_host_definition(gs4d, which):
    ctx = gs4d.Context(64, 64)
    totals = np.zeros(3, np.int64)
    for what, rec, nodes, lat in wc.calls(gs4d, which):
        for first in (0, 7):
            totals += one_call(gs4d, ctx, rec, nodes, lat, first, f"{what}, dst_first = {first}")
    assert (totals > 1000).all(), totals                        # warped, copied, clamped
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_arrays_allocate_and_give_the_same_records(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 300
    rec = tc.records(gs4d, "4d_vel", n)
    lat = wc.lattice_for(gs4d, rec, (3, 2, 4, 5), 8)
    nodes = wc.nodes_for(gs4d, lat)
    src = ctx.buffer(rec)
    want = gs4d.warp_records_host(rec, nodes, lat)
    dst = ctx.warp_records(src, n, nodes.reshape(5, 4, 2, 3, 4), lat, dst_first=2)
    assert ctx.device_ptr(dst)[1] >= (2 + n) * 96
    assert wc.same_bits(ctx.read(dst, f32, n * 24, offset=2 * 96).reshape(n, 24), want).all()
    held = ctx.buffer(nodes)
    assert wc.same_bits(ctx.read(ctx.warp_records(src, n, held, lat), f32, n * 24).reshape(n, 24), want).all()
    with pytest.raises(ValueError):
        ctx.warp_records(src, n, nodes[:-1], lat)               # not the lattice's node count
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    rec = tc.records(gs4d, "hostile", 4)
    lat = wc.lattice_for(gs4d, rec, (2, 2, 2, 1))
    values = wc.nodes_for(gs4d, lat)
    src, nodes, dst = ctx.buffer(rec), ctx.buffer(values), fill(ctx, 96 * 8)
    ctx.warp_records(src, 0, nodes, lat, dst=dst)
    ctx.warp_records(src, 0, nodes, lat, dst=dst, dst_first=8)
    ctx.finish()
    assert untouched(ctx, dst, 96 * 8) and ctx.shadow_builds(dst) == 0 and same_bytes(ctx, src, rec) and same_bytes(ctx, nodes, values)
    ctx.close()


# ---- 2. equivalences on the device ---------------------------------------------------------------------------------------------------------------
# Two device calls are compared (tests/test_gpu_pose.py says why the bits of two kernels are promised only up to the sign and payload of a word that
# is a NaN in both): the bytes are demanded on the clean sets, whose results stay finite, and elsewhere every word that is not a NaN in both.
def test_a_zero_lattice_gives_the_bytes_of_transform_records_under_the_identity(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 769
    xf = ctx.buffer(IDENTITY)
    for which in wc.SETS:
        rec = tc.records(gs4d, which, n)
        src, a, b = ctx.buffer(rec), fill(ctx, n * 96), fill(ctx, n * 96)
        ctx.transform_records(src, n, xf, 1, dst=a)
        want = ctx.read(a, np.uint8, n * 96)
        for dims in wc.DIMS:
            lat = wc.lattice_for(gs4d, rec, dims, 0xF)
            zeros = np.zeros((wc.count_of(dims), 4), f32)
            ctx.warp_records(src, n, zeros, lat, dst=b)
            got = ctx.read(b, np.uint8, n * 96)
            if which != "hostile":                                                    # (every centre is clamped into the box: every record is warped)
                assert_same_device_records(want, got, which, f"dims {dims}", True)
            else:                                                                     # Sigma and the colour: the identity row makes NaNs of an Inf centre
                warped = wc.by_the_text(rec, zeros, lat)[1]
                assert warped.sum() > 700
                assert wc.same_bits(got.view(f32).reshape(n, 24)[warped, 4:], want.view(f32).reshape(n, 24)[warped, 4:]).all(), f"{which}, dims {dims}"
    ctx.close()


def test_two_equal_nodes_on_an_axis_give_the_bytes_of_one_node(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 769
    for which in wc.SETS:
        rec = tc.records(gs4d, which, n)
        src, a, b = ctx.buffer(rec), fill(ctx, n * 96), fill(ctx, n * 96)
        for what, nodes, lat, nodes2, lat2 in wc.equal_node_pairs(gs4d, rec):
            ctx.warp_records(src, n, nodes, lat, dst=a)
            ctx.warp_records(src, n, nodes2, lat2, dst=b)
            one, two = ctx.read(a, np.uint8, n * 96), ctx.read(b, np.uint8, n * 96)
            if which != "hostile":
                assert_same_device_records(one, two, which, what, True)
            else:                                                                     # the records both calls warp (a NaN centre on the axis is copied by one)
                both = wc.by_the_text(rec, nodes, lat)[1] & wc.by_the_text(rec, nodes2, lat2)[1]
                assert both.sum() > 100
                assert wc.same_bits(one.view(f32).reshape(n, 24)[both], two.view(f32).reshape(n, 24)[both]).all(), f"{which}, {what}"
    ctx.close()


# ---- 3. pictures, the repack ---------------------------------------------------------------------------------------------------------------------
PICTURE_DIMS = {"static": (4, 3, 3, 1), "time": (3, 3, 2, 3)}


def picture_lattice(gs4d, rec, shape, seed=0):
    """a lattice over the picture set that holds roughly half its centres, with a field of some tenths of the box"""
    lat = wc.lattice_for(gs4d, rec, PICTURE_DIMS[shape])
    return lat, wc.nodes_for(gs4d, lat, "smooth", seed)


def warped_frame(s, mode, t, warp=None):
    """Scene.frame with a warp call in the place of the transform, the documented order: (shade), warp, keygen, sort, draw"""
    c, gs4d = s.ctx, s.gs4d
    c.clear()
    c.set_uniforms(time=t, min_opacity=0.0, view=s.view, proj=s.proj)
    if warp is not None:
        src, n, nodes, lat = warp
        c.warp_records(src, n, nodes, lat, dst=s.db)
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
@pytest.mark.parametrize("shape", tuple(PICTURE_DIMS))
@pytest.mark.parametrize("form", bc.FORMS)
def test_pictures_from_warped_records_equal_those_from_uploaded_records(gs4d, form, shape, mode):
    mode, t = modes(gs4d)[mode], bc.picture_time(form)
    rec = picture_records(gs4d, form)
    lat, values = picture_lattice(gs4d, rec, shape)
    want_rec = gs4d.warp_records_host(rec, values, lat)
    warped = wc.by_the_text(rec, values, lat)[1]
    assert 50 < warped.sum() < N - 50
    want = host_frame(gs4d, want_rec, mode, t, outputs=True)
    plain = host_frame(gs4d, rec, mode, t)
    s = Scene(gs4d, N, outputs=True)
    warp = (s.ctx.buffer(rec), N, s.ctx.buffer(values), lat)
    assert s.ctx.shadow_builds(s.db) == 0
    warped_frame(s, mode, t, warp)
    got = s.read()
    same(got, want)
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert int((np.abs(got[0] - clear).max(-1) > 1.0 / 255.0).sum()) > 100, "an empty frame"
    assert not np.array_equal(bits(got[0]), bits(plain[0])), "the warped set gives the picture of the set as it was: the test shows nothing"
    # the repack: one for the call followed by a draw, none for a second draw, one more for the next call
    assert s.ctx.shadow_builds(s.db) == 1
    warped_frame(s, mode, t)
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 1, "a second draw repacked"
    warped_frame(s, mode, t, warp)
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 2, "a call must make the next draw repack exactly once"
    s.ctx.finish()
    s.ctx.close()


# ---- 4. ordering without a finish ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tuple(PICTURE_DIMS))
def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch, shape):
    """a call into the buffer that the previous lane's draw still reads: that frame keeps the old set; host writes into nodes and src right behind
    the call do not change its result; warp, keygen, sort and draw are queued back to back"""
    monkeypatch.setenv("GS4D_LANES", "4")
    mode, t = gs4d.MODE_4D_SORTED, bc.T
    old_rec = picture_records(gs4d, "4d_vel", seed=0x4256)
    src_rec = picture_records(gs4d, "4d_2q", seed=0x4257)
    lat, values = picture_lattice(gs4d, src_rec, shape, 1)
    new_rec = gs4d.warp_records_host(src_rec, values, lat)
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
    src, nodes, out = s.ctx.buffer(src_rec), s.ctx.buffer(values), s.ctx.buffer(nbytes=W * H * 4)
    for _ in range(3):
        s.frame(mode, t)                                        # frames in flight that read the old records and their shadow
    warped_frame(s, mode, t, (src, N, nodes, lat))              # the call is the first of the next lane's frame
    s.ctx.subdata(nodes, np.zeros_like(values))                 # directly behind: the call must not see the zeros
    s.ctx.subdata(src, np.zeros_like(src_rec))
    s.ctx.read_frame_rgba8_device(1, s.ctx.device_ptr(out)[0], W * H * 4)
    got = s.read()
    s.ctx.finish()
    assert np.array_equal(s.ctx.read(out, np.uint8, W * H * 4), want_prev), "the frame before the call shows another set than it was drawn with"
    same(got, want)
    assert not np.array_equal(bits(got[0]), bits(host_frame(gs4d, old_rec, mode, t)[0])), "the two sets give the same picture: the test shows nothing"
    assert wc.same_bits(s.ctx.read(s.db, f32, N * 24).reshape(N, 24), new_rec).all(), "the records are not those of src and nodes as they were at the call"
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
    src_rec = tc.records(gs4d, "3d", n)
    lat = wc.lattice_for(gs4d, src_rec, (3, 2, 4, 1))
    values = wc.nodes_for(gs4d, lat)
    fresh = gs4d.Context(Wb, Hb)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    sorted_frame(gs4d, fresh, (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n)), n, staged_cases.T1)
    want = fresh.read_pixels()
    fresh.close()
    ctx = gs4d.Context(Wb, Hb)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    src, nodes = ctx.buffer(src_rec), ctx.buffer(values)
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    ctx.warp_records(src, n, nodes, lat, dst=bufs[0])                                  # no read-back in between
    s1 = ctx.stats()
    assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    got = ctx.read_pixels()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"
    assert wc.same_bits(ctx.read(bufs[0], f32, n * 24).reshape(n, 24), gs4d.warp_records_host(src_rec, values, lat)).all()
    ctx.close()


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_everything_as_it_was(gs4d):
    n, first = 300, 5
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    rec = tc.records(gs4d, "4d_vel", n)
    good = wc.lattice_for(gs4d, rec, (3, 2, 4, 5), 8)
    values = wc.nodes_for(gs4d, good)
    src, nodes = ctx.buffer(rec), ctx.buffer(values)
    dst_bytes = (first + n) * 96
    dst, short_dst, dead = fill(ctx, dst_bytes), fill(ctx, dst_bytes - 16), fill(ctx, 64)
    short_src, short_nodes = ctx.buffer(rec.reshape(-1)[:-1]), ctx.buffer(values.reshape(-1)[:-1])
    ctx.delete(dead)                                            # (last: a buffer made from here on could take its name)

    def call(src=src, n=n, nodes=nodes, lat=good, dst=dst, first=first):
        return lib.gs4d_warp_records(ctx._h, src, n, nodes, ctypes.byref(lat) if lat is not None else None, dst, first)

    big = 1 << 32
    more = wc.lattice_for(gs4d, rec, (3, 2, 4, 6), 8)           # one layer of nodes more than the buffer holds
    bad = {"lat == NULL": dict(lat=None), "n > 0xFFFFFFFF": dict(n=big), "dst_first > 0xFFFFFFFF": dict(first=big), "dst_first + n > 0xFFFFFFFF": dict(first=big - n),
           "src too small": dict(src=short_src), "nodes too small": dict(nodes=short_nodes), "nodes too small for the dims": dict(lat=more),
           "dst too small": dict(dst=short_dst), "dst too small for dst_first": dict(first=first + 1),
           "src == dst": dict(src=dst), "nodes == dst": dict(nodes=dst), "src == nodes": dict(nodes=src)}
    bad.update({what: dict(lat=lat) for what, lat in wc.refused_lattices(gs4d).items()})
    for k in ("src", "nodes", "dst"):
        bad.update({f"dead {k}": {k: dead}, f"no {k}": {k: 0}, f"unknown {k}": {k: 9999}})
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"warp_records" in lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and untouched(ctx, short_dst, dst_bytes - 16), "a refused call wrote something"
    assert same_bytes(ctx, src, rec) and same_bytes(ctx, nodes, values)
    assert call(n=0) == 0 and call(n=0, first=0xFFFFFFFF) == -1          # (a no-op still needs room for dst_first records)
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and ctx.shadow_builds(dst) == 0
    # the call works after the refusals
    assert call() == 0
    got = ctx.read(dst, np.uint8, dst_bytes)
    assert (got[:first * 96] == SENTINEL).all()
    assert wc.same_bits(got[first * 96:].view(f32).reshape(n, 24), gs4d.warp_records_host(rec, values, good)).all()
    assert same_bytes(ctx, src, rec) and same_bytes(ctx, nodes, values)
    ctx.close()


# ---- 6. nodes updated per frame ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tuple(PICTURE_DIMS))
def test_nodes_updated_per_frame(gs4d, shape):
    """three frames, each a subdata of new nodes followed by warp, keygen, sort and draw with no finish in between: every frame's picture is that of
    the host-warped set"""
    mode, t = gs4d.MODE_4D_SORTED, bc.T
    rec = picture_records(gs4d, "4d_vel")
    lat, first = picture_lattice(gs4d, rec, shape)
    fields = [first * f32(0.5 + 0.75 * f) for f in range(3)]                          # the deformation grows
    s = Scene(gs4d, N)
    src, nodes = s.ctx.buffer(rec), s.ctx.buffer(nbytes=first.nbytes)
    outs = [s.ctx.buffer(nbytes=W * H * 4) for _ in fields]
    for values, out in zip(fields, outs):
        s.ctx.subdata(nodes, values)
        warped_frame(s, mode, t, (src, N, nodes, lat))
        s.ctx.read_frame_rgba8_device(0, s.ctx.device_ptr(out)[0], W * H * 4)
    s.ctx.finish()
    got = [s.ctx.read(out, np.uint8, W * H * 4) for out in outs]
    assert s.ctx.shadow_builds(s.db) == 3
    s.ctx.close()
    for f, values in enumerate(fields):
        ref = Scene(gs4d, N, gs4d.warp_records_host(rec, values, lat))
        ref.frame(mode, t)
        out = ref.ctx.buffer(nbytes=W * H * 4)
        ref.ctx.read_frame_rgba8_device(0, ref.ctx.device_ptr(out)[0], W * H * 4)
        ref.ctx.finish()
        want = ref.ctx.read(out, np.uint8, W * H * 4)
        ref.ctx.close()
        assert np.array_equal(got[f], want), f"frame {f}: {int((got[f].reshape(-1, 4) != want.reshape(-1, 4)).any(1).sum())} pixels differ"
        assert f == 0 or not np.array_equal(got[f], got[f - 1]), "two frames show the same picture: the test shows nothing"
