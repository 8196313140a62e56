"""GPU: gs4d_rotate_sh — an SH table turned with the maps that move its records (include/gs4d.h).

The rows are compared word for word with the host definition (tests/sh_rotate_cases.py: equal as uint32, a word that is a NaN on both sides of a
rotated row counting as equal, copied rows and the kept words byte-equal) for all 12 instances of the kernel — degree 0..3 x GS4D_SH_EACH,
GS4D_POSE_INDEX, GS4D_POSE_BLEND4, with small and large tables of maps — on either side of every tile edge, at the three
kinds of stride and with dst_first > 0, with the rest of dst, guard buffers, src, xf and bind compared against what was uploaded.  The picture is
checked through existing calls only: the camera-inverse route of gs4d_transform_records against transform -> rotate_sh -> shade_sh, and the same
for a posed set of three objects.  All calls go through the Python binding over the C ABI."""
import numpy as np
import pytest

import pose_cases as pc
import sh_rotate_cases as rc
import shade_cases as sc
from test_gpu_transform import GUARD, SENTINEL, fill, untouched

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32
PATHS = {"each": (rc.EACH, (1, 3)), "index": (rc.INDEX, (3, 65)), "blend4": (rc.BLEND4, (5, 65))}


def same_bytes(ctx, buf, a):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return np.array_equal(ctx.read(buf, np.uint8, a.size), a)


# ---- 1. the rows -------------------------------------------------------------------------------------------------------------------------------
def one_call(gs4d, ctx, degree, n, stride, m, form, bind_stride, first, call, what, extra=3):
    t = rc.table(n, degree, stride, seed=0x5350 + call, hostile=bool(call % 2))
    maps = rc.map_table(gs4d, m, call)
    table = None if form == rc.EACH else pc.bind_bytes(gs4d, form, n, m, bind_stride, seed=call)
    total = m * n if form == rc.EACH else n
    guards = [fill(ctx, GUARD)]
    src = ctx.buffer(t)
    guards.append(fill(ctx, GUARD))
    xf = ctx.buffer(maps)
    guards.append(fill(ctx, GUARD))
    bind = 0 if table is None else ctx.buffer(table)
    guards.append(fill(ctx, GUARD))
    host = np.full((first + total + extra) * stride + 32, SENTINEL, np.uint8)
    dst = ctx.buffer(host)
    guards.append(fill(ctx, GUARD))
    assert ctx.rotate_sh(src, n, xf, degree, m=m, bind=bind or None, form=form, bind_stride=bind_stride, stride=stride, dst=dst, dst_first=first) == dst
    got = ctx.read(dst, np.uint8, host.size)
    want = gs4d.rotate_sh_host(t, maps, degree, table, None if table is None else form, bind_stride or None)
    rotated = rc.rotated_mask(gs4d, maps, n, table, form, bind_stride)
    source = np.tile(t, (m, 1)) if form == rc.EACH else t
    rc.assert_rows(got[first * stride:(first + total) * stride].view(f32), want, source, rotated, degree, what)
    assert (got[:first * stride] == SENTINEL).all(), f"{what}: bytes of dst in front of row dst_first changed"
    assert (got[(first + total) * stride:] == SENTINEL).all(), f"{what}: bytes of dst behind the last row changed"
    assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
    assert same_bytes(ctx, src, t) and same_bytes(ctx, xf, maps) and (table is None or same_bytes(ctx, bind, table)), f"{what}: src, xf or bind changed"
    for b in guards + [src, xf, dst] + ([bind] if bind else []):
        ctx.delete(b)
    return int((rotated & (degree > 0)).sum()), int((~rotated).sum())


@pytest.mark.parametrize("path", tuple(PATHS))
@pytest.mark.parametrize("degree", rc.DEGREES)
def test_rows_equal_the_host_definition(gs4d, degree, path):
    form, table_sizes = PATHS[path]
    ctx = gs4d.Context(64, 64)
    call = turned = copied = 0
    for n in rc.sizes(degree):
        for stride in rc.strides(degree):
            for m in table_sizes:
                first = (0, 7)[call % 2]
                bind_stride = 0 if form == rc.EACH else pc.STRIDES[form][(call // 2) % 2]
                a, b = one_call(gs4d, ctx, degree, n, stride, m, form, bind_stride, first, call,
                                f"degree {degree}, {path}, n = {n}, stride {stride}, m = {m}, bind_stride {bind_stride}, dst_first = {first}")
                turned, copied, call = turned + a, copied + b, call + 1
    assert degree == 0 or (turned > 1000 and copied > 100)
    ctx.finish()                                                # reports device-side check failures: hostile maps and rows are data
    ctx.close()


def test_arrays_allocate_and_give_the_same_rows(gs4d):
    ctx = gs4d.Context(64, 64)
    n, m, degree = 300, 3, 2
    t, maps = rc.table(n, degree, sc.row_bytes(degree)), rc.map_table(gs4d, m, 1)
    src = ctx.buffer(t)
    dst = ctx.rotate_sh(src, n, maps, degree, dst_first=2)                                    # EACH, the minimal stride, a new buffer
    assert ctx.device_ptr(dst)[1] >= (2 + m * n) * sc.row_bytes(degree)
    got = ctx.read(dst, f32, m * n * t.shape[1], offset=2 * sc.row_bytes(degree)).reshape(m * n, -1)
    assert rc.same_rows(got, gs4d.rotate_sh_host(t, maps, degree)).all()
    idx = pc.index_bind(n, m)
    dst = ctx.rotate_sh(src, n, maps, degree, bind=idx)
    assert rc.same_rows(ctx.read(dst, f32, t.size).reshape(t.shape), gs4d.rotate_sh_host(t, maps, degree, idx)).all()
    rows = gs4d.bind_rows(*pc.blend_bind(n, m))
    dst = ctx.rotate_sh(src, n, maps, degree, bind=rows)
    assert rc.same_rows(ctx.read(dst, f32, t.size).reshape(t.shape), gs4d.rotate_sh_host(t, maps, degree, rows)).all()
    with pytest.raises(TypeError):
        ctx.rotate_sh(src, n, maps, degree, bind=ctx.buffer(idx))                             # a bind buffer needs its form
    ctx.close()


def test_no_rows_and_no_maps(gs4d):
    ctx = gs4d.Context(64, 64)
    t = rc.table(4, 3, 208, hostile=True)
    src, xf, bind, dst = ctx.buffer(t), ctx.buffer(rc.map_table(gs4d, 1)), ctx.buffer(np.zeros(4, u32)), fill(ctx, 208 * 8)
    ctx.rotate_sh(src, 0, xf, 3, m=1, stride=208, dst=dst)                                    # n == 0
    ctx.rotate_sh(src, 4, xf, 3, m=0, stride=208, dst=dst)                                    # m == 0 with GS4D_SH_EACH
    ctx.rotate_sh(src, 0, xf, 3, m=1, bind=bind, form=rc.INDEX, stride=208, dst=dst)
    ctx.finish()
    assert untouched(ctx, dst, 208 * 8)
    ctx.rotate_sh(src, 4, xf, 3, m=0, bind=bind, form=rc.INDEX, stride=208, dst=dst, dst_first=2)      # m == 0 with a bind table: every row copied
    got = ctx.read(dst, np.uint8, 208 * 8)
    assert np.array_equal(got[2 * 208:6 * 208], t.view(np.uint8).reshape(-1)) and (got[:2 * 208] == SENTINEL).all() and (got[6 * 208:] == SENTINEL).all()
    ctx.close()


# ---- 2. the picture ----------------------------------------------------------------------------------------------------------------------------
def colours(ctx, buf, n):
    return ctx.read(buf, f32, n * 24).reshape(n, 24)[:, 4:7].copy()


@pytest.mark.parametrize("name", ("rigid", "scale_2"))
@pytest.mark.parametrize("which", ("3d", "4d"))
def test_the_camera_inverse_route_and_the_route_through_rotate_sh_give_one_picture(gs4d, which, name):
    n, degree, t, cam = rc.PICTURE_N, rc.PICTURE_DEGREE, rc.PICTURE_T, rc.PICTURE_CAM
    rec, rows = rc.picture_set(which)
    l = rc.picture_maps(gs4d)[name]
    assert np.linalg.norm(rec[:, :3] - np.asarray(cam, f32), axis=1).min() > 1.0
    ctx = gs4d.Context(64, 64)
    xf, sh = ctx.buffer(l.reshape(1, 20)), ctx.buffer(rows)
    # route A, the header's workaround: shade the source seen from M^-1 cam, then transform
    a_src = ctx.buffer(rec)
    ctx.shade_sh(a_src, n, sh, degree, t, rc.inverse_camera(l, cam))
    a = colours(ctx, ctx.transform_records(a_src, n, xf, 1), n)
    # route B, the new call: transform, rotate_sh, shade the result seen from cam
    b_rec = ctx.transform_records(ctx.buffer(rec), n, xf, 1)
    turned = ctx.rotate_sh(sh, n, xf, degree, m=1)
    ctx.shade_sh(b_rec, n, turned, degree, t, cam)
    b = colours(ctx, b_rec, n)
    # without the rotation the moved set shows the colours of the old orientation
    ctx.shade_sh(b_rec, n, sh, degree, t, cam)
    stale = colours(ctx, b_rec, n)
    ctx.finish()
    ctx.close()
    ratio = rc.colour_ratio(a, b, rows)
    print(f"{which}, {name}: the two routes differ by {ratio:.3g} sum |c_k| (the unrotated table: {rc.colour_ratio(a, stale, rows):.3g})")
    assert rc.PICTURE_BAR <= 1e-4
    assert ratio <= rc.PICTURE_BAR
    assert rc.colour_ratio(a, stale, rows) > 1000 * rc.PICTURE_BAR, "the rotation does not matter in this case: the test shows nothing"
    # the device routes are the host routes
    assert np.array_equal(a.view(u32), rc.route_a_host(rec, rows, l, cam, t).view(u32)) and np.array_equal(b.view(u32), rc.route_b_host(gs4d, rec, rows, l, cam, t).view(u32))


@pytest.mark.parametrize("which", ("3d", "4d"))
def test_a_posed_set_of_three_objects(gs4d, which):
    """pose_records with GS4D_POSE_INDEX over three objects, rotate_sh with the same xf and bind, shade_sh with the true camera — against the
    camera-inverse route object by object, and against three GS4D_SH_EACH calls on the three subsets"""
    n, degree, t, cam = rc.PICTURE_N, rc.PICTURE_DEGREE, rc.PICTURE_T, rc.PICTURE_CAM
    rec, rows = rc.picture_set(which)
    maps = rc.object_maps(gs4d)
    obj = (np.arange(n) * 7 % 3).astype(u32)
    ctx = gs4d.Context(64, 64)
    xf, bind, sh = ctx.buffer(maps), ctx.buffer(obj), ctx.buffer(rows)
    posed = ctx.pose_records(ctx.buffer(rec), n, xf, bind, rc.INDEX, 3)
    turned = ctx.rotate_sh(sh, n, xf, degree, m=3, bind=bind, form=rc.INDEX)
    ctx.shade_sh(posed, n, turned, degree, t, cam)
    b = colours(ctx, posed, n)
    got_rows = ctx.read(turned, f32, rows.size).reshape(rows.shape)
    worst = 0.0
    for k in range(3):
        sub = np.flatnonzero(obj == k)
        one = ctx.buffer(maps[k:k + 1])
        a_src = ctx.buffer(rec[sub])
        ctx.shade_sh(a_src, sub.size, ctx.buffer(rows[sub]), degree, t, rc.inverse_camera(maps[k], cam))
        a = colours(ctx, ctx.transform_records(a_src, sub.size, one, 1), sub.size)
        worst = max(worst, rc.colour_ratio(a, b[sub], rows[sub]))
        each = ctx.rotate_sh(ctx.buffer(rows[sub]), sub.size, one, degree, m=1)
        assert np.array_equal(ctx.read(each, u32, sub.size * rows.shape[1]).reshape(sub.size, -1), got_rows[sub].view(u32)), f"object {k}: EACH and INDEX rows differ"
    ctx.finish()
    ctx.close()
    print(f"{which}: the posed set differs from the camera-inverse route by {worst:.3g} sum |c_k|")
    assert rc.PICTURE_BAR <= 1e-4 and worst <= rc.PICTURE_BAR


# ---- 3. argument errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_everything_as_it_was(gs4d):
    n, m, first, stride, bs, degree = 300, 3, 5, 208, 48, 3
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    t, maps = rc.table(n, degree, stride), rc.map_table(gs4d, m)
    table = pc.bind_bytes(gs4d, rc.BLEND4, n, m, bs)
    src, xf, bind = ctx.buffer(t), ctx.buffer(maps), ctx.buffer(table)
    dst_bytes = (first + n) * stride
    dst, short_dst, dead = fill(ctx, dst_bytes), fill(ctx, dst_bytes - 16), fill(ctx, 64)
    each_dst = fill(ctx, (first + m * n) * stride - 16)                                      # one piece short of what GS4D_SH_EACH writes
    short_src, short_xf, short_bind = ctx.buffer(t.reshape(-1)[:-1]), ctx.buffer(maps.reshape(-1)[:-1]), ctx.buffer(table[:-16])
    ctx.delete(dead)                                            # (last: a buffer made from here on could take its name)

    def call(src=src, n=n, stride=stride, degree=degree, xf=xf, m=m, bind=bind, form=rc.BLEND4, bs=bs, dst=dst, first=first):
        return lib.gs4d_rotate_sh(ctx._h, src, n, stride, degree, xf, m, bind, form, bs, dst, first)

    big = 1 << 32
    bad = {"n > 0xFFFFFFFF": dict(n=big), "m > 0xFFFFFFFF": dict(m=big), "dst_first > 0xFFFFFFFF": dict(first=big), "dst_first + n > 0xFFFFFFFF": dict(first=big - n),
           "m * n > 0xFFFFFFFF": dict(form=rc.EACH, bind=0, n=1 << 16, m=1 << 16), "degree -1": dict(degree=-1), "degree 4": dict(degree=4),
           "stride 0": dict(stride=0), "stride 24": dict(stride=24), "stride 1040": dict(stride=1040), "stride below the degree's": dict(stride=176),
           "unknown form 3": dict(form=3), "unknown form": dict(form=0xFFFFFFFF), "bind with EACH": dict(form=rc.EACH), "no bind with BLEND4": dict(bind=0),
           "no bind with INDEX": dict(form=rc.INDEX, bind=0, bs=4), "blend stride 16": dict(bs=16), "blend stride 0": dict(bs=0), "blend stride 40": dict(bs=40),
           "index stride 0": dict(form=rc.INDEX, bs=0), "index stride 2": dict(form=rc.INDEX, bs=2), "index stride 6": dict(form=rc.INDEX, bs=6),
           "src too small": dict(src=short_src), "xf too small": dict(xf=short_xf), "bind too small": dict(bind=short_bind), "dst too small": dict(dst=short_dst),
           "dst too small for dst_first": dict(first=first + 1), "xf too small for m": dict(m=m + 1), "bind too small for the stride": dict(bs=64),
           "src too small for the stride": dict(stride=224), "dst too small for m * n": dict(form=rc.EACH, bind=0, dst=each_dst),
           "src == dst": dict(src=dst), "xf == dst": dict(xf=dst), "bind == dst": dict(bind=dst), "src == xf": dict(xf=src), "src == bind": dict(bind=src),
           "xf == bind": dict(bind=xf)}
    for k in ("src", "xf", "dst"):
        bad.update({f"dead {k}": {k: dead}, f"no {k}": {k: 0}, f"unknown {k}": {k: 9999}})
    bad.update({"dead bind": dict(bind=dead), "unknown bind": dict(bind=9999)})
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"rotate_sh" in lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes) and untouched(ctx, short_dst, dst_bytes - 16) and untouched(ctx, each_dst, (first + m * n) * stride - 16), "a refused call wrote something"
    assert same_bytes(ctx, src, t) and same_bytes(ctx, xf, maps) and same_bytes(ctx, bind, table)
    assert call(n=0) == 0 and call(n=0, first=0xFFFFFFFF) == -1          # (a no-op still needs room for dst_first rows)
    ctx.finish()
    assert untouched(ctx, dst, dst_bytes)
    # the call works after the refusals; a table is no record buffer: no shadow is built for src or dst
    assert call() == 0
    got = ctx.read(dst, np.uint8, dst_bytes)
    assert (got[:first * stride] == SENTINEL).all()
    assert rc.same_rows(got[first * stride:].view(f32).reshape(n, -1), gs4d.rotate_sh_host(t, maps, degree, table, rc.BLEND4, bs)).all()
    assert ctx.shadow_builds(dst) == 0 and ctx.shadow_builds(src) == 0
    assert same_bytes(ctx, src, t) and same_bytes(ctx, xf, maps) and same_bytes(ctx, bind, table)
    ctx.close()
