"""GPU: gs4d_shade_sh_t and gs4d_collapse_sh — the time-varying SH colour of trained 4D sets (include/gs4d.h).

Collapsed rows are checked against gs4d_host_collapse_sh (uint32-equal, or a NaN on both sides), shaded records byte for byte against
gs4d_host_shade_sh_t, with the rest of every buffer, sentinel bytes and guard buffers compared against what was uploaded; the identity
shade_sh_t(rows) == shade_sh(collapse_sh(rows)) is checked on the device for every (degree, degree_t); pictures drawn after a shade are compared bit
for bit with those of a fresh context whose records were uploaded already shaded by the host definition; a frozen frame keeps its view dependence;
a posed 4D table goes through the existing gs4d_rotate_sh.  All calls go through the Python binding over the C ABI."""
import ctypes

import numpy as np
import pytest

import scenes
import sh_rotate_cases as rc
import shade_cases as sc
import shade_t_cases as tc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
EXTRA = 3                                                       # records / rows >= n that must stay as they are
f32, u32 = np.float32, np.uint32
IP = 0.25                                                       # period 4 against mu_t within 2 of T: |u| up to 1/2


def bits(a):
    return np.ascontiguousarray(a).view(u32)


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


def check_collapse(ctx, gs4d, rec, tab, n, degree, degree_t, t, ip, dst_stride, what):
    """uploads the records and the table between guard buffers, collapses the first n rows into a buffer of sentinel bytes: rows < n against the host
    definition, everything else against the upload"""
    total, stride = rec.shape[0], tab.shape[1] * 4
    g0, data, g1 = fill(ctx, GUARD), ctx.buffer(rec), fill(ctx, GUARD)
    sh, g2 = ctx.buffer(tab), fill(ctx, GUARD)
    dst, g3 = fill(ctx, total * dst_stride + GUARD), fill(ctx, GUARD)
    assert ctx.collapse_sh(data, n, sh, degree, degree_t, t, ip, sh_stride=stride, dst=dst, dst_stride=dst_stride) == dst
    got = ctx.read(dst, np.uint8, total * dst_stride + GUARD)
    want = gs4d.collapse_sh_host(rec[:n], tab[:n], degree, degree_t, t, ip, stride, dst_stride)
    rows = got[:n * dst_stride].view(f32).reshape(n, dst_stride // 4)
    ok = tc.same_rows(rows, want)
    assert ok.all(), f"{what}: {int((~ok).any(1).sum())} of {n} rows differ from the host definition, first word at {np.argwhere(~ok)[0].tolist()}"
    assert not bits(rows[:, tc.row_words(degree):]).any(), f"{what}: the padding of a row is not zero"
    assert (got[n * dst_stride:] == SENTINEL).all(), f"{what}: bytes behind row n - 1 of dst changed"
    assert untouched(ctx, g0) and untouched(ctx, g1) and untouched(ctx, g2) and untouched(ctx, g3), f"{what}: a guard buffer changed"
    assert np.array_equal(bits(ctx.read(data, f32, rec.size)), bits(rec).reshape(-1)), f"{what}: data changed"
    assert np.array_equal(ctx.read(sh, u32, tab.size).reshape(tab.shape), bits(tab)), f"{what}: sh changed"
    for b in (g0, data, g1, sh, g2, dst, g3):
        ctx.delete(b)
    return want


def check_shade(ctx, gs4d, rec, tab, n, degree, degree_t, t, ip, cam, what):
    """uploads the records (with a sentinel tail behind them) and the table between guard buffers, shades the first n: every byte against the host
    definition, everything else against the upload"""
    total, stride = rec.shape[0], tab.shape[1] * 4
    host = np.concatenate([rec.view(np.uint8).reshape(-1), np.full(GUARD, SENTINEL, np.uint8)])
    g0, data, g1 = fill(ctx, GUARD), ctx.buffer(host), fill(ctx, GUARD)
    sh, g2 = ctx.buffer(tab), fill(ctx, GUARD)
    ctx.shade_sh_t(data, n, sh, degree, degree_t, t, ip, cam, sh_stride=stride)
    got = ctx.read(data, np.uint8, host.size)
    want = rec.copy()
    want[:n] = gs4d.shade_sh_t_host(rec[:n], tab[:n], degree, degree_t, t, ip, cam, stride)
    got_rec = got[:total * 96].view(u32).reshape(total, 24)
    differ = (got_rec[:n, 4:7] != bits(want[:n, 4:7])).any(1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {n} colours differ from the host definition, first at record {int(np.flatnonzero(differ)[0])}"
    assert np.array_equal(got_rec, bits(want)), f"{what}: a word outside floats 4..6 of the first n records changed"
    assert (got[total * 96:] == SENTINEL).all(), f"{what}: bytes behind the records changed"
    assert untouched(ctx, g0) and untouched(ctx, g1) and untouched(ctx, g2), f"{what}: a guard buffer changed"
    assert np.array_equal(ctx.read(sh, u32, tab.size).reshape(tab.shape), bits(tab)), f"{what}: sh changed"
    for b in (g0, data, g1, sh, g2):
        ctx.delete(b)
    return want


# ---- 1. the two calls against the host definitions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,degree_t", tc.PAIRS)
def test_collapsed_rows_equal_the_host_definition(gs4d, degree, degree_t):
    ctx = gs4d.Context(64, 64)
    for k, n in enumerate(tc.SIZES):
        rec = sc.records(n + EXTRA, seed=0x5360 + n)
        for j, stride in enumerate(tc.strides_t(degree, degree_t)):
            dst_stride = tc.dst_strides(degree)[(j + k) % 3]
            tab = tc.table_t(n + EXTRA, degree, degree_t, stride, seed=0x5361 + n)
            want = check_collapse(ctx, gs4d, rec, tab, n, degree, degree_t, sc.T, IP, dst_stride, f"n = {n}, stride {stride} -> {dst_stride}")
            if n >= 63 and degree_t:
                assert (bits(want[:, :tc.row_words(degree)]) != bits(tab[:n, :tc.row_words(degree)])).mean() > 0.9      # the time blocks say something
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


@pytest.mark.parametrize("degree,degree_t", tc.PAIRS)
def test_collapse_of_hostile_coefficients_and_times(gs4d, degree, degree_t):
    ctx = gs4d.Context(64, 64)
    n = tc.TILE + 37
    rec = tc.hostile_mu_t(n + EXTRA)
    tab = tc.table_t(n + EXTRA, degree, degree_t, tc.strides_t(degree, degree_t)[1], hostile=True)
    for name, t, ip in (("hostile coefficients", sc.T, IP),) + tc.HOSTILE_TIMES:
        check_collapse(ctx, gs4d, rec, tab, n, degree, degree_t, t, ip, sc.row_bytes(degree), name)
    ctx.finish()
    ctx.close()


@pytest.mark.parametrize("degree,degree_t", tc.PAIRS)
def test_colours_equal_the_host_definition_byte_for_byte(gs4d, degree, degree_t):
    ctx = gs4d.Context(64, 64)
    for n in tc.SIZES:
        rec = sc.records(n + EXTRA, seed=0x5362 + n)
        for stride in tc.strides_t(degree, degree_t):
            tab = tc.table_t(n + EXTRA, degree, degree_t, stride, seed=0x5363 + n)
            want = check_shade(ctx, gs4d, rec, tab, n, degree, degree_t, sc.T, IP, sc.CAM, f"n = {n}, stride = {stride}")
            if n >= 63:
                assert (want[:n, 4:7] > 0).mean() > 0.7 and np.unique(bits(want[:n, 4:7])).size > n      # colours that say something
    ctx.finish()
    ctx.close()


@pytest.mark.parametrize("degree,degree_t", ((1, 1), (3, 2), (2, 2), (0, 1)))
def test_hostile_records_times_and_coefficients(gs4d, degree, degree_t):
    ctx = gs4d.Context(64, 64)
    stride = tc.row_bytes_t(degree, degree_t)
    for name, rec, t, cam in sc.hostile():
        n = rec.shape[0]
        check_shade(ctx, gs4d, rec, tc.table_t(n, degree, degree_t, stride), n, degree, degree_t, t, IP, cam, name)
    n = tc.TILE + 37
    rec, tab = tc.hostile_mu_t(n), tc.table_t(n, degree, degree_t, stride, hostile=True)
    for name, t, ip in (("hostile coefficients", sc.T, IP),) + tc.HOSTILE_TIMES:
        check_shade(ctx, gs4d, rec, tab, n, degree, degree_t, t, ip, sc.CAM, name)
    ctx.finish()                                                # no device error
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    data, sh, dst = fill(ctx, 96 * 4), fill(ctx, 576 * 4), fill(ctx, 192 * 4)
    ctx.shade_sh_t(data, 0, sh, 3, 2, sc.T, IP, sc.CAM)
    ctx.collapse_sh(data, 0, sh, 3, 2, sc.T, IP, dst=dst)
    ctx.finish()
    assert untouched(ctx, data, 96 * 4) and untouched(ctx, sh, 576 * 4) and untouched(ctx, dst, 192 * 4)
    ctx.close()


# ---- 2. the identity, on the device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,degree_t", tc.PAIRS)
def test_shade_sh_t_is_shade_sh_of_the_collapsed_rows(gs4d, degree, degree_t):
    ctx = gs4d.Context(64, 64)
    n = 3 * tc.TILE + 1
    rec = tc.hostile_mu_t(n)
    for hostile, (t, ip) in ((False, (sc.T, IP)), (True, (sc.T + 0.6, 1.0 / 50.0)), (True, (sc.T, 1.5e38))):
        tab = tc.table_t(n, degree, degree_t, tc.row_bytes_t(degree, degree_t), hostile=hostile)
        data, other, sh = ctx.buffer(rec), ctx.buffer(rec), ctx.buffer(tab)
        ctx.shade_sh_t(data, n, sh, degree, degree_t, t, ip, sc.CAM)
        rows = ctx.collapse_sh(data, n, sh, degree, degree_t, t, ip)
        ctx.shade_sh(other, n, rows, degree, t, sc.CAM)
        got, want = ctx.read(data, u32, n * 24), ctx.read(other, u32, n * 24)
        assert np.array_equal(got, want), f"{int((got != want).reshape(n, 24).any(1).sum())} records differ (hostile: {hostile})"
        assert not np.array_equal(got, bits(rec).reshape(-1))
        if degree_t == 0:                                       # ... and gs4d_shade_sh on the same buffers
            ctx.subdata(other, rec)
            ctx.shade_sh(other, n, sh, degree, t, sc.CAM)
            assert np.array_equal(got, ctx.read(other, u32, n * 24))
        for b in (data, other, sh, rows):
            ctx.delete(b)
    ctx.finish()
    ctx.close()


# ---- 3. the shadow patch -------------------------------------------------------------------------------------------------------------------------
W, H, N = 64, 48, 300
CAM_DIR = (0.0, 0.0, -1.0)
DEGREE, DEGREE_T = 3, 2


def camera(k=0):
    """a camera in front of the cloud that moves with k"""
    return (4.0 * k - 6.0, 3.0 - 1.5 * k, 150.0 + 2.0 * k)


def record_set(gs4d):
    """one 4D record set with a symmetric sig (the 72-byte layout of the SoA shadow)"""
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(N, seed=0x5364)
    pos4 = pos4.copy()
    pos4[:, :3] *= 0.2
    pos4[:, 3] = sc.T - 1.0 + pos4[:, 3] / 25.0
    rec = gs4d.build_records_4d(pos4, q, scale * 12.0, life * 4.0, fade, vel * 0.2, rgba)
    sig = rec[:, 8:].reshape(-1, 4, 4)
    iu = np.triu_indices(4, 1)
    sig[:, iu[1], iu[0]] = sig[:, iu[0], iu[1]]
    return rec


def picture_table():
    return tc.table_t(N, DEGREE, DEGREE_T, tc.row_bytes_t(DEGREE, DEGREE_T), seed=0x5365)


class Scene:
    def __init__(self, gs4d, rec):
        self.gs4d, self.rec, self.n = gs4d, rec, rec.shape[0]
        self.ctx = c = gs4d.Context(W, H)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        self.db = c.buffer(rec)
        self.kb, self.ib = c.buffer(nbytes=4 * self.n), c.buffer(nbytes=4 * self.n)
        self.proj = gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)

    def frame(self, mode, k=0, t=sc.T, shade=None):
        """one frame from camera(k); shade: the 4D table buffer, shaded first (the documented order)"""
        c, gs4d, cam = self.ctx, self.gs4d, camera(k)
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=gs4d.look_at(cam, CAM_DIR), proj=self.proj)
        if shade is not None:
            c.shade_sh_t(self.db, self.n, shade, DEGREE, DEGREE_T, t, IP, cam)
        if mode == gs4d.MODE_4D_SORTED:
            c.keygen(self.db, t, cam, self.kb, self.ib, self.n)
            c.sort_pairs(self.kb, self.ib, self.n)
        c.set_mode(mode)
        if mode == gs4d.MODE_4D_SORTED:
            c.bind(1, self.ib)
            c.bind(2, self.db)
        else:
            c.bind(1, self.db)                                  # (instance k is record k)
        c.draw_instanced(self.n)


def host_shaded_frame(gs4d, rec, tab, mode, k, t=sc.T):
    """the picture of a fresh context whose records were uploaded already shaded by the host definition"""
    s = Scene(gs4d, gs4d.shade_sh_t_host(rec, tab, DEGREE, DEGREE_T, t, IP, camera(k)))
    s.frame(mode, k, t)
    out = s.ctx.read_pixels()
    assert s.ctx.shadow_builds(s.db) == 1
    s.ctx.close()
    return out


def modes(gs4d):
    return {"sorted": gs4d.MODE_4D_SORTED, "direct": gs4d.MODE_4D_DIRECT}


@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_a_shade_patches_the_current_shadow(gs4d, mode):
    mode = modes(gs4d)[mode]
    rec, tab = record_set(gs4d), picture_table()
    want = host_shaded_frame(gs4d, rec, tab, mode, 1)
    s = Scene(gs4d, rec)
    sh = s.ctx.buffer(tab)
    s.frame(mode, 0)                                            # builds the shadow, with the uploaded colours
    first = s.ctx.read_pixels()
    assert s.ctx.shadow_builds(s.db) == 1
    s.frame(mode, 1, shade=sh)
    got = s.ctx.read_pixels()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ: the colour planes are not the host-shaded ones"
    assert s.ctx.shadow_builds(s.db) == 1, "the shade made the draw repack"
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert int((np.abs(got - clear).max(-1) > 1.0 / 255.0).sum()) > 100, "an empty frame"
    assert not np.array_equal(bits(first), bits(got))
    # the time blocks are in the picture: the DC block alone is another one
    plain = Scene(gs4d, gs4d.shade_sh_t_host(rec, tab, DEGREE, 0, sc.T, IP, camera(1), tab.shape[1] * 4))
    plain.frame(mode, 1)
    assert int((np.abs(plain.ctx.read_pixels() - got).max(-1) > 1.0 / 255.0).sum()) > 100, "the time blocks changed nothing visible"
    plain.ctx.close()
    # the records themselves: the AoS was written too, and nothing but the colours
    assert np.array_equal(bits(s.ctx.read(s.db, f32, N * 24)).reshape(N, 24), bits(gs4d.shade_sh_t_host(rec, tab, DEGREE, DEGREE_T, sc.T, IP, camera(1))))
    s.ctx.finish()
    s.ctx.close()


@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_eight_shaded_frames_build_the_shadow_once(gs4d, mode):
    mode = modes(gs4d)[mode]
    rec, tab = record_set(gs4d), picture_table()
    s = Scene(gs4d, rec)
    sh = s.ctx.buffer(tab)
    s.frame(mode, 0)
    for k in range(1, 9):                                       # no read-back in between: frames in flight on every lane
        s.frame(mode, k, t=sc.T + 0.05 * k, shade=sh)
    assert s.ctx.shadow_builds(s.db) == 1
    got = s.ctx.read_pixels()
    assert s.ctx.shadow_builds(s.db) == 1
    want = host_shaded_frame(gs4d, rec, tab, mode, 8, t=sc.T + 0.05 * 8)
    assert np.array_equal(bits(got), bits(want))
    s.ctx.finish()
    s.ctx.close()


def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch):
    """a shade right behind a draw of the same buffer on the previous lane: the earlier frame keeps the old colours; a host write into the table
    right behind the call does not change its result"""
    monkeypatch.setenv("GS4D_LANES", "4")
    mode = gs4d.MODE_4D_SORTED
    rec, tab = record_set(gs4d), picture_table()
    old = Scene(gs4d, rec)
    old.frame(mode, 0)
    old_rgba8 = old.ctx.buffer(nbytes=W * H * 4)
    old.ctx.read_frame_rgba8_device(0, old.ctx.device_ptr(old_rgba8)[0], W * H * 4)
    old.ctx.finish()
    want_prev = old.ctx.read(old_rgba8, np.uint8, W * H * 4)
    old.ctx.close()
    want = host_shaded_frame(gs4d, rec, tab, mode, 1)
    s = Scene(gs4d, rec)
    assert s.ctx.stats()["lanes"] == 4
    sh, out = s.ctx.buffer(tab), s.ctx.buffer(nbytes=W * H * 4)
    for _ in range(3):
        s.frame(mode, 0)                                        # frames in flight that read the records and the shadow
    s.frame(mode, 1, shade=sh)                                  # the shade is the first call of the next lane's frame
    s.ctx.subdata(sh, np.zeros_like(tab))                       # directly behind: the call must not see the zeros
    s.ctx.read_frame_rgba8_device(1, s.ctx.device_ptr(out)[0], W * H * 4)
    got = s.ctx.read_pixels()
    s.ctx.finish()
    assert np.array_equal(s.ctx.read(out, np.uint8, W * H * 4), want_prev), "the frame before the shade shows other colours than it was drawn with"
    assert np.array_equal(bits(got), bits(want))
    assert s.ctx.shadow_builds(s.db) == 1
    s.ctx.close()


# ---- 4. a frozen frame keeps its view dependence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,degree_t", ((3, 2), (2, 1)))
def test_freeze_keeps_its_view_dependence(gs4d, degree, degree_t):
    """freeze at t, collapse_sh of the source at t, gather_records of the collapsed rows through kept_index, shade_sh of the frozen set from two
    cameras — byte for byte the colours shade_sh_t gives the source from the same cameras, gathered through kept_index: the slice's conditional
    centre is the centre gs4d_shade_sh takes, and at t == mu_t_out the frozen record's own mean is that centre.  The slice conditions with the time
    COLUMN of sig (words 11, 15, 19), gs4d_shade_sh with the time ROW (words 20..22): the records here hold the same bits in both, as a symmetric
    sig does; where a builder rounds the two halves apart, the two centres may differ in the last bit."""
    n, t = 2 * tc.TILE + 45, sc.T + 0.25
    rec = sc.records(n, seed=0x5366)
    rec[::5, 7] = 0.0                                           # every fifth record shows nothing: the frozen set is a subset
    rec[:, [11, 15, 19]] = rec[:, 20:23]                        # a symmetric time row and column
    stride = tc.row_bytes_t(degree, degree_t)
    tab = tc.table_t(n, degree, degree_t, stride, seed=0x5367)
    ctx = gs4d.Context(64, 64)
    data, sh = ctx.buffer(rec), ctx.buffer(tab)
    frozen, kept_index, count = ctx.freeze(data, n, t)
    kept, _ = ctx.read_compact_count(count)
    keep = ctx.read(kept_index, u32, kept)
    assert np.array_equal(keep, np.flatnonzero(rec[:, 7] > 0)) and 0 < kept < n
    collapsed = ctx.collapse_sh(data, n, sh, degree, degree_t, t, IP)
    rows = ctx.gather_records(kept_index, kept, collapsed, n, stride=sc.row_bytes(degree))
    seen = []
    for cam in (sc.CAM, (-40.0, 22.0, -95.0)):
        ctx.shade_sh(frozen, kept, rows, degree, t, cam)
        got = ctx.read(frozen, f32, kept * 24).reshape(kept, 24)[:, 4:7].copy()
        ctx.subdata(data, rec)
        ctx.shade_sh_t(data, n, sh, degree, degree_t, t, IP, cam)
        want = ctx.read(data, f32, n * 24).reshape(n, 24)[keep, 4:7]
        assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(1).sum())} of {kept} colours differ from camera {cam}"
        assert np.array_equal(bits(want), bits(gs4d.shade_sh_t_host(rec, tab, degree, degree_t, t, IP, cam)[keep, 4:7]))
        seen.append(got)
    assert (bits(seen[0]) != bits(seen[1])).any(1).mean() > 0.9, "the frozen set shows one colour from both cameras"
    ctx.finish()
    ctx.close()


# ---- 5. a posed 4D table through the existing gs4d_rotate_sh -----------------------------------------------------------------------------------------
def colours(ctx, buf, n):
    return ctx.read(buf, f32, n * 24).reshape(n, 24)[:, 4:7].copy()


def test_a_posed_4d_table_goes_through_rotate_sh_as_it_stands(gs4d):
    """degree 3, degree_t 2: the table of n rows of 576 bytes is a table of 3 n rows of 192 bytes, which gs4d_rotate_sh turns with one map
    (GS4D_SH_EACH) — or with GS4D_POSE_INDEX and every bind word three times.  Measured through the host definitions: 7.7e-8 of sum |c| over all
    blocks between the two routes; the bar is sh_rotate_cases.PICTURE_BAR."""
    n, degree, degree_t, t, cam = rc.PICTURE_N, tc.POSED_DEGREE, tc.POSED_DEGREE_T, rc.PICTURE_T, rc.PICTURE_CAM
    rec, tab = tc.posed_set()
    l = rc.picture_maps(gs4d)["rigid"]
    ctx = gs4d.Context(64, 64)
    xf, sh = ctx.buffer(l.reshape(1, 20)), ctx.buffer(tab)
    # route A, the camera-inverse route: shade the source seen from M^-1 cam, then transform
    a_src = ctx.buffer(rec)
    ctx.shade_sh_t(a_src, n, sh, degree, degree_t, t, tc.POSED_INV_PERIOD, rc.inverse_camera(l, cam))
    a = colours(ctx, ctx.transform_records(a_src, n, xf, 1), n)
    # route B: transform, rotate_sh of the 3 n rows, shade the result seen from cam
    b_rec = ctx.transform_records(ctx.buffer(rec), n, xf, 1)
    turned = ctx.rotate_sh(sh, 3 * n, xf, 3, m=1)
    ctx.shade_sh_t(b_rec, n, turned, degree, degree_t, t, tc.POSED_INV_PERIOD, cam)
    b = colours(ctx, b_rec, n)
    # GS4D_POSE_INDEX with every bind word repeated degree_t + 1 times turns the same rows
    index = ctx.rotate_sh(sh, 3 * n, xf, 3, m=1, bind=ctx.buffer(np.repeat(np.zeros(n, u32), 3)), form=rc.INDEX)
    assert np.array_equal(ctx.read(index, u32, tab.size), ctx.read(turned, u32, tab.size))
    # without the rotation the moved set shows the colours of the old orientation
    ctx.shade_sh_t(b_rec, n, sh, degree, degree_t, t, tc.POSED_INV_PERIOD, cam)
    stale = colours(ctx, b_rec, n)
    ctx.finish()
    ctx.close()
    ratio, off = tc.colour_ratio_t(a, b, tab), tc.colour_ratio_t(a, stale, tab)
    print(f"posed 4D table: the two routes differ by {ratio:.3g} sum |c| (the unrotated table: {off:.3g})")
    assert rc.PICTURE_BAR <= 1e-4
    assert ratio <= rc.PICTURE_BAR
    assert off > 1000 * rc.PICTURE_BAR, "the rotation does not matter in this case: the test shows nothing"
    # the device routes are the host routes
    ha, hb, _ = tc.posed_routes_host(gs4d, rec, tab, l, cam, t)
    assert np.array_equal(bits(a), bits(ha)) and np.array_equal(bits(b), bits(hb))


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_everything_as_it_was(gs4d):
    n, stride, dst_stride = 300, 576, 208
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    tab = tc.table_t(n, 3, 2, stride)
    data, sh, dst = fill(ctx, 96 * n), ctx.buffer(tab), fill(ctx, dst_stride * n)
    short_data, short_sh, short_dst, dead = fill(ctx, 96 * n - 16), ctx.buffer(tab.reshape(-1)[:-4]), fill(ctx, dst_stride * n - 16), fill(ctx, 64)
    ctx.delete(dead)
    sz = ctypes.c_size_t

    def query(degree=3, degree_t=2, reserved=0):
        q = gs4d.sh_time_query(3, 2, sc.T, IP, sc.CAM)
        q.degree, q.degree_t, q.reserved = degree, degree_t, reserved
        return ctypes.byref(q)

    def shade(data=data, n=n, sh=sh, stride=stride, q=None, **kw):
        return lib.gs4d_shade_sh_t(ctx._h, data, sz(n), sh, sz(stride), query(**kw) if q is None else q)

    def collapse(data=data, n=n, sh=sh, stride=stride, q=None, dst=dst, dst_stride=dst_stride, **kw):
        return lib.gs4d_collapse_sh(ctx._h, data, sz(n), sh, sz(stride), query(**kw) if q is None else q, dst, sz(dst_stride))

    null = ctypes.POINTER(gs4d.ShTime)()
    both = {                                                    # what: (arguments, the operand gs4d_last_error names)
        "no query": (dict(q=null), "q == NULL"), "n > 0xFFFFFFFF": (dict(n=1 << 32), "records"),
        "degree -1": (dict(degree=-1), "q->degree "), "degree 4": (dict(degree=4), "q->degree "),
        "degree_t -1": (dict(degree_t=-1), "q->degree_t"), "degree_t 3": (dict(degree_t=3), "q->degree_t"), "reserved": (dict(reserved=1), "reserved"),
        "stride 0": (dict(stride=0), "sh_stride"), "stride not a multiple of 16": (dict(stride=584), "sh_stride"), "stride above 1024": (dict(stride=1040), "sh_stride"),
        "stride below the blocks": (dict(stride=560), "sh_stride"), "stride of degree_t 1": (dict(stride=384), "sh_stride"),
        "stride 48 at degree 1 / degree_t 1": (dict(stride=48, degree=1, degree_t=1), "sh_stride"),
        "dead data": (dict(data=dead), ": data ("), "dead sh": (dict(sh=dead), ": sh ("), "unknown name": (dict(sh=9999), ": sh (9999)"),
        "no data": (dict(data=0), ": data is 0"), "no sh": (dict(sh=0), ": sh is 0"), "data == sh": (dict(sh=data), ": sh and data"),
        "data too small": (dict(data=short_data), ": data holds fewer"), "sh too small": (dict(sh=short_sh), ": sh holds fewer"),
        "sh too small for the stride": (dict(stride=592), ": sh holds fewer"),
    }
    only_collapse = {
        "dst_stride 0": (dict(dst_stride=0), "dst_stride"), "dst_stride not a multiple of 16": (dict(dst_stride=200), "dst_stride"),
        "dst_stride above 1024": (dict(dst_stride=1040), "dst_stride"), "dst_stride below the row": (dict(dst_stride=176), "dst_stride"),
        "dst_stride 16 at degree 1": (dict(dst_stride=16, degree=1), "dst_stride"),
        "dead dst": (dict(dst=dead), ": dst ("), "no dst": (dict(dst=0), ": dst is 0"), "dst == data": (dict(dst=data), ": dst and data"),
        "dst == sh": (dict(dst=sh), ": dst and sh"), "dst too small": (dict(dst=short_dst), ": dst holds fewer"),
        "dst too small for the stride": (dict(dst_stride=224), ": dst holds fewer"),
    }
    for call, fn, cases in ((shade, "shade_sh_t: ", both), (collapse, "collapse_sh: ", {**both, **only_collapse})):
        for what, (kw, named) in cases.items():
            assert call(**kw) == -1, f"{fn}{what}"
            message = lib.gs4d_last_error(ctx._h).decode()
            assert message.startswith(fn) and named in message, (fn, what, message)
    ctx.finish()
    assert untouched(ctx, data, 96 * n) and untouched(ctx, short_data, 96 * n - 16) and untouched(ctx, dst, dst_stride * n) and untouched(ctx, short_dst, dst_stride * n - 16), \
        "a refused call wrote something"
    assert np.array_equal(ctx.read(sh, u32, tab.size).reshape(tab.shape), bits(tab))
    # the calls work after the refusals — on records this time
    rec = sc.records(n)
    ctx.subdata(data, rec)
    assert collapse() == 0 and collapse(n=0) == 0 and collapse(degree_t=1) == 0 and collapse(degree=1, degree_t=2, dst_stride=48) == 0 and collapse() == 0
    assert tc.same_rows(ctx.read(dst, f32, n * dst_stride // 4).reshape(n, -1), gs4d.collapse_sh_host(rec, tab, 3, 2, sc.T, IP, stride, dst_stride)).all()
    assert shade() == 0 and shade(n=0) == 0 and shade(degree_t=1) == 0 and shade(degree=2, degree_t=0) == 0 and shade() == 0
    assert np.array_equal(bits(ctx.read(data, f32, n * 24)).reshape(n, 24), bits(gs4d.shade_sh_t_host(rec, tab, 3, 2, sc.T, IP, sc.CAM)))
    ctx.close()
