"""GPU: gs4d_shade_sh — view-dependent colour from spherical harmonics, written into the records and patched into a current SoA shadow
(include/gs4d.h).

The colours are checked byte for byte against the numpy restatement (tests/shade_cases.py: the header's float32 operations), with the rest of
the record buffer, a guard region and the table compared against what was uploaded; pictures drawn after a shade are compared bit for bit with
those of a fresh context whose records were uploaded already shaded by the restatement; gs4d_debug_shadow_builds shows that a shade does not
cause a repack.  All calls go through the Python binding over the C ABI."""
import ctypes

import numpy as np
import pytest

import scenes
import shade_cases as sc
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


def check_shade(ctx, rec, tab, n, degree, t, cam, what):
    """uploads the records (with a sentinel tail behind them) and the table between guard buffers, shades the first n: every byte against the
    restatement, everything else against the upload"""
    total, stride = rec.shape[0], tab.shape[1] * 4
    host = np.concatenate([rec.view(np.uint8).reshape(-1), np.full(GUARD, SENTINEL, np.uint8)])
    g0, data, g1 = fill(ctx, GUARD), ctx.buffer(host), fill(ctx, GUARD)
    sh, g2 = ctx.buffer(tab), fill(ctx, GUARD)
    ctx.shade_sh(data, n, sh, degree, t, cam, sh_stride=stride)
    got = ctx.read(data, np.uint8, host.size)
    want = sc.shaded_records(rec, tab, degree, t, cam, n=n)
    got_rec = got[:total * 96].view(np.uint32).reshape(total, 24)
    assert np.array_equal(got_rec[:n, 4:7], bits(want[:n, 4:7])), f"{what}: {int((got_rec[:n, 4:7] != bits(want[:n, 4:7])).any(1).sum())} of {n} colours differ from the restatement"
    assert np.array_equal(got_rec, bits(want)), f"{what}: a word outside floats 4..6 of the first n records changed"
    assert (got[total * 96:] == SENTINEL).all(), f"{what}: bytes behind the records changed"
    assert untouched(ctx, g0) and untouched(ctx, g1) and untouched(ctx, g2), f"{what}: a guard buffer changed"
    assert np.array_equal(ctx.read(sh, np.uint32, tab.size).reshape(tab.shape), bits(tab)), f"{what}: sh changed"
    for b in (g0, data, g1, sh, g2):
        ctx.delete(b)
    return want


# ---- 1. the colours ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", range(4))
def test_colours_equal_the_restatement_byte_for_byte(gs4d, degree):
    ctx = gs4d.Context(64, 64)
    extra = 3                                                   # records >= n that must stay as they are
    for n in sc.SIZES:
        rec = sc.records(n + extra, seed=0x5348 + n)
        coeff = sc.coefficients(n + extra, degree, seed=0x5349 + n)
        for stride in sc.strides(degree):
            want = check_shade(ctx, rec, sc.table(coeff, stride), n, degree, sc.T, sc.CAM, f"degree {degree}, n = {n}, stride = {stride}")
            if n >= 63:
                assert (want[:n, 4:7] > 0).mean() > 0.7 and np.unique(bits(want[:n, 4:7])).size > n      # colours that say something
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


@pytest.mark.parametrize("stride", (sc.row_bytes(3), sc.PADDED_STRIDE))
def test_a_degree_3_table_shaded_at_lower_degrees_reads_a_prefix(gs4d, stride):
    ctx = gs4d.Context(64, 64)
    n = sc.TILE + 1
    rec, coeff = sc.records(n), sc.coefficients(n, 3)
    results = []
    for degree in range(4):
        tab = sc.table(coeff, stride)
        want = check_shade(ctx, rec, tab, n, degree, sc.T, sc.CAM, f"degree-3 rows of {stride} bytes at degree {degree}")
        assert np.array_equal(bits(want), bits(sc.shaded_records(rec, coeff[:, :3 * sc.coeffs(degree)], degree, sc.T, sc.CAM)))
        results.append(want[:, 4:7])
        # the coefficients past the prefix as NaNs: the same colours, so they were not used
        poisoned = tab.copy()
        poisoned[:, 3 * sc.coeffs(degree):] = np.nan
        check_shade(ctx, rec, poisoned, n, degree, sc.T, sc.CAM, f"poisoned past the prefix, degree {degree}")
    for a, b in zip(results, results[1:]):
        assert (bits(a) != bits(b)).any(1).mean() > 0.9         # every band changes the colours
    ctx.finish()
    ctx.close()


def test_hostile_records(gs4d):
    ctx = gs4d.Context(64, 64)
    for name, rec, t, cam in sc.hostile():
        n = rec.shape[0]
        for degree in (1, 3):
            check_shade(ctx, rec, sc.table(sc.coefficients(n, degree), sc.row_bytes(degree)), n, degree, t, cam, f"{name}, degree {degree}")
    ctx.finish()                                                # no device error
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    data, sh = fill(ctx, 96 * 4), fill(ctx, 192 * 4)
    ctx.shade_sh(data, 0, sh, 3, sc.T, sc.CAM)
    ctx.finish()
    assert untouched(ctx, data, 96 * 4) and untouched(ctx, sh, 192 * 4)
    ctx.close()


# ---- 2. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_records_as_they_were(gs4d):
    n, stride, degree = 300, 192, 3
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    tab = sc.table(sc.coefficients(n, 3), stride)
    data, sh = fill(ctx, 96 * n), ctx.buffer(tab)
    short_data, short_sh, dead = fill(ctx, 96 * n - 16), ctx.buffer(tab.reshape(-1)[:-4]), fill(ctx, 64)
    ctx.delete(dead)
    sz = ctypes.c_size_t
    cam = (ctypes.c_float * 3)(*sc.CAM)

    def shade(data=data, n=n, sh=sh, stride=stride, degree=degree, cam=cam):
        return lib.gs4d_shade_sh(ctx._h, data, sz(n), sh, sz(stride), degree, ctypes.c_float(sc.T), cam)

    bad = {
        "n > 0xFFFFFFFF": dict(n=1 << 32), "degree -1": dict(degree=-1), "degree 4": dict(degree=4), "stride 0": dict(stride=0),
        "stride not a multiple of 16": dict(stride=200), "stride above 1024": dict(stride=1040), "stride below the degree's row": dict(stride=176),
        "stride 16 at degree 1": dict(stride=16, degree=1), "stride 96 at degree 2": dict(stride=96, degree=2), "no camera": dict(cam=None),
        "dead data": dict(data=dead), "dead sh": dict(sh=dead), "unknown name": dict(sh=9999), "no data": dict(data=0), "no sh": dict(sh=0),
        "data == sh": dict(sh=data), "data too small": dict(data=short_data), "sh too small": dict(sh=short_sh), "sh too small for the stride": dict(stride=208),
    }
    for what, kw in bad.items():
        assert shade(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    assert untouched(ctx, data, 96 * n) and untouched(ctx, short_data, 96 * n - 16), "a refused call wrote something"
    assert np.array_equal(ctx.read(sh, np.uint32, tab.size).reshape(tab.shape), bits(tab))
    # the call works after the refusals — on records this time
    rec = sc.records(n)
    ctx.subdata(data, rec)
    assert shade() == 0 and shade(n=0) == 0 and shade(degree=1, stride=192) == 0 and shade() == 0
    assert np.array_equal(bits(ctx.read(data, f32, n * 24)).reshape(n, 24), bits(sc.shaded_records(rec, tab, 3, sc.T, sc.CAM)))
    ctx.close()


# ---- 3. the shadow patch -------------------------------------------------------------------------------------------------------------------------
W, H, N = 64, 48, 300
CAM_DIR = (0.0, 0.0, -1.0)
DEGREE = 3
LAYOUT_BYTES = {"static3d": 64, "symmetric": 72, "full": 96}


def camera(k=0):
    """a camera in front of the cloud that moves with k"""
    return (4.0 * k - 6.0, 3.0 - 1.5 * k, 150.0 + 2.0 * k)


def record_set(gs4d, layout):
    """one record set per layout of the SoA shadow: static 3D splats, a symmetric sig, a sig that is not symmetric"""
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(N, seed=0x5350)
    pos4 = pos4.copy()
    pos4[:, :3] *= 0.2
    pos4[:, 3] = sc.T - 1.0 + pos4[:, 3] / 25.0
    if layout == "static3d":
        rec = gs4d.build_records_3d(pos4[:, :3].copy(), q, scale * 12.0, rgba)
        rec[:, 3] = sc.T                                        # the same mu_t in every record: still the static layout, and alive at T
        return rec
    rec = gs4d.build_records_4d(pos4, q, scale * 12.0, life * 4.0, fade, vel * 0.2, rgba)
    # the 72-byte layout wants sig[c][r] == sig[r][c] bit for bit; the builder's products round the two halves apart in some records: mirror one
    sig = rec[:, 8:].reshape(-1, 4, 4)
    iu = np.triu_indices(4, 1)
    sig[:, iu[1], iu[0]] = sig[:, iu[0], iu[1]]
    if layout == "full":
        rec[:, 8 + 1] *= f32(1.25)                              # sig[0][1] != sig[1][0]
    return rec


class Scene:
    def __init__(self, gs4d, rec, outputs=False):
        self.gs4d, self.rec, self.n = gs4d, rec, rec.shape[0]
        self.ctx = c = gs4d.Context(W, H)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        if outputs:
            c.set_id_outputs(True)                              # (a frame with ID outputs has aux outputs too)
        self.outputs = outputs
        self.db = c.buffer(rec)
        self.kb, self.ib = c.buffer(nbytes=4 * self.n), c.buffer(nbytes=4 * self.n)
        self.proj = gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)

    def frame(self, mode, k=0, t=sc.T, shade=None, where="first"):
        """one frame from camera(k); shade: the table buffer — shaded first (the documented order) or between the sort and the draw"""
        c, gs4d, cam = self.ctx, self.gs4d, camera(k)
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=gs4d.look_at(cam, CAM_DIR), proj=self.proj)
        if shade is not None and where == "first":
            c.shade_sh(self.db, self.n, shade, DEGREE, t, cam)
        if mode == gs4d.MODE_4D_SORTED:
            c.keygen(self.db, t, cam, self.kb, self.ib, self.n)
            c.sort_pairs(self.kb, self.ib, self.n)
        if shade is not None and where == "between":
            c.shade_sh(self.db, self.n, shade, DEGREE, t, cam)
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


def host_shaded_frame(gs4d, rec, tab, mode, k, outputs, t=sc.T):
    """the frame of a fresh context whose records were uploaded already shaded by the restatement"""
    s = Scene(gs4d, sc.shaded_records(rec, tab, DEGREE, t, camera(k)), outputs)
    s.frame(mode, k, t)
    out, layout = s.read(), s.ctx.stats()["record_read_bytes"]
    assert s.ctx.shadow_builds(s.db) == 1
    s.ctx.close()
    return out, layout


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w)), f"{int((bits(g) != bits(w)).sum())} words differ"


def modes(gs4d):
    return {"sorted": gs4d.MODE_4D_SORTED, "direct": gs4d.MODE_4D_DIRECT}


@pytest.mark.parametrize("outputs", (False, True), ids=("colour", "aux+ids"))
@pytest.mark.parametrize("mode", ("sorted", "direct"))
@pytest.mark.parametrize("layout", tuple(LAYOUT_BYTES))
def test_a_shade_patches_the_current_shadow(gs4d, layout, mode, outputs):
    mode = modes(gs4d)[mode]
    rec = record_set(gs4d, layout)
    tab = sc.table(sc.coefficients(N, DEGREE), sc.row_bytes(DEGREE))
    want, want_layout = host_shaded_frame(gs4d, rec, tab, mode, 1, outputs)
    s = Scene(gs4d, rec, outputs)
    sh = s.ctx.buffer(tab)
    s.frame(mode, 0)                                            # builds the shadow, with the uploaded colours
    first = s.read()
    assert s.ctx.shadow_builds(s.db) == 1
    s.frame(mode, 1, shade=sh)
    got = s.read()
    st = s.ctx.stats()
    assert st["record_read_bytes"] == want_layout == LAYOUT_BYTES[layout], (st["record_read_bytes"], want_layout)
    same(got, want)
    assert s.ctx.shadow_builds(s.db) == 1, "the shade made the draw repack"
    # the pictures say something: splats on screen, and colours that the shade changed
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert int((np.abs(got[0] - clear).max(-1) > 1.0 / 255.0).sum()) > 100, "an empty frame"
    unshaded = Scene(gs4d, rec, outputs)
    unshaded.frame(mode, 1)
    assert int((np.abs(unshaded.read()[0] - got[0]).max(-1) > 1.0 / 255.0).sum()) > 100, "the shade changed nothing visible"
    unshaded.ctx.close()
    # the records themselves: the AoS was written too, and nothing but the colours
    assert np.array_equal(bits(s.ctx.read(s.db, f32, N * 24)).reshape(N, 24), bits(sc.shaded_records(rec, tab, DEGREE, sc.T, camera(1))))
    assert not np.array_equal(bits(first[0]), bits(got[0]))
    s.ctx.finish()
    s.ctx.close()


@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_eight_shaded_frames_build_the_shadow_once(gs4d, mode):
    mode = modes(gs4d)[mode]
    rec = record_set(gs4d, "symmetric")
    s = Scene(gs4d, rec)
    sh = s.ctx.buffer(sc.table(sc.coefficients(N, DEGREE), sc.row_bytes(DEGREE)))
    s.frame(mode, 0)
    for k in range(1, 9):                                       # no read-back in between: frames in flight on every lane
        s.frame(mode, k, t=sc.T + 0.01 * k, shade=sh)
    assert s.ctx.shadow_builds(s.db) == 1
    got = s.read()
    assert s.ctx.shadow_builds(s.db) == 1
    want, _ = host_shaded_frame(gs4d, rec, sc.table(sc.coefficients(N, DEGREE), sc.row_bytes(DEGREE)), mode, 8, False, t=sc.T + 0.01 * 8)
    same(got, want)
    s.ctx.finish()
    s.ctx.close()


@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_a_shade_before_the_first_draw_writes_the_records_only(gs4d, mode):
    mode = modes(gs4d)[mode]
    rec = record_set(gs4d, "symmetric")
    tab = sc.table(sc.coefficients(N, DEGREE), sc.row_bytes(DEGREE))
    want, _ = host_shaded_frame(gs4d, rec, tab, mode, 2, False)
    s = Scene(gs4d, rec)
    sh = s.ctx.buffer(tab)
    assert s.ctx.shadow_builds(s.db) == 0
    s.frame(mode, 2, shade=sh)                                  # no shadow exists yet
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 1
    # ... and a host write between two shades makes the next draw repack, as it always did: the patch is for a CURRENT shadow only
    s.ctx.subdata(s.db, rec)
    s.frame(mode, 2, shade=sh)
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 2
    s.ctx.close()


def test_a_shade_between_keygen_and_draw_still_gives_the_picture(gs4d):
    rec = record_set(gs4d, "symmetric")
    tab = sc.table(sc.coefficients(N, DEGREE), sc.row_bytes(DEGREE))
    want, _ = host_shaded_frame(gs4d, rec, tab, gs4d.MODE_4D_SORTED, 3, False)
    s = Scene(gs4d, rec)
    sh = s.ctx.buffer(tab)
    s.frame(gs4d.MODE_4D_SORTED, 0)
    s.frame(gs4d.MODE_4D_SORTED, 3, shade=sh, where="between")  # the data version moves under the sort's provenance: the draw reads the index
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 1
    s.ctx.close()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------------------------
def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch):
    """a shade right behind a draw of the same buffer on the previous lane: the earlier frame keeps the old colours; a host write into the table
    right behind the call does not change its result"""
    monkeypatch.setenv("GS4D_LANES", "4")
    mode = gs4d.MODE_4D_SORTED
    rec = record_set(gs4d, "symmetric")
    tab = sc.table(sc.coefficients(N, DEGREE), sc.row_bytes(DEGREE))
    old = Scene(gs4d, rec)
    old.frame(mode, 0)
    old_rgba8 = old.ctx.buffer(nbytes=W * H * 4)
    old.ctx.read_frame_rgba8_device(0, old.ctx.device_ptr(old_rgba8)[0], W * H * 4)
    old.ctx.finish()
    want_prev = old.ctx.read(old_rgba8, np.uint8, W * H * 4)
    old.ctx.close()
    want, _ = host_shaded_frame(gs4d, rec, tab, mode, 1, False)
    s = Scene(gs4d, rec)
    assert s.ctx.stats()["lanes"] == 4
    sh, out = s.ctx.buffer(tab), s.ctx.buffer(nbytes=W * H * 4)
    for _ in range(3):
        s.frame(mode, 0)                                        # frames in flight that read the records and the shadow
    s.frame(mode, 1, shade=sh)                                  # the shade is the first call of the next lane's frame
    s.ctx.subdata(sh, np.zeros_like(tab))                       # directly behind: the call must not see the zeros
    s.ctx.read_frame_rgba8_device(1, s.ctx.device_ptr(out)[0], W * H * 4)
    got = s.read()
    s.ctx.finish()
    assert np.array_equal(s.ctx.read(out, np.uint8, W * H * 4), want_prev), "the frame before the shade shows other colours than it was drawn with"
    same(got, want)
    assert s.ctx.shadow_builds(s.db) == 1
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


def test_a_shade_waits_for_a_rerun(gs4d, monkeypatch):
    """staged_cases' case a (as tests/test_gpu_compact.py): frames at T0 teach the guesses, the frame at T1 outgrows a segment block; the shade
    behind it settles the draw first — the re-run uses the old colours"""
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    rec, _ = staged_cases.build(gs4d, "a")
    Wb, Hb, n = staged_cases.W, staged_cases.H, rec.shape[0]
    tab = sc.table(sc.coefficients(n, 1), sc.row_bytes(1))
    fresh = gs4d.Context(Wb, Hb)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    sorted_frame(gs4d, fresh, (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n)), n, staged_cases.T1)
    want = fresh.read_pixels()
    fresh.close()
    ctx = gs4d.Context(Wb, Hb)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    sh = ctx.buffer(tab)
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    ctx.shade_sh(bufs[0], n, sh, 1, staged_cases.T1, staged_cases.CAM[0])      # no read-back in between
    s1 = ctx.stats()
    assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    got = ctx.read_pixels()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"
    assert np.array_equal(bits(ctx.read(bufs[0], f32, n * 24)).reshape(n, 24), bits(sc.shaded_records(rec, tab, 1, staged_cases.T1, staged_cases.CAM[0])))
    ctx.close()


# ---- 5. the table carried along ------------------------------------------------------------------------------------------------------------------
def test_a_compaction_carries_the_table_along(gs4d):
    n, stride = 3 * sc.TILE + 1, sc.PADDED_STRIDE
    rec = sc.records(n)
    tab = sc.table(sc.coefficients(n, DEGREE), stride)
    ctx = gs4d.Context(64, 64)
    stats = np.zeros(n, gs4d.Context.RECORD_STAT)
    stats["pixels"] = (np.arange(n) * 7) % 5                     # the rule drops every record whose count is 0
    stats["wmax"], stats["wsum"] = 1.0, 1 << 24
    data, sh, table = ctx.buffer(rec), ctx.buffer(tab), ctx.buffer(stats)
    dst, kept_index = fill(ctx, 96 * n), fill(ctx, 4 * n)
    count = ctx.compact_records(table, n, src=data, dst=dst, kept_index=kept_index, min_pixels=1)
    kept, _ = ctx.read_compact_count(count)
    keep = np.flatnonzero(stats["pixels"] >= 1)
    assert kept == keep.size and 0 < kept < n
    assert np.array_equal(ctx.read(kept_index, np.uint32, kept), keep)
    rows = ctx.gather_records(kept_index, kept, sh, n, stride=stride)
    ctx.shade_sh(dst, kept, rows, DEGREE, sc.T, sc.CAM, sh_stride=stride)
    ctx.shade_sh(data, n, sh, DEGREE, sc.T, sc.CAM, sh_stride=stride)
    full = ctx.read(data, f32, n * 24).reshape(n, 24)
    got = ctx.read(dst, f32, kept * 24).reshape(kept, 24)
    assert np.array_equal(bits(full), bits(sc.shaded_records(rec, tab, DEGREE, sc.T, sc.CAM)))
    assert np.array_equal(bits(got), bits(full[keep])), "the compacted set's colours are not those of the kept rows"
    ctx.finish()
    ctx.close()
