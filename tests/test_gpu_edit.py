"""GPU: gs4d_edit_colours — the rgba of the selected records of a set edited in place, written into the records and patched into a current SoA
shadow (include/gs4d.h).

The records are checked byte for byte against the numpy restatement (tests/edit_cases.py: the header's float32 operations), with the tail of
the buffer, guard buffers, the table and the source compared against what was uploaded; pictures drawn after an edit are compared bit for bit
with those of a fresh context whose records were uploaded already edited by the restatement; gs4d_debug_shadow_builds shows that an edit does
not cause a repack; hiding a selection draws the bits of the compacted complement.  All calls go through the Python binding over the C ABI."""
import ctypes

import numpy as np
import pytest

import edit_cases as ec
import scenes
import staged_cases

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
f32 = np.float32
OP_NAMES = ("set", "mul", "lerp", "copy")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


class Bench:
    """the buffers of one size between sentinel guard buffers: data (n + EXTRA records and a sentinel tail), a table of exactly n rows, a source"""

    def __init__(self, ctx, rec, src, n):
        self.ctx, self.rec, self.src, self.n, self.total = ctx, rec, src, n, rec.shape[0]
        self.host = np.concatenate([rec.view(np.uint8).reshape(-1), np.full(GUARD, SENTINEL, np.uint8)])
        self.g0, self.data, self.g1 = fill(ctx, GUARD), ctx.buffer(self.host), fill(ctx, GUARD)
        self.stats, self.g2 = ctx.buffer(nbytes=16 * n), fill(ctx, GUARD)
        self.from_, self.g3 = ctx.buffer(src), fill(ctx, GUARD)
        self.table = None

    def set_table(self, table):
        self.table = table
        self.ctx.subdata(self.stats, table)

    def check(self, op, channels, value, amount, selection, what):
        """one call on freshly uploaded records: every byte of the data buffer against the restatement"""
        c = self.ctx
        c.subdata(self.data, self.host)
        stats, rule, invert = (self.table, *selection) if selection else (None, (1, 0, 0), False)
        kw = ec.rule_keywords(rule, invert) if selection else {}
        c.edit_colours(self.data, self.n, op, value, channels, amount, stats=self.stats if selection else None,
                       from_=self.from_ if op == "copy" else None, **kw)
        got = c.read(self.data, np.uint8, self.host.size)
        want = ec.edit(self.rec, op, channels, value, amount, stats=stats, rule=rule, invert=invert, from_=self.src, n=self.n)
        got_rec = got[:self.total * 96].view(f32).reshape(self.total, 24)
        if op in ("set", "copy"):
            assert np.array_equal(bits(got_rec), bits(want)), f"{what}: {int((bits(got_rec) != bits(want)).any(1).sum())} records differ from the restatement"
        assert ec.same_bits(got_rec, want), f"{what}: {int((bits(got_rec) != bits(want)).any(1).sum())} records differ from the restatement"
        assert np.array_equal(bits(got_rec[self.n:]), bits(self.rec[self.n:])), f"{what}: a record behind n changed"
        assert (got[self.total * 96:] == SENTINEL).all(), f"{what}: bytes behind the records changed"
        return want

    def check_the_rest(self, what):
        c = self.ctx
        assert untouched(c, self.g0) and untouched(c, self.g1) and untouched(c, self.g2) and untouched(c, self.g3), f"{what}: a guard buffer changed"
        if self.table is not None:
            assert np.array_equal(c.read(self.stats, np.uint8, 16 * self.n), self.table.view(np.uint8)), f"{what}: stats changed"
        assert np.array_equal(bits(c.read(self.from_, f32, self.total * 24)), bits(self.src).reshape(-1)), f"{what}: from changed"

    def delete(self):
        for b in (self.g0, self.data, self.g1, self.stats, self.g2, self.from_, self.g3):
            self.ctx.delete(b)


# ---- 1. bits -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OP_NAMES)
def test_the_records_equal_the_restatement_byte_for_byte(gs4d, op):
    ctx = gs4d.Context(64, 64)
    for n in ec.SIZES:
        total = n + ec.EXTRA
        b = Bench(ctx, ec.records(total, seed=0x4544 + n), ec.records(total, seed=0x4644 + n), n)
        for channels in ec.MASKS:
            want = b.check(op, channels, ec.VALUE, ec.AMOUNT, None, f"{op}, n = {n}, channels = {channels}, no table")
            assert (bits(want[:n]) != bits(b.rec[:n])).any(1).all(), "an edit that changes nothing"
        b.check_the_rest(f"{op}, n = {n}, no table")
        for name, (table, rule, invert) in ec.tables(n).items():
            b.set_table(table)
            for channels in ec.MASKS:
                b.check(op, channels, ec.VALUE, ec.AMOUNT, (rule, invert), f"{op}, n = {n}, channels = {channels}, table {name}")
            b.check_the_rest(f"{op}, n = {n}, table {name}")
        b.delete()
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_hostile_operands(gs4d):
    ctx = gs4d.Context(64, 64)
    n = ec.TILE + 37
    total = n + ec.EXTRA
    b = Bench(ctx, ec.hostile_records(total), ec.hostile_records(total, seed=0x4547), n)
    table, rule, invert = ec.tables(n)["alternating"]
    b.set_table(table)
    for op in OP_NAMES:
        for value, amount in ec.hostile_operands():
            for channels in (15, 10):
                b.check(op, channels, value, amount, (rule, invert), f"{op}, value = {value}, amount = {amount}, channels = {channels}")
    b.check_the_rest("hostile operands")
    ctx.finish()                                                # no device error
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    data, stats, src = fill(ctx, 96 * 4), fill(ctx, 16 * 4), fill(ctx, 96 * 4)
    ctx.edit_colours(data, 0, "lerp", ec.VALUE, "rgba", 0.5, stats=stats, min_pixels=1)
    ctx.edit_colours(data, 0, "copy", channels="rgba", from_=src)
    ctx.finish()
    assert untouched(ctx, data, 96 * 4) and untouched(ctx, stats, 16 * 4) and untouched(ctx, src, 96 * 4)
    ctx.close()


# ---- 2. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_records_as_they_were(gs4d):
    n = 300
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    table, rule, _ = ec.tables(n)["alternating"]
    src = ec.records(n, seed=7)
    data, stats, from_ = fill(ctx, 96 * n), ctx.buffer(table), ctx.buffer(src)
    short_data, short_stats, short_from, dead = fill(ctx, 96 * n - 16), ctx.buffer(table[:-1]), ctx.buffer(src.reshape(-1)[:-4]), fill(ctx, 64)
    ctx.delete(dead)
    sz = ctypes.c_size_t

    def edit_struct(op=ec.LERP, channels=15, reserved=0):
        e = gs4d.colour_edit(op, ec.VALUE, channels, ec.AMOUNT)
        e["reserved"] = reserved
        return e

    def rule_struct(flags=0, reserved=0):
        k = np.zeros(1, gs4d.KEEP_RULE)
        k["min_pixels"], k["min_wmax"], k["min_wsum"], k["flags"], k["reserved"] = rule[0], rule[1], rule[2], flags, reserved
        return k

    NO = object()

    def call(data=data, n=n, edit=None, stats=stats, rule=None, from_=0):
        e = edit_struct() if edit is None else edit
        k = rule_struct() if rule is None else rule
        ptr = lambda a: None if a is NO else a.ctypes.data_as(ctypes.c_void_p)
        return lib.gs4d_edit_colours(ctx._h, data, sz(n), ptr(e), stats, ptr(k), from_)

    copy = edit_struct(op=ec.COPY)
    bad = {
        "edit == NULL": dict(edit=NO), "unknown op": dict(edit=edit_struct(op=4)), "op 0xFFFFFFFF": dict(edit=edit_struct(op=0xFFFFFFFF)),
        "channels 0": dict(edit=edit_struct(channels=0)), "channels 16": dict(edit=edit_struct(channels=16)), "edit.reserved": dict(edit=edit_struct(reserved=1)),
        "n > 0xFFFFFFFF": dict(n=1 << 32), "dead data": dict(data=dead), "no data": dict(data=0), "unknown data": dict(data=9999),
        "data too small": dict(data=short_data), "stats without a rule": dict(rule=NO), "a rule without stats": dict(stats=0),
        "unknown flag": dict(rule=rule_struct(flags=2)), "rule.reserved": dict(rule=rule_struct(reserved=1)), "dead stats": dict(stats=dead),
        "unknown stats": dict(stats=9999), "stats too small": dict(stats=short_stats), "copy without from": dict(edit=copy),
        "copy from a dead buffer": dict(edit=copy, from_=dead), "copy from an unknown name": dict(edit=copy, from_=9999),
        "copy from too few records": dict(edit=copy, from_=short_from), "lerp with from": dict(from_=from_), "set with from": dict(edit=edit_struct(op=ec.SET), from_=from_),
        "data == stats": dict(stats=data), "data == from": dict(edit=copy, from_=data), "stats == from": dict(edit=copy, from_=stats),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    assert call(data=short_data, stats=0, rule=NO) == -1 and call(edit=copy, stats=0, rule=NO, from_=short_from) == -1      # ... without a table too
    ctx.finish()
    assert untouched(ctx, data, 96 * n) and untouched(ctx, short_data, 96 * n - 16), "a refused call wrote something"
    assert np.array_equal(ctx.read(stats, np.uint8, 16 * n), table.view(np.uint8)) and np.array_equal(bits(ctx.read(from_, f32, n * 24)), bits(src).reshape(-1))
    # the call works after the refusals — on records this time
    rec = ec.records(n)
    ctx.subdata(data, rec)
    assert call() == 0 and call(n=0) == 0 and call(stats=0, rule=NO, edit=edit_struct(op=ec.MUL, channels=8)) == 0
    assert call(edit=copy, from_=from_, rule=rule_struct(flags=gs4d.KEEP_INVERT)) == 0
    want = ec.edit(rec, "lerp", 15, stats=table, rule=rule)
    want = ec.edit(want, "mul", 8)
    want = ec.edit(want, "copy", 15, stats=table, rule=rule, invert=True, from_=src)
    assert np.array_equal(bits(ctx.read(data, f32, n * 24)).reshape(n, 24), bits(want))
    ctx.close()


# ---- 3. the shadow patch -------------------------------------------------------------------------------------------------------------------------
W, H, N = 64, 48, 300
T = 25.0
CAM_DIR = (0.0, 0.0, -1.0)
LAYOUT_BYTES = {"static3d": 64, "symmetric": 72, "full": 96}
TINT = dict(op="lerp", value=(1.0, 0.1, 0.9, 0.35), channels=15, amount=0.75)


def camera(k=0):
    """a camera in front of the cloud that moves with k"""
    return (4.0 * k - 6.0, 3.0 - 1.5 * k, 150.0 + 2.0 * k)


def record_set(gs4d, layout):
    """one record set per layout of the SoA shadow (as tests/test_gpu_shade.py builds them): static 3D splats, a symmetric sig, a sig that is not
    symmetric"""
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(N, seed=0x4550)
    pos4 = pos4.copy()
    pos4[:, :3] *= 0.2
    pos4[:, 3] = T - 1.0 + pos4[:, 3] / 25.0
    if layout == "static3d":
        rec = gs4d.build_records_3d(pos4[:, :3].copy(), q, scale * 12.0, rgba)
        rec[:, 3] = T                                           # the same mu_t in every record: still the static layout, and alive at T
        return rec
    rec = gs4d.build_records_4d(pos4, q, scale * 12.0, life * 4.0, fade, vel * 0.2, rgba)
    # the 72-byte layout wants sig[c][r] == sig[r][c] bit for bit; the builder's products round the two halves apart in some records: mirror one
    sig = rec[:, 8:].reshape(-1, 4, 4)
    iu = np.triu_indices(4, 1)
    sig[:, iu[1], iu[0]] = sig[:, iu[0], iu[1]]
    if layout == "full":
        rec[:, 8 + 1] *= f32(1.25)                              # sig[0][1] != sig[1][0]
    return rec


def half_table():
    """the table and the rule that select every other record of N"""
    table, rule, _ = ec.tables(N)["alternating"]
    return table, rule


def tinted(rec, table, rule, invert=False):
    return ec.edit(rec, TINT["op"], TINT["channels"], TINT["value"], TINT["amount"], stats=table, rule=rule, invert=invert)


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

    def frame(self, mode, k=0, t=T, edit=None, where="first", data=None, count=None):
        """one frame from camera(k); edit: a callable — run first (the documented order) or between the sort and the draw; data, count: the
        set to draw (default: the scene's own)"""
        c, gs4d, cam = self.ctx, self.gs4d, camera(k)
        data, count = (self.db, self.n) if data is None else (data, count)
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=gs4d.look_at(cam, CAM_DIR), proj=self.proj)
        if edit is not None and where == "first":
            edit()
        if mode == gs4d.MODE_4D_SORTED:
            c.keygen(data, t, cam, self.kb, self.ib, count)
            c.sort_pairs(self.kb, self.ib, count)
        if edit is not None and where == "between":
            edit()
        c.set_mode(mode)
        if mode == gs4d.MODE_4D_SORTED:
            c.bind(1, self.ib)
            c.bind(2, data)
        else:
            c.bind(1, data)                                     # (instance k is record k)
        c.draw_instanced(count)

    def tint(self, stats, rule, invert=False):
        """the TINT edit of the scene's records by a table buffer, as a callable for frame()"""
        return lambda: self.ctx.edit_colours(self.db, self.n, TINT["op"], TINT["value"], TINT["channels"], TINT["amount"], stats=stats,
                                             **ec.rule_keywords(rule, invert))

    def read(self):
        c = self.ctx
        out = [c.read_pixels()]
        if self.outputs:
            out += [c.read_aux(), *c.read_ids()]
        return out

    def records(self):
        return self.ctx.read(self.db, f32, self.n * 24).reshape(self.n, 24)


def fresh_frame(gs4d, rec, mode, k, outputs, t=T):
    """the frame of a fresh context whose records were uploaded as they are"""
    s = Scene(gs4d, rec, outputs)
    s.frame(mode, k, t)
    out, layout = s.read(), s.ctx.stats()["record_read_bytes"]
    assert s.ctx.shadow_builds(s.db) == 1
    s.ctx.close()
    return out, layout


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w)), f"{int((bits(g) != bits(w)).sum())} words differ"


def differing_pixels(a, b):
    return int((np.abs(a - b).max(-1) > 1.0 / 255.0).sum())


def modes(gs4d):
    return {"sorted": gs4d.MODE_4D_SORTED, "direct": gs4d.MODE_4D_DIRECT}


@pytest.mark.parametrize("outputs", (False, True), ids=("colour", "aux+ids"))
@pytest.mark.parametrize("mode", ("sorted", "direct"))
@pytest.mark.parametrize("layout", tuple(LAYOUT_BYTES))
def test_an_edit_patches_the_current_shadow(gs4d, layout, mode, outputs):
    mode = modes(gs4d)[mode]
    rec = record_set(gs4d, layout)
    table, rule = half_table()
    edited = tinted(rec, table, rule)
    assert int((bits(edited) != bits(rec)).any(1).sum()) == N // 2
    want, want_layout = fresh_frame(gs4d, edited, mode, 1, outputs)
    s = Scene(gs4d, rec, outputs)
    stats = s.ctx.buffer(table)
    s.frame(mode, 0)                                            # builds the shadow, with the uploaded colours
    first = s.read()
    assert s.ctx.shadow_builds(s.db) == 1
    s.frame(mode, 1, edit=s.tint(stats, rule))
    got = s.read()
    st = s.ctx.stats()
    assert st["record_read_bytes"] == want_layout == LAYOUT_BYTES[layout], (st["record_read_bytes"], want_layout)
    same(got, want)
    assert s.ctx.shadow_builds(s.db) == 1, "the edit made the draw repack"
    # the pictures say something: splats on screen, and colours that the edit changed
    clear = np.array(gs4d.CLEAR_COLOR, f32)
    assert differing_pixels(got[0], clear) > 100, "an empty frame"
    unedited, _ = fresh_frame(gs4d, rec, mode, 1, outputs)
    assert differing_pixels(unedited[0], got[0]) > 100, "the edit changed nothing visible"
    # the records themselves: the AoS was written too, and nothing but the selected colours
    assert np.array_equal(bits(s.records()), bits(edited))
    assert not np.array_equal(bits(first[0]), bits(got[0]))
    s.ctx.finish()
    s.ctx.close()


@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_eight_edited_frames_build_the_shadow_once(gs4d, mode):
    mode = modes(gs4d)[mode]
    rec = record_set(gs4d, "symmetric")
    table, rule = half_table()
    s = Scene(gs4d, rec)
    stats = s.ctx.buffer(table)
    s.frame(mode, 0)
    want_rec = rec
    for k in range(1, 9):                                       # no read-back in between: frames in flight on every lane; the halves take turns
        s.frame(mode, k, t=T + 0.01 * k, edit=s.tint(stats, rule, invert=bool(k & 1)))
        want_rec = tinted(want_rec, table, rule, invert=bool(k & 1))
    assert s.ctx.shadow_builds(s.db) == 1
    got = s.read()
    assert s.ctx.shadow_builds(s.db) == 1
    want, _ = fresh_frame(gs4d, want_rec, mode, 8, False, t=T + 0.01 * 8)
    same(got, want)
    assert np.array_equal(bits(s.records()), bits(want_rec))
    s.ctx.finish()
    s.ctx.close()


@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_an_edit_before_the_first_draw_writes_the_records_only(gs4d, mode):
    mode = modes(gs4d)[mode]
    rec = record_set(gs4d, "symmetric")
    table, rule = half_table()
    want, _ = fresh_frame(gs4d, tinted(rec, table, rule), mode, 2, False)
    s = Scene(gs4d, rec)
    stats = s.ctx.buffer(table)
    assert s.ctx.shadow_builds(s.db) == 0
    s.frame(mode, 2, edit=s.tint(stats, rule))                  # no shadow exists yet
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 1
    # ... and a host write before an edit makes the next draw repack, as it always did: the patch is for a CURRENT shadow only
    s.ctx.subdata(s.db, rec)
    s.frame(mode, 2, edit=s.tint(stats, rule))
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 2
    s.ctx.close()


def test_an_edit_between_keygen_and_draw_still_gives_the_picture(gs4d):
    rec = record_set(gs4d, "symmetric")
    table, rule = half_table()
    want, _ = fresh_frame(gs4d, tinted(rec, table, rule), gs4d.MODE_4D_SORTED, 3, False)
    s = Scene(gs4d, rec)
    stats = s.ctx.buffer(table)
    s.frame(gs4d.MODE_4D_SORTED, 0)
    s.frame(gs4d.MODE_4D_SORTED, 3, edit=s.tint(stats, rule), where="between")      # the data version moves under the sort's provenance: the draw reads the index
    same(s.read(), want)
    assert s.ctx.shadow_builds(s.db) == 1
    s.ctx.close()


# ---- 4. hide equals compact ----------------------------------------------------------------------------------------------------------------------
def visibility_table():
    """a table that hides a scattered 40 % of N by the rule {pixels >= 1}: three of every eight records and every tenth"""
    i = np.arange(N)
    hidden = (i % 8 < 3) | (i % 10 == 0)
    table = ec.mask_table(hidden, (1, 0, 0))
    assert N // 4 <= int(hidden.sum()) <= 3 * N // 4
    return table, hidden


@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_hiding_a_selection_draws_the_compacted_complement(gs4d, mode):
    mode = modes(gs4d)[mode]
    rec = record_set(gs4d, "symmetric")
    assert np.isfinite(rec).all() and (rec[:, 23] > 0).all()
    table, hidden = visibility_table()
    kept = np.flatnonzero(~hidden)
    for outputs in (True, False):                               # the planes with ID outputs; the record statistics in a colour frame
        s = Scene(gs4d, rec, outputs)
        c = s.ctx
        stats = c.buffer(table)
        dst, kept_index = c.buffer(nbytes=96 * N), c.buffer(nbytes=4 * N)
        count = c.compact_records(stats, N, src=s.db, dst=dst, kept_index=kept_index, min_pixels=1, invert=True)
        assert c.read_compact_count(count) == (kept.size, kept.size) and np.array_equal(c.read(kept_index, np.uint32, kept.size), kept)
        c.hide(s.db, N, stats, min_pixels=1)
        assert np.array_equal(bits(s.records()), bits(ec.edit(rec, "set", 8, (0.0, 0.0, 0.0, 0.0), stats=table)))
        if outputs:
            s.frame(mode, 1)
            got = s.read()
            s.frame(mode, 1, data=dst, count=kept.size)
            want = s.read()
            same(got[:2], want[:2])                             # the colour image and the aux planes
            (rid, draw, weight), (crid, cdraw, cweight) = got[2:], want[2:]
            assert np.array_equal(bits(weight), bits(cweight)) and np.array_equal(draw, cdraw)
            seen = rid != gs4d.Context.ID_NONE
            assert seen.sum() > 200 and np.array_equal(crid != gs4d.Context.ID_NONE, seen)
            assert np.array_equal(kept[crid[seen]], rid[seen]) and not hidden[rid[seen]].any()
            shown, _ = fresh_frame(gs4d, rec, mode, 1, False)
            assert differing_pixels(shown[0], got[0]) > 100, "hiding changed nothing visible"
        else:
            sb, csb = c.record_stats(N), c.record_stats(kept.size)
            c.set_record_stats(sb, N)
            s.frame(mode, 1)
            c.set_record_stats(csb, kept.size)
            s.frame(mode, 1, data=dst, count=kept.size)
            full, comp = c.read_record_stats(sb, N), c.read_record_stats(csb, kept.size)
            assert np.array_equal(full[kept].view(np.uint8), comp.view(np.uint8))
            assert not full[hidden].view(np.uint8).any(), "a hidden record has statistics"
            assert (full["pixels"] > 0).sum() > 50
        c.finish()
        c.close()


# ---- 5. restore ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("sorted", "direct"))
def test_restore_puts_the_uploaded_colours_back(gs4d, mode):
    mode = modes(gs4d)[mode]
    rec = record_set(gs4d, "full")
    s = Scene(gs4d, rec)
    c = s.ctx
    pristine = c.buffer(rec)
    tabs = ec.tables(N)
    (ta, ra, _), (tb, rb, _) = tabs["alternating"], tabs["one_in_the_last_tile"]
    tc, _ = visibility_table()
    a, b, cc_ = c.buffer(ta), c.buffer(tb), c.buffer(tc)
    s.frame(mode, 1)
    first = s.read()
    c.edit_colours(s.db, N, "set", (0.9, 0.8, 0.1, 0.0), "rgb", stats=a, **ec.rule_keywords(ra))
    c.edit_colours(s.db, N, "mul", (1.0, 1.0, 1.0, 0.25), "a", stats=b, **ec.rule_keywords(rb, True))
    c.edit_colours(s.db, N, "lerp", (0.0, 1.0, 0.0, 1.0), "rgba", 0.5, stats=cc_, min_pixels=1)
    want = ec.edit(rec, "set", 7, (0.9, 0.8, 0.1, 0.0), stats=ta, rule=ra)
    want = ec.edit(want, "mul", 8, (1.0, 1.0, 1.0, 0.25), stats=tb, rule=rb, invert=True)
    want = ec.edit(want, "lerp", 15, (0.0, 1.0, 0.0, 1.0), 0.5, stats=tc)
    assert np.array_equal(bits(s.records()), bits(want)) and (bits(want) != bits(rec)).any(1).all()
    s.frame(mode, 1)
    assert differing_pixels(s.read()[0], first[0]) > 100
    c.restore_colours(s.db, N, pristine)
    assert np.array_equal(bits(s.records()), bits(rec)), "the records are not the uploaded bytes again"
    s.frame(mode, 1)
    same(s.read(), first)
    assert c.shadow_builds(s.db) == 1
    c.finish()
    c.close()


# ---- 6. the chain, end to end --------------------------------------------------------------------------------------------------------------------
RECT = (20, 14, 24, 20)                                        # x, y, w, h: the middle of the 64 x 48 image
HIGHLIGHT = (1.0, 0.0, 1.0, 0.0)


def test_what_a_rectangle_shows_is_tinted_without_a_read_back(gs4d):
    mode = gs4d.MODE_4D_SORTED
    rec = record_set(gs4d, "symmetric")
    before, _ = fresh_frame(gs4d, rec, mode, 1, True)
    x, y, w, h = RECT
    rid = before[2][y:y + h, x:x + w]
    shown = np.unique(rid[rid != gs4d.Context.ID_NONE])
    assert 5 < shown.size < N - 5, shown.size
    s = Scene(gs4d, rec, True)
    c = s.ctx
    stats = c.record_stats(N)
    s.frame(mode, 1)
    c.count_ids(stats, N, rect=RECT)
    c.edit_colours(s.db, N, "lerp", HIGHLIGHT, "rgb", 1.0, stats=stats, min_pixels=1)      # no read-back in between
    s.frame(mode, 1)
    after = s.read()
    got = s.records()
    changed = np.flatnonzero((bits(got) != bits(rec)).any(1))
    assert np.array_equal(changed, shown), "the records that changed are not the records the rectangle shows"
    selected = np.zeros(N, bool)
    selected[shown] = True
    table = ec.mask_table(selected, (1, 0, 0))
    assert np.array_equal(bits(got), bits(ec.edit(rec, "lerp", 7, HIGHLIGHT, 1.0, stats=table)))
    assert np.array_equal(c.read_record_stats(stats, N)["pixels"] > 0, selected)
    # an rgb edit moves no weight: the same planes, and in the rectangle every covered pixel's front-most weight now carries the highlight colour
    same(after[1:], before[1:])
    covered = rid != gs4d.Context.ID_NONE
    target = np.array(HIGHLIGHT[:3], f32)
    d0 = np.linalg.norm(before[0][y:y + h, x:x + w, :3] - target, axis=-1)[covered]
    d1 = np.linalg.norm(after[0][y:y + h, x:x + w, :3] - target, axis=-1)[covered]
    print(f"mean distance to the highlight colour over {int(covered.sum())} covered pixels: {d0.mean():.4f} -> {d1.mean():.4f}")
    assert covered.sum() > 100 and d1.mean() < d0.mean() and (d1 < d0).mean() > 0.5
    assert c.shadow_builds(s.db) == 1
    c.finish()
    c.close()


# ---- 7. ordering without a finish ----------------------------------------------------------------------------------------------------------------
def test_the_call_is_ordered_without_a_finish(gs4d, monkeypatch):
    """an edit right behind draws of the same buffer on the previous lanes: the earlier frame keeps the old colours; a host write into the table
    right behind the call does not change its result"""
    monkeypatch.setenv("GS4D_LANES", "4")
    mode = gs4d.MODE_4D_SORTED
    rec = record_set(gs4d, "symmetric")
    table, rule = half_table()
    old = Scene(gs4d, rec)
    old.frame(mode, 0)
    old_rgba8 = old.ctx.buffer(nbytes=W * H * 4)
    old.ctx.read_frame_rgba8_device(0, old.ctx.device_ptr(old_rgba8)[0], W * H * 4)
    old.ctx.finish()
    want_prev = old.ctx.read(old_rgba8, np.uint8, W * H * 4)
    old.ctx.close()
    want, _ = fresh_frame(gs4d, tinted(rec, table, rule), mode, 1, False)
    s = Scene(gs4d, rec)
    assert s.ctx.stats()["lanes"] == 4
    stats, out = s.ctx.buffer(table), s.ctx.buffer(nbytes=W * H * 4)
    for _ in range(3):
        s.frame(mode, 0)                                        # frames in flight that read the records and the shadow
    tint = s.tint(stats, rule)

    def edit_then_zero_the_table():
        tint()
        s.ctx.subdata(stats, np.zeros_like(table))              # directly behind: the call must not see the zeros

    s.frame(mode, 1, edit=edit_then_zero_the_table)             # the edit is the first call of the next lane's frame
    s.ctx.read_frame_rgba8_device(1, s.ctx.device_ptr(out)[0], W * H * 4)
    got = s.read()
    s.ctx.finish()
    assert np.array_equal(s.ctx.read(out, np.uint8, W * H * 4), want_prev), "the frame before the edit shows other colours than it was drawn with"
    same(got, want)
    assert np.array_equal(bits(s.records()), bits(tinted(rec, table, rule)))
    assert s.ctx.shadow_builds(s.db) == 1
    s.ctx.close()


def test_an_edit_by_the_table_a_draw_adds_to_waits_for_the_draw(gs4d):
    """a draw with record statistics on, then an edit by that table: the same records with and without a finish in between"""
    mode = gs4d.MODE_4D_DIRECT
    rec = record_set(gs4d, "symmetric")
    results = []
    for finish in (True, False):
        s = Scene(gs4d, rec)
        c = s.ctx
        sb = c.record_stats(N)
        c.set_record_stats(sb, N)
        threshold = 1
        if not finish:
            threshold = results[0][2]
        for k in range(3):                                      # frames on three lanes add to the table
            s.frame(mode, k)
        if finish:
            c.finish()
            threshold = int(np.median(c.read_record_stats(sb, N)["pixels"]))
        c.edit_colours(s.db, N, "lerp", TINT["value"], "rgba", TINT["amount"], stats=sb, min_pixels=threshold)
        got = s.records()
        results.append((got, c.read_record_stats(sb, N), threshold))
        c.finish()
        c.close()
    (slow, table, threshold), (fast, table_fast, _) = results
    assert np.array_equal(table.view(np.uint8), table_fast.view(np.uint8))
    assert np.array_equal(bits(fast), bits(slow)), "without a finish the edit saw another table"
    want = ec.edit(rec, "lerp", 15, TINT["value"], TINT["amount"], stats=np.ascontiguousarray(table).view(ec.STAT), rule=(threshold, 0, 0))
    assert np.array_equal(bits(slow), bits(want))
    changed = int((bits(slow) != bits(rec)).any(1).sum())
    assert N // 4 <= changed <= 3 * N // 4 + 1, changed


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


def test_an_edit_waits_for_a_rerun(gs4d, monkeypatch):
    """staged_cases' case a (as tests/test_gpu_shade.py): frames at T0 teach the guesses, the frame at T1 outgrows a segment block; the edit
    behind it settles the draw first — the re-run uses the old colours"""
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    rec, _ = staged_cases.build(gs4d, "a")
    Wb, Hb, n = staged_cases.W, staged_cases.H, rec.shape[0]
    fresh = gs4d.Context(Wb, Hb)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    sorted_frame(gs4d, fresh, (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n)), n, staged_cases.T1)
    want = fresh.read_pixels()
    fresh.close()
    ctx = gs4d.Context(Wb, Hb)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    ctx.edit_colours(bufs[0], n, TINT["op"], TINT["value"], TINT["channels"], TINT["amount"])      # no read-back in between
    s1 = ctx.stats()
    assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
    assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    got = ctx.read_pixels()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"
    assert np.array_equal(bits(ctx.read(bufs[0], f32, n * 24)).reshape(n, 24), bits(ec.edit(rec, TINT["op"], TINT["channels"], TINT["value"], TINT["amount"])))
    ctx.close()
