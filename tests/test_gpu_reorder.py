"""GPU: gs4d_spatial_order and gs4d_gather_records — a record set in Morton order of its positions, and the gather that applies an index list to
records and side tables (include/gs4d.h).

order_index is checked byte for byte against the numpy restatement (tests/reorder_cases.py: the header's float32 operations, a stable argsort);
the gather against src[index], with sentinel-filled outputs and guard buffers around every buffer; and a draw of the reordered set gives the
bits of a draw of the original one in every output when no two records share a depth key.  All calls go through the Python binding over the C ABI."""
import ctypes
import functools

import numpy as np
import pytest

import compact_cases as cc
import reorder_cases as rc
import scenes

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD):
    return bool((ctx.read(buf, np.uint8, nbytes) == SENTINEL).all())


def check_order(ctx, pos, stride, pos_offset, what):
    """uploads the records between guard buffers, orders them into a sentinel-filled index between guards: every byte against the restatement"""
    n = pos.shape[0]
    g0 = fill(ctx, GUARD)
    src = ctx.buffer(rc.records_with_positions(pos, stride, pos_offset))
    g1 = fill(ctx, GUARD)
    oi = fill(ctx, 4 * n + 64)
    g2 = fill(ctx, GUARD)
    assert ctx.spatial_order(src, n, stride=stride, pos_offset=pos_offset, order_index=oi) == oi
    got = ctx.read(oi, np.uint8, 4 * n + 64)
    want = rc.order(pos)
    assert np.array_equal(got[:4 * n].view(np.uint32), want), f"{what}: order_index differs from the reference in {int((got[:4 * n].view(np.uint32) != want).sum())} of {n} entries"
    assert (got[4 * n:] == SENTINEL).all(), f"{what}: bytes behind the n entries changed"
    assert untouched(ctx, g0) and untouched(ctx, g1) and untouched(ctx, g2), f"{what}: a guard buffer changed"
    assert np.array_equal(ctx.read(src, np.uint32, n * stride // 4).reshape(n, -1), rc.records_with_positions(pos, stride, pos_offset)), f"{what}: src changed"
    for b in (g0, src, g1, oi, g2):
        ctx.delete(b)
    return want


# ---- 1. the order --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", rc.ALL_PATTERNS)
def test_the_order_equals_the_reference_byte_for_byte(gs4d, pattern):
    ctx = gs4d.Context(64, 64)
    for n in rc.SIZES:
        pos = rc.positions(pattern, n)
        want = check_order(ctx, pos, 96, 0, f"{pattern}, n = {n}")
        ident = np.arange(n, dtype=np.uint32)
        if pattern in ("identical", "sorted", "hostile/unplaced_all"):
            assert np.array_equal(want, ident)
        if pattern.startswith("hostile/"):
            un = np.flatnonzero(~rc.placed(pos))
            assert np.array_equal(want[n - un.size:], un), "the unplaced records come last, in their original order"
            if pattern in ("hostile/nan", "hostile/inf", "hostile/mixed", "hostile/flat3") and n >= 63:
                assert 0 < un.size < n
    ctx.finish()                                              # reports device-side check failures
    ctx.close()


@pytest.mark.parametrize("stride", rc.STRIDES)
def test_every_stride_and_position_offset(gs4d, stride):
    ctx = gs4d.Context(64, 64)
    for pos_offset in rc.pos_offsets(stride):
        for n in rc.STRIDE_SIZES:
            for pattern in ("uniform", "hostile/mixed"):
                check_order(ctx, rc.positions(pattern, n), stride, pos_offset, f"{pattern}, n = {n}, stride = {stride}, pos_offset = {pos_offset}")
    ctx.finish()
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    src, oi, idx, dst = ctx.buffer(cc.records(4, 96)), fill(ctx, 64), ctx.buffer(np.zeros(4, np.uint32)), fill(ctx, 4 * 96)
    ctx.spatial_order(src, 0, order_index=oi)
    ctx.gather_records(idx, 0, src, 4, dst=dst)
    ctx.gather_records(idx, 4, src, 0, dst=dst)               # no record to take: every entry is out of range
    ctx.finish()
    assert untouched(ctx, oi, 64) and untouched(ctx, dst, 4 * 96)
    ctx.close()


# ---- 2. the gather -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", rc.GATHER_STRIDES)
def test_the_gather_equals_the_reference_and_touches_nothing_else(gs4d, stride):
    ctx = gs4d.Context(64, 64)
    for nsrc in (1, 65, 2049):
        src_host = cc.records(nsrc, stride)
        for name, index in rc.index_lists(nsrc).items():
            m = index.size
            # a guard on both sides of every buffer
            bufs = []
            for payload in (index, src_host, np.full(m * stride, SENTINEL, np.uint8)):
                bufs += [fill(ctx, GUARD), ctx.buffer(payload)]
            bufs.append(fill(ctx, GUARD))
            g0, ib, g1, sb, g2, db, g3 = bufs
            assert ctx.gather_records(ib, m, sb, nsrc, stride=stride, dst=db) == db
            got = ctx.read(db, np.uint32, m * stride // 4).reshape(m, -1)
            want = rc.gather_reference(index, src_host, np.full((m, stride // 4), 0xA5A5A5A5, np.uint32))
            what = f"{name}, nsrc = {nsrc}, m = {m}, stride = {stride}"
            assert np.array_equal(got, want), f"{what}: {int((got != want).any(1).sum())} slots differ"
            if name == "out_of_range":
                skipped = index >= nsrc
                assert skipped.sum() >= 2 and (got[skipped] == 0xA5A5A5A5).all(), f"{what}: a skipped slot changed"
            assert all(untouched(ctx, g) for g in (g0, g1, g2, g3)), f"{what}: a guard buffer changed"
            assert np.array_equal(ctx.read(ib, np.uint32, m), index) and np.array_equal(ctx.read(sb, np.uint32, nsrc * stride // 4).reshape(nsrc, -1), src_host)
            for b in bufs:
                ctx.delete(b)
    ctx.finish()
    ctx.close()


def test_round_trip_records_and_a_side_table(gs4d):
    n = 70_001
    pos = rc.positions("uniform", n)
    rec = rc.records_with_positions(pos, 96, 0)
    ctx = gs4d.Context(64, 64)
    data, table = ctx.buffer(rec), ctx.buffer(rc.side_table(n))
    dst, oi = ctx.reorder_spatial(data, n)
    rows = ctx.gather_records(oi, n, table, n, stride=8)      # the 8-byte side table through the same index
    order = ctx.read(oi, np.uint32, n)
    assert np.array_equal(order, rc.order(pos))
    got = ctx.read(dst, np.uint32, n * 24).reshape(n, 24)
    assert np.array_equal(got, rec[order])
    got_rows = ctx.read(rows, np.uint32, n * 2).reshape(n, 2)
    assert np.array_equal(got_rows[:, 0], order) and np.array_equal(got_rows[:, 1], ~order), "a row no longer names its record"
    # the rows still sit beside their records: word 4 of cc.records is a function of the record's index, the row says which
    assert np.array_equal(got[:, 4], cc.records(n, 96)[got_rows[:, 0], 4])
    # ... and the inverse gather brings the original back: index list = the inverse permutation, itself made by a gather of words
    inv = np.empty(n, np.uint32)
    inv[order] = np.arange(n, dtype=np.uint32)
    back = ctx.gather_records(ctx.buffer(inv), n, dst, n)
    assert np.array_equal(ctx.read(back, np.uint32, n * 24).reshape(n, 24), rec)
    ctx.close()


# ---- 3. argument errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_as_they_were(gs4d):
    n, stride = 300, 96
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    rec = rc.records_with_positions(rc.positions("uniform", n), stride, 0)
    src, oi, dst, idx = ctx.buffer(rec), fill(ctx, 4 * n), fill(ctx, n * stride), ctx.buffer(np.arange(n, dtype=np.uint32))
    short_src, short_oi, short_dst, short_idx, dead = ctx.buffer(rec[:-1]), fill(ctx, 4 * n - 4), fill(ctx, n * stride - 16), ctx.buffer(np.arange(n - 1, dtype=np.uint32)), fill(ctx, 64)
    ctx.delete(dead)
    sz = ctypes.c_size_t

    def order(src=src, n=n, stride=stride, pos_offset=0, oi=oi):
        return lib.gs4d_spatial_order(ctx._h, src, sz(n), sz(stride), sz(pos_offset), oi)

    def gather(idx=idx, m=n, src=src, nsrc=n, stride=stride, dst=dst):
        return lib.gs4d_gather_records(ctx._h, idx, sz(m), src, sz(nsrc), sz(stride), dst)

    bad_order = {
        "n > 0xFFFFFFFF": dict(n=1 << 32), "stride 0": dict(stride=0), "stride not a multiple of 16": dict(stride=100), "stride above 1024": dict(stride=1040),
        "pos_offset not a multiple of 4": dict(pos_offset=2), "pos_offset past the record": dict(pos_offset=88), "pos_offset far past": dict(pos_offset=1 << 40),
        "dead buffer": dict(oi=dead), "unknown name": dict(src=9999), "no src": dict(src=0), "no order_index": dict(oi=0), "src == order_index": dict(oi=src),
        "src too small": dict(src=short_src), "order_index too small": dict(oi=short_oi),
    }
    bad_gather = {
        "m > 0xFFFFFFFF": dict(m=1 << 32), "nsrc > 0xFFFFFFFF": dict(nsrc=1 << 32), "stride 0": dict(stride=0), "stride not a multiple of 16": dict(stride=40),
        "stride 12": dict(stride=12), "stride above 1024": dict(stride=2048), "dead buffer": dict(dst=dead), "unknown name": dict(idx=9999), "no index": dict(idx=0), "no src": dict(src=0),
        "no dst": dict(dst=0), "index == src": dict(idx=src), "index == dst": dict(dst=idx), "src == dst": dict(dst=src), "index too small": dict(idx=short_idx),
        "src too small": dict(src=short_src), "dst too small": dict(dst=short_dst),
    }
    for what, kw in bad_order.items():
        assert order(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    for what, kw in bad_gather.items():
        assert gather(**kw) == -1 and lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    for b, nbytes in ((oi, 4 * n), (dst, n * stride), (short_oi, 4 * n - 4), (short_dst, n * stride - 16)):
        assert untouched(ctx, b, nbytes), "a refused call wrote something"
    assert np.array_equal(ctx.read(src, np.uint32, n * 24).reshape(n, 24), rec) and np.array_equal(ctx.read(idx, np.uint32, n), np.arange(n, dtype=np.uint32))
    # the calls work after the refusals
    assert order() == 0 and gather(idx=oi) == 0
    want = rc.order(rec[:, :3].view(np.float32))
    assert np.array_equal(ctx.read(oi, np.uint32, n), want) and np.array_equal(ctx.read(dst, np.uint32, n * 24).reshape(n, 24), rec[want])
    ctx.close()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------------
W, H, N = 256, 256, 3000
T = 25.0


@functools.lru_cache(maxsize=1)
def cube4d(gs4d):
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(N)
    rec = gs4d.build_records_4d(pos4, q, scale * 3.0, life, fade, vel, rgba)          # (a few pixels per splat at this size)
    rec.setflags(write=False)
    return rec


class Scene:
    """a context with a 4D set whose depth keys at (T, the cube camera) are pairwise distinct, and the same set in spatial order"""

    def __init__(self, gs4d, distinct=True):
        self.gs4d = gs4d
        self.ctx = c = gs4d.Context(W, H)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        self.view, self.proj = gs4d.look_at(*scenes.CAM_CUBE), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
        rec = np.array(cube4d(gs4d))
        if distinct:
            # the condition of the guarantee: the later record of every pair with equal keys is dropped before the upload
            db = c.buffer(rec)
            kb, ib = c.buffer(nbytes=4 * N), c.buffer(nbytes=4 * N)
            c.keygen(db, T, scenes.CAM_CUBE[0], kb, ib, N)
            keys = c.read(kb, np.uint32, N)
            _, first = np.unique(keys, return_index=True)
            rec = rec[np.sort(first)]
            for b in (db, kb, ib):
                c.delete(b)
        self.rec, self.n = rec, rec.shape[0]
        assert self.n > 0.9 * N
        self.db = c.buffer(rec)
        self.kb, self.ib = c.buffer(nbytes=4 * self.n), c.buffer(nbytes=4 * self.n)
        self.rdb, oi = c.reorder_spatial(self.db, self.n)
        self.order = c.read(oi, np.uint32, self.n)
        assert np.array_equal(self.order, rc.order(rec[:, :3]))
        assert np.array_equal(bits(c.read(self.rdb, np.float32, self.n * 24)).reshape(-1, 24), bits(rec[self.order]))
        assert (self.order != np.arange(self.n)).sum() > 0.9 * self.n                  # the reorder moves nearly every record

    def frame(self, reordered, t=T):
        c, gs4d = self.ctx, self.gs4d
        data = self.rdb if reordered else self.db
        c.clear()
        c.set_uniforms(time=t, min_opacity=0.0, view=self.view, proj=self.proj)
        c.keygen(data, t, scenes.CAM_CUBE[0], self.kb, self.ib, self.n)
        c.sort_pairs(self.kb, self.ib, self.n)
        c.set_mode(gs4d.MODE_4D_SORTED)
        c.bind(1, self.ib)
        c.bind(2, data)
        c.draw_instanced(self.n)


def test_the_reordered_set_draws_the_same_bits_in_every_output(gs4d, monkeypatch):
    monkeypatch.delenv("GS4D_STAGED", raising=False)
    s = Scene(gs4d)
    c = s.ctx
    c.set_id_outputs(True)                                    # (a frame with ID outputs has aux outputs too)
    s.frame(False)
    keys = c.read(s.kb, np.uint32, s.n)
    assert np.unique(keys).size == s.n, "the condition of the guarantee: pairwise distinct depth keys"
    full, aux, (rid, draw, weight) = c.read_pixels(), c.read_aux(), c.read_ids()
    s.frame(True)
    assert np.unique(c.read(s.kb, np.uint32, s.n)).size == s.n
    got, raux, (rrid, rdraw, rweight) = c.read_pixels(), c.read_aux(), c.read_ids()
    assert np.array_equal(bits(got), bits(full)), f"{int((bits(got) != bits(full)).any(-1).sum())} pixels differ"
    assert np.array_equal(bits(raux), bits(aux))
    assert np.array_equal(bits(rweight), bits(weight)) and np.array_equal(rdraw, draw)
    seen = rid != gs4d.Context.ID_NONE
    assert seen.sum() > 200 and np.array_equal(rrid != gs4d.Context.ID_NONE, seen)
    assert np.array_equal(s.order[rrid[seen]], rid[seen])
    clear = np.array(gs4d.CLEAR_COLOR, np.float32)
    assert int((np.abs(full - clear).max(-1) > 1.0 / 255.0).sum()) > 200, "an empty frame"
    # the record statistics, in frames of their own (they are defined for colour-only frames)
    c.set_id_outputs(False)
    c.set_aux_outputs(False)
    sb, rsb = c.record_stats(s.n), c.record_stats(s.n)
    c.set_record_stats(sb, s.n)
    s.frame(False)
    c.set_record_stats(rsb, s.n)
    s.frame(True)
    st, rst = c.read_record_stats(sb, s.n), c.read_record_stats(rsb, s.n)
    assert np.array_equal(st[s.order].view(np.uint8), rst.view(np.uint8))
    assert (st["pixels"] > 0).sum() > 100
    c.finish()
    c.close()


# ---- 5. ordering -----------------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_ordered_without_a_finish(gs4d, monkeypatch):
    """frames in flight on three lanes; on the fourth a host write into src, the order and the gather straight behind it, a host write into src
    and into the index behind those; then keygen, sort and draw of dst, and a second reorder on the next lane into the same outputs: the result
    is that of call order"""
    monkeypatch.setenv("GS4D_LANES", "4")
    s = Scene(gs4d)
    c, n, rec = s.ctx, s.n, s.rec
    assert c.stats()["lanes"] == 4
    for k in range(3):
        s.frame(False, T - 1.0 + k)
    c.clear()
    other = np.array(rec[::-1])                               # the same records the other way round: another permutation entirely
    oi, dst = fill(c, 4 * n), fill(c, 96 * n)
    c.subdata(s.db, other)                                    # directly in front: the call sees the new bytes
    c.spatial_order(s.db, n, order_index=oi)
    c.gather_records(oi, n, s.db, n, dst=dst)
    c.subdata(s.db, np.zeros((n, 24), np.float32))            # directly behind: it must not see the zeros
    want = rc.order(other[:, :3])
    assert not np.array_equal(want, s.order)
    got_dst = c.read(dst, np.float32, n * 24).reshape(n, 24)
    c.subdata(oi, np.zeros(n, np.uint32))                     # (behind the read of dst, which waited for the gather only)
    assert np.array_equal(bits(got_dst), bits(other[want]))
    # the dst of the call as the data of a frame on the next lane, against the original set drawn the same way
    c.subdata(s.db, rec)
    s.frame(False)
    full = c.read_pixels()
    keep = s.rdb
    s.rdb = dst
    s.frame(True)
    got = c.read_pixels()
    s.rdb = keep
    assert np.array_equal(bits(got), bits(full)), f"{int((bits(got) != bits(full)).any(-1).sum())} pixels differ"      # (distinct depth keys: the guarantee)
    # a second reorder, of the original set, into the same outputs while the frame above may still be in flight on its lane
    s.frame(True)
    c.spatial_order(s.db, n, order_index=oi)
    c.gather_records(oi, n, s.db, n, dst=dst)
    s.frame(False)
    assert np.array_equal(c.read(oi, np.uint32, n), s.order)
    assert np.array_equal(bits(c.read(dst, np.float32, n * 24)).reshape(n, 24), bits(rec[s.order]))
    c.finish()
    c.close()
