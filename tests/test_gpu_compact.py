"""GPU: gs4d_compact_records — a record set pruned by its record statistics, on the device (include/gs4d.h).

Contract: record i is kept iff (pixels >= min_pixels && wmax >= min_wmax && wsum >= min_wsum) != invert; the kept records land in dst in ascending
i, their indices in kept_index, {kept, written} in count; no slot at or beyond the capacity of the outputs is written.  An integer problem: every
comparison is exact, against compact_cases.reference (np.flatnonzero on the rule).  All calls go through the Python binding over the C ABI."""
import ctypes
import functools

import numpy as np
import pytest

import compact_cases as cc
import id_cases
import staged_cases
import stats_cases as sc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@functools.lru_cache(maxsize=4)
def records(n, stride):
    r = cc.records(n, stride)
    r.setflags(write=False)
    return r


def bits_to_float(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def rule_kw(rule, invert=False):
    return {"min_pixels": rule[0], "min_wmax": bits_to_float(rule[1]), "min_wsum": rule[2], "invert": invert}


class Table:
    """one context holding n records of `stride` bytes and a statistics table of n rows; run() compacts into fresh sentinel-filled outputs"""

    def __init__(self, gs4d, n, stride=96, with_src=True):
        self.gs4d, self.n, self.stride = gs4d, n, stride
        self.ctx = gs4d.Context(64, 64)
        self.src_host = records(n, stride) if with_src else None
        self.src = (self.ctx.buffer(self.src_host) if n else self.ctx.buffer(nbytes=16)) if with_src else None
        self.stats = self.ctx.buffer(nbytes=max(16, 16 * n))
        self.count = self.ctx.buffer(np.full(8, SENTINEL, np.uint8))

    def upload(self, table):
        self.table = table
        if self.n:
            self.ctx.subdata(self.stats, table)

    def sentinel(self, slots, unit):
        """a buffer of `slots` units (at least 16 bytes), and a guard buffer created right after it, both filled with the sentinel"""
        nbytes = max(16, slots * unit)
        return self.ctx.buffer(np.full(nbytes, SENTINEL, np.uint8)), self.ctx.buffer(np.full(4096, SENTINEL, np.uint8)), nbytes

    def run(self, rule, invert=False, cap_dst="n", cap_idx="n", check=True):
        """cap_dst / cap_idx: slots of the output, 'n' for room for every record, None: output not given.  Returns (kept, written, idx)."""
        c, n, stride = self.ctx, self.n, self.stride
        cd = n if cap_dst == "n" else cap_dst
        ci = n if cap_idx == "n" else cap_idx
        dst = guard_d = idx = guard_i = None
        if cd is not None:
            dst, guard_d, dbytes = self.sentinel(cd, stride)
        if ci is not None:
            idx, guard_i, ibytes = self.sentinel(ci, 4)
        c.compact_records(self.stats, n, src=self.src if dst else None, stride=stride, dst=dst, kept_index=idx, count=self.count, **rule_kw(rule, invert))
        kept, written = c.read_compact_count(self.count)
        # what the buffers hold: their real capacities in slots (a buffer is at least 16 bytes)
        real_d = None if cd is None else dbytes // stride
        real_i = None if ci is None else ibytes // 4
        want_d, want_i, want_kept, want_written = cc.reference(self.table, rule, self.src_host if dst else None, stride, real_d, real_i, invert)
        got_i = None
        if check:
            assert (kept, written) == (want_kept, want_written), (kept, written, want_kept, want_written)
        if dst:
            got = c.read(dst, np.uint8, dbytes)
            assert np.array_equal(got[:written * stride].reshape(written, stride), want_d), "dst differs from the reference"
            assert (got[written * stride:] == SENTINEL).all(), "bytes of dst beyond the written slots changed"
            assert (c.read(guard_d, np.uint8, 4096) == SENTINEL).all(), "the buffer created after dst changed"
        if idx:
            got = c.read(idx, np.uint8, ibytes)
            got_i = got[:written * 4].view(np.uint32).copy()
            assert np.array_equal(got_i, want_i), "kept_index differs from the reference"
            assert (got[written * 4:] == SENTINEL).all(), "bytes of kept_index beyond the written slots changed"
            assert (c.read(guard_i, np.uint8, 4096) == SENTINEL).all(), "the buffer created after kept_index changed"
        for b in (dst, guard_d, idx, guard_i):
            if b:
                c.delete(b)
        return kept, written, got_i

    def close(self):
        self.ctx.close()


# ---- 1. exact against numpy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cc.SIZES)
def test_every_pattern_equals_the_reference(gs4d, n):
    t = Table(gs4d, n)
    for pattern in cc.PATTERNS:
        t.upload(cc.pattern_table(pattern, n))
        kept, written, idx = t.run(cc.RULES["prune"])
        assert kept == written == cc.pattern_kept(pattern, n), pattern
        ikept, _, inv = t.run(cc.RULES["prune"], invert=True)
        assert ikept == n - kept
        assert np.array_equal(np.sort(np.concatenate([idx, inv])), np.arange(n, dtype=np.uint32)), "the two index lists must partition 0..n-1"
    for pattern in ("p50", "alternating"):                                     # the same patterns, every field with a threshold (a 64-bit one for wsum)
        t.upload(cc.pattern_table(pattern, n, cc.RULES["all_fields"]))
        assert t.run(cc.RULES["all_fields"])[0] == cc.pattern_kept(pattern, n)
    t.close()


def test_the_large_case_equals_the_reference(gs4d):
    n = cc.LARGE
    t = Table(gs4d, n)
    for pattern in ("p50", "tile", "p03", "p97", "all", "last"):
        t.upload(cc.pattern_table(pattern, n))
        kept, written, idx = t.run(cc.RULES["prune"])
        assert kept == written == cc.pattern_kept(pattern, n), pattern
        ikept, _, inv = t.run(cc.RULES["prune"], invert=True, cap_dst=None)
        assert ikept == n - kept and np.array_equal(np.sort(np.concatenate([idx, inv])), np.arange(n, dtype=np.uint32))
    t.close()


@pytest.mark.parametrize("n, stride", [(None, 16), (3 * 4096 + 1, 96), (33 * 4096 - 3, 96)])
def test_rows_that_straddle_each_threshold(gs4d, n, stride):
    """the 90 edge rows alone (one tile), and repeated across tiles at stride 96: every row on many lanes, wave offsets and tile edges"""
    st = cc.threshold_table(n)
    t = Table(gs4d, st.size, stride=stride)
    t.upload(st)
    for name, rule in cc.RULES.items():
        for invert in (False, True):
            kept, _, _ = t.run(rule, invert=invert)
            assert kept == int(cc.keeps(st, rule, invert).sum())
    if n is None:
        assert t.run(cc.RULES["all_fields"])[0] == 3 * 2 * 3 * 2
    assert t.run(cc.RULES["anything"])[0] == st.size and t.run(cc.RULES["anything"], invert=True)[0] == 0
    t.close()


@pytest.mark.parametrize("stride", cc.STRIDES)
@pytest.mark.parametrize("n", cc.STRIDE_SIZES)
def test_every_stride(gs4d, n, stride):
    t = Table(gs4d, n, stride)
    for pattern in ("p50", "all", "p03", "last"):
        t.upload(cc.pattern_table(pattern, n))
        assert t.run(cc.RULES["prune"])[0] == cc.pattern_kept(pattern, n)
    t.close()


# ---- 2. capacity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, cc.LARGE])
def test_outputs_smaller_than_the_kept_set(gs4d, n):
    t = Table(gs4d, n)
    t.upload(cc.pattern_table("p50", n))
    kept = cc.pattern_kept("p50", n)
    for cap in (kept - 1, kept // 2, 0):
        for cap_dst, cap_idx in ((cap, cap), (cap, "n"), ("n", cap), (cap, None), (None, cap)) if n < cc.LARGE else ((cap, cap), (cap, None), (None, cap)):
            k, w, _ = t.run(cc.RULES["prune"], cap_dst=cap_dst, cap_idx=cap_idx)
            real = min(max(16, cap * 96) // 96 if cap_dst == cap else n, max(16, cap * 4) // 4 if cap_idx == cap else n)      # (a buffer is at least 16 bytes)
            assert k == kept and w == min(kept, real), (cap_dst, cap_idx, k, w)
    t.close()


# ---- 3. optional outputs ----------------------------------------------------------------------------------------------------------------------------
def test_optional_outputs(gs4d):
    n = 4097
    kept = cc.pattern_kept("p50", n)
    t = Table(gs4d, n, with_src=False)                                         # index only, src = dst = 0
    t.upload(cc.pattern_table("p50", n))
    assert t.run(cc.RULES["prune"], cap_dst=None)[:2] == (kept, kept)
    assert t.run(cc.RULES["prune"], cap_dst=None, cap_idx=None)[:2] == (kept, kept)      # count only
    t.close()
    t = Table(gs4d, n)
    t.upload(cc.pattern_table("p50", n))
    assert t.run(cc.RULES["prune"], cap_idx=None)[:2] == (kept, kept)          # records only
    assert t.run(cc.RULES["prune"], cap_dst=None, cap_idx=None)[:2] == (kept, kept)      # count only, src named or not
    t.close()
    t = Table(gs4d, 0)                                                         # n == 0 writes {0, 0}
    t.upload(np.zeros(0, cc.STAT))
    for cap_dst, cap_idx in (("n", "n"), (None, None), (4, 4)):
        assert t.run(cc.RULES["anything"], cap_dst=cap_dst, cap_idx=cap_idx)[:2] == (0, 0)
    t.close()


# ---- 4. argument errors -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_queue_nothing(gs4d):
    n, stride = 300, 96
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    fill = lambda nbytes: ctx.buffer(np.full(nbytes, SENTINEL, np.uint8))
    st = cc.pattern_table("all", n)
    stats, src, dst, idx, count = ctx.buffer(st), ctx.buffer(records(n, stride)), fill(n * stride), fill(n * 4), fill(8)
    short_stats, short_src, short_count, dead = ctx.buffer(st[:-1]), ctx.buffer(records(n, stride)[:-1]), fill(4), fill(64)
    ctx.delete(dead)

    def rule(min_pixels=1, min_wmax=0, min_wsum=0, flags=0, reserved=0):
        r = np.zeros(1, gs4d.Context.KEEP_RULE)
        r["min_pixels"], r["min_wmax"], r["min_wsum"], r["flags"], r["reserved"] = min_pixels, min_wmax, min_wsum, flags, reserved
        return r

    def call(stats=stats, n=n, r=rule(), src=src, stride=stride, dst=dst, idx=idx, count=count):
        return lib.gs4d_compact_records(ctx._h, stats, ctypes.c_size_t(n), None if r is None else r.ctypes.data_as(ctypes.c_void_p), src, stride, dst, idx, count)

    bad = {
        "n > 0xFFFFFFFF": dict(n=1 << 32),
        "stats too small": dict(stats=short_stats),
        "src too small": dict(src=short_src),
        "count too small": dict(count=short_count),
        "dst without src": dict(src=0),
        "stats == src": dict(src=stats),
        "src == dst": dict(dst=src),
        "dst == kept_index": dict(idx=dst),
        "kept_index == count": dict(count=idx),
        "stats == count": dict(count=stats),
        "stats == dst": dict(dst=stats),
        "rule == NULL": dict(r=None),
        "reserved != 0": dict(r=rule(reserved=1)),
        "unknown flag": dict(r=rule(flags=2)),
        "unknown flag beside the known one": dict(r=rule(flags=gs4d.KEEP_INVERT | 0x80000000)),
        "stride 0": dict(stride=0),
        "stride not a multiple of 16": dict(stride=100),
        "stride above 1024": dict(stride=1040),
        "no count": dict(count=0),
        "no stats": dict(stats=0),
        "dead buffer": dict(idx=dead),
        "unknown name": dict(dst=9999),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert lib.gs4d_last_error(ctx._h), what
    ctx.finish()
    for b, nbytes in ((dst, n * stride), (idx, n * 4), (count, 8), (short_count, 4)):
        assert (ctx.read(b, np.uint8, nbytes) == SENTINEL).all(), "a refused call wrote something"
    assert np.array_equal(ctx.read(stats, cc.STAT, n), st)
    assert call() == 0                                                          # the same arguments, valid: the call works after the refusals
    assert ctx.read_compact_count(count) == (n, n)
    assert np.array_equal(ctx.read(dst, np.uint32, n * stride // 4).reshape(n, -1), records(n, stride))
    ctx.close()


# ---- 5., 6., 8.: ordering -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["auto", "ordered"])
def draw_path(request, monkeypatch):
    """both draw paths, as tests/test_gpu_record_stats.py has them"""
    if request.param == "ordered":
        monkeypatch.setenv("GS4D_DRAW_PATH", "ordered")
    else:
        monkeypatch.delenv("GS4D_DRAW_PATH", raising=False)
    return request.param


W5 = H5 = 96
PRUNE = dict(min_pixels=1, min_wmax=1.0 / 255.0)
PRUNE_RULE = (1, cc.BITS_1_255, 0)


@functools.lru_cache(maxsize=1)
def layered_params():
    """400 overlapping records on 96 x 96 pixels, a fifth of them off the image, alphas from 0.001 (below one 8-bit step) to 1"""
    rng = np.random.default_rng(cc.seed("compact/layered"))
    n = 400
    px, py = rng.uniform(-2.0, W5 + 2.0, n), rng.uniform(-2.0, H5 + 2.0, n)
    px[::5] += 3.0 * W5
    s = np.where(rng.uniform(size=n) < 0.33, sc.S_LARGE, sc.S_SMALL) * rng.uniform(0.7, 1.2, n)
    alpha = np.where(rng.uniform(size=n) < 0.25, rng.uniform(0.001, 0.003, n), rng.uniform(0.05, 1.0, n))
    rgba = np.concatenate([rng.uniform(0.0, 1.0, (n, 3)), alpha[:, None]], 1)
    return px, py, rng.uniform(-8.0, 8.0, n), s, rgba


class Direct:
    """a context drawing `rec` with GS4D_MODE_4D_DIRECT (instance k is record k) and statistics on"""

    def __init__(self, gs4d, W, H, rec):
        self.n = rec.shape[0]
        self.ctx = c = gs4d.Context(W, H)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        self.db, self.sb = c.buffer(rec), c.record_stats(self.n)
        view, proj = sc.mats(gs4d, W, H)
        c.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
        c.set_mode(gs4d.MODE_4D_DIRECT)
        c.bind(1, self.db)
        c.set_record_stats(self.sb, self.n)

    def frame(self):
        self.ctx.clear()
        self.ctx.draw_instanced(self.n)

    def outputs(self):
        return self.ctx.buffer(np.full(self.n * 96, SENTINEL, np.uint8)), self.ctx.buffer(np.full(self.n * 4, SENTINEL, np.uint8))


def check_against_table(ctx, table, rec, dst, idx, count, rule=PRUNE_RULE):
    """the outputs of a compaction of `rec` equal the reference applied to `table`; returns the kept indices"""
    n = rec.shape[0]
    want_d, want_i, kept, written = cc.reference(table_bits(table), rule, rec, 96, n, n)
    assert ctx.read_compact_count(count) == (kept, written)
    assert np.array_equal(ctx.read(idx, np.uint32, kept), want_i)
    assert np.array_equal(ctx.read(dst, np.uint8, kept * 96).reshape(-1, 96), want_d)
    return want_i


def table_bits(table):
    """read_record_stats' array (wmax float32) as compact_cases.STAT (wmax as its bit pattern)"""
    return np.ascontiguousarray(table).view(cc.STAT)


def test_compaction_waits_for_the_draws_of_every_lane(gs4d, draw_path):
    rec = sc.records(gs4d, W5, H5, *layered_params())
    d = Direct(gs4d, W5, H5, rec)
    frames = 2 * d.ctx.stats()["lanes"] + 1
    for _ in range(frames):
        d.frame()
    dst, idx = d.outputs()
    count = d.ctx.compact_records(d.sb, d.n, src=d.db, dst=dst, kept_index=idx, **PRUNE)      # immediately: no read-back, no finish
    table = d.ctx.read_record_stats(d.sb, d.n)                                                 # only now
    kept_idx = check_against_table(d.ctx, table, rec, dst, idx, count)
    assert 0 < kept_idx.size < d.n
    assert (table["pixels"] > 0).sum() > kept_idx.size                                         # the wmax threshold drops records that did show
    d.ctx.close()
    # a fresh context that drew the same frames and was read back frame by frame: the statistics are deterministic
    f = Direct(gs4d, W5, H5, rec)
    for _ in range(frames):
        f.frame()
        slow = f.ctx.read_record_stats(f.sb, f.n)
    f.ctx.close()
    assert np.array_equal(table_bits(slow), table_bits(table))
    assert np.array_equal(np.flatnonzero(cc.keeps(table_bits(slow), PRUNE_RULE)), kept_idx)


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


def test_compaction_waits_for_a_rerun(gs4d, monkeypatch, draw_path):
    """staged_cases' case a: frames at T0 teach the guesses, the frame at T1 outgrows a segment block; the library re-runs it with exact lists
    when the compaction asks for the table"""
    monkeypatch.setenv("GS4D_NB", str(staged_cases.NB))
    rec, _ = staged_cases.build(gs4d, "a")
    W, H, n = staged_cases.W, staged_cases.H, rec.shape[0]
    fresh = gs4d.Context(W, H)
    fresh.set_clear_color(gs4d.CLEAR_COLOR)
    fb = (fresh.buffer(rec), fresh.buffer(nbytes=4 * n), fresh.buffer(nbytes=4 * n))
    fsb = fresh.record_stats(n)
    fresh.set_record_stats(fsb, n)
    sorted_frame(gs4d, fresh, fb, n, staged_cases.T1)
    want = fresh.read_record_stats(fsb, n)
    fresh.close()
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    bufs = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    sb = ctx.record_stats(n)
    for _ in range(2 * ctx.stats()["lanes"] + 8):
        sorted_frame(gs4d, ctx, bufs, n, staged_cases.T0)
    ctx.finish()
    s0 = ctx.stats()
    dst, idx = ctx.buffer(np.full(n * 96, SENTINEL, np.uint8)), ctx.buffer(np.full(n * 4, SENTINEL, np.uint8))
    ctx.set_record_stats(sb, n)
    sorted_frame(gs4d, ctx, bufs, n, staged_cases.T1)
    count = ctx.compact_records(sb, n, src=bufs[0], dst=dst, kept_index=idx, **PRUNE)          # no read-back in between
    s1 = ctx.stats()
    if draw_path == "auto":
        assert s0["staged_draws"] > 0 and s0["reruns"] == 0, s0
        assert s1["reruns"] == s0["reruns"] + 1 and s1["staged_misses"] == s0["staged_misses"] + 1, (s0, s1)      # the re-run happened, inside the call
    kept_idx = check_against_table(ctx, want, rec, dst, idx, count)
    assert 0 < kept_idx.size < n
    assert np.array_equal(table_bits(ctx.read_record_stats(sb, n)), table_bits(want))
    ctx.close()


def test_lanes_order_themselves_around_a_compaction(gs4d):
    rec = sc.records(gs4d, W5, H5, *layered_params())
    d = Direct(gs4d, W5, H5, rec)
    c = d.ctx
    d.frame()
    old = c.read_record_stats(d.sb, d.n)
    dst, idx = d.outputs()
    d.frame()                                                                  # (the table now holds two frames)
    count = c.compact_records(d.sb, d.n, src=d.db, dst=dst, kept_index=idx, min_pixels=2 * int(old["pixels"].max()))
    c.subdata(d.sb, np.zeros(d.n, gs4d.Context.RECORD_STAT))                   # a host write waits for the reader
    d.frame()
    two = table_bits(old).copy()
    two["pixels"] *= 2
    two["wsum"] *= 2
    top = check_against_table(c, two, rec, dst, idx, count, rule=(2 * int(old["pixels"].max()), 0, 0))
    assert top.size >= 1                                                       # zeros would have kept nothing
    assert np.array_equal(table_bits(c.read_record_stats(d.sb, d.n)), table_bits(old))      # ... and the draw after the upload counted from zero
    # the dst of one call as the src of a second one on the next frame lane, rule {0, 0, 0, 0}: unchanged
    count1 = c.compact_records(d.sb, d.n, src=d.db, dst=dst, kept_index=idx, **PRUNE)           # on the lane of the last draw
    kept = int(cc.keeps(table_bits(old), PRUNE_RULE).sum())
    c.clear()                                                                  # the next frame: the next lane (where there is more than one)
    dst2, idx2 = d.outputs()
    count2 = c.compact_records(d.sb, kept, src=dst, dst=dst2, kept_index=idx2, min_pixels=0)
    assert c.read_compact_count(count2) == (kept, kept)
    first = check_against_table(c, old, rec, dst, idx, count1)
    assert first.size == kept and 0 < kept < d.n
    assert np.array_equal(c.read(dst2, np.uint8, kept * 96), c.read(dst, np.uint8, kept * 96))
    assert np.array_equal(c.read(idx2, np.uint32, kept), np.arange(kept, dtype=np.uint32))
    c.close()


@pytest.mark.parametrize("frames_unread", [0, 1])
def test_a_draw_on_the_next_lane_waits_for_the_compaction(gs4d, frames_unread):
    """The continuing-path use: statistics stay on, compact the large table, then clear and draw on the next frame lane at once.  The draw adds to
    the table the compaction's two kernels are still reading; the result must be that of the table as it stood at the call.  The first rows of
    the table belong to the drawn records and the rule's min_pixels sits one above their largest count, so the draw that follows pushes rows over
    the threshold; the rest is the p50 pattern.  frames_unread = 1: one more frame before the call that nobody read back (the call settles it)."""
    rec = sc.records(gs4d, W5, H5, *layered_params())
    m, n = rec.shape[0], cc.LARGE
    c = gs4d.Context(W5, H5)
    c.set_clear_color(gs4d.CLEAR_COLOR)
    view, proj = sc.mats(gs4d, W5, H5)
    c.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
    c.set_mode(gs4d.MODE_4D_DIRECT)
    db = c.buffer(rec)
    c.bind(1, db)
    mask = cc.pattern_mask("p50", n)
    t0 = np.zeros(n, cc.STAT)
    t0["wmax"] = cc.BITS_1_255
    t0["pixels"][mask] = 1 << 20
    t0["wmax"][~mask & (np.arange(n) % 2 == 1)] = cc.BITS_1_255 - 1      # the dropped rows fail on pixels (0) or on wmax, by one
    t0["pixels"][~mask & (np.arange(n) % 2 == 1)] = 1 << 20
    t0[:m] = np.zeros(m, cc.STAT)
    sb, src = c.buffer(t0), c.buffer(records(n, 96))
    dst, idx = c.buffer(np.full(n * 96, SENTINEL, np.uint8)), c.buffer(np.full(n * 4, SENTINEL, np.uint8))
    c.set_record_stats(sb, n)

    def frame():
        c.clear()
        c.draw_instanced(m)

    frame()
    t1 = table_bits(c.read_record_stats(sb, n))
    table = t1.copy()
    for _ in range(frames_unread):                                             # the statistics are deterministic: every frame adds what the first added
        frame()
        table["pixels"][:m] += t1["pixels"][:m]
        table["wsum"][:m] += t1["wsum"][:m]
    rule = (int(table["pixels"][:m].max()) + 1, cc.BITS_1_255, 0)
    count = c.compact_records(sb, n, src=src, dst=dst, kept_index=idx, **rule_kw(rule))
    frame()                                                                    # the next lane, no read-back in between
    after = table_bits(c.read_record_stats(sb, n))
    want_d, want_i, kept, written = cc.reference(table, rule, records(n, 96), 96, n, n)
    assert c.read_compact_count(count) == (kept, written) and kept == int(mask[m:].sum())
    assert np.array_equal(c.read(idx, np.uint32, kept), want_i)
    assert np.array_equal(c.read(dst, np.uint8, kept * 96).reshape(kept, 96), want_d)
    lanes = c.stats()["lanes"]
    c.close()
    assert np.array_equal(after["pixels"][:m], table["pixels"][:m] + t1["pixels"][:m]) and np.array_equal(after[m:], t0[m:])      # the draw did add, to its rows only
    assert int(cc.keeps(after, rule).sum()) > kept and lanes >= 1              # ... and pushed rows over the threshold: a compaction that saw them would differ


# ---- 7. the pruned set draws the same picture ---------------------------------------------------------------------------------------------------------
W7 = H7 = 65                                              # the image's centre is the centre of pixel (32, 32)


@functools.lru_cache(maxsize=1)
def four_groups(gs4d):
    """(records, group of every record): 0 visible — layers of alpha <= 0.9; 1 hidden — specks on the centre pixel behind a record of alpha 1
    centred there (cg = 1, al = 1: T reaches exactly 0); 2 off-screen; 3 zero alpha; 4 dead at uTime = 0 (mu_t = 50, a lifetime of 0.01).
    Depths: the hidden ones farthest, the opaque one nearest, so that the depth sort and the instance order agree on who is behind it."""
    rng = np.random.default_rng(cc.seed("compact/four_groups"))
    nv, nh, no, nz, nd = 150, 6, 40, 30, 30
    vis = (rng.uniform(1.0, W7 - 1.0, nv), rng.uniform(1.0, H7 - 1.0, nv), rng.uniform(-3.0, 6.0, nv), np.where(rng.uniform(size=nv) < 0.4, sc.S_LARGE, sc.S_SMALL),
           np.concatenate([rng.uniform(0.0, 1.0, (nv, 3)), rng.uniform(0.05, 0.9, (nv, 1))], 1))
    hid = (np.full(nh, 32.5), np.full(nh, 32.5), np.linspace(-7.0, -5.0, nh), np.full(nh, 0.05), np.concatenate([rng.uniform(0.0, 1.0, (nh, 3)), np.full((nh, 1), 0.8)], 1))
    opaque = (np.array([32.5]), np.array([32.5]), np.array([9.0]), np.array([sc.S_SMALL]), np.array([[0.9, 0.8, 0.1, 1.0]]))
    off = (rng.uniform(2.0 * W7, 3.0 * W7, no), rng.uniform(-2.0 * H7, -H7, no), rng.uniform(-3.0, 6.0, no), np.full(no, sc.S_SMALL),
           np.concatenate([rng.uniform(0.0, 1.0, (no, 3)), np.full((no, 1), 0.7)], 1))
    zero = (rng.uniform(1.0, W7 - 1.0, nz), rng.uniform(1.0, H7 - 1.0, nz), rng.uniform(-3.0, 6.0, nz), np.full(nz, sc.S_LARGE), np.concatenate([rng.uniform(0.0, 1.0, (nz, 3)), np.zeros((nz, 1))], 1))
    parts = [sc.records(gs4d, W7, H7, *g) for g in (hid, vis, off, zero)]
    pos, q, scale = sc.world(gs4d, W7, H7, rng.uniform(1.0, W7 - 1.0, nd), rng.uniform(1.0, H7 - 1.0, nd), rng.uniform(-3.0, 6.0, nd), np.full(nd, sc.S_LARGE))
    dead = gs4d.build_records_4d(np.concatenate([pos, np.full((nd, 1), 50.0, np.float32)], 1), q, scale, np.full(nd, 0.01), np.full(nd, 0.5), np.zeros((nd, 3)),
                                 np.concatenate([rng.uniform(0.0, 1.0, (nd, 3)), np.full((nd, 1), 0.9)], 1))
    parts += [dead, sc.records(gs4d, W7, H7, *opaque)]
    group = np.concatenate([np.full(nh, 1), np.full(nv, 0), np.full(no, 2), np.full(nz, 3), np.full(nd, 4), np.full(1, 0)])
    # the visible records come in an interleaved order so that pruning closes gaps everywhere: hidden first, the opaque one last
    rec = np.concatenate(parts)
    mid = np.arange(nh, rec.shape[0] - 1)
    perm = np.concatenate([np.arange(nh), rng.permutation(mid), [rec.shape[0] - 1]])
    rec, group = np.ascontiguousarray(rec[perm]), group[perm]
    rec.setflags(write=False)
    return rec, group


@pytest.mark.parametrize("mode", ["direct", "sorted"])
def test_the_pruned_set_draws_the_same_picture(gs4d, mode):
    rec, group = four_groups(gs4d)
    n = rec.shape[0]
    c = gs4d.Context(W7, H7)
    c.set_clear_color(gs4d.CLEAR_COLOR)
    view, proj = sc.mats(gs4d, W7, H7)
    c.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
    db, sb = c.buffer(rec), c.record_stats(n)
    kb, ib = c.buffer(nbytes=4 * n), c.buffer(nbytes=4 * n)

    def frame(data, count):
        c.clear()
        if mode == "sorted":
            c.keygen(data, 0.0, sc.CAM[0], kb, ib, count)
            c.sort_pairs(kb, ib, count)
            c.set_mode(gs4d.MODE_4D_SORTED)
            c.bind(1, ib)
            c.bind(2, data)
        else:
            c.set_mode(gs4d.MODE_4D_DIRECT)
            c.bind(1, data)
        c.draw_instanced(count)

    c.set_record_stats(sb, n)
    frame(db, n)
    full = c.read_pixels()
    order = c.read(ib, np.uint32, n) if mode == "sorted" else None
    c.set_record_stats(None)
    # the premises, from the numpy restatement of this very draw: no weight underflows, the groups are what they claim
    ref = sc.restate(id_cases.from_device(c.debug_projected(n)), order, W7, H7)
    T = ref["T"]
    assert (T == 0).sum() == 1 and T[32, 32] == 0.0 and T[T > 0].min() > 2.0 ** -60 and not ref["subnormal"]
    assert (ref["stats"]["pixels"][group == 0] > 0).all() and not ref["stats"]["pixels"][group != 0].any()
    table = c.read_record_stats(sb, n)
    assert np.array_equal(table["pixels"] > 0, group == 0)
    dst, kidx, kept = c.prune(sb, n, db)
    assert kept == int((group == 0).sum()) and kept < n
    index = c.read(kidx, np.uint32, kept)
    assert np.array_equal(index, np.flatnonzero(group == 0))
    assert np.array_equal(c.read(dst, np.float32, kept * 24).reshape(kept, 24).view(np.uint32), rec[index].view(np.uint32))
    frame(dst, kept)
    pruned = c.read_pixels()
    assert np.array_equal(pruned.view(np.uint32), full.view(np.uint32)), f"{int((pruned.view(np.uint32) != full.view(np.uint32)).any(-1).sum())} pixels differ"
    shown = int((np.abs(full - np.array(gs4d.CLEAR_COLOR, np.float32)).max(-1) > 1.0 / 255.0).sum())
    assert shown > kept, shown                                                 # not an empty frame: more pixels than visible records show something
    # picks of the pruned frame map back to the original records through kept_index
    c.set_id_outputs(True)
    frame(db, n)
    rid_full, _, _ = c.read_ids()
    frame(dst, kept)
    rid_pruned, _, _ = c.read_ids()
    c.close()
    seen = rid_full != id_cases.ID_NONE
    assert seen.sum() > kept and np.array_equal(rid_pruned != id_cases.ID_NONE, seen)
    assert np.array_equal(index[rid_pruned[seen]], rid_full[seen])
