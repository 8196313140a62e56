"""GPU: the record-set calls at the sizes where their code takes a path that no smaller test reaches ("Sizes under test").

1. gs4d_compact_records and gs4d_compact_time_window past one round of the single-workgroup scan (k_compact_scan: 1024 tile counts per round).
2. gs4d_merge_records past one round of its copy of that scan (k_merge_scan).
3. gs4d_spatial_order past the grid of its box kernel (k_order_box: 1024 workgroups of 256 threads, a grid stride beyond).
4. gs4d_gather_records, gs4d_spatial_order and both compactions over ONE buffer of more than 4 GiB at the largest stride (1024 bytes): the
   byte offset of slot 4 194 304 is 2^32.

Every comparison is exact: uint32 words or bytes against numpy (np.flatnonzero, src[index], reorder_cases.order) or, for the merge, against the
host definition.  Every case asserts on the CPU, before the device call, that its input has the property it is named for (compact_cases.
assert_round_pattern, merge_cases.assert_round_labels, reorder_cases.assert_stride_positions): tests/test_scale_cases.py runs those without a device.
Outputs are sentinel-filled, hold a few bytes more than their slots and are followed by a guard buffer; all three are checked.

Where the line is: only calls whose records may have a stride of 1024 bytes can pass 4 GiB with a few million records.  The calls on 96-byte records
(merge, transform, pose, slice, the grid queries) would need 44.7 M records and 4.3 GB of real records for it and are not tested there; neither
are gs4d_shade_sh and gs4d_nearest_neighbours with rows of 1024 bytes, nor the splits of a launch at 2^30 records (RECORD_MAX_GRID: the loop
itself is driven on the CPU by tests/record_tile_check.cpp).
All calls go through the Python binding over the C ABI."""
import numpy as np
import pytest

import compact_cases as cc
import merge_cases as mc
import reorder_cases as rc
import time_window_cases as tw

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096
T, R = cc.COMPACT_TILE, cc.ROUND
u32 = np.uint32
WINDOW = (24.0, 26.0)


def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD, offset=0):
    return bool((ctx.read(buf, np.uint8, nbytes, offset=offset) == SENTINEL).all())


# ---- 1. compaction past one round of the scan ------------------------------------------------------------------------------------------------------
class Compaction:
    """one context with a table of n rows of either kind and, where records are wanted, n records of 16 bytes"""

    def __init__(self, gs4d, kind, n):
        self.kind, self.n = kind, n
        self.ctx = gs4d.Context(64, 64)
        self.row = 16 if kind == "stats" else 8
        self.table = self.ctx.buffer(nbytes=n * self.row)
        self.count = fill(self.ctx, 8 + 8)
        self.src = self.src_host = None

    def upload(self, mask):
        self.ctx.subdata(self.table, cc.round_table(mask) if self.kind == "stats" else tw.mask_table(mask))

    def records(self):
        if self.src is None:
            self.src_host = cc.records(self.n, 16)
            self.src = self.ctx.buffer(self.src_host)

    def call(self, **kw):
        if self.kind == "stats":
            self.ctx.compact_records(self.table, self.n, count=self.count, min_pixels=1, **kw)
        else:
            self.ctx.compact_time_window(self.table, self.n, *WINDOW, count=self.count, **kw)

    def run(self, mask, what, with_dst=False, cap=None):
        """one call into sentinel-filled outputs against np.flatnonzero(mask).  cap: dst holds that many slots (kept_index always holds every
        record), None: room for every kept row.  Both outputs hold a few bytes more than whole slots."""
        c, n = self.ctx, self.n
        want = np.flatnonzero(mask).astype(u32)
        kept = int(want.size)
        written = kept if cap is None else min(kept, cap)
        ibytes = 4 * (kept + 2) if cap is None else 4 * n + 8
        idx, gi = fill(c, ibytes), fill(c, GUARD)
        dst = gd = None
        kw = {}
        if with_dst or cap is not None:
            self.records()
            dbytes = 16 * (written if cap is not None else kept + 2) + 12
            dst, gd = fill(c, dbytes), fill(c, GUARD)
            kw = dict(src=self.src, stride=16, dst=dst)
        self.call(kept_index=idx, **kw)
        got_count = c.read_compact_count(self.count)
        print(f"{what}: kept {got_count[0]} (numpy {kept}), written {got_count[1]} (numpy {written})")
        assert got_count == (kept, written), f"{what}: count {got_count}, numpy has {(kept, written)}"
        assert untouched(c, self.count, 8, offset=8), f"{what}: bytes behind the count changed"
        got = c.read(idx, np.uint8, max(16, ibytes))
        bad = got[:4 * written].view(u32) != want[:written]
        assert not bad.any(), f"{what}: kept_index differs in {int(bad.sum())} of {written} slots, first at slot {int(np.argmax(bad))}"
        assert (got[4 * written:] == SENTINEL).all() and untouched(c, gi), f"{what}: bytes of kept_index beyond the written slots changed"
        if dst:
            got = c.read(dst, np.uint8, max(16, dbytes))
            assert np.array_equal(got[:16 * written].view(u32).reshape(written, 4), self.src_host[want[:written]]), f"{what}: dst differs from the gathered rows"
            assert (got[16 * written:] == SENTINEL).all() and untouched(c, gd), f"{what}: bytes of dst beyond the written slots changed"
        for b in (idx, gi, dst, gd):
            if b:
                c.delete(b)
        return kept

    def close(self):
        self.ctx.finish()                                     # reports device-side check failures
        self.ctx.close()


@pytest.mark.parametrize("kind", ["stats", "spans"])
@pytest.mark.parametrize("n", cc.ROUND_SIZES, ids=["R", "R+1", "R+T+1", "2R+1"])
def test_compaction_past_one_round_of_the_scan(gs4d, n, kind):
    """k_compact_scan (csrc/compact.hip), the loop `for (base = 0; base < ntiles; base += 1024u)`: `const uint32_t carry = carry_s;` in front of the
    first barrier, `if (threadIdx.x == 1023u) carry_s = before + incl;` between the two, `const uint32_t kept = carry_s;` behind the loop.
    sparse: every tile base of round 2 and 3 is the carry plus a prefix — a lost carry restarts kept_index's slots at 0 in round 2 (the rows of
    round 1 are overwritten, the tail stays sentinel), a carry read behind the write counts thread 1023's total twice; seam: the base of the first
    tile of round 2 is the carry alone; first_round: nothing is kept behind round 1, so the count is the carry as the last round left it;
    last_round: the carry is 0 until the last round.  At n = R there is no second round: the count is read from the carry of a full round.
    For one pattern per size the 16-byte records go along (dst); both instantiations (statistics rows under min_pixels, time spans under a
    window) run the same kernels over rows of 16 and 8 bytes."""
    t = Compaction(gs4d, kind, n)
    for k, pattern in enumerate(cc.ROUND_PATTERNS):
        mask = cc.round_mask(pattern, n)
        cc.assert_round_pattern(pattern, n, mask)
        t.upload(mask)
        kept = t.run(mask, f"{kind}, n = {n}, {pattern}", with_dst=(k == cc.ROUND_SIZES.index(n)))
        assert kept == int(cc.round_sums(mask).sum()) > 0
    t.close()


@pytest.mark.parametrize("kind", ["stats", "spans"])
def test_a_capacity_between_the_last_base_of_round_1_and_the_first_of_round_2(gs4d, kind):
    """k_compact_scatter (csrc/compact.hip): `if (base >= cap) return;` and `room = cap - base` with the bases that k_compact_scan's second round
    wrote.  dst holds more slots than the last tile of round 1 begins at and fewer than the first tile of round 2 does: the last tile of round 1
    is cut, every tile of round 2 leaves at once.  A base of round 2 without the carry would be below the capacity: rows of round 2 would be
    written over those of round 1 and `written` slots would no longer be np.flatnonzero's first ones."""
    n = R + T + 1
    mask = cc.round_mask("sparse", n)
    cc.assert_round_pattern("sparse", n, mask)
    bases = np.concatenate([[0], np.cumsum(cc.tile_counts(mask))])
    cap = int(bases[cc.SCAN_THREADS - 1] + bases[cc.SCAN_THREADS]) // 2
    assert bases[cc.SCAN_THREADS - 1] < cap < bases[cc.SCAN_THREADS] < bases[-1], "the capacity cuts the last tile of round 1"
    t = Compaction(gs4d, kind, n)
    t.upload(mask)
    assert t.run(mask, f"{kind}, capacity {cap}", cap=cap) == int(bases[-1]) > cap
    t.close()


# ---- 2. merge past one round of the scan -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def round_set(gs4d):
    """one context holding merge_cases.ROUND_N records, uploaded once for the tests of this section"""
    rec = mc.round_records(gs4d)
    rec.setflags(write=False)
    ctx = gs4d.Context(64, 64)
    guard0 = fill(ctx, GUARD)
    data = ctx.buffer(rec)
    guard1 = fill(ctx, GUARD)
    yield ctx, data, rec
    assert untouched(ctx, guard0) and untouched(ctx, guard1), "a guard buffer beside the records changed"
    ctx.finish()                                              # reports device-side check failures
    ctx.close()


def merge_call(gs4d, round_set, case, cut=0):
    """one gs4d_merge_records call over the round set against merge_records_host; cut: dst and groups hold that many slots fewer than there are
    groups (0: three more)."""
    ctx, data, rec = round_set
    n = mc.ROUND_N
    labels, stats, rule = mc.round_labels(case, gs4d)
    member = mc.members_of(rec, labels, None if stats is None else mc.passes(stats))
    groups = mc.assert_round_labels(case, labels, member)
    host = gs4d.merge_records_host(rec, labels, 0.5, stats, **rule)
    assert int(host[3]["groups"]) == groups and int(host[3]["members"]) == int(member.sum())
    cap = groups - cut if cut else groups + 3
    lab = ctx.buffer(labels)
    table = ctx.buffer(stats) if stats is not None else None
    dst, g0 = fill(ctx, cap * 96 + 32), fill(ctx, GUARD)
    rows, g1 = fill(ctx, cap * 16 + 8), fill(ctx, GUARD)
    mg, g2 = fill(ctx, 4 * n + 16), fill(ctx, GUARD)
    count = fill(ctx, 32)
    ctx.merge_records(data, n, lab, 0.5, stats=table, dst=dst, groups=rows, member_group=mg, count=count, **rule)
    c = ctx.read_merge_count(count)
    what = f"{case}, capacity {cap}"
    print(f"{what}: count {c}, the host definition has {host[3]}")
    w = min(groups, cap)
    raw_d, raw_r, raw_m = ctx.read(dst, np.uint8, cap * 96 + 32), ctx.read(rows, np.uint8, cap * 16 + 8), ctx.read(mg, np.uint8, 4 * n + 16)
    assert (raw_d[96 * w:] == SENTINEL).all() and (raw_r[16 * w:] == SENTINEL).all() and (raw_m[4 * n:] == SENTINEL).all(), f"{what}: bytes at or above the capacity changed"
    assert untouched(ctx, count, 16, offset=16) and untouched(ctx, g0) and untouched(ctx, g1) and untouched(ctx, g2), f"{what}: a guard changed"
    got = (raw_d[:96 * w].view(np.float32).reshape(w, 24), raw_r[:16 * w].view(gs4d.MERGE_GROUP), raw_m[:4 * n].view(u32), c)
    mc.assert_device_equals_host(what, got, host, written=cap)
    assert mc.same_bytes(ctx, lab, labels) and (stats is None or mc.same_bytes(ctx, table, stats)), f"{what}: an input changed"
    for b in (lab, table, dst, g0, rows, g1, mg, g2, count):
        if b is not None:
            ctx.delete(b)
    return host


@pytest.mark.parametrize("case", mc.ROUND_CASES)
def test_merge_past_one_round_of_the_scan(gs4d, round_set, case):
    """k_merge_scan (csrc/merge.hip), the same loop as k_compact_scan's: `const uint32_t carry = carry_s;`, `if (threadIdx.x == 1023u) carry_s =
    before + incl;` and, behind the loop, `const uint32_t groups = carry_s`.  1026 tiles of sorted keys, two of them in round 2.
    heads_in_round_2 / rule: the numbers of the groups whose heads lie in tiles 1024 and 1025 are the carry plus a prefix — without it
    k_merge_heads writes their starts over start[0 ..] and member_group names the first groups again: dst, groups and member_group all differ;
    no_heads_in_round_2: a suffix of non-members longer than two tiles — the last tile of round 1 and both tiles of round 2 count 0, and `groups`
    is the carry that round 1 left.
    The yardstick is merge_records_host, every word: merge_cases.by_the_text loops over the groups in Python and would take minutes here, and
    tests/test_merge_host.py already ties the host definition to the text."""
    host = merge_call(gs4d, round_set, case)
    assert int(host[3]["groups"]) > 250_000 and int(host[3]["left_out"]) == {"heads_in_round_2": 0, "rule": 1000, "no_heads_in_round_2": 2 * mc.MERGE_TILE + 501}[case]


def test_merge_past_one_round_with_a_capacity_just_below_the_group_count(gs4d, round_set):
    """k_merge_groups (csrc/merge.hip): `const bool live = g < written;` with `written = groups < cap ? groups : cap` from the state block that
    k_merge_scan wrote behind its second round — the last five groups, whose heads lie in round 2, are counted and not written: the slots are
    sentinel, count.groups is the full number."""
    merge_call(gs4d, round_set, "heads_in_round_2", cut=5)


# ---- 3. the grid stride of the ordering box --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trip", rc.STRIDE_TRIPS)
def test_the_box_kernel_strides_past_its_grid(gs4d, trip):
    """k_order_box (csrc/reorder.hip): `for (uint64_t i = blockIdx.x * RO_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RO_THREADS)` with
    gridDim.x = ORDER_BOX_GROUPS = 1024.  n = 1024 * 256 + 257: the first workgroup's threads and one thread of the second take a second trip.
    second: all six extremes of the box are held by records of the second trip (lanes 0 and 63 of a wave, thread 255, the second workgroup's
    thread 0) — a thread that stops after one trip, or a stride of the wrong width, leaves a smaller box and nearly every key changes; first: the
    mirror — a second trip that read other records than its own (a wrong stride lands on the far extremes' neighbours or past the end) would
    widen nothing, but the three unplaced records and the eleven ties of the second trip must still come out last and in index order."""
    pos = rc.stride_positions(trip)
    rc.assert_stride_positions(trip, pos)
    n = rc.STRIDE_SIZE
    ctx = gs4d.Context(64, 64)
    g0 = fill(ctx, GUARD)
    rec = rc.records_with_positions(pos, 16, 0)
    src = ctx.buffer(rec)
    g1 = fill(ctx, GUARD)
    oi = fill(ctx, 4 * n + 64)
    g2 = fill(ctx, GUARD)
    ctx.spatial_order(src, n, stride=16, pos_offset=0, order_index=oi)
    got = ctx.read(oi, np.uint8, 4 * n + 64)
    want = rc.order(pos)
    bad = got[:4 * n].view(u32) != want
    print(f"{trip}: {int(bad.sum())} of {n} entries differ from the restatement")
    assert not bad.any(), f"{trip}: order_index differs from the restatement in {int(bad.sum())} of {n} entries"
    assert (got[4 * n:] == SENTINEL).all() and untouched(ctx, g0) and untouched(ctx, g1) and untouched(ctx, g2), f"{trip}: bytes outside order_index changed"
    assert np.array_equal(ctx.read(src, u32, 4 * n).reshape(n, 4), rec), f"{trip}: src changed"
    unplaced = np.flatnonzero(~rc.placed(pos))
    assert unplaced.size == 3 and np.array_equal(want[n - 3:], unplaced), "the unplaced records come last, in their original order"
    ties = np.flatnonzero(rc.keys(pos) == rc.keys(pos)[5])
    assert ties.size >= 12 and np.array_equal(np.sort(want[np.isin(want, ties)]), want[np.isin(want, ties)]), "equal keys keep their order"
    ctx.finish()
    ctx.close()


# ---- 4. byte offsets past 4 GiB --------------------------------------------------------------------------------------------------------------------
BIG_STRIDE, BIG_POS = 1024, 1008
FIRST_PAST = (1 << 32) // BIG_STRIDE                          # slot 4 194 304 begins at byte 2^32
BIG_N = FIRST_PAST + T + 1
POOL = 257


def big_pool():
    """257 distinct rows of 1024 bytes with a position at byte 1008; rows 255 and 256 hold the two corners of the box"""
    pos = rc.uniform(POOL, "big_pool")
    pos[POOL - 2], pos[POOL - 1] = np.float32(-100.0), np.float32(100.0)
    return rc.records_with_positions(pos, BIG_STRIDE, BIG_POS), pos


def test_byte_offsets_past_4_gib(gs4d):
    """One buffer `big` of BIG_N = 4 194 304 + 2049 slots of 1024 bytes, filled on the device, then read by every call that takes a stride of 1024.
    A byte offset formed in 32 bits in any of these lines — by a product in bytes, as in 2., or by an address that keeps only 32 bits of a
    piece index times 16 — wraps at slot 4 194 304 and lands exactly 4 GiB in front of where it should:
    1. k_gather_records as the writer: `uint4* const out = dst + slot0 * q;` and `out[j] = v[u]` (csrc/reorder.hip) — the slots from 4 194 304
       on would be written over slots 0 .., and the read-back of slots 0 .. 2 and 4 194 303 .. 4 194 305 and of the last 2049 would not hold
       their pool rows;
    2. record_pos: `src + i * stride + pos_offset` in k_order_box and k_order_keys, a product in bytes — the two corners of the box are patched
       in at slots past byte 2^32 only, so a wrapped address never sees them: another box, other keys, another order;
    3. k_compact_scatter: `src[(tile0 + list[rec]) * q + piece]` (csrc/compact.hip) — the rows kept around slot 4 194 304 and in the last tile
       would be copies of slots 0 .. instead;
    4. k_gather_records as the reader: `src[(uint64_t)(rec[u] < nsrc ? rec[u] : 0u) * q + piece[u]]` — likewise.
    (The piece indices of 1., 3. and 4. count 16 bytes: as numbers they stay below 2^32 here, what can wrap is the address made from them.)
    Each step is checked before the next one runs.  Skips only when the library cannot allocate the 4.3 GB."""
    ctx = gs4d.Context(64, 64)
    n, stride, q = BIG_N, BIG_STRIDE, BIG_STRIDE // 4
    assert (n - 1) * stride > 1 << 32 and FIRST_PAST * stride == 1 << 32
    try:
        big = ctx.buffer(nbytes=n * stride)
    except gs4d.Gs4dError as e:
        ctx.close()
        pytest.skip(f"no buffer of {n * stride} bytes: {e}")
    guard = fill(ctx, GUARD)
    pool, pool_pos = big_pool()
    rng = np.random.default_rng(cc.seed("scale/big"))
    index = rng.integers(0, POOL - 2, n).astype(u32)          # never the two corner rows
    # the first 3 slots, those around byte 2^32 and the last tile and one (which begins AT byte 2^32 by the choice of n)
    probes = np.unique(np.concatenate([np.arange(3), np.arange(FIRST_PAST - 1, FIRST_PAST + 2), np.arange(n - (T + 1), n)]))
    assert (index < POOL - 2).all() and probes.size == 3 + 1 + T + 1

    def slots(first, count):
        return ctx.read(big, u32, count * q, offset=first * stride).reshape(count, q)

    def check_big(what):
        for first, count in ((0, 3), (FIRST_PAST - 1, 3), (n - (T + 1), T + 1)):
            got = slots(first, count)
            bad = (got != pool[index[first:first + count]]).any(1)
            assert not bad.any(), f"{what}: {int(bad.sum())} of the {count} slots from {first} do not hold their pool row, first slot {first + int(np.argmax(bad))}"
        assert untouched(ctx, guard), f"{what}: the buffer behind big changed"

    # ---- 1. the gather as a writer
    ib, pb = ctx.buffer(index), ctx.buffer(pool)
    ctx.gather_records(ib, n, pb, POOL, stride=stride, dst=big)
    check_big("gather into big")
    assert np.array_equal(ctx.read(pb, u32, POOL * q).reshape(POOL, q), pool)
    ctx.delete(pb)

    # ---- 2. the spatial order over it: the corners of the box live past byte 2^32 only
    for slot, row in ((FIRST_PAST + 7, POOL - 2), (n - 2, POOL - 1)):
        index[slot] = row
        ctx.subdata(big, pool[row], offset=slot * stride)
    check_big("the two patched slots")
    pos = pool_pos[index]
    lo, hi = pos.argmin(0), pos.argmax(0)
    assert (lo == FIRST_PAST + 7).all() and (hi == n - 2).all() and (pos[:FIRST_PAST].min() > -4.0) and (pos[:FIRST_PAST].max() < 6.0)
    oi, go = fill(ctx, 4 * n + 64), fill(ctx, GUARD)
    ctx.spatial_order(big, n, stride=stride, pos_offset=BIG_POS, order_index=oi)
    got = ctx.read(oi, np.uint8, 4 * n + 64)
    bad = got[:4 * n].view(u32) != rc.order(pos)
    print(f"spatial order over big: {int(bad.sum())} of {n} entries differ from the restatement")
    assert not bad.any(), f"order_index differs from the restatement in {int(bad.sum())} of {n} entries"
    assert (got[4 * n:] == SENTINEL).all() and untouched(ctx, go), "bytes behind order_index changed"
    ctx.delete(oi)
    ctx.delete(go)

    # ---- 3. both compactions with big as src
    mask = np.zeros(n, bool)
    mask[probes] = True
    count = fill(ctx, 16)
    for kind, table in (("stats", cc.round_table(mask)), ("spans", tw.mask_table(mask))):
        tb = ctx.buffer(table)
        dst, gd = fill(ctx, (probes.size + 2) * stride + 16), fill(ctx, GUARD)
        idx, gi = fill(ctx, 4 * (probes.size + 2)), fill(ctx, GUARD)
        if kind == "stats":
            ctx.compact_records(tb, n, src=big, stride=stride, dst=dst, kept_index=idx, count=count, min_pixels=1)
        else:
            ctx.compact_time_window(tb, n, *WINDOW, src=big, stride=stride, dst=dst, kept_index=idx, count=count)
        assert ctx.read_compact_count(count) == (probes.size, probes.size), kind
        got_i = ctx.read(idx, np.uint8, 4 * (probes.size + 2))
        assert np.array_equal(got_i[:4 * probes.size].view(u32), probes.astype(u32)) and (got_i[4 * probes.size:] == SENTINEL).all(), f"{kind}: kept_index"
        got = ctx.read(dst, np.uint8, (probes.size + 2) * stride + 16)
        bad = (got[:probes.size * stride].view(u32).reshape(probes.size, q) != pool[index[probes]]).any(1)
        assert not bad.any(), f"{kind}: {int(bad.sum())} kept rows are not their records, first the row of slot {int(probes[np.argmax(bad)])}"
        assert (got[probes.size * stride:] == SENTINEL).all() and untouched(ctx, gd) and untouched(ctx, gi) and untouched(ctx, count, 8, offset=8), f"{kind}: bytes outside the outputs changed"
        for b in (tb, dst, gd, idx, gi):
            ctx.delete(b)

    # ---- 4. the gather as a reader: the same slots, and two entries that name no record
    pick = np.concatenate([probes[:5], [n], probes[5:], [0xFFFFFFFF]]).astype(u32)
    m = pick.size
    pk = ctx.buffer(pick)
    dst, gd = fill(ctx, m * stride + 16), fill(ctx, GUARD)
    ctx.gather_records(pk, m, big, n, stride=stride, dst=dst)
    got = ctx.read(dst, np.uint8, m * stride + 16)
    rows = got[:m * stride].view(u32).reshape(m, q)
    real = pick < n
    assert (~real).sum() == 2 and (rows[~real] == 0xA5A5A5A5).all(), "the slot of an entry >= nsrc changed"
    bad = (rows[real] != pool[index[pick[real]]]).any(1)
    assert not bad.any(), f"{int(bad.sum())} gathered rows are not their records, first the row of slot {int(pick[real][np.argmax(bad)])}"
    assert (got[m * stride:] == SENTINEL).all() and untouched(ctx, gd), "bytes behind dst changed"
    check_big("after the readers")                            # no reader wrote into big
    ctx.finish()                                              # reports device-side check failures
    ctx.close()
