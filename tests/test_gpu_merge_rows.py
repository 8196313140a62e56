"""GPU: gs4d_merge_rows and gs4d_copy_rows (include/gs4d.h) against merge_rows_host — every word as uint32, no exemption — at the
smallest shapes at which the kernels of csrc/merge_rows.hip can go wrong: group sizes around the eight lanes of a sub-group and one group of 3000
members (more than one pass of a lane, a run across a tile of the head kernels), widths on and either side of a 16-byte piece and of the chunk of
8 words, NaN in the padding, a prefilled dst, dst_first and a capacity that cuts, both weight forms, the shared lane scratch, and the forest that
carries its rows: build_lod with a table, lod_rows of a cut, and the degree-0 colour of a merged set against the merge of the shaded leaves."""
import numpy as np
import pytest

import merge_cases as mc
import merge_rows_cases as rc
import neighbour_cases as nc

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
PATTERN32 = 0xA5A5A5A5
SIZES = rc.GROUP_SIZES + (3000, 3, 1)                         # ascending value = ascending sorted slot: 3000 spans slot 2048, two heads behind it


def device_call(gs4d, ctx, tab, mg, width, rec=None, dst_first=0, capacity=None, what=""):
    """one gs4d_merge_rows call between guard buffers -> (dst uint32 [capacity, words] as the device left it, count tuple), after checking the
    bytes behind dst and count, the guards and the inputs"""
    n, words = tab.shape
    stride = 4 * words
    named = mg[mg != rc.ID_NONE]
    capacity = dst_first + (int(named.max()) + 1 if named.size else 0) + 2 if capacity is None else capacity
    guards = [mc.fill(ctx, mc.GUARD)]
    data = ctx.buffer(rec) if rec is not None else None
    group, rows = (ctx.buffer(mg), ctx.buffer(tab)) if n else (mc.fill(ctx, 16), mc.fill(ctx, 16))
    guards.append(mc.fill(ctx, mc.GUARD))
    dst = mc.fill(ctx, capacity * stride + 8)                 # (8 bytes behind the last row: less than a row of any stride)
    guards.append(mc.fill(ctx, mc.GUARD))
    count = mc.fill(ctx, 32)
    guards.append(mc.fill(ctx, mc.GUARD))
    assert ctx.merge_rows(group, n, rows, stride, width, data=data, dst=dst, dst_first=dst_first, count=count) == (dst, count)
    c = rc.count_tuple(ctx.read_merge_count(count))
    assert mc.untouched(ctx, count, 16, offset=16), f"{what}: bytes behind the count changed"
    assert mc.untouched(ctx, dst, 8, offset=capacity * stride), f"{what}: bytes behind dst changed"
    out = ctx.read(dst, u32, capacity * words).reshape(capacity, words) if capacity else np.zeros((0, words), u32)
    assert all(mc.untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
    if n:
        assert mc.same_bytes(ctx, group, mg) and mc.same_bytes(ctx, rows, tab) and (rec is None or mc.same_bytes(ctx, data, rec)), f"{what}: an input changed"
        assert rec is None or ctx.shadow_builds(data) == 0
    for b in guards + [group, rows, dst, count] + ([data] if data is not None else []):
        ctx.delete(b)
    return out, c


def host_call(gs4d, tab, mg, width, rec, dst_first, capacity):
    dst = np.full((capacity, tab.shape[1]), PATTERN32, u32)
    out, count = gs4d.merge_rows_host(tab, mg, records=rec, width=width, dst=dst, dst_first=dst_first)
    return out.view(u32).reshape(capacity, tab.shape[1]), rc.count_tuple(count)


def assert_same(what, got, want):
    assert got[1] == want[1], f"{what}: count {got[1]} against {want[1]}"
    diff = got[0] != want[0]
    assert not diff.any(), f"{what}: {int(diff.sum())} words of dst differ, first at (row, word) {tuple(np.argwhere(diff)[0])}"


# ---- 1. the reduction -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,stride", rc.SHAPES)
def test_group_sizes_widths_and_strides_in_both_weight_forms(gs4d, width, stride):
    ctx = gs4d.Context(64, 64)
    mg = rc.grouping(SIZES, step=2, seed=width, none=7)
    n = mg.size
    tab, rec = rc.table(n, width, stride, seed=width), rc.records(gs4d, n, seed=width)
    tab[np.flatnonzero(mg == 4)[3], width - 1] = np.inf         # a non-finite word inside width, a massless record: no members
    rec[np.flatnonzero(mg == 16)[1000], 7] = 0.0
    top = 2 * (len(SIZES) - 1)
    for call, (dst_first, capacity) in enumerate(((0, top + 3), (5, top + 9), (3, top))):      # the last: rows top + 3 - 4 .. past the capacity
        weighted = (call + width) % 2 == 0
        for form in ((weighted, not weighted) if call == 0 else (weighted,)):
            what = f"width {width}, stride {stride}, dst_first {dst_first}, capacity {capacity}, weighted {form}"
            want = host_call(gs4d, tab, mg, width, rec if form else None, dst_first, capacity)
            assert want[1][0] == len(SIZES) and want[1][2] == sum(SIZES) - (2 if form else 1)
            assert want[1][1] == (len(SIZES) if call < 2 else len(SIZES) - 2), what
            assert_same(what, device_call(gs4d, ctx, tab, mg, width, rec if form else None, dst_first, capacity, what), want)
            rows = [dst_first + 2 * j for j in range(len(SIZES)) if dst_first + 2 * j < capacity]
            other = np.setdiff1d(np.arange(capacity), rows)
            assert (want[0][other] == PATTERN32).all() and not (want[0][rows][:, width:] != 0).any()
    ctx.finish()
    ctx.close()


@pytest.mark.parametrize("n", (1, 255, 257, 2049))
def test_record_counts_around_the_tiles(gs4d, n):
    ctx = gs4d.Context(64, 64)
    for call, (width, stride) in enumerate(rc.CHUNK_SHAPES + ((48, 192),)):
        rng = np.random.default_rng(n + call)
        mg = rng.integers(0, max(1, n // 3), n).astype(u32) * u32(2)             # groups of about 3: heads in every tile
        if n > 2:
            mg[rng.integers(0, n, n // 10)] = rc.ID_NONE
        tab, rec = rc.table(n, width, stride, seed=n + call), rc.records(gs4d, n, seed=n)
        cap = 2 * max(1, n // 3) + 1
        for form in (True, False):
            what = f"n {n}, width {width}, weighted {form}"
            want = host_call(gs4d, tab, mg, width, rec if form else None, 1, cap)
            assert n < 2049 or want[1][0] > 600                                     # run heads in the second tile of 2048 sorted slots
            assert_same(what, device_call(gs4d, ctx, tab, mg, width, rec if form else None, 1, cap, what), want)
    # no record at all
    count = mc.fill(ctx, 32)
    empty, dst = mc.fill(ctx, 16), mc.fill(ctx, 64)
    ctx.merge_rows(empty, 0, ctx.buffer(nbytes=16), 16, 3, dst=dst, count=count)
    assert rc.count_tuple(ctx.read_merge_count(count)) == (0, 0, 0, 0) and mc.untouched(ctx, count, 16, offset=16) and mc.untouched(ctx, dst, 64)
    ctx.finish()
    ctx.close()


# ---- 2. scratch re-use ---------------------------------------------------------------------------------------------------------------------------
def test_the_scratch_is_shared_with_the_merge_and_the_grid_queries_at_other_sizes(gs4d):
    """a call, another user of the lane's neighbour scratch and pair_sort at another size (gs4d_merge_records, gs4d_count_neighbours), then the same
    call again, nothing read or finished between them: the second gives the first's bytes and the host's"""
    ctx = gs4d.Context(64, 64)
    other = nc.case("cube", 1025)
    odata, ostats = ctx.buffer(other.rec), ctx.record_stats(other.n)
    orec, olab = rc.records(gs4d, 700, seed=1), mc.mixed_labels(700, 1)
    mdata, mlab = ctx.buffer(orec), ctx.buffer(olab)
    width, stride = 27, 112
    for step, n in enumerate((4100, 9, 2049, 4100)):
        mg = np.random.default_rng(step).integers(0, max(1, n // 5), n).astype(u32)
        tab, rec = rc.table(n, width, stride, seed=step), rc.records(gs4d, n, seed=step)
        cap = max(1, n // 5)
        want = host_call(gs4d, tab, mg, width, rec, 0, cap)
        data, group, rows = ctx.buffer(rec), ctx.buffer(mg), ctx.buffer(tab)
        outs = [(mc.fill(ctx, cap * stride), mc.fill(ctx, 16)) for _ in range(2)]
        ctx.merge_rows(group, n, rows, stride, width, data=data, dst=outs[0][0], count=outs[0][1])
        if step % 2 == 0:
            mdst, mcount = ctx.merge_records(mdata, 700, mlab)
        else:
            ctx.subdata(ostats, nc.table("zero", other.n))
            ctx.count_neighbours(ostats, other.n, odata, other.r)
        ctx.merge_rows(group, n, rows, stride, width, data=data, dst=outs[1][0], count=outs[1][1])
        for k in (1, 0):
            got = ctx.read(outs[k][0], u32, cap * stride // 4).reshape(cap, -1), rc.count_tuple(ctx.read_merge_count(outs[k][1]))
            assert_same(f"step {step}, n {n}, call {k}", got, want)
        if step % 2 == 0:
            hout, _, _, hcount = gs4d.merge_records_host(orec, olab)
            g = int(hcount["groups"])
            assert int(ctx.read_merge_count(mcount)["groups"]) == g and np.array_equal(ctx.read(mdst, u32, 24 * g), mc.bits(hout[:g]).reshape(-1))
        for b in (data, group, rows, outs[0][0], outs[0][1], outs[1][0], outs[1][1]):
            ctx.delete(b)
    ctx.finish()
    ctx.close()


# ---- 3. gs4d_copy_rows and the refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 257))
@pytest.mark.parametrize("stride", (16, 208))
def test_copy_rows(gs4d, m, stride):
    ctx = gs4d.Context(64, 64)
    src_first, dst_first, total = 3, 7, m + 12
    a = np.random.default_rng(m + stride).integers(0, 256, (total, stride)).astype(np.uint8)
    a[:, :4] = np.array([np.nan], f32).view(np.uint8)           # NaN words travel as they are
    src, dst, guard = ctx.buffer(a), mc.fill(ctx, total * stride), mc.fill(ctx, mc.GUARD)
    assert ctx.copy_rows(src, m, stride, dst=dst, src_first=src_first, dst_first=dst_first) == dst
    want = np.full((total, stride), mc.SENTINEL, np.uint8)
    want[dst_first:dst_first + m] = a[src_first:src_first + m]
    assert np.array_equal(ctx.read(dst, np.uint8, total * stride).reshape(total, stride), want) and mc.same_bytes(ctx, src, a) and mc.untouched(ctx, guard)
    ctx.copy_rows(src, 0, stride, dst=dst, src_first=total, dst_first=total)          # m == 0: a no-op
    new = ctx.copy_rows(src, m, stride)                                               # a buffer of its own
    assert mc.same_bytes(ctx, new, a[:m])
    for bad in (dict(src_first=13), dict(dst_first=13), dict(stride=stride + 8), dict(dst=src)):
        with pytest.raises(gs4d.Gs4dError):
            ctx.copy_rows(src, **{"m": m, "stride": stride, "dst": dst, "src_first": 0, "dst_first": 0, **bad})
    assert np.array_equal(ctx.read(dst, np.uint8, total * stride).reshape(total, stride), want)
    ctx.finish()
    ctx.close()


def test_refusals_are_loud_and_write_nothing(gs4d):
    ctx = gs4d.Context(64, 64)
    mg = rc.grouping((3, 4, 9), seed=2)
    n = mg.size
    tab, rec = rc.table(n, 12, 48), rc.records(gs4d, n)
    data, group, rows = ctx.buffer(rec), ctx.buffer(mg), ctx.buffer(tab)
    dst, count = mc.fill(ctx, 3 * 48), mc.fill(ctx, 16)
    good = dict(member_group=group, n=n, rows=rows, stride=48, width=12, data=data, dst=dst, dst_first=0, count=count)
    short = ctx.buffer(nbytes=48 * n - 16)
    dead = ctx.buffer(nbytes=64)
    ctx.delete(dead)
    for bad in (dict(stride=40), dict(stride=8), dict(stride=1040), dict(width=0), dict(width=13), dict(n=0xFFFFFFFF), dict(dst_first=0xFFFFFFFF),
                dict(member_group=0), dict(rows=0), dict(dst=0), dict(count=0), dict(data=dead), dict(rows=dead), dict(dst=rows), dict(count=group),
                dict(data=rows), dict(member_group=dst), dict(rows=short), dict(n=n + 1), dict(count=ctx.buffer(nbytes=8)), dict(data=short)):
        with pytest.raises(gs4d.Gs4dError):
            ctx.merge_rows(**{**good, **bad})
    for field in ("flags", "reserved"):
        q = gs4d.rows_query(48, 12)
        setattr(q, field, 1)
        with pytest.raises(gs4d.Gs4dError):
            ctx.merge_rows(**good, query=q)
    assert gs4d._lib.gs4d_merge_rows(ctx._h, data, n, group, rows, None, dst, 0, count) == -1       # q == NULL
    assert mc.untouched(ctx, dst, 3 * 48) and mc.untouched(ctx, count, 16)
    ctx.merge_rows(**good)
    assert rc.count_tuple(ctx.read_merge_count(count)) == (3, 3, n, 0) and ctx.shadow_builds(data) == 0
    ctx.finish()
    ctx.close()


# ---- 4. the forest carries its rows ----------------------------------------------------------------------------------------------------------------
def test_build_lod_with_a_table_and_the_rows_of_the_cuts(gs4d):
    import scenes
    n = 3000
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale * 3.0, rgba)
    rng = np.random.default_rng(0x4C4F)
    sh = gs4d.sh_rows(rng.normal(0, 1, (n, 3)), rng.normal(0, 0.3, (n, 9)), 1)      # degree 1: 12 words, stride 48
    assert sh.shape == (n, 48)
    ctx = gs4d.Context(64, 64)
    data, table = ctx.buffer(rec), ctx.buffer(sh)
    grids = [gs4d.cell_grid((-200.0, -200.0, -200.0), 400.0 / cells, (cells, cells, cells)) for cells in (8, 3)]
    forest = ctx.build_lod(data, n, grids, rows=table, row_stride=48)
    first, N = forest.level_first, forest.n
    assert forest.levels == 3 and (forest.row_stride, forest.row_width) == (48, 12) and first[1] == n and first[2] - first[1] > first[3] - first[2] > 1
    plain = ctx.build_lod(data, n, grids)
    assert plain.rows is None and plain.level_first == first
    # merge_rows_host level by level
    want, below, below_rows = [sh.view(u32).reshape(n, 12)], rec, sh
    for grid in grids:
        out, _, member_group, count = gs4d.merge_records_host(below, gs4d.cell_labels_host(below, grid), 1.0)
        g = int(count["groups"])
        merged, c = gs4d.merge_rows_host(below_rows, member_group, records=below, stride=48, dst=np.zeros((g, 48), np.uint8))
        assert rc.count_tuple(c) == (g, g, below.shape[0], 0)
        want.append(merged.view(u32).reshape(g, 12))
        below, below_rows = np.ascontiguousarray(out[:g]), merged
    want = np.concatenate(want)
    assert want.shape[0] == N and np.array_equal(ctx.read(forest.rows, u32, 12 * N).reshape(N, 12), want)
    eye, index = scenes.CAM_CUBE[0], ctx.buffer(nbytes=4 * N)
    # ratio 0: the cut is the leaves, and its rows are the leaf rows
    c = ctx.read_lod_count(ctx.lod_cut(forest, eye, 0.0, 0.0, cut_index=index))
    assert int(c["drawn"]) == n
    cut_rows = ctx.lod_rows(forest, index, n)
    assert np.array_equal(ctx.read(cut_rows, np.uint8, 48 * n).reshape(n, 48), sh)
    # ratio +inf: the roots — the top level, and whatever the merges left out
    parent = ctx.read(forest.parent, u32, N).astype(np.int64)
    level = np.searchsorted(np.asarray(first[1:]), np.arange(N), side="right")
    roots = np.flatnonzero(~((parent >= np.asarray(first)[level + 1]) & (parent < N)))
    c = ctx.read_lod_count(ctx.lod_cut(forest, eye, 0.0, np.inf, cut_index=index))
    d = int(c["drawn"])
    assert d == roots.size >= N - first[2] and np.array_equal(ctx.read(index, u32, d), roots) and (roots[-(N - first[2]):] == np.arange(first[2], N)).all()
    dst = mc.fill(ctx, 48 * d + 16)
    assert ctx.lod_rows(forest, index, d, dst=dst) == dst
    assert np.array_equal(ctx.read(dst, u32, 12 * d).reshape(d, 12), want[roots]) and mc.untouched(ctx, dst, 16, offset=48 * d)
    with pytest.raises(ValueError):
        ctx.lod_rows(plain, index, d)
    ctx.finish()
    ctx.close()


def test_degree_0_colour_of_the_merged_set_is_the_merge_of_the_shaded_leaves(gs4d):
    """shade_sh at degree 0 is colour = C0 * dc + 0.5 where the clamp does not act (merge_rows_cases.degree0_case checks that it does not), and it is
    linear: shading the merged records with their merged rows must give the rgb of merge_records of the shaded leaves.  Bound, derived: one side
    rounds the merged dc (a mean of values below 1.4, times C0 < 0.3), the product and the sum in float32 — three roundings of values below 1, at most
    2^-24 each; the other rounds the final cast of the double mean, 2^-25, of leaf colours that each carry the two roundings of their own shade,
    2 * 2^-25 in the mean; the double sums are negligible.  4 * 2^-24 absolute covers the sum."""
    rec, labels, sh = rc.degree0_case(gs4d)
    n = rec.shape[0]
    ctx = gs4d.Context(64, 64)
    cam = (3.0, -2.0, 40.0)
    data, lab, table = ctx.buffer(rec), ctx.buffer(labels), ctx.buffer(sh)
    member_group = ctx.buffer(nbytes=4 * n)
    merged, count = ctx.merge_records(data, n, lab, member_group=member_group)
    g = int(ctx.read_merge_count(count)["groups"])
    assert 20 < g < n
    merged_rows, rcount = ctx.merge_rows(member_group, n, table, 16, 3, data=data)
    assert rc.count_tuple(ctx.read_merge_count(rcount)) == (g, g, int(ctx.read_merge_count(count)["members"]), int(ctx.read_merge_count(count)["left_out"]))
    ctx.shade_sh(merged, g, merged_rows, 0, 0.0, cam)
    one = ctx.read(merged, f32, 24 * g).reshape(g, 24)[:, 4:7]
    assert np.array_equal(one, rc.degree0_colour(ctx.read(merged_rows, np.uint8, 16 * g).reshape(g, 16)))      # shade_sh, by its text
    ctx.shade_sh(data, n, table, 0, 0.0, cam)
    shaded, count2 = ctx.merge_records(data, n, lab)
    assert int(ctx.read_merge_count(count2)["groups"]) == g
    two = ctx.read(shaded, f32, 24 * g).reshape(g, 24)[:, 4:7]
    worst = float(np.abs(one.astype(np.float64) - two.astype(np.float64)).max())
    print(f"degree-0 consistency: worst difference {worst:.3e} = {worst * 2 ** 24:.3f} * 2^-24 over {g} groups")
    assert worst <= 4.0 * 2.0 ** -24
    ctx.finish()
    ctx.close()
