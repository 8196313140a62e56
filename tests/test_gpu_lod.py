"""GPU: gs4d_lod_append and gs4d_lod_cut — a forest of merged levels assembled on the device, and the cut a camera and a time make through it
(include/gs4d.h).

The device's dst, cut_index, stats and count are compared with the host definition as uint32 words, every word and without an exemption: the call
copies records and computes no new float output (the host definition is compared with the header's text in tests/test_lod_host.py).  The shapes lie
around the tile of 1024 nodes of the level kernel, its rounds of 256 and its waves of 64, and around the tile of 2048 of the compaction.  Slots at
or beyond the capacity, guard buffers and the inputs are compared with what was uploaded (tests/lod_cases.py: device_call).  All calls go through
the Python binding over the C ABI."""
import numpy as np
import pytest

import lod_cases as lc
import scenes

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


# ---- 1. the cut ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", lc.LEAVES)
def test_level_sizes_around_the_tiles_at_1_2_5_and_16_levels(gs4d, leaves):
    ctx = gs4d.Context(64, 64)
    drawn = inner = 0
    for call, levels in enumerate(lc.LEVELS):
        which = lc.SETS[(call + leaves) % 4]                                          # the hostile records among them
        rec, parent, first = lc.random_forest(gs4d, which, leaves, levels, call, fan=2 if levels == 16 else 3)
        assert first[-1] == rec.shape[0] and (levels < 5 or first[2] == first[3])     # an empty level from five levels on
        mid = lc.middle_ratio(rec, lc.EYE, lc.T)
        for ratio, near in ((0.0, 0.0), (np.inf, 0.0), (mid, 0.0), (mid * 0.1, 1e30)):
            host = lc.check(gs4d, ctx, rec, parent, first, f"{which}, {leaves} leaves, {levels} levels, ratio {ratio}, near {near}", ratio=ratio, near=near)
            c = host[3]
            if levels == 1:
                assert tuple(int(v) for v in c) == (leaves,) * 4                      # a single level: the cut is the set itself
            drawn, inner = drawn + int(c["drawn"]), inner + int(c["drawn"]) - int(c["drawn_leaves"])
    assert drawn > 0 and (leaves < 63 or inner > 0)
    ctx.finish()                                                                      # reports device-side check failures
    ctx.close()


@pytest.mark.parametrize("fill", (False, True))
def test_single_tested_lanes_and_skipped_waves(gs4d, fill):
    ctx = gs4d.Context(64, 64)
    rec, parent, first, lanes = lc.skipped_wave_forest(gs4d, fill=fill)
    n = first[-1]
    stats = lc.stats_table(gs4d, n, 5)
    host = lc.check(gs4d, ctx, rec, parent, first, "skipped waves", stats=stats)
    roots = first[3] - first[2]
    # the roots, one of them not fine; of level 1 only the children of that root, none of them fine; their leaves
    assert tuple(int(v) for v in host[3]) == (roots - 1 + len(lanes), roots - 1 + len(lanes), roots + 2 * len(lanes), len(lanes))
    assert host[1][:len(lanes)].tolist() == lanes
    waves = {lane // 64 for lane in lanes}
    assert len(waves) < (first[1] + 63) // 64 - 20                                    # most waves of the two lower levels test nothing
    assert {0, 63, lc.LOD_TILE - 1, lc.LOD_TILE} <= set(lanes)
    ctx.finish()
    ctx.close()


def test_extents_that_do_not_grow_and_hostile_parent_words(gs4d):
    ctx = gs4d.Context(64, 64)
    first = lc.firsts([4, 4, 4])
    rec = lc.sized_record(gs4d, 12, lc.LARGE)
    parent = np.r_[np.arange(4, 8), np.arange(8, 12), [lc.ID_NONE] * 4].astype(u32)
    rec[8, [8, 13, 18]] = lc.SMALL                                                    # a grandparent that is fine above a parent that is not
    rec[[5, 1], 8:19:5] = lc.SMALL                                                    # a parent that is fine under a grandparent that is not
    rec[10, [8, 13, 18]] = lc.SMALL
    host = lc.check(gs4d, ctx, rec, parent, first, "extents")
    assert host[1][:4].tolist() == [3, 5, 8, 10]
    rec, parent, first = lc.hostile_parent_forest(gs4d)
    for ratio in (1.0, np.inf, 0.0):
        host = lc.check(gs4d, ctx, rec, parent, first, f"hostile parents, ratio {ratio}", ratio=ratio, stats=lc.stats_table(gs4d, first[-1], 9))
        assert int(host[3]["drawn"]) == (300 if ratio != np.inf else 16)
    ctx.finish()
    ctx.close()


@pytest.mark.parametrize("which", ("hostile", "4d_2q"))
def test_hostile_records_eyes_and_times(gs4d, which):
    ctx = gs4d.Context(64, 64)
    rec, parent, first = lc.random_forest(gs4d, which, 769, 5, 11)
    mid = lc.middle_ratio(rec, lc.EYE, lc.T)
    if which == "hostile":
        assert np.isnan(rec[:, [8, 13, 18]]).any() and np.isinf(rec).any() and (rec[:, 23] == 0).any() and np.isnan(rec[:, :4]).any()
    for eye, t in ((lc.EYE, lc.T), ((np.nan, 0.0, 0.0), 0.0), ((np.inf, -np.inf, 1e30), 1.0), (lc.EYE, np.nan), (lc.EYE, np.inf), (tuple(rec[5, :3]), float(rec[5, 3]))):
        for ratio, near in ((mid, 0.0), (np.inf, 0.0), (mid, 3.0e38)):
            lc.check(gs4d, ctx, rec, parent, first, f"{which}, eye {eye}, t {t}, ratio {ratio}, near {near}", eye=eye, t=t, ratio=ratio, near=near)
    ctx.finish()
    ctx.close()


def test_capacities_below_drawn_with_every_combination_of_outputs(gs4d):
    ctx = gs4d.Context(64, 64)
    rec, parent, first = lc.random_forest(gs4d, "4d_vel", 2 * lc.COMPACT_TILE + 5, 5, 21)
    n = first[-1]
    mid = lc.middle_ratio(rec, lc.EYE, lc.T)
    stats = lc.stats_table(gs4d, n, 3)
    _, where, _, count = gs4d.lod_cut_host(rec, parent, gs4d.lod_query(first, lc.EYE, lc.T, mid))
    drawn = int(count["drawn"])
    tiles = where[:drawn] // lc.COMPACT_TILE                                          # the compaction tile of every drawn node
    assert drawn > 1000 and len(set(tiles.tolist())) == 3 and tiles[drawn // 2 + 37] < tiles[drawn - 2]      # capacities that end in two different tiles
    call = 0
    for with_dst in (True, False):
        for with_index in (True, False):
            for table in (stats, None):
                cap_dst, cap_index = ((drawn - 1, drawn // 2 + 37), (0, 1), (7, 3), (drawn, drawn + 5))[call % 4]
                host = lc.check(gs4d, ctx, rec, parent, first, f"dst {with_dst} ({cap_dst}), cut_index {with_index} ({cap_index}), stats {table is not None}",
                                ratio=mid, stats=table, with_dst=with_dst, with_index=with_index, cap_dst=cap_dst, cap_index=cap_index)
                assert int(host[3]["drawn"]) == drawn
                call += 1
    ctx.finish()
    ctx.close()


def test_no_nodes_and_refusals_are_loud(gs4d):
    ctx = gs4d.Context(64, 64)
    rec, parent, first = lc.random_forest(gs4d, "3d", 300, 2, 4)
    n = first[-1]
    nodes, par = ctx.buffer(rec), ctx.buffer(parent)
    forest = gs4d.LodForest(nodes, par, first)
    count = lc.fill(ctx, 32)
    empty = gs4d.LodForest(nodes, par, [0, 0, 0])
    assert ctx.lod_cut(empty, lc.EYE, lc.T, 1.0, count=count) == count
    assert tuple(ctx.read_lod_count(count)) == (0, 0, 0, 0) and lc.untouched(ctx, count, 16, offset=16)
    new = ctx.lod_cut(forest, lc.EYE, lc.T, 0.0)                                     # a count buffer of its own
    assert tuple(ctx.read_lod_count(new)) == (300, 300, n, 300)
    dst, index, stats = lc.fill(ctx, 96 * n), lc.fill(ctx, 4 * n), ctx.buffer(np.zeros(n, gs4d.RECORD_STAT))
    for over in (dict(ratio=np.nan), dict(ratio=-1.0), dict(near=np.inf), dict(near=-1.0)):
        with pytest.raises(gs4d.Gs4dError):
            ctx.lod_cut(forest, lc.EYE, lc.T, **{"ratio": 1.0, **over}, dst=dst, cut_index=index, stats=stats, count=count)
    for field, value in (("levels", 0), ("levels", 17), ("flags", 1)):
        q = gs4d.lod_query(first, lc.EYE, lc.T, 1.0)
        setattr(q, field, value)
        with pytest.raises(gs4d.Gs4dError):
            ctx.lod_cut(forest, None, None, None, dst=dst, count=count, query=q)
    for k, v in ((0, 1), (1, n + 1), (2, n - 1), (3, 1)):
        q = gs4d.lod_query(first, lc.EYE, lc.T, 1.0)
        (q.reserved if k == 3 else q.level_first)[k if k < 3 else 2] = v
        with pytest.raises(gs4d.Gs4dError):
            ctx.lod_cut(forest, None, None, None, dst=dst, count=count, query=q)
    assert gs4d._lib.gs4d_lod_cut(ctx._h, nodes, par, n, None, dst, index, stats, count) == -1      # q == NULL
    short = ctx.buffer(nbytes=16 * n - 16)
    for bad in (dict(dst=nodes), dict(cut_index=par), dict(stats=dst), dict(count=index), dict(stats=short), dict(count=ctx.buffer(nbytes=8))):
        with pytest.raises(gs4d.Gs4dError):
            ctx.lod_cut(forest, lc.EYE, lc.T, 1.0, **{"dst": dst, "cut_index": index, "stats": stats, "count": count, **bad})
    with pytest.raises(gs4d.Gs4dError):
        ctx.lod_cut(gs4d.LodForest(nodes, par, [0, 300, n + 1]), lc.EYE, lc.T, 1.0, count=count)      # nodes and parent hold n
    # refused calls wrote nothing
    assert tuple(ctx.read_lod_count(count)) == (0, 0, 0, 0) and lc.untouched(ctx, dst, 96 * n) and lc.untouched(ctx, index, 4 * n)
    assert not ctx.read(stats, np.uint8, 16 * n).any() and ctx.shadow_builds(nodes) == 0
    ctx.finish()
    ctx.close()


# ---- 2. the forest ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m, c", ((255, 257), (256, 256), (257, 255), (1, 0), (0, 300), (300, 1)))
def test_append_around_256_nodes_and_children(gs4d, m, c):
    ctx = gs4d.Context(64, 64)
    rng = np.random.default_rng(m * 1000 + c)
    level = lc.tc.records(gs4d, "hostile", max(m, 1))[:m]                             # NaN payloads travel as they are
    mg = rng.integers(0, max(m, 1), c).astype(u32)
    if c >= 3:
        mg[[0, c // 2, c - 1]] = (m, max(m, 1) - 1, lc.ID_NONE)                       # a group beyond `written`, the last one written, a record left out
    for child_first, first, total in ((0, c, c + m), (3, c + 3, c + m + 9), (2, c + 7, c + m + 7)):      # child_first + c == first twice; a gap once
        got = lc.device_append(gs4d, ctx, level, mg, m, c, first, child_first, total, f"m {m}, c {c}, first {first}")
        want = lc.append_by_the_text(level, mg, m, c, first, child_first, total)
        assert np.array_equal(got[0], want[0]), "nodes"
        assert np.array_equal(got[1], want[1]), "parent"
    got = lc.device_append(gs4d, ctx, level, None, m, 0, 5, 0, m + 6, "the leaf level")
    want = lc.append_by_the_text(level, None, m, 0, 5, 0, m + 6)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ctx.finish()
    ctx.close()


def test_append_refusals_are_loud(gs4d):
    ctx = gs4d.Context(64, 64)
    level, mg = ctx.buffer(lc.tc.records(gs4d, "3d", 10)), ctx.buffer(np.zeros(20, u32))
    nodes, parent = lc.fill(ctx, 96 * 30), lc.fill(ctx, 4 * 30)
    for bad in (dict(child_first=1), dict(c=21, first=21), dict(first=21), dict(member_group=None), dict(level=nodes), dict(parent=mg), dict(nodes=level),
                dict(m=11), dict(first=0xFFFFFFFE - 9, child_first=0, c=0, member_group=None)):
        a = {"level": level, "m": 10, "nodes": nodes, "parent": parent, "first": 20, "member_group": mg, "child_first": 0, "c": 20, **bad}
        with pytest.raises(gs4d.Gs4dError):
            ctx.lod_append(a.pop("level"), a.pop("m"), a.pop("nodes"), a.pop("parent"), a.pop("first"), **a)
    ctx.lod_append(level, 0, nodes, parent, 30)                                       # nothing to do
    ctx.finish()
    assert lc.untouched(ctx, nodes, 96 * 30) and lc.untouched(ctx, parent, 4 * 30)
    ctx.close()


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------------------
def frame(gs4d, ctx, data, n, W, H):
    cam = scenes.CAM_CUBE
    keys, idx = ctx.buffer(nbytes=max(16, 4 * n)), ctx.buffer(nbytes=max(16, 4 * n))
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.clear()
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=gs4d.look_at(cam[0], cam[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
    ctx.keygen(data, 0.0, cam[0], keys, idx, n)
    ctx.sort_pairs(keys, idx, n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, idx)
    ctx.bind(2, data)
    ctx.draw_instanced(n)
    return ctx.read_pixels()


def test_build_lod_and_the_cuts_of_a_cube_set(gs4d):
    W = H = 64
    n = 4096
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale * 3.0, rgba)
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(rec)
    grids = [gs4d.cell_grid((-200.0, -200.0, -200.0), 400.0 / cells, (cells, cells, cells)) for cells in (12, 6, 3)]
    forest = ctx.build_lod(data, n, grids)
    first, N = forest.level_first, forest.n
    assert forest.levels == 4 and first[0] == 0 and first[1] == n and N > n and all(a > b > 0 for a, b in zip(np.diff(first)[:-1], np.diff(first)[1:]))
    nodes, parent = ctx.read(forest.nodes, f32, 24 * N).reshape(N, 24), ctx.read(forest.parent, u32, N)
    assert np.array_equal(lc.bits(nodes[:n]), lc.bits(rec))
    # the levels are merge_records of the level below under cell_labels, linked by member_group
    below = rec
    for k, grid in enumerate(grids):
        labels = gs4d.cell_labels_host(below, grid)
        out, _, member_group, count = gs4d.merge_records_host(below, labels, 1.0)
        g = int(count["groups"])
        assert g == first[k + 2] - first[k + 1] and np.array_equal(lc.bits(nodes[first[k + 1]:first[k + 2]]), lc.bits(out[:g]))
        want = np.where(member_group < g, first[k + 1] + member_group.astype(np.int64), lc.ID_NONE).astype(u32)
        assert np.array_equal(parent[first[k]:first[k + 1]], want)
        below = np.ascontiguousarray(out[:g])
    assert (parent[first[3]:] == lc.ID_NONE).all()
    eye, dst, index = scenes.CAM_CUBE[0], ctx.buffer(nbytes=96 * N), ctx.buffer(nbytes=4 * N)
    # ratio 0: the cut is level 0, byte for byte, and its frame has the bits of the full set's frame
    c = ctx.read_lod_count(ctx.lod_cut(forest, eye, 0.0, 0.0, dst=dst, cut_index=index))
    assert tuple(int(v) for v in c) == (n, n, N, n) and np.array_equal(ctx.read(dst, u32, 24 * n), lc.bits(rec).reshape(-1))
    assert ctx.shadow_builds(forest.nodes) == 0
    full, cut = frame(gs4d, ctx, data, n, W, H), frame(gs4d, ctx, dst, n, W, H)
    assert np.array_equal(lc.bits(cut), lc.bits(full)) and float(np.abs(full - np.array(gs4d.CLEAR_COLOR, f32)).max()) > 0.05
    # ratio +inf: the roots
    level = np.searchsorted(np.asarray(first[1:]), np.arange(N), side="right")
    child = (parent.astype(np.int64) >= np.asarray(first)[level + 1]) & (parent.astype(np.int64) < N)
    c = ctx.read_lod_count(ctx.lod_cut(forest, eye, 0.0, np.inf, dst=dst, cut_index=index))
    roots = np.flatnonzero(~child)
    assert int(c["drawn"]) == roots.size == int(c["tested"]) and np.array_equal(ctx.read(index, u32, roots.size), roots)
    # a middle ratio: the device cut is lod_cut_host of the forest read back, and the cut accounts for every leaf
    mid = lc.middle_ratio(nodes[first[1]:first[3]], eye, 0.0)
    stats = ctx.buffer(np.zeros(N, gs4d.RECORD_STAT))
    c = ctx.read_lod_count(ctx.lod_cut(forest, eye, 0.0, mid, dst=dst, cut_index=index, stats=stats))
    hdst, hindex, hstats, hc = gs4d.lod_cut_host(nodes, parent, gs4d.lod_query(first, eye, 0.0, mid), stats=np.zeros(N, gs4d.RECORD_STAT))
    d = int(c["drawn"])
    assert tuple(int(v) for v in c) == tuple(int(v) for v in hc) and 0 < int(c["drawn_leaves"]) < d < n
    assert np.array_equal(ctx.read(dst, u32, 24 * d), lc.bits(hdst[:d]).reshape(-1)) and np.array_equal(ctx.read(index, u32, d), hindex[:d])
    assert np.array_equal(ctx.read(stats, u32, 4 * N), hstats.view(u32))
    cut_index = ctx.read(index, u32, d)
    drawn = np.zeros(N, bool)
    drawn[cut_index] = True
    covered = drawn.copy()                                                            # a node is covered iff it or an ancestor is drawn: top down
    for k in range(forest.levels - 2, -1, -1):
        i = np.arange(first[k], first[k + 1])
        covered[i] |= child[i] & covered[np.where(child[i], parent[i], 0)]
    under = int(covered[:n].sum()) - int(drawn[:n].sum())                             # leaves under a drawn node above them
    assert int(drawn[:n].sum()) + under == n and under > 0
    # exactly one drawn node on the chain of every leaf
    assert lc.chains_draw_once(parent, first, np.where(drawn, lc.DRAW, lc.STOP).astype(np.uint8)) == n
    img = frame(gs4d, ctx, dst, d, W, H)
    assert float(np.abs(img.astype(np.float64) - full.astype(np.float64)).mean()) < 0.25      # a picture of the same cube (no reference exists for the approximation)
    ctx.finish()
    ctx.close()
