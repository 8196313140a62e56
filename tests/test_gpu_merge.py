"""GPU: gs4d_cell_labels and gs4d_merge_records — a label per record from a 4D cell grid, one moment-matched record per labelled group
(include/gs4d.h).

The device's dst, groups, member_group and count are compared with the host definition as uint32 words, every word and without an exemption (the
host definition is compared with the header's text in tests/test_merge_host.py), around the edges of the kernel: group sizes around the eight lanes
of a sub-group, group counts around a wave of 8 groups and a workgroup of 32, sets around the tile of 2048 sorted keys.  Slots at or above the
capacity, guard buffers and the inputs are compared with what was uploaded (tests/merge_cases.py: device_call).  All calls go through the Python
binding over the C ABI."""
import numpy as np
import pytest

import merge_cases as mc
import neighbour_cases as nc
import reorder_cases as rc
import scenes
import transform_cases as tc

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


def check(gs4d, ctx, rec, labels, what, alpha_max=1.0, stats=None, written=None, **kw):
    rule = {k: kw[k] for k in ("min_pixels", "invert") if k in kw}
    host = gs4d.merge_records_host(rec, labels, alpha_max, stats, **rule)
    got = mc.device_call(gs4d, ctx, rec, labels, what, alpha_max, stats, **kw)
    mc.assert_device_equals_host(what, got, host, written)
    return host


# ---- 1. the records ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", mc.SETS)
def test_every_edge_group_size_in_one_call(gs4d, which):
    ctx = gs4d.Context(64, 64)
    n = sum(mc.EDGE_SIZES)
    rec = tc.records(gs4d, which, n)
    if which != "hostile":
        rec = rec[mc.members_of(rec, np.zeros(n, u32))]                              # (a needle without an area is no member: the sizes are exact)
        rec = np.ascontiguousarray(np.concatenate([rec, rec])[:n])
    labels = mc.sized_labels(mc.EDGE_SIZES)                                           # labels 0 .. 0xFFFFFFFE, the members of a group far apart
    assert labels.min() == 0 and labels.max() == 0xFFFFFFFE
    for alpha_max in (1.0, 1e-3):
        host = check(gs4d, ctx, rec, labels, f"{which}, alpha_max {alpha_max}", alpha_max)
        g = int(host[3]["groups"])
        if which != "hostile":
            assert sorted(host[1]["size"][:g].tolist()) == sorted(mc.EDGE_SIZES) and int(host[3]["left_out"]) == 0
        else:
            assert int(host[3]["left_out"]) > 100 and int(host[3]["members"]) > 100 and g >= 8
    ctx.finish()                                                                      # reports device-side check failures
    ctx.close()


@pytest.mark.parametrize("count", mc.EDGE_COUNTS)
def test_group_counts_around_the_sub_group_the_wave_and_the_workgroup(gs4d, count):
    ctx = gs4d.Context(64, 64)
    sizes = [(3 * j) % 11 + 1 for j in range(count)]                                  # 1 .. 11 members
    n = sum(sizes)
    rec = tc.records(gs4d, "4d_2q", n + 8)
    rec = np.ascontiguousarray(rec[mc.members_of(rec, np.zeros(n + 8, u32))][:n])
    assert rec.shape[0] == n
    host = check(gs4d, ctx, rec, mc.sized_labels(sizes, first_label=7, seed=count), f"{count} groups")
    assert int(host[3]["groups"]) == count
    ctx.finish()
    ctx.close()


@pytest.mark.parametrize("which", mc.SETS)
def test_sets_around_the_tiles_with_and_without_a_table(gs4d, which):
    ctx = gs4d.Context(64, 64)
    members = left_out = 0
    for call, n in enumerate(mc.SIZES):
        rec, labels = tc.records(gs4d, which, n), mc.mixed_labels(n, call)
        stats = mc.stats_table(gs4d, n, call)
        for what, table, rule in (("no table", None, {}), ("rule", stats, {"min_pixels": 1}), ("inverted rule", stats, {"min_pixels": 1, "invert": True})):
            host = check(gs4d, ctx, rec, labels, f"{which}, n = {n}, {what}", (1.0, 0.25, 1e-3)[call % 3], table, **rule)
            members, left_out = members + int(host[3]["members"]), left_out + int(host[3]["left_out"])
    assert members > 1000 and left_out > 1000
    ctx.finish()
    ctx.close()


def test_a_capacity_below_the_group_count(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 769
    rec, labels = tc.records(gs4d, "4d_vel", n), mc.mixed_labels(n)
    groups = int(gs4d.merge_records_host(rec, labels)[3]["groups"])
    assert groups > 70
    for cap_dst, cap_groups, with_groups in ((groups - 1, n, True), (n, 33, True), (8, 9, True), (40, 0, False), (0, 5, True), (2, 1, True), (groups, groups, True)):
        cap = min(cap_dst, cap_groups) if with_groups else cap_dst
        check(gs4d, ctx, rec, labels, f"dst holds {cap_dst}, groups {cap_groups if with_groups else 'not given'}", written=cap, cap_dst=cap_dst,
              cap_groups=cap_groups, with_groups=with_groups)
    check(gs4d, ctx, rec, labels, "no member_group", with_member_group=False)
    check(gs4d, ctx, rec, labels, "dst alone", with_groups=False, with_member_group=False)
    ctx.finish()
    ctx.close()


def test_no_members_no_records_and_one_group_of_all(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 300
    rec = tc.records(gs4d, "3d", n)
    host = check(gs4d, ctx, rec, np.full(n, mc.ID_NONE, u32), "no label")
    assert tuple(host[3]) == (0, 0, 0, n)
    hidden = rec.copy()
    hidden[:, 7] = 0.0
    host = check(gs4d, ctx, hidden, np.zeros(n, u32), "no mass")
    assert tuple(host[3]) == (0, 0, 0, n)
    host = check(gs4d, ctx, np.zeros((0, 24), f32), np.zeros(0, u32), "n == 0")
    assert tuple(host[3]) == (0, 0, 0, 0)
    n = 5000
    rec = tc.records(gs4d, "4d_vel", n)
    host = check(gs4d, ctx, rec, np.full(n, 0xFFFFFFFE, u32), "one group of 5000 records", alpha_max=1e9)
    assert int(host[3]["groups"]) == 1 and int(host[1]["size"][0]) == int(host[3]["members"]) > 4900
    ctx.finish()
    ctx.close()


def test_buffers_are_allocated_and_refusals_are_loud(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 300
    rec, labels = tc.records(gs4d, "4d_2q", n), mc.mixed_labels(n)
    data, lab = ctx.buffer(rec), ctx.buffer(labels)
    dst, count = ctx.merge_records(data, n, lab, 0.5)
    host = gs4d.merge_records_host(rec, labels, 0.5)
    c = ctx.read_merge_count(count)
    assert tuple(c) == tuple(host[3]) and ctx.device_ptr(dst)[1] >= 96 * n
    g = int(c["groups"])
    assert np.array_equal(ctx.read(dst, u32, 24 * g), host[0][:g].view(u32).reshape(-1))
    for alpha_max in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(gs4d.Gs4dError):
            ctx.merge_records(data, n, lab, alpha_max, dst=dst, count=count)
    q = gs4d.merge_query(1.0)
    q.flags = 1
    with pytest.raises(gs4d.Gs4dError):
        ctx.merge_records(data, n, lab, dst=dst, count=count, query=q)
    with pytest.raises(TypeError):
        ctx.merge_records(data, n, lab, dst=dst, count=count, min_pixels=1)           # a rule without a table
    stats = ctx.buffer(mc.stats_table(gs4d, n))
    rule = gs4d._keep_rule()
    h, p = ctx._h, gs4d._ptr
    import ctypes
    assert gs4d._lib.gs4d_merge_records(h, data, n, lab, ctypes.byref(gs4d.merge_query(1.0)), stats, None, dst, 0, 0, count) == -1      # a table without a rule
    assert gs4d._lib.gs4d_merge_records(h, data, n, lab, ctypes.byref(gs4d.merge_query(1.0)), 0, p(rule), dst, 0, 0, count) == -1       # a rule without a table
    for bad in (dict(dst=data), dict(dst=lab), dict(count=dst), dict(member_group=ctx.buffer(nbytes=4 * n - 4)), dict(count=ctx.buffer(nbytes=8)), dict(groups=count)):
        with pytest.raises(gs4d.Gs4dError):
            ctx.merge_records(data, n, lab, **{"dst": dst, "count": count, **bad})
    with pytest.raises(gs4d.Gs4dError):
        ctx.merge_records(data, n + 1, lab, dst=dst, count=count)                     # data and labels hold n
    assert tuple(ctx.read_merge_count(count)) == tuple(host[3])                       # a refused call writes nothing
    ctx.finish()
    ctx.close()


# ---- 2. the labels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.GRIDS))
def test_cell_labels_equal_the_host_definition(gs4d, name):
    ctx = gs4d.Context(64, 64)
    grid, lo, edge, dims = mc.grid(gs4d, name)
    rec = mc.grid_records(gs4d, lo, edge, dims)
    n = rec.shape[0]
    guards = [mc.fill(ctx, mc.GUARD)]
    data = ctx.buffer(rec)
    labels = mc.fill(ctx, 4 * n + 16)
    guards.append(mc.fill(ctx, mc.GUARD))
    assert ctx.cell_labels(data, n - 1, grid, labels) == labels
    want = gs4d.cell_labels_host(rec, grid)
    assert np.array_equal(ctx.read(labels, u32, n - 1), want[:n - 1]) and mc.untouched(ctx, labels, 20, offset=4 * (n - 1))
    ctx.cell_labels(data, n, grid, labels)
    assert np.array_equal(ctx.read(labels, u32, n), want) and mc.untouched(ctx, labels, 16, offset=4 * n)
    assert all(mc.untouched(ctx, g) for g in guards) and mc.same_bytes(ctx, data, rec)
    assert ctx.shadow_builds(data) == 0
    if name == "largest":
        assert want[0] == 0xFFFFFFFB
    ctx.finish()
    ctx.close()


def test_refused_grids_and_no_records(gs4d):
    ctx = gs4d.Context(64, 64)
    rec = tc.records(gs4d, "3d", 5)
    data, labels = ctx.buffer(rec), mc.fill(ctx, 32)
    for what, (edge, dims, reserved) in mc.REFUSED_GRIDS.items():
        g = gs4d.cell_grid((0, 0, 0, 0), edge, dims)
        g.reserved[:] = reserved
        with pytest.raises(gs4d.Gs4dError):
            ctx.cell_labels(data, 5, g, labels)
    ok = gs4d.cell_grid((0, 0, 0), 1.0, (4, 4, 4))
    with pytest.raises(gs4d.Gs4dError):
        ctx.cell_labels(data, 9, ok, labels)                                          # labels holds 8 words, data 5 records
    with pytest.raises(gs4d.Gs4dError):
        ctx.cell_labels(data, 5, ok, data)
    ctx.cell_labels(data, 0, ok, labels)
    ctx.finish()
    assert mc.untouched(ctx, labels, 32)
    ctx.close()


# ---- 3. a level of detail -----------------------------------------------------------------------------------------------------------------------
def frame(gs4d, ctx, data, n, W, H):
    cam = scenes.CAM_CUBE
    keys, idx = ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
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


@pytest.fixture(scope="module")
def cube_records(gs4d):
    pos, q, scale, rgba = scenes.cube_params(20000)
    return gs4d.build_records_3d(pos, q, scale * 3.0, rgba)


@pytest.mark.parametrize("edge", (25.0, 80.0))
def test_lod_of_a_cube_set_draws(gs4d, cube_records, edge):
    W, H, n = 320, 180, 20000
    rec = cube_records
    cells = int(np.ceil(400.0 / edge))
    grid = gs4d.cell_grid((-200.0, -200.0, -200.0), edge, (cells, cells, cells))
    ctx = gs4d.Context(W, H)
    data = ctx.buffer(rec)
    dst, count = ctx.lod(data, n, grid, alpha_max=1.0)
    c = ctx.read_merge_count(count)
    labels = gs4d.cell_labels_host(rec, grid)
    members = mc.members_of(rec, labels)
    assert int(c["groups"]) == len(set(labels[members].tolist())) == int(c["written"]) and int(c["members"]) == int(members.sum())
    assert 2.0 < int(c["members"]) / int(c["groups"]) and int(c["groups"]) > 100
    host = gs4d.merge_records_host(rec, labels, 1.0)
    g = int(c["groups"])
    assert np.array_equal(ctx.read(dst, u32, 24 * g), host[0][:g].view(u32).reshape(-1))
    assert ctx.shadow_builds(dst) == 0
    img = frame(gs4d, ctx, dst, g, W, H)
    assert float(np.abs(img.astype(np.float64) - np.array(gs4d.CLEAR_COLOR, np.float64)).max()) > 0.05, "empty frame"
    full = frame(gs4d, ctx, data, n, W, H)
    # not a threshold on the approximation (no reference exists for one): the merged picture is a picture of the same cube, not of something else
    assert float(np.abs(img.astype(np.float64) - full.astype(np.float64)).mean()) < 0.25
    ctx.finish()                                                                      # reports device-side check failures
    assert ctx.shadow_builds(dst) == 1
    ctx.close()


# ---- 4. scratch re-use ---------------------------------------------------------------------------------------------------------------------------
class Outputs:
    """sentinel-filled dst, groups, member_group and count of one merge of n records, a guard buffer behind them; nothing is read before read()"""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.sizes = ((n + 3) * 96 + 32, (n + 3) * 16 + 8, 4 * n + 16, 32)
        self.dst, self.groups, self.mg, self.count = (mc.fill(ctx, b) for b in self.sizes)
        self.guard = mc.fill(ctx, mc.GUARD)

    def queue(self, data, lab, alpha_max):
        self.ctx.merge_records(data, self.n, lab, alpha_max, dst=self.dst, groups=self.groups, member_group=self.mg, count=self.count)

    def read(self, gs4d, what):
        """-> (what assert_device_equals_host takes, every byte of the four buffers); what lies behind the written part still holds the sentinel"""
        ctx, n = self.ctx, self.n
        raw = [ctx.read(b, np.uint8, size) for b, size in zip((self.dst, self.groups, self.mg, self.count), self.sizes)]
        c = raw[3][:16].view(gs4d.MERGE_COUNT)[0]
        w = int(c["written"])
        assert w == int(c["groups"]) <= n, f"{what}: count {c}"
        for a, used in zip(raw, (96 * w, 16 * w, 4 * n, 16)):
            assert (a[used:] == mc.SENTINEL).all(), f"{what}: bytes behind the written part of an output changed"
        assert mc.untouched(ctx, self.guard), f"{what}: the guard buffer changed"
        got = (raw[0][:96 * w].view(f32).reshape(w, 24), raw[1][:16 * w].view(gs4d.MERGE_GROUP), raw[2][:4 * n].view(u32), c)
        return got, b"".join(a.tobytes() for a in raw)

    def delete(self):
        for b in (self.dst, self.groups, self.mg, self.count, self.guard):
            self.ctx.delete(b)


def test_the_scratch_is_shared_with_the_grid_queries_and_the_spatial_order_at_other_sizes(gs4d):
    """large, small, large again on one lane; behind every merge a gs4d_count_neighbours, gs4d_label_components or gs4d_spatial_order call of another
    size and the same merge once more, the three queued without a read or a finish between them.  The merge keeps keys, sorted indices, run starts,
    tile counts and the state block at offsets of the lane's neighbour_scratch that depend on n (launch_merge_records, csrc/merge.hip: keys = scratch,
    index = keys + n4, ...) and sorts through the lane's pair_sort; the grid queries lay out the same scratch by their own n, the spatial order sizes
    the same pair_sort.  A call that kept a pointer or a size of the scratch from an earlier, larger or smaller call — or a scratch that is grown
    while a queued kernel still uses the old storage — would give the second merge other run starts or keys: its dst, groups or member_group would
    differ from the first merge's and from the host definition's."""
    ctx = gs4d.Context(64, 64)
    assert ctx.stats()["lanes"] >= 1
    other = nc.case("cube", 1025)
    odata, ostats = ctx.buffer(other.rec), ctx.record_stats(other.n)
    want_counts = nc.host(other.rec, other.t, other.r, 0xFFFFFFFF, 0, nc.table("zero", other.n))
    want_labels = gs4d.label_components_host(other.rec, other.r, with_stats=False)[0]
    opos = rc.positions("uniform", 70_001)
    osrc, want_order = ctx.buffer(rc.records_with_positions(opos, 16, 0)), rc.order(opos)
    for step, n in enumerate((4100, 9, 2049, 769, 4100)):
        what = f"step {step}, n = {n}"
        rec, labels = tc.records(gs4d, "4d_vel", n), mc.mixed_labels(n, step)
        alpha_max = (1.0, 0.25, 1e-3)[step % 3]
        host = gs4d.merge_records_host(rec, labels, alpha_max)
        assert int(host[3]["groups"]) >= 2 and int(host[3]["left_out"]) >= 0
        data, lab = ctx.buffer(rec), ctx.buffer(labels)
        first, second = Outputs(ctx, n), Outputs(ctx, n)
        olabels, oindex = mc.fill(ctx, 4 * other.n + 16), mc.fill(ctx, 4 * 70_001 + 16)
        ctx.subdata(ostats, nc.table("zero", other.n))
        # ---- the three calls, nothing read or finished between them
        first.queue(data, lab, alpha_max)
        if step % 3 == 0:
            ctx.count_neighbours(ostats, other.n, odata, other.r)
        elif step % 3 == 1:
            ctx.label_components(other.n, odata, other.r, labels=olabels)
        else:
            ctx.spatial_order(osrc, 70_001, stride=16, order_index=oindex)
        second.queue(data, lab, alpha_max)
        # ---- only now
        got2, bytes2 = second.read(gs4d, f"{what}, again")
        got1, bytes1 = first.read(gs4d, what)
        mc.assert_device_equals_host(what, got1, host)
        mc.assert_device_equals_host(f"{what}, again", got2, host)
        assert bytes2 == bytes1, f"{what}: the second merge differs from the first"
        if step % 3 == 0:
            assert ctx.read(ostats, nc.STAT, other.n).tobytes() == want_counts.tobytes(), f"{what}: count_neighbours between the merges"
        elif step % 3 == 1:
            assert np.array_equal(ctx.read(olabels, u32, other.n), want_labels) and mc.untouched(ctx, olabels, 16, offset=4 * other.n), f"{what}: label_components between the merges"
        else:
            assert np.array_equal(ctx.read(oindex, u32, 70_001), want_order) and mc.untouched(ctx, oindex, 16, offset=4 * 70_001), f"{what}: spatial_order between the merges"
        assert mc.same_bytes(ctx, data, rec) and mc.same_bytes(ctx, lab, labels), f"{what}: an input changed"
        first.delete()
        second.delete()
        for b in (data, lab, olabels, oindex):
            ctx.delete(b)
    ctx.finish()                                                                      # reports device-side check failures
    ctx.close()
