"""What the tests of gs4d_lod_append and gs4d_lod_cut share (include/gs4d.h): the header's text restated in numpy — float32, one numpy
call per operation, which rounds each on its own — forests over the record sets of transform_cases with level sizes around the tiles of the
kernels, parent words of every kind, and the device calls between guard buffers."""
import numpy as np

import centre_cases as cc
import transform_cases as tc

f32, u32, u8 = np.float32, np.uint32, np.uint8
ID_NONE = 0xFFFFFFFF
STOP, DESCEND, DRAW = 0, 1, 2
LOD_TILE = 1024                                              # nodes per workgroup of the level kernel (gs4d_internal.h), 4 rounds of 256 threads
LOD_THREADS = 256
COMPACT_TILE = 2048
SETS = tc.SETS                                               # the clean 3D, 4D_VEL and 4D_2Q sets and the hostile set
LEAVES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)
LEVELS = (1, 2, 5, 16)
SENTINEL = 0xA5
GUARD = 4096
T = 0.75
EYE = (3.0, -2.0, 40.0)


def bits(a):
    return np.ascontiguousarray(a).view(u32)


# ---- the header's text -------------------------------------------------------------------------------------------------------------------------
def fine_by_the_text(rec, eye, t, ratio, near):
    """bool [n]: float32, every product and sum rounded on its own"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    m, _, _ = cc.centre(rec, t)
    with np.errstate(all="ignore"):
        dx, dy, dz = m[:, 0] - f32(eye[0]), m[:, 1] - f32(eye[1]), m[:, 2] - f32(eye[2])
        dist2 = np.add(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(dz, dz))
        n2 = np.multiply(f32(near), f32(near))
        e = np.where(dist2 > n2, dist2, n2)                                    # (a NaN distance: near)
        v = rec[:, 8]
        v = np.where(rec[:, 13] > v, rec[:, 13], v)
        v = np.where(rec[:, 18] > v, rec[:, 18], v)
        r2 = np.multiply(f32(ratio), f32(ratio))
        out = v <= np.multiply(r2, e)
    assert dist2.dtype == f32 and e.dtype == f32 and v.dtype == f32
    return out


def states_by_the_text(rec, parent, level_first, eye, t, ratio, near):
    """(state uint8 [n], tested): the levels from the top down"""
    parent, n = np.asarray(parent, u32), int(level_first[-1])
    fine = fine_by_the_text(rec, eye, t, ratio, near) if n else np.zeros(0, bool)
    state, tested = np.full(n, STOP, u8), 0
    for k in range(len(level_first) - 2, -1, -1):
        i = np.arange(level_first[k], level_first[k + 1])
        p = parent[i].astype(np.int64)
        child = (p >= level_first[k + 1]) & (p < n)
        test = ~child | (state[np.where(child, p, 0)] == DESCEND)
        leaf = i < level_first[1]
        state[i] = np.where(test, np.where(leaf | fine[i], DRAW, DESCEND), STOP)
        tested += int(test.sum())
    return state, tested


def cut_by_the_text(rec, parent, level_first, eye, t, ratio, near=0.0, capacity=None, stats=None):
    """(dst [written, 24], cut_index [written], stats table or None, (drawn, written, tested, drawn_leaves), state)"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    state, tested = states_by_the_text(rec, parent, level_first, eye, t, ratio, near)
    index = np.flatnonzero(state == DRAW).astype(u32)
    drawn = index.size
    written = drawn if capacity is None else min(drawn, capacity)
    table = None
    if stats is not None:
        table = np.array(stats, copy=True).view(cc.STAT)
        table["pixels"][index] += u32(1)
        table["wmax"][index] = np.maximum(table["wmax"][index], cc.ONE_BITS)
        table["wsum"][index] += np.uint64(1 << 24)
    return rec[index[:written]], index[:written], table, (drawn, written, tested, int((index < level_first[1]).sum())), state


def chains_draw_once(parent, level_first, state):
    """the property of the header: on every chain of valid parent links from a leaf, exactly one node is DRAW.  Returns the number of leaves."""
    parent, n = np.asarray(parent, np.int64), int(level_first[-1])
    level = np.searchsorted(np.asarray(level_first[1:]), np.arange(n), side="right")
    nxt = np.asarray(level_first)[level + 1]
    child = (parent >= nxt) & (parent < n)
    at = np.arange(level_first[1])
    seen = (state[at] == DRAW).astype(np.int64)
    alive = np.ones(at.size, bool)
    for _ in range(len(level_first)):
        alive &= child[at]
        at = np.where(alive, parent[at], at)
        seen += alive & (state[at] == DRAW)
    assert (seen == 1).all(), f"{int((seen != 1).sum())} chains with {sorted(set(seen.tolist()))} DRAW nodes"
    return int(level_first[1])


# ---- forests -----------------------------------------------------------------------------------------------------------------------------------
def level_sizes(leaves, levels, fan=3):
    """the leaves, then each level about 1 / fan of the one below, at least one node — except level 2 of a forest of five or more, which is empty"""
    sizes = [leaves]
    for k in range(1, levels):
        sizes.append(max(1, -(-sizes[-1] // fan)))
    if levels >= 5:
        sizes[2] = 0
    return sizes


def firsts(sizes):
    return [0] + np.cumsum(sizes).tolist()


def random_forest(gs4d, which, leaves, levels, seed=0, fan=3):
    """(rec [N, 24], parent [N], level_first): records of a set in every level, so the extents grow towards the roots on some chains and not on
    others; a parent in the next level that has nodes, about one node in eight a level further up, about one in sixteen a root"""
    rng = np.random.default_rng(0x4C4F + seed + 131 * leaves + levels)
    sizes = level_sizes(leaves, levels, fan)
    first = firsts(sizes)
    N = first[-1]
    rec = tc.records(gs4d, which, N, seed=0x4C4F + seed).copy()
    parent = np.full(N, ID_NONE, u32)
    for k in range(levels - 1):
        above = [j for j in range(k + 1, levels) if sizes[j]]
        if not above:
            break
        for i in range(first[k], first[k + 1]):
            j = above[1] if len(above) > 1 and rng.random() < 0.125 else above[0]
            parent[i] = first[j] + int(rng.integers(0, sizes[j]))
    parent[rng.random(N) < 1.0 / 16] = ID_NONE
    return rec, parent, first


def middle_ratio(rec, eye, t):
    """a ratio at which about half of the records with usable numbers are fine"""
    rec = np.ascontiguousarray(rec, f32)
    m, _, _ = cc.centre(rec, t)
    with np.errstate(all="ignore"):
        d2 = ((m - np.asarray(eye, f32)) ** 2).sum(1).astype(np.float64)
        q = np.sqrt(rec[:, [8, 13, 18]].max(1).astype(np.float64) / d2)
    q = q[np.isfinite(q) & (q > 0)]
    return float(np.median(q)) if q.size else 1.0


def sized_record(gs4d, n, var, seed=0):
    """n clean 3D records whose three rest variances are `var` (a number or n of them)"""
    rec = tc.records(gs4d, "3d", n, seed=0x535A + seed).copy()
    rec[:, 8] = rec[:, 13] = rec[:, 18] = np.asarray(var, f32)
    return rec


SMALL, LARGE = 1e-20, 1e20                                   # a variance that is fine / not fine at ratio 1 from any distance the clean sets have


def skipped_wave_forest(gs4d, children=2 * LOD_TILE + 300, lanes=(0, 63, 64, 255, 256, 1023, 1024, 1087, 2 * LOD_TILE + 299), roots=70, fill=False):
    """three levels: level 2 holds `roots` roots, all DRAW at ratio 1 except root 5, which is DESCEND; level 1 holds
    `children` nodes, all children of DRAW roots (STOP) except those at the offsets `lanes`, children of root 5 — single tested lanes at lanes 0 and 63
    of a wave, either side of a round of 256 and of a workgroup's tile of 1024; fill: also the whole second wave of the second tile.  Level 0 holds
    one leaf under every node of level 1."""
    lanes = sorted(set(lanes) | (set(range(LOD_TILE + 64, LOD_TILE + 128)) if fill else set()))
    first = firsts([children, children, roots])
    rec = np.concatenate([sized_record(gs4d, children, SMALL, 1), sized_record(gs4d, children, LARGE, 2), sized_record(gs4d, roots, SMALL, 3)])
    rec[first[2] + 5, [8, 13, 18]] = LARGE
    parent = np.full(first[-1], ID_NONE, u32)
    parent[first[1]:first[2]] = first[2] + (np.arange(children) % (roots - 6)) + 6            # roots 6 ..: DRAW
    parent[first[1] + np.asarray(lanes)] = first[2] + 5
    parent[:children] = first[1] + np.arange(children)
    return rec, parent, first, lanes


def hostile_parent_forest(gs4d):
    """three levels of 300, 40 and 6 nodes, every node not fine at ratio 1 (so every valid link is followed to the leaves) and parent words of every
    kind: itself, a lower level, its own level, N, N - 1 in the top level, GS4D_ID_NONE, a child that skips a level"""
    first = firsts([300, 40, 6])
    N = first[-1]
    rec = sized_record(gs4d, N, LARGE, 4)
    parent = np.full(N, ID_NONE, u32)
    parent[:300] = first[1] + np.arange(300) % 40
    parent[first[1]:first[2]] = first[2] + np.arange(40) % 6
    parent[0:7] = (0, 299, N, N - 1, ID_NONE, first[2] + 2, 0xFFFFFFFE)          # itself, its own level, N, a node two levels up (twice: N - 1 is one), none, past the end
    parent[first[1]:first[1] + 6] = (first[1], 17, first[1] + 39, N, N - 1, ID_NONE)      # itself, a lower level, its own level, N, the last root, none
    parent[first[2]:] = (first[2], N - 1, N, 5, first[1], ID_NONE)               # the top level: itself, N - 1, N, lower levels, none — all roots
    return rec, parent, first


# ---- the device --------------------------------------------------------------------------------------------------------------------------------
def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD, offset=0):
    return bool((ctx.read(buf, np.uint8, nbytes, offset=offset) == SENTINEL).all())


def same_bytes(ctx, buf, a):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return np.array_equal(ctx.read(buf, np.uint8, a.size), a)


def device_call(gs4d, ctx, rec, parent, query, what, cap_dst=None, cap_index=None, with_dst=True, with_index=True, stats=None):
    """One gs4d_lod_cut call between guard buffers: returns (dst [written, 24] or None, cut_index [written] or None, the table or None, count), after
    checking that slots at or beyond the capacity, the guards and the inputs hold the bytes that were uploaded.  cap_dst / cap_index: slots the two
    buffers hold (default n + 3: more than any call can write)."""
    n = rec.shape[0]
    cap_dst = n + 3 if cap_dst is None else cap_dst
    cap_index = n + 3 if cap_index is None else cap_index
    guards = [fill(ctx, GUARD)]
    nodes = ctx.buffer(rec) if n else fill(ctx, 96)
    par = ctx.buffer(np.ascontiguousarray(parent, u32)) if n else fill(ctx, 16)
    guards.append(fill(ctx, GUARD))
    dst = fill(ctx, cap_dst * 96 + 32) if with_dst else None
    guards.append(fill(ctx, GUARD))
    index = ctx.buffer(np.full(cap_index * 4 + 3, SENTINEL, np.uint8)) if with_index else None      # (less than a slot behind the last one: the capacity is bytes / 4)
    table = ctx.buffer(stats) if stats is not None else None
    guards.append(fill(ctx, GUARD))
    count = fill(ctx, 32)
    guards.append(fill(ctx, GUARD))
    forest = gs4d.LodForest(nodes, par, [int(query.level_first[k]) for k in range(int(query.levels) + 1)])
    assert forest.n == n
    assert ctx.lod_cut(forest, None, None, None, dst=dst, cut_index=index, stats=table, count=count, query=query) == count
    c = ctx.read_lod_count(count)
    cap = min([0xFFFFFFFF] + ([cap_dst] if with_dst else []) + ([cap_index] if with_index else []))
    assert int(c["written"]) == min(int(c["drawn"]), cap), f"{what}: written {c['written']} of {c['drawn']} drawn, capacity {cap}"
    w = int(c["written"])
    assert untouched(ctx, count, 16, offset=16), f"{what}: bytes behind the count changed"
    out = idx = after = None
    if with_dst:
        assert untouched(ctx, dst, (cap_dst - w) * 96 + 32, offset=w * 96), f"{what}: slots of dst at or beyond the capacity changed"
        out = ctx.read(dst, f32, w * 24).reshape(w, 24)
    if with_index:
        assert untouched(ctx, index, (cap_index - w) * 4 + 3, offset=w * 4), f"{what}: slots of cut_index at or beyond the capacity changed"
        idx = ctx.read(index, u32, w)
    if stats is not None:
        after = ctx.read(table, np.uint8, 16 * n).view(cc.STAT)
    assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
    if n:
        assert same_bytes(ctx, nodes, rec) and same_bytes(ctx, par, np.ascontiguousarray(parent, u32)), f"{what}: an input changed"
    for b in guards + [nodes, par, count] + [b for b in (dst, index, table) if b is not None]:
        ctx.delete(b)
    return out, idx, after, c


def assert_device_equals_host(what, got, host):
    """the outputs of device_call against lod_cut_host's at the same capacity, as uint32 words"""
    out, idx, after, c = got
    hdst, hidx, hstats, hc = host
    assert tuple(int(v) for v in c) == tuple(int(v) for v in hc), f"{what}: count {c} against {hc}"
    w = int(hc["written"])
    if out is not None:
        assert out.shape[0] == w and np.array_equal(bits(out), bits(np.ascontiguousarray(hdst[:w]))), f"{what}: dst"
    if idx is not None:
        assert np.array_equal(idx, hidx[:w]), f"{what}: cut_index"
    if after is not None:
        assert np.array_equal(after.view(u32), np.ascontiguousarray(hstats).view(u32)), f"{what}: stats"


def check(gs4d, ctx, rec, parent, first, what, eye=EYE, t=T, ratio=1.0, near=0.0, stats=None, **kw):
    """device against host for one call; returns the host's outputs"""
    q = gs4d.lod_query(first, eye, t, ratio, near)
    got = device_call(gs4d, ctx, rec, parent, q, what, stats=stats, **kw)
    caps = [rec.shape[0] + 3]
    caps += [kw["cap_dst"]] if kw.get("with_dst", True) and kw.get("cap_dst") is not None else []
    caps += [kw["cap_index"]] if kw.get("with_index", True) and kw.get("cap_index") is not None else []
    cap = min(caps)
    host = gs4d.lod_cut_host(rec, parent, q, capacity=cap, stats=stats)
    assert_device_equals_host(what, got, host)
    return host


def stats_table(gs4d, n, seed=0):
    """a non-zero RECORD_STAT table: rows of several fragments, rows whose wmax is above and below the bits of 1.0f, wsum next to a carry"""
    rng = np.random.default_rng(0x4C53 + seed)
    st = np.zeros(n, gs4d.RECORD_STAT)
    st["pixels"] = rng.integers(0, 5, n)
    st["wmax"] = rng.choice(np.array([0.0, 0.5, 1.0, 1.5], f32), n)
    st["wsum"] = rng.choice(np.array([0, 1 << 24, 0xFFFFFFFF, 0xFFFFFFFFFF000000], np.uint64), n)
    return st


def device_append(gs4d, ctx, level, member_group, m, c, first, child_first, total, what):
    """One gs4d_lod_append call into sentinel-filled forest buffers of `total` nodes between guard buffers: returns (nodes bytes [total, 96], parent
    bytes [total, 4]) after checking the guards, the bytes behind the buffers and the inputs."""
    guards = [fill(ctx, GUARD)]
    lev = ctx.buffer(level) if level.size else fill(ctx, 96)
    mg = None if member_group is None else (ctx.buffer(member_group) if member_group.size else fill(ctx, 16))
    guards.append(fill(ctx, GUARD))
    nodes, parent = fill(ctx, total * 96 + 32), fill(ctx, total * 4 + 12)
    guards.append(fill(ctx, GUARD))
    ctx.lod_append(lev, m, nodes, parent, first, member_group=mg, child_first=child_first, c=c)
    got_nodes = ctx.read(nodes, np.uint8, total * 96).reshape(total, 96)
    got_parent = ctx.read(parent, np.uint8, total * 4).reshape(total, 4)
    assert untouched(ctx, nodes, 32, offset=total * 96) and untouched(ctx, parent, 12, offset=total * 4), f"{what}: bytes behind the forest changed"
    assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
    assert not level.size or same_bytes(ctx, lev, level), f"{what}: level changed"
    assert member_group is None or not member_group.size or same_bytes(ctx, mg, member_group), f"{what}: member_group changed"
    for b in guards + [lev, nodes, parent] + ([mg] if mg is not None else []):
        ctx.delete(b)
    return got_nodes, got_parent


def append_by_the_text(level, member_group, m, c, first, child_first, total):
    """the same two arrays from the header's text"""
    nodes, parent = np.full((total, 96), SENTINEL, np.uint8), np.full(total, 0xA5A5A5A5, u32)
    nodes[first:first + m] = np.ascontiguousarray(level[:m]).view(np.uint8).reshape(m, 96)
    parent[first:first + m] = ID_NONE
    if member_group is not None:
        g = member_group[:c].astype(np.int64)
        parent[child_first:child_first + c] = np.where(g < m, first + g, ID_NONE).astype(u32)
    return nodes, parent.view(np.uint8).reshape(total, 4)
