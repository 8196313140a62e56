"""What the tests of gs4d_cell_labels and gs4d_merge_records share (include/gs4d.h): the header's text restated in numpy — float32 for
area_time, mass and the cell, float64 for the sums of a group, every operation rounded on its own, which numpy's add, multiply, divide and sqrt do
correctly — labellings with group sizes and group counts around the edges of the kernel (a sub-group of 8 lanes, a wave of 8 groups, a workgroup of
32), statistics tables, grids, and the comparison of four outputs as uint32 words."""
import numpy as np

import transform_cases as tc

f32, f64, u32 = np.float32, np.float64, np.uint32
ID_NONE = 0xFFFFFFFF
SLOTS = 8                                                     # interleaved partial sums of a group; lanes of a sub-group
GROUPS_PER_WAVE, GROUPS_PER_WORKGROUP = 8, 32
MERGE_TILE = 2048                                            # sorted keys per workgroup of the head kernels (gs4d_internal.h)
SETS = tc.SETS                                               # the clean 3D, 4D_VEL and 4D_2Q sets and the hostile set
SIZES = (1, 9, 257, 769, 2049, 4100)                         # one record; a group and one; either side of tiles of 256 and 2048; two tiles of 2048 and more
EDGE_SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000)   # members per group: the slots, two rounds, a wave's worth of members and many
EDGE_COUNTS = (1, 7, 8, 9, 31, 32, 33)                       # groups per call: the sub-group, wave and workgroup edges
SENTINEL = 0xA5
GUARD = 4096


def bits(a):
    return np.ascontiguousarray(a).view(u32)


# ---- labellings -------------------------------------------------------------------------------------------------------------------------------
def mixed_labels(n, seed=0):
    """n labels for the CPU comparison: groups of 1 to a few dozen members interleaved through the set, singletons with large labels (0xFFFFFFFE
    among them), label 0, and every 11th record without a label"""
    rng = np.random.default_rng(0x4D47 + seed)
    small = max(1, n // 6)
    lab = rng.integers(0, small, n).astype(u32) * u32(3)                      # about 6 members per label on average, far apart in memory
    lab[rng.random(n) < 0.25] = 0 if seed % 2 == 0 else 5                     # one crowded group: more than 8 members from n = 40 up
    single = np.flatnonzero(rng.random(n) < 0.1)
    lab[single] = (0xFFFFFFFE - np.arange(single.size)).astype(u32)           # groups of one, in descending label as the index ascends
    lab[np.arange(n) % 11 == 10] = ID_NONE
    return lab


def sized_labels(sizes, first_label=0, step=3, seed=1):
    """labels of sum(sizes) records: group j has sizes[j] members and the label first_label + step * j (the last one 0xFFFFFFFE when there are at
    least two), the members of all groups shuffled through the set by one fixed permutation — far apart in memory, in no order of label"""
    lab = np.concatenate([np.full(s, first_label + step * j, u32) for j, s in enumerate(sizes)])
    if len(sizes) > 1:
        lab[lab == lab[-1]] = 0xFFFFFFFE
    return lab[np.random.default_rng(0x5A5A + seed).permutation(lab.size)]


def stats_table(gs4d, n, seed=0):
    """a RECORD_STAT table whose rule min_pixels = 1 passes about two rows in three"""
    st = np.zeros(n, gs4d.RECORD_STAT)
    st["pixels"] = np.random.default_rng(0x5354 + seed).integers(0, 3, n)
    st["wmax"], st["wsum"] = 1.0, st["pixels"].astype(np.uint64) << np.uint64(24)
    return st


def passes(stats, min_pixels=1, invert=False):
    return (stats["pixels"] >= min_pixels) != invert


# ---- past one round of the scan ------------------------------------------------------------------------------------------------------------------
# k_merge_scan (csrc/merge.hip) is ONE workgroup of 1024 threads that walks the per-tile head counts in rounds of 1024 words; the groups of the
# earlier rounds travel in one LDS word.
SCAN_THREADS = 1024
ROUND = SCAN_THREADS * MERGE_TILE                            # sorted slots per round of the scan
ROUND_N = ROUND + MERGE_TILE + 1                             # 1026 tiles: two of them in round 2
ROUND_CASES = ("heads_in_round_2", "rule", "no_heads_in_round_2")


def round_records(gs4d):
    """ROUND_N clean 4d_vel records: a pool of a few thousand that members_of accepts, taken round and round"""
    pool = tc.records(gs4d, "4d_vel", 3000)
    pool = pool[members_of(pool, np.zeros(pool.shape[0], u32))]
    assert pool.shape[0] > 2000
    return np.ascontiguousarray(np.resize(pool, (ROUND_N, 24)))


def round_labels(case, gs4d):
    """(labels, stats table or None, rule keywords) of ROUND_N records that are all members where their label and the rule let them:
    heads_in_round_2     about ROUND_N / 7 labels, multiples of 3, at random, and one record alone with the largest label: every record is a member,
                         and the one slot of the last tile is a head;
    rule                 the random labels, 300 records without one, and a table whose rule min_pixels = 1 leaves out another 700: the members end
                         in the first tile of round 2;
    no_heads_in_round_2  the last 2 * MERGE_TILE + 501 records without a label: the non-members are a suffix of the sorted keys longer than two tiles, the
                         members end in the last tile but one of round 1."""
    n = ROUND_N
    rng = np.random.default_rng(0x524E + ROUND_CASES.index(case))
    lab = rng.integers(0, n // 7, n).astype(u32) * u32(3)
    stats, rule = None, {}
    if case == "no_heads_in_round_2":
        lab[n - (2 * MERGE_TILE + 501):] = ID_NONE
    elif case == "heads_in_round_2":
        lab[n // 3] = 0xFFFFFFFE
    if case == "rule":
        out = rng.choice(n, 1000, replace=False)
        lab[out[:300]] = ID_NONE
        stats, rule = np.zeros(n, gs4d.RECORD_STAT), {"min_pixels": 1}
        stats["pixels"], stats["wmax"], stats["wsum"] = 1, 1.0, 1 << 24
        stats["pixels"][out[300:]] = 0
    return lab, stats, rule


def assert_round_labels(case, labels, member):
    """the property the case is named for, from the stable-sorted member labels (numpy alone).  Returns the number of groups."""
    keys = np.sort(labels[member], kind="stable")
    heads = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    per_tile = np.bincount(heads // MERGE_TILE, minlength=ROUND_N // MERGE_TILE + 1)
    assert per_tile.size == SCAN_THREADS + 2 and ROUND_N - keys.size < (MERGE_TILE if case != "no_heads_in_round_2" else ROUND_N)
    assert (per_tile[:SCAN_THREADS - 1] > 0).all(), "heads in every tile of round 1 in front of its last"
    if case == "no_heads_in_round_2":
        assert keys.size == ROUND - MERGE_TILE - 500 and not per_tile[SCAN_THREADS - 1:].any(), "no member, so no head, behind tile 1022: none in round 2"
    elif case == "rule":
        assert per_tile[SCAN_THREADS] > 0 and per_tile[SCAN_THREADS + 1] == 0 and heads[-1] >= ROUND, "heads in the first tile of round 2"
    else:
        assert keys.size == ROUND_N and per_tile[SCAN_THREADS] > 0 and per_tile[SCAN_THREADS + 1] == 1 and heads[-1] == ROUND_N - 1, "heads in both tiles of round 2"
    return heads.size


# ---- the header's text -------------------------------------------------------------------------------------------------------------------------
def S(rec, c, r):
    return rec[..., 8 + 4 * c + r]


def area_time(rec):
    """float32, every product, difference and sum rounded on its own"""
    rec = np.asarray(rec, f32)
    with np.errstate(all="ignore"):
        sxx, syy, szz = S(rec, 0, 0), S(rec, 1, 1), S(rec, 2, 2)
        e2 = ((sxx * syy - S(rec, 1, 0) * S(rec, 0, 1)) + (sxx * szz - S(rec, 2, 0) * S(rec, 0, 2))) + (syy * szz - S(rec, 2, 1) * S(rec, 1, 2))
        out = np.sqrt(S(rec, 3, 3) * e2)
    assert out.dtype == f32
    return out


def mass(rec):
    with np.errstate(all="ignore"):
        return np.asarray(rec, f32)[..., 7] * area_time(rec)


def members_of(rec, labels, keep=None):
    """bool [n]: the header's four conditions"""
    rec = np.asarray(rec, f32).reshape(-1, 24)
    a = mass(rec)
    words = np.isfinite(rec[:, :7]).all(1) & np.isfinite(rec[:, 8:]).all(1)
    m = (np.asarray(labels, u32) != ID_NONE) & np.isfinite(a) & (a > 0) & words
    return m if keep is None else m & keep


TRIANGLE = [(c, r) for c in range(4) for r in range(c + 1)]                  # the stored triangle r <= c


def merged_record(group, alpha_max):
    """the record of a group of two or more members [k, 24] in ascending record index"""
    a = mass(group).astype(f64)
    origin = group[0, :4].astype(f64)
    d = group[:, :4].astype(f64) - origin
    terms = [a] + [a * d[:, r] for r in range(4)] + [a * (S(group, c, r).astype(f64) + d[:, r] * d[:, c]) for c, r in TRIANGLE] \
        + [a * group[:, 4 + j].astype(f64) for j in range(3)]
    terms = np.stack(terms, 1)                                                 # [k, 18]: what member k adds to W, M, Q, C
    # slot s adds members s, s + 8, ... to +0.0 one after the other (cumsum is sequential); an empty slot stays +0.0
    slot = [np.cumsum(np.vstack([np.zeros((1, 18)), terms[s::SLOTS]]), axis=0)[-1] for s in range(SLOTS)]
    total = ((slot[0] + slot[1]) + (slot[2] + slot[3])) + ((slot[4] + slot[5]) + (slot[6] + slot[7]))
    W, M, Q, C = total[0], total[1:5], total[5:15], total[15:18]
    out = np.zeros(24, f32)
    m = M / W
    with np.errstate(all="ignore"):                                            # (a sum of squares of 1e30 words overflows float32: inf, as on the device)
        out[:4] = (origin + m).astype(f32)
        out[4:7] = (C / W).astype(f32)
        for e, (c, r) in enumerate(TRIANGLE):
            out[8 + 4 * c + r] = out[8 + 4 * r + c] = f32(Q[e] / W - m[r] * m[c])
        v = W / f64(area_time(out))
    out[7] = f32(v) if v < f64(f32(alpha_max)) else f32(alpha_max)
    return out, W


def by_the_text(rec, labels, alpha_max=1.0, keep=None):
    """(out [groups, 24], groups [groups] of (label, size, first), member_group [n], (groups, members, left_out), W [groups]: the double mass of
    every group of two or more, 0 for a group of one)"""
    rec, labels = np.ascontiguousarray(rec, f32).reshape(-1, 24), np.asarray(labels, u32)
    n = rec.shape[0]
    idx = np.flatnonzero(members_of(rec, labels, keep))
    idx = idx[np.argsort(labels[idx], kind="stable")]                         # ascending label, ascending record index within a label
    heads = np.flatnonzero(np.r_[True, labels[idx][1:] != labels[idx][:-1]]) if idx.size else np.zeros(0, np.int64)
    ends = np.r_[heads[1:], idx.size]
    out, rows, W = np.zeros((heads.size, 24), f32), np.zeros((heads.size, 3), u32), np.zeros(heads.size, f64)
    member_group = np.full(n, ID_NONE, u32)
    for g, (a, b) in enumerate(zip(heads, ends)):
        who = idx[a:b]
        if who.size == 1:
            out[g] = rec[who[0]]
        else:
            out[g], W[g] = merged_record(rec[who], alpha_max)
        rows[g] = labels[who[0]], who.size, who[0]
        member_group[who] = g
    return out, rows, member_group, (heads.size, idx.size, n - idx.size), W


def assert_equal(what, got, want):
    """(out, groups, member_group, count) of the library (merge_records_host's return, or the same read from a device) against by_the_text's, as
    uint32 words, every word"""
    out, groups, member_group, count = got
    wout, wrows, wmg, (ng, nm, nl), _ = want
    assert (int(count["groups"]), int(count["members"]), int(count["left_out"])) == (ng, nm, nl), f"{what}: count {count} against {(ng, nm, nl)}"
    assert np.array_equal(bits(member_group), bits(wmg)), f"{what}: member_group"
    g = np.ascontiguousarray(groups[:ng])
    assert np.array_equal(np.stack([g["label"], g["size"], g["first"]], 1), wrows) and not g["reserved"].any(), f"{what}: groups"
    diff = bits(np.ascontiguousarray(out[:ng])) != bits(wout)
    assert not diff.any(), f"{what}: {int(diff.sum())} words of dst differ, first at (group, word) {tuple(np.argwhere(diff)[0])}"


# ---- grids -------------------------------------------------------------------------------------------------------------------------------------
def cell_labels_by_the_text(rec, lo, edge, dims):
    """uint32 [n]: the header's text in float32; lo, edge, dims of four entries"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    n = rec.shape[0]
    cell, none = np.zeros((4, n), np.uint64), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for a in range(4):
            if int(dims[a]) == 1:
                continue
            g = (rec[:, a] - f32(lo[a])) / f32(edge[a])
            assert g.dtype == f32
            none |= np.isnan(g)
            c = np.minimum(np.floor(g), f32(int(dims[a]) - 1))
            cell[a] = np.where(~np.isnan(g) & (g >= 0), c, 0).astype(np.uint64)
    d = [np.uint64(int(v)) for v in dims]
    lab = ((cell[3] * d[2] + cell[2]) * d[1] + cell[1]) * d[0] + cell[0]
    return np.where(none, ID_NONE, lab).astype(u32)


def grid_records(gs4d, lo, edge, dims, seed=0):
    """records whose rest means sit on cell borders, one float32 step either side of them, outside the grid on both sides, at NaN and at +-inf"""
    rng = np.random.default_rng(0x4752 + seed)
    rec = tc.records(gs4d, "4d_vel", 1200, seed=0x4752 + seed).copy()
    n = rec.shape[0]
    lo, edge = np.asarray(lo, f32), np.asarray(edge, f32)
    for a in range(4):
        k = rng.integers(-2, int(dims[a]) + 3, n).astype(f32)
        with np.errstate(all="ignore"):                                        # (an axis of one cell may have any lo and edge)
            border = (lo[a] + k * edge[a]).astype(f32)
        step = rng.integers(-1, 2, n)
        rec[:, a] = np.where(step < 0, np.nextafter(border, f32(-np.inf)), np.where(step > 0, np.nextafter(border, f32(np.inf)), border))
        inside = rng.random(n) < 0.3
        rec[inside, a] = (lo[a] + rng.random(int(inside.sum())).astype(f32) * edge[a] * f32(dims[a])).astype(f32)
    for a, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (3, np.inf), (0, -np.inf), (0, 1e38), (1, -1e38)):
        rec[rng.integers(2, n, 12), a] = v
    rec[0, :4], rec[1, :4] = np.inf, -np.inf                                  # the last cell and cell 0, whatever the grid
    return rec


GRIDS = {                                                     # lo, edge, dims
    "cube":      ((-50.0, -50.0, -50.0, 0.0), (12.5, 10.0, 7.0, 2.5), (8, 10, 15, 10)),
    "static":    ((-50.0, -50.0, -50.0, 0.0), (9.0, 9.0, 9.0, np.nan), (11, 12, 13, 1)),      # dims of 1: lo and edge of that axis are not looked at
    "one_cell":  ((np.nan, 0.0, 0.0, 0.0), (0.0, -1.0, np.inf, np.nan), (1, 1, 1, 1)),
    "line":      ((-1.0, 0.0, 0.0, 0.0), (0.03125, 1.0, 1.0, 1.0), (65536, 1, 1, 1)),
    # the largest product of four factors of at most 65536 that is at most 0xFFFFFFFE: 49981 * 42966 * 2 = 0xFFFFFFFC (found by search: neither
    # 0xFFFFFFFD nor 0xFFFFFFFE = 2 * 2147483647 splits into four such factors); its last cell has the label 0xFFFFFFFB
    "largest":   ((-60.0, -60.0, -60.0, -1.0), (0.0025, 0.003, 60.0, np.inf), (49981, 42966, 2, 1)),
    "two_axes":  ((-60.0, -60.0, -60.0, -1.0), (40.0, 0.002, 30.0, 0.0004), (1, 1, 65536, 65535)),      # 0xFFFF0000 cells in z and t
}
LARGEST_CELLS = 0xFFFFFFFC
REFUSED_GRIDS = {                                             # edge, dims, reserved
    "dims 0": ((1, 1, 1, 1), (4, 0, 4, 4), (0, 0, 0, 0)),
    "dims above 65536": ((1, 1, 1, 1), (65537, 1, 1, 1), (0, 0, 0, 0)),
    "2^32 cells": ((1, 1, 1, 1), (65536, 65536, 1, 1), (0, 0, 0, 0)),
    "2 * 0xFFFFFFFC cells": ((1, 1, 1, 1), (49981, 42966, 2, 2), (0, 0, 0, 0)),
    "2 * 0xFFFF0000 cells": ((1, 1, 1, 1), (65536, 65535, 1, 2), (0, 0, 0, 0)),
    "edge 0": ((1, 0, 1, 1), (4, 4, 4, 4), (0, 0, 0, 0)),
    "edge negative": ((1, 1, -1, 1), (4, 4, 4, 4), (0, 0, 0, 0)),
    "edge inf": ((1, 1, 1, np.inf), (4, 4, 4, 4), (0, 0, 0, 0)),
    "edge nan": ((np.nan, 1, 1, 1), (4, 4, 4, 4), (0, 0, 0, 0)),
    "reserved": ((1, 1, 1, 1), (4, 4, 4, 4), (0, 0, 1, 0)),
}


def grid(gs4d, name):
    lo, edge, dims = GRIDS[name]
    return gs4d.cell_grid(lo, edge, dims), lo, edge, dims


# ---- the device --------------------------------------------------------------------------------------------------------------------------------
def fill(ctx, nbytes):
    return ctx.buffer(np.full(max(16, nbytes), SENTINEL, np.uint8))


def untouched(ctx, buf, nbytes=GUARD, offset=0):
    return bool((ctx.read(buf, np.uint8, nbytes, offset=offset) == SENTINEL).all())


def same_bytes(ctx, buf, a):
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return np.array_equal(ctx.read(buf, np.uint8, a.size), a)


def device_call(gs4d, ctx, rec, labels, what, alpha_max=1.0, stats=None, cap_dst=None, cap_groups=None, with_groups=True, with_member_group=True, **rule):
    """One gs4d_merge_records call between guard buffers: returns (out [written, 24], groups [written], member_group [n] or None, count), after
    checking that slots >= capacity of dst and groups, the guards and the inputs hold the bytes that were uploaded.  cap_dst / cap_groups: slots the
    two buffers hold (default n + 3: more than any call can write)."""
    n = rec.shape[0]
    cap_dst = n + 3 if cap_dst is None else cap_dst
    cap_groups = n + 3 if cap_groups is None else cap_groups
    guards = [fill(ctx, GUARD)]
    data = ctx.buffer(rec) if n else fill(ctx, 96)
    lab = ctx.buffer(labels) if n else fill(ctx, 16)
    guards.append(fill(ctx, GUARD))
    table = ctx.buffer(stats) if stats is not None else None
    dst = fill(ctx, cap_dst * 96 + 32)
    guards.append(fill(ctx, GUARD))
    groups = fill(ctx, cap_groups * 16 + 8) if with_groups else None
    mg = fill(ctx, 4 * n + 16) if with_member_group else None
    guards.append(fill(ctx, GUARD))
    count = fill(ctx, 32)
    guards.append(fill(ctx, GUARD))
    assert ctx.merge_records(data, n, lab, alpha_max, stats=table, dst=dst, groups=groups, member_group=mg, count=count, **rule) == (dst, count)
    c = ctx.read_merge_count(count)
    cap = min(cap_dst, cap_groups) if with_groups else cap_dst
    assert int(c["written"]) == min(int(c["groups"]), cap), f"{what}: written {c['written']} of {c['groups']} groups, capacity {cap}"
    w = int(c["written"])
    assert untouched(ctx, count, 16, offset=16), f"{what}: bytes behind the count changed"
    assert untouched(ctx, dst, (cap_dst - w) * 96 + 32, offset=w * 96), f"{what}: slots of dst at or above the capacity changed"
    out = ctx.read(dst, f32, w * 24).reshape(w, 24)
    rows = np.zeros(0, gs4d.MERGE_GROUP)
    if with_groups:
        assert untouched(ctx, groups, (cap_groups - w) * 16 + 8, offset=w * 16), f"{what}: slots of groups at or above the capacity changed"
        rows = ctx.read(groups, u32, w * 4).view(gs4d.MERGE_GROUP)
    member_group = None
    if with_member_group:
        assert untouched(ctx, mg, 16, offset=4 * n), f"{what}: bytes behind member_group changed"
        member_group = ctx.read(mg, u32, n)
    assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
    if n:
        assert same_bytes(ctx, data, rec) and same_bytes(ctx, lab, labels) and (stats is None or same_bytes(ctx, table, stats)), f"{what}: an input changed"
    for b in guards + [data, lab, dst, count] + [b for b in (table, groups, mg) if b is not None]:
        ctx.delete(b)
    return out, rows, member_group, c


def assert_device_equals_host(what, got, host, written=None):
    """the four outputs of device_call against merge_records_host's, as uint32 words; written: the capacity clamp (default: every group)"""
    out, rows, member_group, c = got
    hout, hrows, hmg, hc = host
    ng = int(hc["groups"])
    w = ng if written is None else min(ng, written)
    assert (int(c["groups"]), int(c["written"]), int(c["members"]), int(c["left_out"])) == (ng, w, int(hc["members"]), int(hc["left_out"])), f"{what}: count {c} against {hc}"
    assert out.shape[0] == w and np.array_equal(bits(out), bits(np.ascontiguousarray(hout[:w]))), f"{what}: dst"
    if rows.size or w == 0:
        assert np.array_equal(rows.view(u32), np.ascontiguousarray(hrows[:w]).view(u32)), f"{what}: groups"
    if member_group is not None:
        assert np.array_equal(member_group, hmg), f"{what}: member_group"
