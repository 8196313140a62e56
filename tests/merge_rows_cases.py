"""What the tests of gs4d_merge_rows and gs4d_copy_rows share (include/gs4d.h): the header's text restated in numpy — float64 sums in
eight explicit slots and the fixed tree, every operation rounded on its own — tables with NaN in their padding, groupings with group sizes around
the eight lanes of a sub-group, and the inputs of the degree-0 consistency test with their premise checked here, on the CPU."""
import numpy as np

import merge_cases as mc
import transform_cases as tc

f32, f64, u32 = np.float32, np.float64, np.uint32
ID_NONE = mc.ID_NONE
SLOTS = 8
CHUNK = 8                                                     # words of a row one sub-group of the device reduces (csrc/merge_rows.hip)
GROUP_SIZES = (1, 2, 7, 8, 9, 16, 17, 65)
# (width, stride): every width and every stride of the issue; widths on and either side of a 16-byte piece (3, 4, 5), below and above one chunk
# (5, 12), whole chunks (48, 64, 256), chunks and a part (27: 8, 8, 8, 3), padding inside the last piece (27), whole pieces and whole chunks of
# padding (208, 1024)
SHAPES = ((1, 16), (3, 16), (4, 16), (5, 48), (12, 48), (27, 112), (48, 192), (48, 208), (64, 1024), (256, 1024))
# more widths for the device: on the chunk and one word either side of it, and one word above two chunks
CHUNK_SHAPES = ((7, 32), (8, 32), (9, 48), (17, 80))
PATTERN = 0xA5


def bits(a):
    return np.ascontiguousarray(a).view(u32)


def grouping(sizes, step=1, first=0, seed=0, none=0):
    """member_group of sum(sizes) + none records: group j has sizes[j] members and the value first + step * j, `none` records have ID_NONE, all
    shuffled through the set by one fixed permutation"""
    mg = np.concatenate([np.full(s, first + step * j, u32) for j, s in enumerate(sizes)] + [np.full(none, ID_NONE, u32)])
    return mg[np.random.default_rng(0x4D52 + seed).permutation(mg.size)]


def table(n, width, stride, seed=0, padding=np.nan):
    """float32 [n, stride / 4]: words below width at random (a few exact zeros, negative zeros and denormals among them), the padding NaN"""
    rng = np.random.default_rng(0x5442 + seed)
    t = np.full((n, stride // 4), padding, f32)
    t[:, :width] = rng.normal(0.0, 1.0, (n, width)).astype(f32)
    if n > 4:
        t[rng.integers(0, n, max(1, n // 9)), rng.integers(0, width)] = [0.0, -0.0, 1e-42][seed % 3]
    return t


def records(gs4d, n, seed=0):
    """n clean 4d_vel records that are all members by their mass, taken round and round from a pool"""
    pool = tc.records(gs4d, "4d_vel", max(64, min(n, 3000)), seed=0x5452 + seed)
    pool = pool[mc.members_of(pool, np.zeros(pool.shape[0], u32))]
    assert pool.shape[0] > 32
    return np.ascontiguousarray(np.resize(pool, (n, 24)))


def members_of(tab, member_group, width, rec=None):
    m = (np.asarray(member_group, u32) != ID_NONE) & np.isfinite(tab[:, :width]).all(1)
    return m if rec is None else m & mc.members_of(rec, np.zeros(len(member_group), u32))


def merged_row(rows, a):
    """words [width] of a group of two or more members: rows [k, width] float32 in ascending record index, a [k] float32"""
    a = a.astype(f64)
    terms = np.concatenate([a[:, None], a[:, None] * rows.astype(f64)], 1)           # what member k adds to W and R
    width = rows.shape[1]
    # slot s adds members s, s + 8, ... to +0.0 one after the other (cumsum is sequential); an empty slot stays +0.0
    slot = [np.cumsum(np.vstack([np.zeros((1, width + 1)), terms[s::SLOTS]]), axis=0)[-1] for s in range(SLOTS)]
    total = ((slot[0] + slot[1]) + (slot[2] + slot[3])) + ((slot[4] + slot[5]) + (slot[6] + slot[7]))
    return (total[1:] / total[0]).astype(f32)


def by_the_text(tab, member_group, width, rec=None, dst=None, dst_first=0):
    """(dst as uint32 [capacity, stride / 4], (groups, written, members, left_out)): the header's text over tab float32 [n, stride / 4];
    dst: the table the call finds (default: zeros with room for every group)"""
    tab, mg = np.ascontiguousarray(tab, f32), np.asarray(member_group, u32)
    n, words = tab.shape
    idx = np.flatnonzero(members_of(tab, mg, width, rec))
    idx = idx[np.argsort(mg[idx], kind="stable")]
    if dst is None:
        dst = np.zeros((dst_first + (int(mg[idx].max()) + 1 if idx.size else 0), words), u32)
    out = np.array(bits(dst), copy=True).reshape(-1, words)
    a = mc.mass(rec) if rec is not None else np.ones(n, f32)
    heads = np.flatnonzero(np.r_[True, mg[idx][1:] != mg[idx][:-1]]) if idx.size else np.zeros(0, np.int64)
    written = 0
    for lo, hi in zip(heads, np.r_[heads[1:], idx.size]):
        who, row = idx[lo:hi], dst_first + int(mg[idx[lo]])
        if row >= out.shape[0]:
            continue
        written += 1
        out[row] = 0
        out[row, :width] = bits(tab[who[0], :width]) if who.size == 1 else bits(merged_row(tab[who, :width], a[who]))
    return out, (heads.size, written, idx.size, n - idx.size)


def count_tuple(c):
    return tuple(int(c[k]) for k in ("groups", "written", "members", "left_out"))


# ---- the degree-0 consistency test -------------------------------------------------------------------------------------------------------------------
C0 = f32(0.28209479177387814)


def degree0_case(gs4d, n=700, seed=5):
    """(records [n, 24], labels uint32 [n], sh rows uint8 [n, 16]) of a clean set whose DC coefficients keep every degree-0 colour of gs4d_shade_sh in
    [0.1, 0.9], so its clamp never acts — checked here — in groups of 1 to a few dozen members"""
    rec = records(gs4d, n, seed)
    rng = np.random.default_rng(0x4430 + seed)
    dc = rng.uniform(-1.4, 1.4, (n, 3)).astype(f32)
    colour = (C0 * dc + f32(0.5)).astype(f32)
    assert colour.dtype == f32 and (colour >= 0.1).all() and (colour <= 0.9).all(), "the premise: the clamp of gs4d_shade_sh never acts"
    labels = mc.mixed_labels(n, seed)
    return rec, labels, gs4d.sh_rows(dc, None, 0)


def degree0_colour(rows16):
    """the colour gs4d_shade_sh gives at degree 0 for rows uint8 [m, 16], by the header's text"""
    dc = np.ascontiguousarray(rows16).view(f32).reshape(-1, 4)[:, :3]
    v = (C0 * dc).astype(f32) + f32(0.5)
    return np.where(v > 0, v, f32(0)).astype(f32)
