"""Inputs for the gs4d_warp_records tests (include/gs4d.h): lattices of displacement nodes placed over the record sets, and the
definition restated as a numpy float32 loop of the header's text.

sets      those of tests/transform_cases.py: clean 3D, 4D_VEL and 4D_2Q sets and the hostile block.  From 255 records on, the first records of a set
          have their centres moved to the places where the cell arithmetic can go wrong: on nodes, at u == top, on each face of the lattice and just
          outside each face, on every axis that takes part.
lattices  a single node, a cube, a cell with a time axis, unequal dims (a wrong index order shows), singleton axes mixed in, and the capacity of the
          workgroup's LDS copy and one node more (the nodes then come from global memory).  The box of a lattice is laid from the set's own centres
          so that roughly half of them lie inside.
nodes     "smooth": an affine field plus a ripple, a fraction of the box in size, with a dt component; "hostile": the same with NaN, +-Inf, 1e30
          and -0 nodes implanted round and round.
clamp     no axis, every axis, time only.
"""
import os
import re

import numpy as np

import pose_cases as pc
import transform_cases as tc

f32 = np.float32
u32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERNAL = open(os.path.join(ROOT, "4dgaussiansplatrendering_amd", "csrc", "gs4d_internal.h")).read()
TILE = int(re.search(r"constexpr uint32_t WARP_TILE = (\d+);", INTERNAL).group(1))
LDS_NODES = int(re.search(r"constexpr uint32_t WARP_LDS_NODES = (\d+);", INTERNAL).group(1))
EDGE = LDS_NODES or 512                                      # (a build that ships the global gather sets the constant to 0)
SETS = tc.SETS
SIZES = tc.SIZES + (6 * TILE + 1,)                           # one record, either side of a tile, three tiles plus one, seven tiles with a short last one
DIMS = ((1, 1, 1, 1), (2, 2, 2, 1), (2, 2, 2, 2), (3, 2, 4, 5), (1, 3, 1, 2), (EDGE, 1, 1, 1), (EDGE + 1, 1, 1, 1))
CLAMPS = {"none": 0, "all": 0xF, "time": 8}
KINDS = ("smooth", "hostile")
FAULTS = (np.nan, np.inf, -np.inf, 1e30, -0.0)
bits, same_bits = tc.bits, tc.same_bits


# ---- lattices ------------------------------------------------------------------------------------------------------------------------------------
def count_of(dims):
    return int(dims[0]) * int(dims[1]) * int(dims[2]) * int(dims[3])


def box_of(rec, dims):
    """(lo, hi) per axis from the finite centres of a set: the quantiles that leave, over the axes that take part, roughly half the centres inside"""
    p = np.asarray(rec, np.float64).reshape(-1, 24)[:, :4]
    axes = sum(d >= 2 for d in dims)
    cut = (1.0 - 0.5 ** (1.0 / max(axes, 1))) / 2.0
    lo, hi = np.zeros(4), np.ones(4)
    for a in range(4):
        v = p[:, a][np.isfinite(p[:, a]) & (np.abs(p[:, a]) < 1e6)]
        if v.size:
            lo[a], hi[a] = np.quantile(v, cut), np.quantile(v, 1.0 - cut)
        if not hi[a] - lo[a] > 1e-3:                         # (one record, or a static set on the time axis: a box of its own around the centres)
            lo[a], hi[a] = lo[a] - 1.0, lo[a] + 1.0
    return lo, hi


def lattice_for(gs4d, rec, dims, clamp=0):
    lo, hi = box_of(rec, dims)
    return gs4d.lattice(lo, hi, dims, "".join(ch for a, ch in enumerate("xyzt") if clamp >> a & 1))


def nodes_for(gs4d, lat, kind="smooth", seed=0):
    """[count, 4] float32 displacements: an affine field with a shear, a velocity column and a retiming, plus a ripple — some tenths of the box"""
    rng = np.random.default_rng([0x5741, seed])
    pts = gs4d.lattice_points(lat).reshape(-1, 4).astype(np.float64)
    dims = tuple(lat.dims)
    size = np.array([(dims[a] - 1) / lat.inv[a] if dims[a] >= 2 else 1.0 for a in range(4)])
    mid = np.array(lat.lo) + 0.5 * size * np.array([d >= 2 for d in dims])
    q = (pts - mid) / size
    M = rng.uniform(-0.3, 0.3, (4, 4))
    d = (q @ M.T + 0.1 * np.sin(6.0 * q[:, ::-1] + rng.uniform(0.0, 6.0, 4)) + rng.uniform(-0.2, 0.2, 4)) * size
    d = d.astype(f32)
    if kind == "hostile":
        at = rng.permutation(d.size)[:max(1, d.size // 7)]
        d.reshape(-1)[at] = np.array(FAULTS, f32)[(np.arange(at.size) + seed) % len(FAULTS)]
    return np.ascontiguousarray(d)


def u_of(p, lat, a):
    """u of the header's text for the coordinates p on axis a, in float32"""
    with np.errstate(all="ignore"):
        return (np.asarray(p, f32) - f32(lat.lo[a])) * f32(lat.inv[a])


def special_centres(gs4d, lat):
    """[k, 4] float32: the middle of the box with one coordinate moved, per axis that takes part, onto the first face, just in front of it, to
    u == top and just behind it; then a few centres on nodes"""
    dims = tuple(lat.dims)
    mid = np.array([lat.lo[a] + (0.5 * (dims[a] - 1) / lat.inv[a] if dims[a] >= 2 else 0.0) for a in range(4)], f32)
    out = []
    for a in range(4):
        if dims[a] < 2:
            continue
        top = f32(dims[a] - 1)
        last = f32(np.float64(lat.lo[a]) + (dims[a] - 1) / np.float64(lat.inv[a]))
        for _ in range(64):                                  # the coordinate whose u is top exactly, if float32 has one near by
            u = u_of(last, lat, a)
            if u == top:
                break
            last = np.nextafter(last, f32(-np.inf) if u > top else f32(np.inf))
        behind = last
        for _ in range(64):
            behind = np.nextafter(behind, f32(np.inf))
            if u_of(behind, lat, a) > top:
                break
        for v in (f32(lat.lo[a]), np.nextafter(f32(lat.lo[a]), f32(-np.inf)), last, behind):
            c = mid.copy()
            c[a] = v
            out.append(c)
    pts = gs4d.lattice_points(lat).reshape(-1, 4)
    out.extend(pts[np.unique(np.linspace(0, pts.shape[0] - 1, 8).astype(int))])
    return np.ascontiguousarray(np.stack(out), f32)


def records_for(gs4d, which, n, lat):
    """the set, its first records moved to the special centres of the lattice once there is room for them beside as many ordinary records"""
    rec = tc.records(gs4d, which, n).copy()
    sp = special_centres(gs4d, lat)
    if n >= 2 * sp.shape[0]:
        rec[:sp.shape[0], :4] = sp
    return rec


def calls(gs4d, which, sizes=SIZES):
    """(what, rec, nodes, lat) over every size, lattice and clamp mask of a set; the node values alternate between smooth and hostile"""
    call = 0
    for n in sizes:
        base = tc.records(gs4d, which, n)
        for dims in DIMS:
            for cname, clamp in CLAMPS.items():
                lat = lattice_for(gs4d, base, dims, clamp)
                kind = KINDS[call % 2]
                nodes = nodes_for(gs4d, lat, kind, call)
                rec = records_for(gs4d, which, n, lat)
                call += 1
                yield f"{which}, n = {n}, dims {dims}, clamp {cname}, {kind} nodes", rec, nodes, lat


# ---- the equal-node property, lattices that are refused --------------------------------------------------------------------------------------------
def doubled(nodes, dims, a):
    """the nodes of a lattice with one node on axis a, with two equal nodes there: (nodes, dims)"""
    grid = np.asarray(nodes, f32).reshape(dims[3], dims[2], dims[1], dims[0], 4)
    assert dims[a] == 1
    two = np.repeat(grid, 2, axis=3 - a)
    return np.ascontiguousarray(two.reshape(-1, 4)), tuple(2 if b == a else d for b, d in enumerate(dims))


def equal_node_pairs(gs4d, rec):
    """(what, nodes, lat, nodes2, lat2): a lattice with one node on an axis, and the same with two equal nodes there — once with a box that holds
    every finite centre on that axis, once clamped there"""
    p = rec[:, :4].astype(np.float64)
    p = p[(np.isfinite(p) & (np.abs(p) < 1e6)).all(1)]
    for dims, a in (((3, 1, 4, 1), 1), ((3, 2, 1, 1), 3), ((1, 3, 2, 2), 0)):
        one = lattice_for(gs4d, rec, dims)
        nodes = nodes_for(gs4d, one, "smooth", a)
        assert not (bits(nodes) == 0x80000000).any() and np.isfinite(nodes).all()
        nodes2, dims2 = doubled(nodes, dims, a)
        lo, hi = box_of(rec, dims)
        lo[a], hi[a] = p[:, a].min() - 1.0, p[:, a].max() + 1.0
        yield f"dims {dims}, axis {a}, a box around every centre", nodes, one, nodes2, gs4d.lattice(lo, hi, dims2)
        lo[a], hi[a] = np.quantile(p[:, a], 0.3), np.quantile(p[:, a], 0.7) + 1.0
        yield f"dims {dims}, axis {a}, clamped", nodes, one, nodes2, gs4d.lattice(lo, hi, dims2, "xyzt"[a])


def refused_lattices(gs4d):
    """{what: Lattice} of everything gs4d_warp_records refuses in a lattice (the null pointer apart), each one node in its buffer's eyes"""
    def lat(dims=(1, 1, 1, 1), clamp=0, pad=(0, 0, 0)):
        q = gs4d.lattice((0,) * 4, (1,) * 4, (1, 1, 1, 1))
        q.dims[:], q.clamp, q.pad[:] = dims, clamp, pad
        return q
    bad = {f"dim {a} is 0": lat(tuple(0 if b == a else 1 for b in range(4))) for a in range(4)}
    bad.update({f"dim {a} is 65536": lat(tuple(65536 if b == a else 1 for b in range(4))) for a in range(4)})
    bad.update({"more than 2^28 nodes": lat((65535, 65535, 1, 1)), "2^29 nodes": lat((1 << 14, 1 << 14, 1, 2)), "a product that wraps 32 bits": lat((65535, 65535, 65535, 65535)),
                "clamp bit 4": lat(clamp=16), "clamp bit 31": lat(clamp=1 << 31), "pad[0]": lat(pad=(1, 0, 0)), "pad[2]": lat(pad=(0, 0, 7))})
    return bad


# ---- the definition, restated -------------------------------------------------------------------------------------------------------------------
def by_the_text(rec, nodes, lat):
    """the header's text in numpy float32, one operation at a time (numpy rounds every product, sum and difference on its own).  Returns (out
    [n, 24], warped, copied, clamped bool [n]): a copied record is a copy byte for byte; clamped: a warped record whose u the clamp changed on
    some axis"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    nodes = np.ascontiguousarray(nodes, f32).reshape(-1, 4)
    n, dims = rec.shape[0], [int(d) for d in lat.dims]
    assert nodes.shape[0] == count_of(dims)
    lo, inv = [f32(v) for v in lat.lo], [f32(v) for v in lat.inv]
    inside, clamped = np.ones(n, bool), np.zeros(n, bool)
    base = np.zeros(n, np.int64)
    f, flat, step = [None] * 4, [np.ones(n, bool)] * 4, [0] * 4
    stride = 1
    with np.errstate(all="ignore"):
        for a in range(4):
            d = dims[a]
            step[a] = stride
            if d >= 2:
                u = (rec[:, a] - lo[a]) * inv[a]
                top = f32(d - 1)
                changed = np.zeros(n, bool)
                if lat.clamp >> a & 1:
                    low = u < f32(0.0)
                    u = np.where(low, f32(0.0), u)
                    high = u > top
                    u = np.where(high, top, u)
                    changed = low | high
                ins = (u >= f32(0.0)) & (u <= top)
                i = np.minimum(np.where(ins, u, f32(0.0)).astype(u32), u32(d - 2))      # converted only when inside
                f[a] = (u - i.astype(f32)).astype(f32)
                flat[a] = changed
                clamped |= changed
                inside &= ins
                base += i.astype(np.int64) * stride
            stride *= d
        base = np.where(inside, base, 0)                     # (a record that is copied fetches nothing: the first cell stands in for its cell)

        def sample(A, j):
            """(value [n, 4], [derivative along axis b [n, 4] for b < A]) of the sub-lattice at node j reduced along the axes below A"""
            if A == 0:
                return nodes[j], []
            a = A - 1
            lo_v, lo_g = sample(a, j)
            if dims[a] < 2:
                return lo_v, lo_g + [np.zeros((n, 4), f32)]
            hi_v, hi_g = sample(a, j + step[a])
            fa = f[a][:, None]
            diff = hi_v - lo_v
            v = lo_v + (fa * diff)
            g = [lg + (fa * (hg - lg)) for lg, hg in zip(lo_g, hi_g)]
            return v, g + [diff * inv[a]]

        D, G = sample(4, base)
        assert D.dtype == f32 and all(g.dtype == f32 for g in G)
        a20 = np.zeros((n, 20), f32)
        for c in range(4):
            for r in range(4):
                g = np.where(flat[c], f32(0.0), G[c][:, r])
                a20[:, 4 * c + r] = f32(1.0 if r == c else 0.0) + g
        out = pc.record_by_the_text(rec, a20)               # the T and Sigma' lines (its mean is replaced below)
        for r in range(4):
            out[:, r] = rec[:, r] + D[:, r]
    assert out.dtype == f32
    out.view(u32)[~inside] = rec.view(u32)[~inside]
    return out, inside, ~inside, clamped & inside


def assert_records(got, want, rec, warped, what):
    """the rule of gs4d.h: a warped record equal as uint32 but for NaN = NaN, a copied record byte-equal"""
    pc.assert_records(got, want, rec, warped, what)
