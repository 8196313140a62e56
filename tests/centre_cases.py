"""gs4d_count_centres (include/gs4d.h) restated in numpy, and the record sets, queries, masks and tables of its tests.

Test infrastructure only (tests/test_centres_host.py pins gs4d_host_count_centres to the restatement on the CPU; tests/test_gpu_centres.py runs the
device call against it).  Plain numpy: float32 arrays, one ufunc per operation of the definition, so every product and every sum is rounded on its
own; the two fused operations are evaluated exactly (fma32).

A query is a dict: tests (OR of the CQ_* bits), op, t, frame (12), box_lo, box_hi (3), sphere (4), view, proj (16), rect (x, y, w, h), depth (min,
max).  struct() turns it into the binding's CentreQuery.

Sizes: the kernel gives one workgroup of TILE threads a tile of TILE records.  SIZES hits its edges.
"""
import functools
import importlib

import numpy as np

import scenes

f32, f64 = np.float32, np.float64
TILE = 256                                                # CENTRES_TILE (csrc/gs4d_internal.h)
SIZES = (0, 1, TILE - 1, TILE, TILE + 1, 1000)
EXTRA = 3                                                 # records behind n that no call may look at
W, H = 64, 48                                             # the image of every context of these tests
BOX, SPHERE, SCREEN, FRAME, SKIP_HIDDEN, SKIP_DEAD = 1, 2, 4, 8, 16, 32      # GS4D_CQ_*
ALL_BITS = 63
ADD, REMOVE = 0, 1
DEAD_ARG = f32(-106.0)                                    # GS4D_TIME_DEAD_ARG
ONE_BITS = np.uint32(0x3F800000)
STAT = np.dtype([("pixels", "<u4"), ("wmax", "<u4"), ("wsum", "<u8")])       # wmax as its bit pattern
T = 25.0
CAM = ((0.0, 0.0, 150.0), (0.0, 0.0, -1.0))
KINDS = ("static3d", "symmetric", "sheared")
NAN, INF = float("nan"), float("inf")


def _gs4d():
    return importlib.import_module("4dgaussiansplatrendering_amd")


# ---- arithmetic --------------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf on float32 operands, rounded once.  The product of two float32 is exact in float64; the sum is rounded to odd there (TwoSum gives
    its error exactly), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 that of the exact value."""
    a, b, c = (np.asarray(v, f32).astype(f64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        move = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & even
        s = np.where(move, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
        return s.astype(f32)


def centre(rec, t):
    """m [n, 3], dt, 1 / s44: the time-conditioned centre of the definition"""
    rec = np.ascontiguousarray(rec, f32)
    with np.errstate(all="ignore"):
        dt = f32(t) - rec[:, 3]
        inv = f32(1.0) / rec[:, 23]
        k = inv * dt
        m = rec[:, 0:3] + (k[:, None] * rec[:, 20:23])
    return m, dt, inv


def window(rec, q, width=W, height=H):
    """(wx, wy, -pc.z, ps.w) of the definition's screen test"""
    m, _, _ = centre(rec, q["t"])
    V, P = np.asarray(q["view"], f32), np.asarray(q["proj"], f32)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        pc = [(((V[r] * m[:, 0]) + (V[4 + r] * m[:, 1])) + (V[8 + r] * m[:, 2])) + (V[12 + r] * one) for r in range(4)]
        ps = [(((P[r] * pc[0]) + (P[4 + r] * pc[1])) + (P[8 + r] * pc[2])) + (P[12 + r] * pc[3]) for r in range(4)]
        rw = one / ps[3]
        nx, ny = rw * ps[0], rw * ps[1]
        hw, hh = f32(width) * f32(0.5), f32(height) * f32(0.5)
        return fma32(nx, hw, hw), fma32(ny, hh, hh), -pc[2], ps[3]


def takes_part(rec, q, mask=None, width=W, height=H):
    """which of the records take part in query q — the definition, test by test"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    n, tests = rec.shape[0], int(q["tests"])
    m, dt, inv = centre(rec, q["t"])
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        if tests & SKIP_HIDDEN:
            ok &= rec[:, 7] > f32(0.0)
        if tests & SKIP_DEAD:
            ok &= ~((((f32(-0.5) * dt) * inv) * dt) < DEAD_ARG)
        v = m
        if tests & FRAME:
            f = np.asarray(q["frame"], f32)
            v = np.stack([(((f[r] * m[:, 0]) + (f[3 + r] * m[:, 1])) + (f[6 + r] * m[:, 2])) + f[9 + r] for r in range(3)], 1)
        if tests & BOX:
            lo, hi = np.asarray(q["box_lo"], f32), np.asarray(q["box_hi"], f32)
            for a in range(3):
                ok &= (lo[a] <= v[:, a]) & (v[:, a] <= hi[a])
        if tests & SPHERE:
            s = np.asarray(q["sphere"], f32)
            d = [v[:, a] - s[a] for a in range(3)]
            ok &= (((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])) <= s[3] * s[3]
        if tests & SCREEN:
            x, y, w, h = (int(c) for c in q["rect"])
            wx, wy, depth, psw = window(rec, q, width, height)
            inside = (psw > f32(0.0)) & (f32(q["depth"][0]) <= depth) & (depth <= f32(q["depth"][1]))
            inside &= (wx >= f32(x)) & (wx < f32(x + w)) & (wy >= f32(y)) & (wy < f32(y + h))
            if mask is not None:
                mk = np.asarray(mask).reshape(h, w)
                col = np.where(inside, np.floor(wx), f32(x)).astype(np.int64) - x
                row = np.where(inside, np.floor(wy), f32(y)).astype(np.int64) - y
                inside &= mk[row, col] != 0
            ok &= inside
    return ok


def restate(rec, q, table, mask=None, width=W, height=H):
    """the table after the call: a copy of `table` (STAT, at least n rows) with the rows of the records that take part updated"""
    out = np.array(table, STAT, copy=True)
    n = np.ascontiguousarray(rec).reshape(-1, 24).shape[0]
    part = takes_part(rec, q, mask, width, height)
    rows = np.flatnonzero(part)
    if int(q["op"]) == ADD:
        out["pixels"][rows] = out["pixels"][rows] + np.uint32(1)                    # (mod 2^32, as the device's)
        out["wmax"][rows] = np.maximum(out["wmax"][rows], ONE_BITS)
        out["wsum"][rows] = out["wsum"][rows] + np.uint64(1 << 24)
    else:
        out[rows] = np.zeros(1, STAT)[0]
    assert out.shape[0] >= n
    return out, part


def struct(q):
    """the query as the binding's CentreQuery"""
    g = _gs4d()
    s = g.CentreQuery()
    s.tests, s.op, s.t, s.reserved = int(q["tests"]), int(q["op"]), float(f32(q["t"])), 0
    for name, count in (("frame", 12), ("box_lo", 3), ("box_hi", 3), ("sphere", 4), ("view", 16), ("proj", 16)):
        getattr(s, name)[:] = [float(v) for v in np.asarray(q[name], f32).reshape(count)]
    s.x, s.y, s.w, s.h = (int(c) for c in q["rect"])
    s.depth_min, s.depth_max = float(f32(q["depth"][0])), float(f32(q["depth"][1]))
    return s


# ---- record sets -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records(kind, n, seed=0x4343):
    """n records in front of CAM, positions in [-40, 40]^3: "static3d" (build_records_3d), "symmetric" (build_records_4d_tvar, mirrored so that
    floats 11, 15, 19 are the bits of 20, 21, 22) or "sheared" (the symmetric set under a shear, transform_records_host: its halves round apart).
    Every fifth record is hidden (alpha 0, -0.5 or -0), every seventh is dead at T (mu_t so far off that the time argument is below
    GS4D_TIME_DEAD_ARG): no test is vacuous for want of records to skip."""
    g = _gs4d()
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(max(n, 1), seed=seed)
    pos4, rgba = pos4[:n].copy(), rgba[:n].copy()
    q, scale, life, fade, vel = q[:n], scale[:n], life[:n], fade[:n], vel[:n]
    pos4[:, :3] *= f32(0.2)
    pos4[:, 3] = T - 0.5 + pos4[:, 3] / 50.0
    i = np.arange(n)
    rgba[i % 5 == 2, 3] = np.array([0.0, -0.5, -0.0], f32)[(i[i % 5 == 2] // 5) % 3]
    dead = i % 7 == 3
    if kind == "static3d":
        rec = g.build_records_3d(pos4[:, :3].copy(), q, scale * 4.0, rgba)
        rec[:, 3] = T
        rec[dead, 3] = T + 20.0                                 # s44 = 1: the argument is -200; sig3 = 0: the centre stays
        rec.setflags(write=False)                               # (shared between the tests)
        return rec
    tvar = g.time_variance(life * 4.0, fade)
    pos4[dead, 3] = T + 40.0 * np.sqrt(tvar[dead])              # the argument is -800
    rec = g.build_records_4d_tvar(pos4, q, scale * 4.0, vel * 0.2, tvar, rgba)
    sig = rec[:, 8:].reshape(-1, 4, 4)
    iu = np.triu_indices(4, 1)
    sig[:, iu[0], iu[1]] = sig[:, iu[1], iu[0]]                 # column c, row 3 <- column 3, row c: floats 11, 15, 19 become 20, 21, 22
    if kind == "symmetric":
        rec.setflags(write=False)
        return rec
    l = np.eye(4, dtype=f32)
    # L[r, c]: a shear in space, one along time, and a time row that is not (0, 0, 0, 1) — with that row the two halves of the time column would
    # be the same sums of the same products; the offset keeps T where it was (1.25 T - 0.25 T)
    l[0, 1], l[1, 2], l[2, 0], l[1, 3], l[3, 0], l[3, 3] = 0.3, -0.2, 0.15, 0.1, 0.004, 1.25
    xf = np.concatenate([l.T.reshape(-1), np.array([1.0, -2.0, 0.5, -0.25 * T], f32)])
    out = g.transform_records_host(rec, xf)
    if n >= TILE - 1:
        assert (np.ascontiguousarray(out[:, [11, 15, 19]]).view(np.uint32) != np.ascontiguousarray(out[:, 20:23]).view(np.uint32)).any(), "the shear left the set symmetric"
    out.setflags(write=False)
    return out


def mats():
    g = _gs4d()
    return g.look_at(*CAM), g.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)


# ---- queries -----------------------------------------------------------------------------------------------------------------------------------------
RECT = (24, 14, 15, 17)                                       # inside the image, odd sizes
EDGE_RECTS = ((0, 0, 33, 25), (30, 22, 34, 26), (0, 14, 64, 17), (24, 0, 15, 48))      # left + bottom; right + top; both sides; bottom + top


def query(tests, op=ADD, t=T, rect=RECT, **over):
    """the query of these tests with the given test bits: every test on its own leaves records in and out, and so do all of them together"""
    view, proj = mats()
    c, s = np.cos(0.35), np.sin(0.35)
    rot = np.array([[c, -s, 0.0], [s, c, 0.1], [0.05, 0.0, 1.0]], f32)       # frame[3 * column + row]: a turn about z with a little shear
    q = dict(tests=tests, op=op, t=t, frame=np.concatenate([rot.T.reshape(-1), np.array([2.0, -1.0, 3.0], f32)]),
             box_lo=(-30.0, -25.0, -28.0), box_hi=(22.0, 30.0, 26.0), sphere=(4.0, -3.0, 2.0, 38.0), view=view, proj=proj, rect=rect,
             depth=(125.0, 172.0))
    q.update(over)
    return q


def mask_for(rect):
    """a lasso of rect's size: a disc-like blob with a hole pattern — about half of the bytes set, bytes other than 1 among them"""
    _, _, w, h = rect
    r, c = np.mgrid[0:h, 0:w]
    m = (((r // 2 + c // 3) % 2) == 0) | ((r + c) % 7 == 0)
    return np.where(m, ((r * 31 + c * 17) % 255) + 1, 0).astype(np.uint8)


def subsets():
    return range(ALL_BITS + 1)


def nonfinite_queries():
    """(name, query): a non-finite t, box end, radius, frame or matrix element — data, not errors"""
    out = []
    for name, v in (("nan", NAN), ("pinf", INF), ("ninf", -INF)):
        out.append((f"t_{name}", query(ALL_BITS, t=v)))
        out.append((f"t_{name}_no_skip", query(BOX | SPHERE | SCREEN, t=v)))
        lo, hi = list(query(0)["box_lo"]), list(query(0)["box_hi"])
        lo[1], hi[2] = v, v
        out.append((f"box_lo_{name}", query(BOX | FRAME, box_lo=lo)))
        out.append((f"box_hi_{name}", query(BOX, box_hi=hi)))
        out.append((f"radius_{name}", query(SPHERE | SKIP_HIDDEN, sphere=(4.0, -3.0, 2.0, v))))
        out.append((f"sphere_centre_{name}", query(SPHERE, sphere=(v, -3.0, 2.0, 38.0))))
        for which, at in (("view", 14), ("view", 5), ("proj", 0), ("proj", 11), ("frame", 4), ("frame", 10)):
            base = query(ALL_BITS)
            m = np.array(base[which], f32, copy=True)
            m[at] = v
            out.append((f"{which}{at}_{name}", query(ALL_BITS, **{which: m})))
        out.append((f"depth_min_{name}", query(SCREEN, depth=(v, 172.0))))
        out.append((f"depth_max_{name}", query(SCREEN, depth=(125.0, v))))
    out.append(("box_inverted", query(BOX, box_lo=(22.0, 30.0, 26.0), box_hi=(-30.0, -25.0, -28.0))))
    out.append(("radius_negative", query(SPHERE, sphere=(4.0, -3.0, 2.0, -38.0))))          # r * r: the same ball
    out.append(("radius_3e38", query(SPHERE, sphere=(4.0, -3.0, 2.0, 3e38))))              # r * r = +inf
    out.append(("zero_matrices", query(SCREEN, view=np.zeros(16, f32), proj=np.zeros(16, f32))))
    return out


def hostile_queries(case):
    """the queries run on a set of tests/hostile_cases.py: the case's own time and camera, a rectangle of the 64 x 48 image"""
    base = dict(t=case.t, view=case.view, proj=case.proj, depth=(0.0, INF), box_lo=(-60.0, -60.0, -60.0), box_hi=(60.0, 60.0, 200.0),
                sphere=(0.0, 0.0, 0.0, 150.0))
    return [query(tests, rect=rect, **base) for tests, rect in ((ALL_BITS, (0, 0, W, H)), (SCREEN, (8, 6, 47, 35)), (BOX | SPHERE, RECT),
                                                                (SKIP_HIDDEN | SKIP_DEAD, RECT), (SCREEN | FRAME | SKIP_DEAD, (0, 0, W, H)))]


# ---- tables ------------------------------------------------------------------------------------------------------------------------------------------
def table(kind, n, seed=0x5443):
    """"zero", or "random": no row is zero, and the rows run through the edges of the update — pixels at 2^32 - 1, wmax below, at and above the
    bits of 1.0f (and +inf), a wsum whose low word carries and one that wraps"""
    st = np.zeros(n, STAT)
    if kind == "zero" or n == 0:
        return st
    u = lambda s: (scenes.uniform(n, s, seed=seed) * 2.0 ** 32).astype(np.uint64)
    st["pixels"] = (u(0) | np.uint64(1)).astype(np.uint32)
    st["wmax"] = (u(1) >> np.uint64(2)).astype(np.uint32)
    st["wsum"] = (u(2) << np.uint64(20)) | u(3)
    i = np.arange(n)
    st["pixels"][i % 11 == 1] = 0xFFFFFFFF
    edge_w = np.array([0, 0x3F7FFFFF, 0x3F800000, 0x3F800001, 0x7F800000, 0xFFFFFFFF], np.uint32)
    st["wmax"][i % 3 == 0] = edge_w[(i[i % 3 == 0] // 3) % edge_w.size]
    edge_s = np.array([0xFFFFFFFF, 0xFF000000, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFF000000, 1], np.uint64)
    st["wsum"][i % 4 == 2] = edge_s[(i[i % 4 == 2] // 4) % edge_s.size]
    return st
