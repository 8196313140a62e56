"""Inputs for the gs4d_decompose_records tests (include/gs4d.h): record sets, the yardstick of the round trip and the comparisons.

Sets (name -> the form its records are taken out in):
3d, 4d_vel   records of gs4d_host_build_records_3d / _4d_tvar from random parameters: variance ratios 1, 10^4 and 10^8 (the scale ratios 1, 10^2, 10^4
             in turn, the middle scale anywhere between), overall scales 10^-3 .. 10^3, unit and non-unit quaternions.
4d_2q        records of gs4d_host_build_records_4d_2q, taken out as 4D_VEL.
hard_3d,     named records, one case each, written word by word: an already diagonal Sigma3 (sorted and not), a sphere, two equal eigenvalues
hard_4d      (axis-aligned and rotated), flat discs and needles with exact zeros, denormal off-diagonals, 1e30 entries, an indefinite and a
             negative-definite Sigma3, upper and lower triangles that disagree, NaN, +Inf and -Inf in each word group; hard_4d also Sigma44 = 0, -0,
             negative and Inf, and td = 0 with -0 entries.
Every record carries a flag: whether it is finite with a positive-semidefinite Sigma3 (and Sigma44 > 0), by construction.  Only those take part in the
round trip and in the property tests.

The round trip's yardstick is not the code under test: the same route with the decomposition by numpy.linalg.eigh in float64, its outputs rounded to
float32 and pushed through the same host builder (eigh_route).  BOUND: the definition's worst relative Frobenius error of a set may be at most
BOUND times that route's worst (each of the 3 * sweeps float32 rotations adds about one rounding to the eigenvectors' orthogonality; float64 adds none).
"""
import numpy as np

import build_cases as bc

f32 = np.float32
f64 = np.float64
u32 = np.uint32
TILE = 256                                                   # DECOMPOSE_TILE (csrc/gs4d_internal.h)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)                 # the wave and workgroup edges of a 256-thread tile
FIRSTS = (0, 7)                                              # src_first
COUNT = 1000                                                 # records of a random set
BOUND = 8.0                                                  # see above
KEPT = 0.9                                                   # the share of all records that must take part in the round trip
SETS = ("3d", "4d_vel", "4d_2q", "hard_3d", "hard_4d")
NAMES = ("pos", "rot", "scale", "rgba", "dir", "tvar")
SPATIAL = (8, 9, 10, 12, 13, 14, 16, 17, 18)                 # floats of the 3x3 block, column-major
GROUPS = {"mean": (0, 1, 2, 3), "rgba": (4, 5, 6, 7), "block": SPATIAL, "time column": (20, 21, 22), "time row": (11, 15, 19), "s44": (23,)}
same_bits = bc.same_bits
bits = bc.bits


def form_of(gs4d, which):
    return gs4d.PARAMS_3D if which in ("3d", "hard_3d") else gs4d.PARAMS_4D_VEL


def rows_of(gs4d, which):
    return gs4d.PARAM_ROWS[form_of(gs4d, which)]


def scales(rng, n, width):
    """variance ratios 1, 10^4, 10^8 in turn: the largest scale `overall`, the smallest overall / 10^k, the others anywhere between, shuffled"""
    k = np.array([0.0, 2.0, 4.0])[np.arange(n) % 3][:, None]
    overall = 10.0 ** rng.uniform(-3.0, 3.0, (n, 1))
    e = np.concatenate([np.zeros((n, 1)), np.ones((n, 1)), rng.uniform(0.0, 1.0, (n, width - 2))], 1)
    return rng.permuted(overall * 10.0 ** (-k * e), axis=1).astype(f32)


def random_records(gs4d, which, n=COUNT, seed=0x4443):
    rng = np.random.default_rng([seed, SETS.index(which)])
    pos = rng.uniform(-200.0, 200.0, (n, 4)).astype(f32)
    pos[:, 3] = rng.uniform(0.0, 50.0, n)
    rgba, q = rng.uniform(0.0, 1.0, (n, 4)).astype(f32), bc.quaternions(rng, n)
    if which == "3d":
        return gs4d.build_records_3d(pos[:, :3], q, scales(rng, n, 3), rgba)
    if which == "4d_vel":
        return gs4d.build_records_4d_tvar(pos, q, scales(rng, n, 3), rng.uniform(-5.0, 5.0, (n, 3)).astype(f32), (10.0 ** rng.uniform(-1.3, 0.7, n)).astype(f32), rgba)
    return gs4d.build_records_4d_2q(pos, q, bc.quaternions(rng, n), scales(rng, n, 4), rgba)


def with_block(base, m):
    """a copy of the record with the symmetric (or not) 3x3 matrix m[row][col] as its spatial block"""
    r = base.copy()
    m = np.asarray(m, f32)
    for c in range(3):
        for k in range(3):
            r[8 + 4 * c + k] = m[k][c]
    return r


def hard_records(gs4d, which):
    """([m, 24] records, [m] finite-and-PSD flags, [m] names)"""
    four = which == "hard_4d"
    rng = np.random.default_rng(0x4444)
    base = np.zeros(24, f32)
    base[:4], base[4:8], base[23] = (1.5, -2.0, 3.25, 7.0 if four else 0.0), (0.25, 0.5, 0.75, 1.0), 1.0
    rot = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    sym = lambda d: rot @ np.diag(d) @ rot.T
    out = []
    add = lambda name, rec, ok: out.append((name, rec, ok))
    for name, m, ok in (("diagonal, sorted", np.diag([4.0, 2.0, 1.0]), True), ("diagonal, unsorted", np.diag([1.0, 4.0, 2.0]), True),
                        ("sphere", np.diag([3.0, 3.0, 3.0]), True), ("two equal, on the axes", np.diag([2.0, 5.0, 5.0]), True),
                        ("two equal, rotated", sym([5.0, 5.0, 1.0]), True), ("three equal, tiny", np.diag([1e-12] * 3), True),
                        ("disc xy", np.diag([4.0, 4.0, 0.0]), True), ("disc xz", np.diag([4.0, 0.0, 9.0]), True),
                        ("needle x", np.diag([9.0, 0.0, 0.0]), True), ("needle z", np.diag([0.0, 0.0, 9.0]), True), ("zero", np.zeros((3, 3)), True),
                        ("needle, rotated", sym([9.0, 0.0, 0.0]), True), ("disc, rotated", sym([4.0, 1.0, 0.0]), True),
                        ("denormal off-diagonals", np.diag([3.0, 2.0, 1.0]) + 1e-42 * (1 - np.eye(3)), True),
                        ("denormal off-diagonals, equal diagonal", np.diag([2.0, 2.0, 2.0]) + 1e-42 * (1 - np.eye(3)), True),
                        ("1e30", 1e30 * np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.5], [0.0, 0.5, 1.0]]), True), ("1e30, rotated", sym([1e30, 3e29, 1e29]), True),
                        ("indefinite", [[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], False), ("indefinite, rotated", sym([2.0, -1.0, 0.5]), False),
                        ("negative definite", -np.diag([3.0, 2.0, 1.0]), False), ("negative definite, rotated", sym([-1.0, -2.0, -3.0]), False)):
        add(name, with_block(base, m), ok)
    lower = sym([3.0, 2.0, 0.5])
    add("triangles disagree", with_block(base, np.tril(lower) + np.triu(np.full((3, 3), 77.0), 1)), True)
    add("triangles disagree, NaN above", with_block(base, np.tril(lower) + np.triu(np.full((3, 3), np.nan), 1)), True)
    clean = with_block(base, sym([4.0, 1.0, 0.25]))
    if four:
        moving = clean.copy()
        td = np.array([0.5, -0.25, 1.0], f32)
        moving[20:23], moving[[11, 15, 19]] = td, td
        moving[list(SPATIAL)] += np.outer(td, td).astype(f32).T.reshape(-1)
        add("moving", moving, True)
        for name, v in (("s44 0", 0.0), ("s44 -0", -0.0), ("s44 negative", -0.75), ("s44 inf", np.inf), ("s44 denormal", 1e-42)):
            for rec in (clean, moving):
                r = rec.copy()
                r[23] = v
                add(name, r, False)
        r = clean.copy()
        r[20:23], r[[11, 15, 19]] = (-0.0, 0.0, -0.0), (-0.0, 0.0, -0.0)
        add("td 0 with -0 entries", r, True)
        clean = moving
    for group, words in GROUPS.items():
        for v in (np.nan, np.inf, -np.inf):
            for w in (words[0], words[-1], None):
                r = clean.copy()
                r[list(words) if w is None else w] = v
                # only the words the form reads decide whether the record stays well-formed; the flag goes by the whole record: not finite, left out
                add(f"{v} in {group}", r, False)
    names, recs, ok = zip(*out)
    return np.ascontiguousarray(np.stack(recs), f32), np.array(ok, bool), names


_BASE = {}


def base(gs4d, which):
    """(records, finite-and-PSD flags) of a set: COUNT random records, or the named hard ones"""
    if which not in _BASE:
        if which.startswith("hard"):
            rec, ok, _ = hard_records(gs4d, which)
        else:
            rec, ok = random_records(gs4d, which), np.ones(COUNT, bool)
            assert np.isfinite(rec).all()
        rec.setflags(write=False)
        _BASE[which] = (rec, ok)
    return _BASE[which]


def records(gs4d, which, count):
    """`count` records of a set, taken round and round"""
    rec = base(gs4d, which)[0]
    return np.ascontiguousarray(rec[np.arange(count) % rec.shape[0]])


def assert_same(got, want, what):
    """every array of `want` in `got` with the comparison of gs4d.h"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        ok = same_bits(got[k], want[k])
        assert ok.all(), f"{what}: {k}: {int((~ok).any(1).sum())} of {ok.shape[0]} rows differ from the host definition, first at {np.argwhere(~ok)[0].tolist()}"


def rebuild(gs4d, form, p):
    """the host builder of the form over a dict of parameters"""
    if form == gs4d.PARAMS_3D:
        return gs4d.build_records_3d(p["pos"], p["rot"], p["scale"], p["rgba"])
    return gs4d.build_records_4d_tvar(p["pos"], p["rot"], p["scale"], p["dir"], p["tvar"], p["rgba"])


def cov64(rec, four):
    """[n, 4, 4] float64: the covariance the call reads — the lower triangle of the spatial block mirrored; 4D: the time column mirrored, Sigma44"""
    n = rec.shape[0]
    c = np.zeros((n, 4, 4), f64)
    m = rec[:, 8:24].astype(f64).reshape(n, 4, 4).transpose(0, 2, 1)       # m[i, row, col]
    low = np.tril(m[:, :3, :3])
    c[:, :3, :3] = low + np.tril(low, -1).transpose(0, 2, 1)
    if four:
        c[:, :3, 3], c[:, 3, :3], c[:, 3, 3] = m[:, :3, 3], m[:, :3, 3], m[:, 3, 3]
    return c


def round_trip_error(gs4d, rec, form, p):
    """per record: |cov(build(p)) - cov(rec)|_F / |cov(rec)|_F in float64 (0 for a zero covariance rebuilt as zero)"""
    four = form != gs4d.PARAMS_3D
    want, got = cov64(rec, four), cov64(rebuild(gs4d, form, p), four)
    num, den = np.sqrt(((got - want) ** 2).sum((1, 2))), np.sqrt((want ** 2).sum((1, 2)))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), num)


def quat64(R):
    """w x y z of a proper rotation matrix, float64, w >= 0 (Shepperd)"""
    t = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(t))
    q = ((t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]), (R[2, 1] - R[1, 2], t[1], R[1, 0] + R[0, 1], R[0, 2] + R[2, 0]),
         (R[0, 2] - R[2, 0], R[1, 0] + R[0, 1], t[2], R[2, 1] + R[1, 2]), (R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[2, 1] + R[1, 2], t[3]))[k]
    q = np.array(q) / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def eigh_route(gs4d, rec, form):
    """the yardstick: the parameters of finite PSD records by numpy.linalg.eigh in float64, rounded to float32"""
    four = form != gs4d.PARAMS_3D
    n = rec.shape[0]
    c = cov64(rec, four)
    a = c[:, :3, :3].copy()
    p = {"pos": rec[:, :4 if four else 3].copy(), "rgba": rec[:, 4:8].copy(), "rot": np.zeros((n, 4), f32), "scale": np.zeros((n, 3), f32)}
    if four:
        td, sd = c[:, :3, 3], c[:, 3, 3]
        a -= td[:, :, None] * td[:, None, :] / sd[:, None, None]
        p["dir"], p["tvar"] = (td / sd[:, None]).astype(f32), sd.astype(f32).reshape(n, 1)
    lam, vec = np.linalg.eigh(a)
    for i in range(n):
        order = np.argsort(-lam[i], kind="stable")
        V = vec[i][:, order]
        if np.linalg.det(V) < 0:
            V[:, 2] = -V[:, 2]
        p["rot"][i], p["scale"][i] = quat64(V), np.sqrt(np.maximum(lam[i][order], 0.0))
    return p
