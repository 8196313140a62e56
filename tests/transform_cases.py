"""Inputs for the gs4d_transform_records tests (include/gs4d.h): record sets, rows of gs4d_affine4, and the definition restated as a
numpy float32 loop of the header's text.

sets        clean 3D, 4D_VEL and 4D_2Q sets from the generators of tests/build_cases.py (host-built records), and "hostile": the implanted records of
            every case of tests/hostile_cases.py (at most three of each) — NaN, +-Inf, 1e30 and 3e38, zero, negative and denormal variances, rank-1 and
            non-symmetric covariances.
transforms  the identity, a rigid map, a non-uniform scale with shear, a retime (time_scale 0.5 with an offset), a velocity column, a singular L, the
            zero matrix, and rows holding NaN, Inf and 1e30.  Rows are 20 float32: l[16] (column-major, L[r, c] = l[4 c + r]) and o[4].
"""
import functools

import numpy as np

import build_cases as bc
import hostile_cases

f32 = np.float32
U = 2.0 ** -24                                               # the unit roundoff of float32
SIZES = (1, 255, 256, 257, 769)                              # one record, either side of a tile of 256, three tiles plus one
INSTANCES = (1, 3)
SETS = ("3d", "4d_vel", "4d_2q", "hostile")
bits, same_bits = bc.bits, bc.same_bits


# ---- record sets --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hostile_block():
    """the implanted records of every hostile case, at most three of each, as float32 [k, 24]"""
    rows = [c.rec[np.flatnonzero(c.hostile)[:3]] for c in hostile_cases.all_cases() if c.hostile.any()]
    block = np.ascontiguousarray(np.concatenate(rows), f32)
    block.setflags(write=False)
    return block


def records(gs4d, which, n, seed=0x5452):
    """n records of a set: a clean set of the form, or the hostile block taken round and round"""
    if which == "hostile":
        block = hostile_block()
        return np.ascontiguousarray(block[(np.arange(n) + n) % block.shape[0]])
    return bc.host_records(gs4d, which, bc.clean(gs4d, which, n, seed=seed + n))


# ---- transforms ---------------------------------------------------------------------------------------------------------------------------------
def row(L, o):
    """20 floats from L as a 4 x 4 array indexed [row, column] and o"""
    return np.concatenate([np.asarray(L, np.float64).T.reshape(16), np.asarray(o, np.float64)]).astype(f32)


def rotation(axis, angle):
    """a rotation matrix (float64) about an axis"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def quaternion(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2.0)], np.sin(angle / 2.0) * a]).astype(f32)


def block4(A=np.eye(3), v=(0.0, 0.0, 0.0), a=1.0):
    """L with the spatial block A, the velocity column v and the time row (0, 0, 0, a)"""
    L = np.zeros((4, 4))
    L[:3, :3], L[:3, 3], L[3, 3] = A, v, a
    return L


RIGID_AXIS, RIGID_ANGLE, RIGID_SHIFT = (1.0, 2.0, -0.5), 0.7, (12.0, -7.5, 20.0)
RETIME = (0.5, 3.25)                                         # time_scale, time_offset
VELOCITY = (1.5, -0.75, 0.25)


@functools.lru_cache(maxsize=None)
def transforms():
    """{name: 20 float32}"""
    shear = np.array([[2.0, 0.3, 0.0], [0.0, 0.5, -0.2], [0.1, 0.0, 1.25]])
    singular = block4(np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, -1.0, 0.25]]), (1.0, 2.0, 0.5), 0.0)      # rank 2 in space, time row 0
    full = np.array([[0.9, -0.2, 0.1, 0.4], [0.3, 1.1, -0.3, -0.2], [0.0, 0.25, 0.8, 0.1], [0.05, -0.02, 0.01, 1.5]])      # a time row that mixes space in
    t = {
        "identity": row(np.eye(4), (0.0, 0.0, 0.0, 0.0)),
        "rigid": row(block4(rotation(RIGID_AXIS, RIGID_ANGLE)), RIGID_SHIFT + (0.0,)),
        "scale_shear": row(block4(shear), (-3.0, 0.5, 8.0, 0.0)),
        "retime": row(block4(a=RETIME[0]), (0.0, 0.0, 0.0, RETIME[1])),
        "velocity": row(block4(v=VELOCITY), (0.0, 0.0, 0.0, 0.0)),
        "full": row(full, (1.0, -2.0, 3.0, 0.5)),
        "singular": row(singular, (1.0, 1.0, 1.0, 2.0)),
        "zero": row(np.zeros((4, 4)), (0.0, -0.0, 5.0, 1.0)),
    }
    for name, v in (("nan", np.nan), ("inf", np.inf), ("1e30", 1e30)):
        r = t["rigid"].copy()
        r[[0, 6, 11, 13]] = v                                # in the spatial block, the time row and the velocity column
        r[2] = -v
        r[17] = v                                            # and in the offset
        t[name] = r
    for r in t.values():
        r.setflags(write=False)
    return t


NAMES = ("identity", "rigid", "scale_shear", "retime", "velocity", "full", "singular", "zero", "nan", "inf", "1e30")
FINITE = NAMES[:8]                                           # the rows whose results stay finite on a clean set
TIME_BLOCK = ("identity", "rigid", "scale_shear", "retime", "velocity")      # time row (0, 0, 0, a) with a != 0: the conditional meaning holds


def rows(names):
    return np.stack([transforms()[k] for k in names])


def rows_for(call, m):
    """the m rows of the call-th call of a test: the transforms taken round and round, so that a handful of calls see all of them"""
    return rows([NAMES[(3 * call + j) % len(NAMES)] for j in range(m)])


# ---- the definition, restated -------------------------------------------------------------------------------------------------------------------
def by_the_text(rec, xf):
    """the header's text in numpy float32, one operation at a time (numpy rounds every product and every sum on its own): records [n, 24] under one row"""
    rec, xf = np.ascontiguousarray(rec, f32).reshape(-1, 24), np.ascontiguousarray(xf, f32).reshape(20)
    l, o = [f32(v) for v in xf[:16]], [f32(v) for v in xf[16:]]
    out = np.empty_like(rec)
    with np.errstate(all="ignore"):
        p = [rec[:, k] for k in range(4)]
        for r in range(4):
            out[:, r] = ((((l[r] * p[0]) + (l[4 + r] * p[1])) + (l[8 + r] * p[2])) + (l[12 + r] * p[3])) + o[r]
        out[:, 4:8] = rec[:, 4:8]
        S = [[rec[:, 8 + 4 * c + k] for k in range(4)] for c in range(4)]
        T = [[(((l[r] * S[c][0]) + (l[4 + r] * S[c][1])) + (l[8 + r] * S[c][2])) + (l[12 + r] * S[c][3]) for r in range(4)] for c in range(4)]
        for c in range(4):
            for r in range(4):
                out[:, 8 + 4 * c + r] = (((T[0][r] * l[c]) + (T[1][r] * l[4 + c])) + (T[2][r] * l[8 + c])) + (T[3][r] * l[12 + c])
    assert out.dtype == f32
    return out


def expected(gs4d, rec, xf_rows):
    """what a call writes: [m * n, 24], instance after instance, from the host definition"""
    return gs4d.transform_records_host(rec, np.ascontiguousarray(xf_rows, f32).reshape(-1, 20)).reshape(-1, 24)


# ---- float64 views ------------------------------------------------------------------------------------------------------------------------------
def matrices(xf):
    """(L [row, column], o) of a row in float64"""
    xf = np.asarray(xf, np.float64)
    return xf[:16].reshape(4, 4).T, xf[16:]


def mean_cov(rec):
    """(p [n, 4], Sigma [n, row, column]) of records in float64"""
    r = np.asarray(rec, np.float64).reshape(-1, 24)
    return r[:, :4], r[:, 8:].reshape(-1, 4, 4).transpose(0, 2, 1)


def conditional(p, S, t):
    """mean [n, 3] and covariance [n, 3, 3] of the spatial part at time t (float64), as the draws condition: the time column over Sigma44"""
    k = (t - p[:, 3]) / S[:, 3, 3]
    return p[:, :3] + k[:, None] * S[:, :3, 3], S[:, :3, :3] - S[:, :3, 3, None] * S[:, None, 3, :3] / S[:, 3, 3, None, None]


def conditional_bound(p, S, t, dp, dS):
    """first-order bound of what elementwise errors dp, dS of (p, S) do to conditional(p, S, t): every partial derivative in absolute value"""
    s44 = np.abs(S[:, 3, 3])
    dt, k = np.abs(t - p[:, 3]), np.abs(t - p[:, 3]) / s44
    col, rw = np.abs(S[:, :3, 3]), np.abs(S[:, 3, :3])
    mean = dp[:, :3] + k[:, None] * dS[:, :3, 3] + col * (dp[:, 3] / s44)[:, None] + col * (dt * dS[:, 3, 3] / s44 ** 2)[:, None]
    cov = (dS[:, :3, :3] + (dS[:, :3, 3, None] * rw[:, None, :] + col[:, :, None] * dS[:, None, 3, :3]) / s44[:, None, None]
           + col[:, :, None] * rw[:, None, :] * (dS[:, 3, 3] / s44 ** 2)[:, None, None])
    return mean, cov
