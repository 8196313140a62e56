"""Inputs for the gs4d_rotate_sh tests (include/gs4d.h) and an independent float64 definition of what the call computes.

the definition   numpy only, and it knows nothing of the header's recurrences: the basis of gs4d_shade_sh (its constants, rounded to float32 as the
                 kernel's are, evaluated in float64) at 200 fixed unit directions S; for an orthogonal Q the matrix D with basis(S) D = basis(S Q)
                 by least squares, so that c' = D c satisfies  sum_k c'_k b_k(d) = sum_k c_k b_k(Q^T d).  D comes out block-diagonal, its band-1
                 block is P Q P^T; both are asserted where D is made.
maps             random rotations; rotations times a uniform scale from 1e-3 to 1e3; a mirror; a gs4d_host_affine4 map with velocity and time terms
                 (which must change nothing); hostile maps — a zero block, rank-2 blocks, NaN and Inf entries, a 1e-30 scale whose squared length
                 underflows, a 1e30 scale whose squared length overflows.
rows             shade_cases' coefficients (the bands falling off as trained sets do) behind NaN-pattern payload bytes; hostile rows hold NaN,
                 Inf and 1e30 coefficients.
bars             measured once with the host library over these seeds and multiplied by 4 (DESIGN.md §4 records the measurements).
"""
import functools

import numpy as np

import pose_cases as pc
import scenes
import shade_cases as sc

f32 = np.float32
f64 = np.float64
u32 = np.uint32
INDEX, BLEND4, EACH = 0, 1, 2                                 # GS4D_POSE_INDEX, GS4D_POSE_BLEND4, GS4D_SH_EACH
DEGREES = (0, 1, 2, 3)
TILE = {0: 256, 1: 256, 2: 256, 3: 128}                       # SHROT_TILE, SHROT_TILE_3 (csrc/gs4d_internal.h)
ID_NONE = pc.ID_NONE
AT = {1: 0, 2: 9, 3: 34}                                      # where D_L starts in d[84]

# 4 x the largest figure the host functions reach over the seeds of this file (DESIGN.md §4 records the measurements: 5.12e-8, 2.49e-7 and 1.66e-7)
IDENTITY_BAR = 2.1e-7                                         # |sum c'_k b_k(d) - sum c_k b_k(R^T d)| over sum_k |c_k|
MATRIX_BAR = 1.0e-6                                           # |d[84] entry - least-squares D entry|
PICTURE_BAR = 6.7e-7                                          # |colour by the camera-inverse route - colour through rotate_sh| over sum_k |c_k|


def coeffs(degree):
    return (degree + 1) ** 2


def strides(degree):
    """the minimal row of the degree, the same with a 16-byte payload behind the prefix, and the widest row"""
    return tuple(dict.fromkeys((sc.row_bytes(degree), sc.row_bytes(degree) + 16, 1024)))


def sizes(degree):
    """one row, either side of the degree's tile, two tiles and one"""
    t = TILE[degree]
    return (1, t - 1, t, t + 1, 2 * t + 1)


# ---- the float64 definition ---------------------------------------------------------------------------------------------------------------------
def basis64(d, degree=3):
    """b_0 .. b_(K-1) of gs4d_shade_sh at the unit directions d [n, 3], float64 [n, K], with the kernel's float32 constants"""
    d = np.asarray(d, f64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    C0, C1, C2, C3 = f64(sc.C0), f64(sc.C1), [f64(v) for v in sc.C2], [f64(v) for v in sc.C3]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    b = [np.full_like(x, C0), -C1 * y, C1 * z, -C1 * x,
         C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
         C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy),
         C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    return np.stack(b[:coeffs(degree)], 1)


def unit_directions(n, seed):
    d = np.stack([scenes.normal(n, s, seed=seed) for s in range(3)], 1)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


S = unit_directions(200, 0x5352)                              # the directions of the least-squares fit
PERM = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])      # (x, y, z) -> (-y, z, -x)


def band_matrices64(Q):
    """D [16, 16] float64 with c' = D c for the orthogonal Q (a rotation or a mirror)"""
    Q = np.asarray(Q, f64)
    assert np.abs(Q @ Q.T - np.eye(3)).max() < 1e-12, "not orthogonal"
    D = np.linalg.lstsq(basis64(S), basis64(S @ Q), rcond=None)[0]          # rows of S @ Q are (Q^T d)^T
    off = D.copy()
    for L in range(4):
        off[L * L:(L + 1) ** 2, L * L:(L + 1) ** 2] = 0
    assert np.abs(off).max() < 1e-12 and abs(D[0, 0] - 1) < 1e-12, "the fit is not block-diagonal"
    assert np.abs(D[1:4, 1:4] - PERM @ Q @ PERM.T).max() < 1e-12, "band 1 is not P Q P^T"
    return D


def d84(D):
    """the words of gs4d_host_sh_rotation from a [16, 16] matrix"""
    return np.concatenate([D[L * L:(L + 1) ** 2, L * L:(L + 1) ** 2].reshape(-1) for L in (1, 2, 3)] + [np.zeros(1)])


def frame64(l):
    """the Gram-Schmidt frame of the spatial block of l (20 or 16 floats) in float64: R [3, 3] with R[:, c] = e_c"""
    a = np.asarray(l, f64)[:12].reshape(3, 4)[:, :3]                         # a[c] = column c
    e0 = a[0] / np.linalg.norm(a[0])
    u1 = a[1] - (e0 @ a[1]) * e0
    e1 = u1 / np.linalg.norm(u1)
    u2 = a[2] - (e0 @ a[2]) * e0 - (e1 @ a[2]) * e1
    return np.stack([e0, e1, u2 / np.linalg.norm(u2)], 1)


def identity_ratio(c_in, c_out, R, degree, seed):
    """the largest |sum_k c'_k b_k(d) - sum_k c_k b_k(R^T d)| / sum_k |c_k| over 50 directions and the channels: float64 from the float32 words
    c_in, c_out [n, >= 3 K] of rows that all went under R"""
    K = coeffs(degree)
    d = unit_directions(50, seed)
    ci, co = (np.asarray(np.asarray(c)[:, :3 * K], f64).reshape(-1, K, 3) for c in (c_in, c_out))
    lhs = np.einsum("dk,nkc->ndc", basis64(d, degree), co)
    rhs = np.einsum("dk,nkc->ndc", basis64(d @ R, degree), ci)
    return float((np.abs(lhs - rhs) / np.abs(ci).sum(1)[:, None, :]).max())


# ---- maps ------------------------------------------------------------------------------------------------------------------------------------------
def quaternion(k, seed=0x5351):
    q = np.array([scenes.normal(1, 4 * k + s, seed=seed)[0] for s in range(4)])
    return (q / np.linalg.norm(q)).astype(f32)


def quat_matrix(q):
    """the rotation matrix of a unit quaternion w x y z, float64"""
    w, x, y, z = (f64(v) for v in q)
    s = w * w + x * x + y * y + z * z
    return np.array([[1 - 2 * (y * y + z * z) / s, 2 * (x * y - w * z) / s, 2 * (x * z + w * y) / s],
                     [2 * (x * y + w * z) / s, 1 - 2 * (x * x + z * z) / s, 2 * (y * z - w * x) / s],
                     [2 * (x * z - w * y) / s, 2 * (y * z + w * x) / s, 1 - 2 * (x * x + y * y) / s]])


SCALES = (1e-3, 0.37, 2.0, 1e3)


@functools.lru_cache(maxsize=None)
def _maps(gs4d):
    out = {}
    for k in range(6):
        out[f"rotation_{k}"] = gs4d.affine4(quaternion(k))
    for k, s in enumerate(SCALES):
        out[f"similarity_{s:g}"] = gs4d.affine4(quaternion(10 + k), scale=s)
    mirror = gs4d.affine4(quaternion(20))
    mirror[8:11] = -mirror[8:11]                                             # column 2 turned round: a rotation times the mirror z -> -z
    out["mirror"] = mirror
    out["moving"] = gs4d.affine4(quaternion(0), translate=(3.0, -40.0, 7.5), velocity=(1.5, -0.75, 0.25), time_scale=0.5, time_offset=3.25)
    out["identity"] = gs4d.affine4()
    for v in out.values():
        v.setflags(write=False)
    return out


def maps(gs4d):
    """name -> 20 float32: the maps that rotate"""
    return dict(_maps(gs4d))


def hostile_maps(gs4d):
    """name -> (20 float32, rotates): True / False where the header's rule decides it whatever the rounding, None where rounding decides"""
    base = gs4d.affine4(quaternion(30), scale=1.5, translate=(1.0, 2.0, 3.0))
    out = {}

    def one(name, rotates, edit):
        r = base.copy()
        edit(r)
        out[name] = (r, rotates)
    one("zero_block", False, lambda r: r.__setitem__(slice(0, 12), 0.0))
    one("negative_zero_block", False, lambda r: r.__setitem__(slice(0, 12), -0.0))
    one("zero_column_1", False, lambda r: r.__setitem__(slice(4, 7), 0.0))
    one("rank_2_equal_columns", None, lambda r: r.__setitem__(slice(8, 11), r[0:3].copy()))
    one("rank_2_parallel_columns", None, lambda r: r.__setitem__(slice(4, 7), -2.0 * r[0:3]))
    one("nan_entry", False, lambda r: r.__setitem__(5, np.nan))
    one("nan_first", False, lambda r: r.__setitem__(0, np.nan))
    one("inf_entry", False, lambda r: r.__setitem__(9, np.inf))
    one("scale_1e-30", False, lambda r: r.__setitem__(slice(0, 12), r[0:12] * f32(1e-30) / f32(1.5)))
    one("scale_1e30", False, lambda r: r.__setitem__(slice(0, 12), r[0:12] * f32(1e30)))
    one("time_terms_nan", True, lambda r: (r.__setitem__(slice(12, 16), np.nan), r.__setitem__(3, np.nan), r.__setitem__(7, np.inf), r.__setitem__(slice(16, 20), np.nan)))
    return out


def map_table(gs4d, m, call=0):
    """[m, 20] float32: the maps that rotate and the hostile ones taken round and round, shifted by the call"""
    pool = list(maps(gs4d).values()) + [v for v, _ in hostile_maps(gs4d).values()]
    return np.stack([pool[(5 * call + k) % len(pool)] for k in range(m)]).astype(f32) if m else np.zeros((0, 20), f32)


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------------
def table(n, degree, stride, seed=0x5350, hostile=False):
    """float32 [n, stride / 4]: coefficients for the degree, then NaN-pattern payload words up to the stride.  hostile: every 7th row holds a NaN,
    an Inf or a 1e30 coefficient, every 11th a -0"""
    c = sc.coefficients(n, degree, seed=seed + degree)
    if hostile and degree:
        K3 = 3 * coeffs(degree)
        i = np.arange(0, n, 7)
        c[i, 3 + (i // 7) % (K3 - 3)] = np.array([np.nan, np.inf, -np.inf, 1e30], f32)[(i // 7) % 4]
        i = np.arange(0, n, 11)
        c[i, 3 + (i // 11 + 5) % (K3 - 3)] = f32(-0.0)
    return sc.table(c, stride)


def used_words(degree):
    return 3 * coeffs(degree)


# ---- which map a row goes under ---------------------------------------------------------------------------------------------------------------------
def chosen_maps(xf, bind, form, bind_stride, n):
    """(a [n, 20] float32, mapped bool [n]) by the text of gs4d_pose_records in numpy float32, one operation at a time"""
    xf = np.ascontiguousarray(xf, f32).reshape(-1, 20)
    m = xf.shape[0]
    j, w = pc.unpacked(bind, form, n, bind_stride)
    rows = np.concatenate([xf, np.zeros((1, 20), f32)])
    part = j < m
    pick = np.where(part, j, m)
    with np.errstate(all="ignore"):
        if form == INDEX:
            return rows[pick[:, 0]], part[:, 0]
        a, mapped = np.zeros((n, 20), f32), np.zeros(n, bool)
        for k in range(4):
            prod = w[:, k, None] * rows[pick[:, k]]
            first, later = part[:, k] & ~mapped, part[:, k] & mapped
            a = np.where(first[:, None], prod, np.where(later[:, None], a + prod, a))
            mapped = mapped | part[:, k]
    assert a.dtype == f32
    return a, mapped


def rotated_mask(gs4d, xf, n, bind=None, form=EACH, bind_stride=0):
    """bool [rows of the result]: the rows the call turns (the others are copied), by the library's own frame rule"""
    xf = np.ascontiguousarray(xf, f32).reshape(-1, 20)
    if form == EACH:
        return np.repeat(np.array([gs4d.sh_rotation(r)[0] for r in xf], bool), n)
    a, mapped = chosen_maps(xf, bind, form, bind_stride, n)
    return np.array([bool(mapped[i]) and gs4d.sh_rotation(a[i])[0] for i in range(n)], bool)


def same_rows(got, want):
    """bool [n, words]: equal as uint32, or a NaN on both sides"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return (got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))


def assert_rows(got, want, src, rotated, degree, what):
    """the rule of gs4d.h: a rotated row has the host's bits but for NaN = NaN; its DC words and everything past the coefficients, and every
    copied row, are the source's bytes (src: the source row of every result row)"""
    assert np.size(got) == np.size(want) == np.size(src), f"{what}: {np.size(got)} words for {np.size(want)}"
    if len(rotated) == 0:
        return
    got, want, src = (np.ascontiguousarray(a, f32).reshape(len(rotated), -1) for a in (got, want, src))
    ok = same_rows(got, want)
    assert ok.all(), f"{what}: {int((~ok).any(1).sum())} of {got.shape[0]} rows differ, first word at {np.argwhere(~ok)[0].tolist()}"
    rot = np.asarray(rotated, bool) & (degree > 0)
    assert np.array_equal(got.view(u32)[~rot], src.view(u32)[~rot]), f"{what}: a copied row is not byte-equal"
    K3 = used_words(degree)
    assert np.array_equal(got.view(u32)[:, :3], src.view(u32)[:, :3]) and np.array_equal(got.view(u32)[:, K3:], src.view(u32)[:, K3:]), \
        f"{what}: DC words or the bytes past the coefficients changed"


# ---- the picture: the camera-inverse route of gs4d_transform_records against the route through gs4d_rotate_sh -----------------------------------------
PICTURE_N, PICTURE_DEGREE = 300, 3
PICTURE_T, PICTURE_CAM = sc.T, sc.CAM                         # the cloud lies in [-50, 50]^3 and moves a few units: the camera stays 80 units off


def picture_set(which):
    """(records [300, 24], table [300, 48]) of a 3D ("3d": static records) or a 4D set ("4d": velocities, mu_t around T)"""
    return sc.records(PICTURE_N, seed=0x5356, static=which == "3d"), table(PICTURE_N, PICTURE_DEGREE, sc.row_bytes(PICTURE_DEGREE), seed=0x5357)


def picture_maps(gs4d):
    """a rigid map and a similarity of scale 2"""
    return {"rigid": gs4d.affine4(quaternion(40), translate=(5.0, -3.0, 8.0)), "scale_2": gs4d.affine4(quaternion(41), scale=2.0, translate=(-4.0, 6.0, 2.5))}


def object_maps(gs4d):
    """three objects, each with a map of its own: [3, 20]"""
    return np.stack([gs4d.affine4(quaternion(42), translate=(12.0, 0.0, -5.0)), gs4d.affine4(quaternion(43), scale=2.0, translate=(-9.0, 4.0, 3.0)),
                     gs4d.affine4(quaternion(44), scale=0.5, translate=(0.0, -7.0, 6.0))]).astype(f32)


def inverse_camera(l, cam):
    """M^-1 cam for the spatial part of a map (20 floats), float64 rounded to float32"""
    l = np.asarray(l, f64)
    A = l[:12].reshape(3, 4)[:, :3].T                                        # A[r, c] = l[4c + r]
    return np.linalg.solve(A, np.asarray(cam, f64) - l[16:19]).astype(f32)


def route_a_host(rec, rows, l, cam, t):
    """the header's workaround by the host definitions: the colours of the SOURCE set seen from M^-1 cam (transform_records copies them)"""
    return sc.shade(rec, rows, PICTURE_DEGREE, t, inverse_camera(l, cam))


def route_b_host(gs4d, rec, rows, l, cam, t):
    """transform, rotate_sh, shade with the true camera, by the host definitions"""
    return sc.shade(gs4d.transform_records_host(rec, np.asarray(l, f32)), gs4d.rotate_sh_host(rows, np.asarray(l, f32).reshape(1, 20), PICTURE_DEGREE), PICTURE_DEGREE, t, cam)


def colour_ratio(a, b, rows):
    """the largest |a - b| over sum_k |c_k| of the record's channel"""
    K = coeffs(PICTURE_DEGREE)
    mass = np.abs(np.asarray(rows, f64)[:, :3 * K].reshape(-1, K, 3)).sum(1)
    return float((np.abs(np.asarray(a, f64) - np.asarray(b, f64)) / mass).max())
