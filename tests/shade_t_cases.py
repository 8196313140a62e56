"""gs4d_shade_sh_t and gs4d_collapse_sh (include/gs4d.h) restated: the weights of the time blocks and the effective row in numpy
float32, one numpy call per operation so that nothing is contracted; the case generators; and the 4DGS formula in float64, built block by block
from tests/shade_cases.py's real spherical harmonics.

Plain numpy: importable and usable without a GPU and without the library.  A 4D table is handled as float32 [n, words] (words = stride / 4); with
K = (degree + 1)^2, coefficient k of block b, channel ch, is word 3 (b K + k) + ch."""
import numpy as np

import shade_cases as sc

f32, f64, u32 = np.float32, np.float64, np.uint32
TILE = 256                                 # records per workgroup of k_shade_sh_t and k_collapse_sh (SHADE_T_TILE, gs4d_internal.h)
SIZES = tuple(dict.fromkeys((1, 63, 64, 65, 255, 256, 257, 769, TILE - 1, TILE, TILE + 1, 3 * TILE + 1)))
DEGREES, DEGREES_T = (0, 1, 2, 3), (0, 1, 2)
PAIRS = tuple((d, dt) for d in DEGREES for dt in DEGREES_T)
PERIODS = (4.0, 50.0)                      # against mu_t within 2 of T: |u| up to 1/2, and a slow series
BLOCK_SCALE = (1.0, 0.5, 0.25)

# T_j = float32((-1)^j (2 pi)^(2j) / (2j)!), j = 1 .. 6, and the bits gs4d.h lists
T_SERIES = tuple(f32(v) for v in (-19.739208802178716, 64.93939402266828, -85.45681720669371, 60.24464137187664, -26.426256783374388, 7.903536371318465))
T_BITS = (0xc19de9e6, 0x4281e0f8, 0xc2aae9e4, 0x4270fa83, 0xc1d368f9, 0x40fce9c5)


def row_words(degree):
    return 3 * sc.coeffs(degree)


def row_bytes_t(degree, degree_t):
    """the minimal stride of a 4D row: 12 (degree + 1)^2 (degree_t + 1) rounded up to 16"""
    return (4 * row_words(degree) * (degree_t + 1) + 15) // 16 * 16


def strides_t(degree, degree_t):
    """the minimal row, the same with 16 bytes of NaN padding behind it, and the widest row"""
    return tuple(dict.fromkeys((row_bytes_t(degree, degree_t), row_bytes_t(degree, degree_t) + 16, 1024)))


def dst_strides(degree):
    return tuple(dict.fromkeys((sc.row_bytes(degree), sc.row_bytes(degree) + 16, 1024)))


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------
def cos_turns(v):
    """w of gs4d.h for the float32 array v (finite entries; others give whatever the operations give)"""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        r = np.subtract(v, np.rint(v))
        a = np.abs(r)
        neg = a > f32(0.25)
        x = np.where(neg, np.subtract(f32(0.5), a), a)
        s = np.multiply(x, x)
        p = np.full(v.shape, T_SERIES[5], f32)
        for tj in T_SERIES[4::-1]:
            p = np.add(np.multiply(p, s), tj)
        c = np.add(np.multiply(p, s), f32(1.0))
        w = np.where(neg, np.negative(c), c)
    assert w.dtype == f32 and s.dtype == f32
    return w


def weights(degree_t, t, inv_period, mu_t):
    """(w [2, n] float32, part [2, n] bool): w[b - 1] of block b = 1 .. degree_t and whether it takes part (w of one that does not: 0)"""
    mu_t = np.atleast_1d(np.asarray(mu_t, f32))
    w, part = np.zeros((2,) + mu_t.shape, f32), np.zeros((2,) + mu_t.shape, bool)
    with np.errstate(all="ignore"):
        u = np.multiply(np.subtract(f32(t), mu_t), f32(inv_period))
        assert u.dtype == f32
        for b in range(1, degree_t + 1):
            v = np.multiply(f32(b), u)
            part[b - 1] = np.isfinite(v)
            w[b - 1] = np.where(part[b - 1], cos_turns(v), f32(0.0))
    return w, part


def collapse(rec, table, degree, degree_t, t, inv_period, dst_stride=None):
    """float32 [n, dst_stride / 4] (default: the minimal row of the degree): the rows gs4d_collapse_sh writes for the records rec [n, 24]"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    table = np.ascontiguousarray(table, f32)
    W = row_words(degree)
    w, part = weights(degree_t, t, inv_period, rec[:, 3])
    e = table[:, :W].copy()
    with np.errstate(all="ignore"):
        for b in range(1, degree_t + 1):
            term = np.add(e, np.multiply(w[b - 1][:, None], table[:, b * W:(b + 1) * W]))
            e = np.where(part[b - 1][:, None], term, e)
    assert e.dtype == f32
    out = np.zeros((rec.shape[0], (sc.row_bytes(degree) if dst_stride is None else dst_stride) // 4), f32)
    out[:, :W] = e
    return out


def shaded_records(rec, table, degree, degree_t, t, inv_period, cam, n=None):
    """the records with floats 4..6 of the first n replaced: shade_cases.shade of the collapsed rows — the bits gs4d_shade_sh_t writes"""
    out = np.array(rec, f32).reshape(-1, 24)
    n = out.shape[0] if n is None else n
    out[:n, 4:7] = sc.shade(out[:n], collapse(out[:n], np.asarray(table)[:n], degree, degree_t, t, inv_period), degree, t, cam)
    return out


def same_rows(got, want):
    """bool [n, words]: equal as uint32, or a NaN on both sides"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return (got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))


# ---- float64: the 4DGS formula -------------------------------------------------------------------------------------------------------------------
def shade64_t(rec, table, degree, degree_t, t, inv_period, cam):
    """(0.5 + sum_b cos(2 pi b u) sum_k Y_k c_(b,k), 0.5 + sum_b |cos(2 pi b u)| sum_k |Y_k c_(b,k)|) in float64, u from the float32 inputs in float64"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    W = row_words(degree)
    u = (f64(f32(t)) - rec[:, 3].astype(f64)) * f64(f32(inv_period))
    val, scale = np.full((rec.shape[0], 3), 0.5), np.full((rec.shape[0], 3), 0.5)
    for b in range(degree_t + 1):
        v, s = sc.shade64(rec, np.asarray(table)[:, b * W:(b + 1) * W], degree, t, cam)
        c = np.cos(2.0 * np.pi * b * u)[:, None]
        val += c * (v - 0.5)
        scale += np.abs(c) * (s - 0.5)
    return val, scale


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
def coefficients_t(n, degree, degree_t, seed=0x5354, hostile=False):
    """float32 [n, 3 K (degree_t + 1)]: block b is shade_cases.coefficients scaled by 1, 1/2, 1/4.  hostile: every 7th row holds a NaN, an Inf or a
    1e30 coefficient and every 11th a -0, in EVERY block"""
    W = row_words(degree)
    c = np.concatenate([sc.coefficients(n, degree, seed=seed + 16 * b) * f32(BLOCK_SCALE[b]) for b in range(degree_t + 1)], 1)
    if hostile:
        for b in range(degree_t + 1):
            i = np.arange(b, n, 7)
            c[i, b * W + (i // 7) % W] = np.array([np.nan, np.inf, -np.inf, 1e30], f32)[(i // 7 + b) % 4]
            i = np.arange(b, n, 11)
            c[i, b * W + (i // 11 + 5) % W] = f32(-0.0)
    return c


def table_t(n, degree, degree_t, stride, seed=0x5354, hostile=False):
    """float32 [n, stride / 4]: the blocks, then NaN bit patterns, so that any read past them shows"""
    return sc.table(coefficients_t(n, degree, degree_t, seed, hostile), stride)


INF, NAN = float("inf"), float("nan")
# (name, t, inv_period): the times and periods that decide who takes part — with mu_t within 2 of sc.T
HOSTILE_TIMES = (
    ("t_nan", NAN, 0.25), ("t_inf", INF, 0.25), ("t_minus_inf", -INF, 0.25), ("t_3e38", 3e38, 0.25),
    ("inv_period_nan", sc.T, NAN), ("inv_period_inf", sc.T, INF), ("inv_period_minus_inf", sc.T, -INF), ("inv_period_0", sc.T, 0.0),
    ("inv_period_1e30", sc.T, 1e30),
    ("2u_overflows", sc.T, 1.5e38),        # |t - mu_t| up to 2: u finite up to 3e38, 2 u overflows where |t - mu_t| > 1.14 — block 1 in, block 2 out
)


def hostile_mu_t(n, seed=0x5355):
    """records with a NaN, +Inf and -Inf mu_t at record 0, in the second wave and last"""
    rec = sc.records(n, seed)
    for i, v in zip((0, 64 + 5, n - 1), (np.nan, np.inf, -np.inf)):
        rec[i, 3] = v
    return rec


# ---- the picture of a posed 4D table: degree 3, degree_t 2, rows of 576 bytes seen as 3 n rows of 192 ---------------------------------------------
POSED_DEGREE, POSED_DEGREE_T, POSED_INV_PERIOD = 3, 2, 0.25


def posed_set():
    """(records [300, 24], table [300, 144]): sh_rotate_cases.picture_set("4d") with two more blocks, scaled 1/2 and 1/4"""
    import sh_rotate_cases as rc
    rec, rows = rc.picture_set("4d")
    more = [rc.table(rc.PICTURE_N, 3, 192, seed=0x5358 + 8 * b) * f32(BLOCK_SCALE[b]) for b in (1, 2)]
    return rec, np.ascontiguousarray(np.concatenate([rows] + more, 1), f32)


def posed_routes_host(gs4d, rec, tab, l, cam, t):
    """(a, b, stale) by the host definitions: a — the source seen from M^-1 cam; b — transform_records, rotate_sh of the table as 3 n rows of
    192 bytes, shade_sh_t with the true camera; stale — b without the rotation"""
    import sh_rotate_cases as rc
    n, l = rec.shape[0], np.asarray(l, f32)
    shade = lambda r, tb, c: gs4d.shade_sh_t_host(r, tb, POSED_DEGREE, POSED_DEGREE_T, t, POSED_INV_PERIOD, c)[:, 4:7]
    a = shade(rec, tab, rc.inverse_camera(l, cam))
    moved = gs4d.transform_records_host(rec, l)
    turned = gs4d.rotate_sh_host(tab.reshape(3 * n, 48), l.reshape(1, 20), POSED_DEGREE).reshape(n, 144)
    return a, shade(moved, turned, cam), shade(moved, tab, cam)


def colour_ratio_t(a, b, tab):
    """the largest |a - b| over sum |c| of the record's channel, over ALL blocks"""
    mass = np.abs(np.asarray(tab, f64)).reshape(tab.shape[0], -1, 3).sum(1)
    return float((np.abs(np.asarray(a, f64) - np.asarray(b, f64)) / mass).max())
