"""gs4d_shade_sh (include/gs4d.h) restated: the definition of the header in numpy float32, one numpy call per operation so that
nothing is contracted; the case generators; and a float64 evaluation of the real spherical-harmonic basis along the same direction, built from
Legendre polynomials and factorials, not from the constants.

Plain numpy: importable and usable without a GPU and without the library.  A table is handled as float32 [n, words] (words = stride / 4); the
coefficient c_k of channel ch is word 3k + ch."""
import math

import numpy as np

import scenes

f32 = np.float32
TILE = 256                                 # records per workgroup of k_shade_sh (SHADE_TILE, gs4d_internal.h)
SIZES = tuple(dict.fromkeys((1, 63, 64, 65, 255, 256, 257, TILE + 1, 3 * TILE + 1)))      # (one tile + 1 is 257 while TILE is 256)
PADDED_STRIDE, MAX_STRIDE = 208, 1024
NAN_BITS = (0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF)      # quiet and signalling NaN patterns for the padding of a row

C0 = f32(0.28209479177387814)
C1 = f32(0.4886025119029199)
C2 = tuple(f32(v) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396))
C3 = tuple(f32(v) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
                            -0.5900435899266435))


def coeffs(degree):
    return (degree + 1) ** 2


def row_bytes(degree):
    """the minimal stride: 12 (degree + 1)^2 rounded up to 16"""
    return (12 * coeffs(degree) + 15) // 16 * 16


def strides(degree):
    return tuple(sorted({row_bytes(degree), PADDED_STRIDE, MAX_STRIDE}))


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------
def direction(rec, t, cam):
    """(x, y, z, directed) of every record: float32 arrays, every operation one numpy call"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    t, cam = f32(t), np.asarray(cam, f32)
    with np.errstate(all="ignore"):
        k = np.multiply(np.divide(f32(1.0), rec[:, 23]), np.subtract(t, rec[:, 3]))
        d = [np.subtract(np.add(rec[:, a], np.multiply(k, rec[:, 20 + a])), cam[a]) for a in range(3)]
        len2 = np.add(np.add(np.multiply(d[0], d[0]), np.multiply(d[1], d[1])), np.multiply(d[2], d[2]))
        inv = np.divide(f32(1.0), np.sqrt(len2))
        x, y, z = (np.multiply(d[a], inv) for a in range(3))
        directed = (len2 > 0) & np.isfinite(len2)
    assert x.dtype == f32 and len2.dtype == f32
    return x, y, z, directed


def basis(x, y, z, degree):
    """b_0 .. b_(K-1) of gs4d.h, each a float32 array"""
    mul, sub = np.multiply, np.subtract
    b = [np.full(x.shape, C0, f32)]
    with np.errstate(all="ignore"):
        if degree >= 1:
            b += [mul(-C1, y), mul(C1, z), mul(-C1, x)]
        if degree >= 2:
            xx, yy, zz, xy, yz, xz = mul(x, x), mul(y, y), mul(z, z), mul(x, y), mul(y, z), mul(x, z)
            b += [mul(C2[0], xy), mul(C2[1], yz), mul(C2[2], sub(sub(mul(f32(2.0), zz), xx), yy)), mul(C2[3], xz), mul(C2[4], sub(xx, yy))]
        if degree >= 3:
            b += [mul(mul(C3[0], y), sub(mul(f32(3.0), xx), yy)),
                  mul(mul(C3[1], xy), z),
                  mul(mul(C3[2], y), sub(sub(mul(f32(4.0), zz), xx), yy)),
                  mul(mul(C3[3], z), sub(sub(mul(f32(2.0), zz), mul(f32(3.0), xx)), mul(f32(3.0), yy))),
                  mul(mul(C3[4], x), sub(sub(mul(f32(4.0), zz), xx), yy)),
                  mul(mul(C3[5], z), sub(xx, yy)),
                  mul(mul(C3[6], x), sub(xx, mul(f32(3.0), yy)))]
    assert len(b) == coeffs(degree) and all(v.dtype == f32 for v in b)
    return b


def shade(rec, table, degree, t, cam):
    """rgb [n, 3] float32 of the records `rec` [n, 24] from the rows `table` (float32 [n, >= 3 K]) — the bits gs4d_shade_sh writes"""
    table = np.ascontiguousarray(table, f32)
    x, y, z, directed = direction(rec, t, cam)
    b = basis(x, y, z, degree)
    out = np.empty((x.shape[0], 3), f32)
    with np.errstate(all="ignore"):
        for ch in range(3):
            dc = np.multiply(b[0], table[:, ch])
            acc = dc
            for k in range(1, coeffs(degree)):
                acc = np.add(acc, np.multiply(b[k], table[:, 3 * k + ch]))
            v = np.add(np.where(directed, acc, dc), f32(0.5))
            out[:, ch] = np.where(v > 0, v, f32(0.0))
    return out


def shaded_records(rec, table, degree, t, cam, n=None):
    """the records with floats 4..6 of the first n replaced"""
    out = np.array(rec, f32).reshape(-1, 24)
    n = out.shape[0] if n is None else n
    out[:n, 4:7] = shade(out[:n], np.asarray(table)[:n], degree, t, cam)
    return out


# ---- float64: the real spherical harmonics themselves -------------------------------------------------------------------------------------------
def real_sh64(x, y, z, degree):
    """Y_l^m(x, y, z) in float64 for l <= degree, index l^2 + l + m: sqrt((2l+1)/(4 pi) (l-|m|)!/(l+|m|)!) times the m-th derivative of the
    Legendre polynomial P_l at z times Re / Im of (x + iy)^|m|, times sqrt 2 for m != 0, with the Condon-Shortley phase (-1)^m — the
    convention of the 3DGS implementation (its b_1 = -C1 y)."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    out = []
    for l in range(degree + 1):
        for m in range(-l, l + 1):
            a = abs(m)
            norm = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - a) / math.factorial(l + a))
            pl = np.polynomial.legendre.Legendre.basis(l).deriv(a)(z) if a else np.polynomial.legendre.Legendre.basis(l)(z)
            w = (x + 1j * y) ** a
            ang = 1.0 if m == 0 else math.sqrt(2.0) * (w.real if m > 0 else w.imag)
            out.append((-1.0) ** a * norm * pl * ang)
    return out


def shade64(rec, table, degree, t, cam):
    """(colour before the clamp, 0.5 + sum |b_k c_k|) in float64 along the direction the float32 definition takes — for records that have one"""
    x, y, z, directed = direction(rec, t, cam)
    assert directed.all()
    d = np.stack([x, y, z], 1).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = real_sh64(d[:, 0], d[:, 1], d[:, 2], degree)
    c = np.asarray(table, np.float64)
    val, scale = np.full((len(d), 3), 0.5), np.full((len(d), 3), 0.5)
    for k in range(coeffs(degree)):
        term = b[k][:, None] * c[:, 3 * k:3 * k + 3]
        val += term
        scale += np.abs(term)
    return val, scale


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
T = 25.0
CAM = (31.0, -12.5, 140.0)


def records(n, seed=0x5348, static=False):
    """n records of a moving cloud: positions in [-50, 50]^3, mu_t within 2 of T, velocities in [-5, 5]^3, Sigma44 in [0.25, 2.25]; every other
    word a function of its index, so that a word that moves shows"""
    u = lambda s: scenes.uniform(n, s, seed=seed)
    rec = ((np.arange(n * 24, dtype=np.uint32).reshape(n, 24) * np.uint32(2654435761)) >> np.uint32(9) | np.uint32(0x3F000000)).view(f32).copy()
    rec[:, 0:3] = np.stack([u(0), u(1), u(2)], 1) * 100.0 - 50.0
    rec[:, 3] = T - 2.0 + 4.0 * u(3)
    rec[:, 20:23] = np.stack([u(4), u(5), u(6)], 1) * 10.0 - 5.0
    rec[:, 23] = 0.25 + 2.0 * u(7)
    if static:
        rec[:, 3], rec[:, 20:23], rec[:, 23] = 0.0, 0.0, 1.0
    return rec


def coefficients(n, degree, seed=0x5349):
    """float32 [n, 3 K]: the DC term in [-1, 1], the bands falling off as trained sets do (a third per band), signs mixed"""
    K = coeffs(degree)
    c = np.stack([scenes.uniform(n, s, seed=seed) for s in range(3 * K)], 1) * 2.0 - 1.0
    band = np.repeat(np.array([int(math.isqrt(k)) for k in range(K)]), 3)
    return (c * (3.0 ** -band)[None, :]).astype(f32)


def table(coeff, stride, pad_nan=True):
    """float32 [n, stride / 4]: the coefficients, then padding — NaN bit patterns, so that any read past the prefix shows in the colour"""
    n, used = coeff.shape
    assert stride % 16 == 0 and stride >= 4 * used
    out = np.empty((n, stride // 4), np.uint32)
    pad = np.array(NAN_BITS, np.uint32)[(np.arange(n)[:, None] + np.arange(stride // 4)[None, :]) % len(NAN_BITS)]
    out[:] = pad if pad_nan else 0
    out[:, :used] = np.ascontiguousarray(coeff, f32).view(np.uint32)
    return out.view(f32)


def hostile(n=TILE + 37, seed=0x534A):
    """(name, records, t, cam) — the classes of tests/hostile_cases.py that fit the call: implants at record 0, in the second wave and last, the
    rest a clean cloud"""
    out = []
    slots = [0, 64 + 5, n - 1]

    def one(name, edit, t=T, cam=CAM):
        rec = records(n, seed)
        for j, i in enumerate(slots):
            edit(rec[i], j)
        out.append((name, rec, t, cam))

    def setf(field, values):
        def edit(r, j):
            r[field] = values[j % len(values)]
        return edit
    one("position_nan", setf(0, [np.nan]))
    one("position_inf", setf(1, [np.inf, -np.inf]))
    one("position_1e30", setf(2, [1e30, -1e30, 3e38]))
    one("sigma44_zero", setf(23, [0.0, -0.0]))
    one("sigma44_negative", setf(23, [-1.0, -0.25]))
    one("sigma44_denormal", setf(23, [1e-40, -1e-40, 1e-45]))
    one("sigma44_inf_nan", setf(23, [np.inf, np.nan]))
    one("mu_t_nan_inf", setf(3, [np.nan, np.inf, -np.inf]))
    one("velocity_overflow", setf(20, [3e38, -3e38, np.inf]))
    one("time_nan", lambda r, j: None, t=np.nan)
    one("time_inf", lambda r, j: None, t=np.inf)
    one("time_3e38", lambda r, j: None, t=3e38)
    one("camera_nan", lambda r, j: None, cam=(np.nan, 0.0, 0.0))
    one("camera_inf", lambda r, j: None, cam=(0.0, -np.inf, 0.0))
    # a camera on a record: a static one, whose conditioned mean is its position exactly
    rec = records(n, seed)
    rec[slots[1], 20:23] = 0.0
    out.append(("camera_on_a_record", rec, T, tuple(float(v) for v in rec[slots[1], 0:3])))
    return out
