"""Inputs for the gs4d_slice_records tests (include/gs4d.h): record sets, slice queries, and the definition restated as a numpy float32
loop of the header's text, with libm's expf called through ctypes.

sets     those of tests/transform_cases.py ("3d", "4d_vel", "4d_2q", "hostile") and "neg_zero", built for the -0 argument of the definition: records
         with a coordinate of exactly -0.0 whose velocity term is -0, covariance elements that are -0, Sigma44 in {1, 0.25, 3}, an asymmetric time
         row / column, and some records with mu_t exactly at a query time.
queries  (t, min_opacity, mu_t_out, s44_out): t at, near and far from the sets' mu_t (the clean sets have mu_t in [0, 50] and a Sigma44 of about
         0.1 .. 3: at t = 25 expf underflows to exactly 0 for part of every set, at t = 1000 for all of it), min_opacity in (0, 0.25), s44_out in
         (1, 0.5, +inf), mu_t_out in (t, 0).
"""
import ctypes
import ctypes.util
import functools
import itertools

import numpy as np

import transform_cases as tc

f32 = np.float32
SETS = tc.SETS + ("neg_zero",)
SIZES = (1, 63, 64, 65, 255, 256, 257, 769)                  # one record, either side of a wave and of a tile of 256, three tiles plus one
FIRSTS = (0, 7)
TIMES = (25.0, 25.3, 0.0, 1000.0)
MIN_OPACITIES = (0.0, 0.25)
S44_OUTS = (1.0, 0.5, float("inf"))
MU_T_OUTS = ("t", 0.0)
bits, same_bits = tc.bits, tc.same_bits
COLUMN, ROW = (11, 15, 19), (20, 21, 22)                     # the time column (what the draw reads) and the time row (what the keys read) of a record


@functools.lru_cache(maxsize=None)
def queries():
    """every (t, min_opacity, mu_t_out, s44_out) of the product above"""
    return tuple((t, m, t if mu == "t" else mu, s) for t, m, s, mu in itertools.product(TIMES, MIN_OPACITIES, S44_OUTS, MU_T_OUTS))


def query_for(call):
    """the query of the call-th call of a test: 7 is coprime to the 48 queries, so 48 calls in a row see all of them"""
    q = queries()
    return q[(7 * call) % len(q)]


# ---- record sets --------------------------------------------------------------------------------------------------------------------------------
def neg_zero(gs4d, n, seed=0x534C):
    """the -0 set, from a clean 4D_VEL set (mu_t in [0, 50]); every record gets one of six edits, round and round"""
    rec = tc.records(gs4d, "4d_vel", n, seed=seed).copy()
    i = np.arange(n)
    rec[:, 23] = np.array([1.0, 0.25, 3.0], f32)[i % 3]
    kind = (i // 3) % 6
    k = kind == 0                                            # x = -0 and a velocity column of -0 in x: k * (-0) = -0 for t > mu_t, (-0) + (-0) = -0
    rec[k, 0], rec[k, 11], rec[k, 20] = -0.0, -0.0, -0.0
    rec[k, 3] = 5.0                                          # (before every non-zero query time: k > 0)
    k = kind == 1                                            # y = -0 with a velocity of +0 in y and t < mu_t: k < 0, k * (+0) = -0
    rec[k, 1], rec[k, 15], rec[k, 21] = -0.0, 0.0, 0.0
    rec[k, 3] = 2000.0
    k = kind == 2                                            # covariance elements that are -0, and a time column whose product with the row is +0
    rec[k, 9], rec[k, 12], rec[k, 18] = -0.0, -0.0, -0.0
    rec[k, 11], rec[k, 20] = -0.0, -0.0
    k = kind == 3                                            # an asymmetric time row / column
    rec[k, 20] = rec[k, 11] * f32(1.25) + f32(0.01)
    rec[k, 22] = -rec[k, 19]
    k = kind == 4                                            # mu_t exactly at a query time: dt = +0
    rec[k, 3] = 25.0
    k = kind == 5                                            # a whole centre of -0 at rest: every term is a signed zero
    rec[k, 0:3] = -0.0
    rec[np.ix_(k, COLUMN)] = -0.0
    rec[np.ix_(k, ROW)] = -0.0
    rec[k, 3] = 25.0
    return np.ascontiguousarray(rec)


def records(gs4d, which, n):
    return neg_zero(gs4d, n) if which == "neg_zero" else tc.records(gs4d, which, n)


def symmetric(rec):
    """per record: the time row has the bits of the time column (the keys read the row, the draws the column)"""
    return (bits(rec[:, COLUMN]) == bits(rec[:, ROW])).all(1)


# ---- the definition, restated -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def libm_expf():
    fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").expf
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return fn


def expf(x):
    """libm's expf, element by element"""
    fn = libm_expf()
    return np.array([fn(float(v)) for v in np.asarray(x, f32).ravel()], f32).reshape(np.shape(x))


def by_the_text(rec, t, min_opacity, mu_t_out, s44_out, exp=expf):
    """the header's text in numpy float32, one operation at a time (numpy rounds every product and every sum on its own): records [n, 24]"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    t, m = f32(t), f32(min_opacity)
    out = np.empty_like(rec)
    with np.errstate(all="ignore"):
        p = [rec[:, k] for k in range(4)]
        S = [[rec[:, 8 + 4 * c + r] for r in range(4)] for c in range(4)]
        s44 = S[3][3]
        dt = t - p[3]
        inv = f32(1.0) / s44
        e = exp(((f32(-0.5) * dt) * inv) * dt)
        ot = np.where(e >= m, e, m).astype(f32)
        k = inv * dt
        a = [S[r][3] for r in range(3)]
        tv = [inv * S[3][c] for c in range(3)]
        for r in range(3):
            out[:, r] = p[r] + (k * a[r])
        out[:, 3] = f32(mu_t_out)
        out[:, 4:7] = rec[:, 4:7]
        out[:, 7] = ot * rec[:, 7]
        for c in range(3):
            for r in range(3):
                out[:, 8 + 4 * c + r] = S[c][r] - (a[r] * tv[c])
        out[:, COLUMN] = f32(-0.0)
        out[:, ROW] = f32(-0.0)
        out[:, 23] = f32(s44_out)
    assert out.dtype == f32
    return out


def expected(gs4d, rec, q):
    """what a call writes, from the host definition"""
    return gs4d.slice_records_host(rec, *q)
