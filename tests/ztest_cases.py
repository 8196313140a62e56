"""Shared pieces of the depth-test tests (tests/test_gpu_depth_test.py, tests/test_depth_test_host.py; gs4d_set_depth_test).

The depth test blends a fragment of record i at pixel p only if d_i < Z[p] (float32).  Its oracle is a TWIN: the same frame without the test,
in which every record hidden at a pixel has alpha 0 in its data.  The projection does not cull alpha-0 records, so the twin has the test
run's own lists, paths and blend order, and a hidden fragment blends as C + 0*c, T*1 — bit for bit what the test does.

Thresholds: a float32 value strictly between two consecutive distinct record depths (so which records it hides does not depend on rounding
anywhere), that hides between 10 % and 90 % of the valid records.  pick_thresholds asserts both conditions."""
import numpy as np

QUARTILES = (0.25, 0.5, 0.75)


def depth_np(rec, view, t):
    """-z_view of the time-conditioned centre, float32 in the projection kernel's order (preprocess.hip project_4d / project3d)"""
    r = rec.astype(np.float32)
    V = np.asarray(view, np.float32)
    dt = np.float32(t) - r[:, 3]
    k = (np.float32(1.0) / r[:, 23]) * dt
    mx, my, mz = r[:, 0] + k * r[:, 11], r[:, 1] + k * r[:, 15], r[:, 2] + k * r[:, 19]
    pcz = ((V[2] * mx + V[6] * my) + V[10] * mz) + V[14] * np.float32(1.0)
    return -pcz


def pick_thresholds(d_valid, quantiles=QUARTILES, window=0.10, min_rel_gap=0.0):
    """One threshold near each quantile of the valid records' depths: the midpoint (float32) of the widest relative gap between consecutive
    distinct depths within +-window (a fraction of the records) of the quantile.  min_rel_gap: the gap must be wider than that times the
    depth (the checker test's margin against rounding in its own depth arithmetic)."""
    d = np.sort(np.asarray(d_valid, np.float32))
    n = d.size
    assert n >= 16, n
    out = []
    for q in quantiles:
        lo, hi = max(0, int((q - window) * n)), min(n, int((q + window) * n) + 1)
        u = np.unique(d[lo:hi])
        assert u.size >= 2, (q, u.size)
        rel = (u[1:].astype(np.float64) - u[:-1].astype(np.float64)) / np.abs(u[:-1].astype(np.float64))
        i = int(np.argmax(rel))
        assert rel[i] > min_rel_gap, (q, rel[i], min_rel_gap)
        a, b = u[i], u[i + 1]
        z = np.float32((np.float64(a) + np.float64(b)) * 0.5)
        assert a < z < b, (a, z, b)                                   # strictly between two consecutive distinct depths ...
        assert not np.any((d > a) & (d < b))                          # ... consecutive in the whole set
        hidden = float((d >= z).mean())
        assert 0.10 <= hidden <= 0.90, (q, hidden)
        out.append(z)
    return out


def per_pixel_plane(W, H, values, seed=7):
    """(H, W) float32: every 8x8 tile takes a random value from `values`, then a diagonal boundary and two 3-pixel stripes cut through tiles"""
    rng = np.random.default_rng(seed)
    ty, tx = (H + 7) // 8, (W + 7) // 8
    vals = np.asarray(values, np.float32)
    tiles = vals[rng.integers(0, vals.size, size=(ty, tx))]
    Z = np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)[:H, :W].copy()
    y, x = np.mgrid[0:H, 0:W]
    Z[3 * x > 5 * y + W // 3] = vals[0]                               # a diagonal boundary (slope 5/3: it crosses tiles at every offset)
    xs = (3 * W // 5) // 8 * 8 + 6                                    # 3-pixel stripes across a tile boundary: columns 8k+6 .. 8k+8, rows likewise
    Z[:, xs:xs + 3] = vals[1 % vals.size]
    ys = (H // 3) // 8 * 8 + 6
    Z[ys:ys + 3, :] = vals[2 % vals.size]
    return Z


def hide_alpha(rec, d, z, alpha_col):
    """a twin's records: alpha 0 where the record fails d < z (z a scalar)"""
    out = rec.copy()
    out[~(d < np.float32(z)), alpha_col] = 0.0
    return out
