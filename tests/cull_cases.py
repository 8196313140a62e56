"""Record sets for tests/test_cull_host.py and tests/test_gpu_cull.py: tile-list entries that cannot change a pixel.

A. A record whose alpha, as the projection computes it (ot * col.w), compares equal to 0 gets no tile-list entry under the default blend
   function.  The 4D set of BASELINE.json configs[3] (scenes.cube_params_4d) has min_opacity = 0: exp(-0.5 dt^2 / Sigma44) underflows for
   about half of its records in the middle of the sweep and for two thirds at its ends.
B. The pixel rectangle is the smaller, per axis, of the quad's box and the box of the fragment test's discard disc (csrc/footprint_rect.h).

The image is 256 x 128 (512 tiles of 8 x 8), a set has N = 3 * 2048 + 100 records: three full segments of the projection kernel and a partial one.
"""
import numpy as np

import scenes

W, H = 256, 128
TILE = 8
SEG = 2048
N = 3 * SEG + 100
CAM = scenes.CAM_CUBE
TIMES = (0.0, 12.5, 25.0, 37.5, 50.0)                      # the sweep of configs[3]: 0 .. 50
SHARES = (0.694, 0.466, 0.389, 0.467, 0.693)               # alpha == 0 among the first 200 000 records of the set at those times
T_HALF, T_NONE = 12.5, -40.0                               # about half of a cut invisible; all of it (|dt| >= 40, Sigma44 < 3: exp(-266) = 0, float32 and float64) with most centres still in view
SCALE_4D = 8.0                                             # footprints at 256 x 128 as the benchmark's at 1080p: a few pixels
COL_W = 7                                                  # float of a 96-byte record that holds the colour's alpha


def mats(gs4d, w=W, h=H):
    return gs4d.look_at(CAM[0], CAM[1]), gs4d.perspective(scenes.FOV, w, h, scenes.ZNEAR, scenes.ZFAR)


def records_4d(gs4d, n=N, scale=SCALE_4D, start=0):
    p4, q, s, life, fade, vel, col = scenes.cube_params_4d(n, start=start)
    return gs4d.build_records_4d(p4, q, s * scale, life, fade, vel, col)


def records_3d(gs4d, n=N, scale=8.0, seed=scenes.SEED):
    pos, q, s, col = scenes.cube_params(n, seed=seed)
    return gs4d.build_records_3d(pos, q, s * scale, col)


def with_alpha(rec, index, value):
    out = rec.copy()
    out[index, COL_W] = np.float32(value)
    return out


def segment_and_wave(gs4d):
    """static splats; the whole second segment and one whole wave of the first (records 320 .. 383) have col.w = 0"""
    rec = records_3d(gs4d)
    idx = np.r_[SEG:2 * SEG, 320:384]
    return with_alpha(rec, idx, 0.0), idx


def negative_zero(gs4d):
    """every third record has col.w = -0.0f: it compares equal to 0"""
    rec = records_3d(gs4d, seed=scenes.SEED + 1)
    idx = np.arange(0, N, 3)
    return with_alpha(rec, idx, -0.0), idx


def big_footprints(gs4d):
    """records 5 and 6 cover more than 16 tiles each (the wave-cooperative walk of count_buckets / place_buckets); record 5 has col.w = 0"""
    pos, q, s, col = scenes.cube_params(N, seed=scenes.SEED + 2)
    s = s * 8.0
    s[5:7] *= 30.0
    pos[5:7] *= 0.25                                       # near the middle of the cube: inside the image
    rec = gs4d.build_records_3d(pos, q, s, col)
    return with_alpha(rec, np.array([5]), 0.0), np.array([5])


def rotated_splats(gs4d, scale):
    """randomly rotated, anisotropic static splats (scale ~ U[0.5, 2]^3 * scale)"""
    return records_3d(gs4d, scale=scale, seed=scenes.SEED + 3)


# ---- what the device's projected records say -------------------------------------------------------------------------------------------
def rects(proj16):
    """gs4d_debug_read_projected: the pixel rectangle is (x0 | y0 << 16, x1 | y1 << 16) in floats 10 and 11"""
    r0 = np.ascontiguousarray(proj16[:, 10]).view(np.uint32).astype(np.int64)
    r1 = np.ascontiguousarray(proj16[:, 11]).view(np.uint32).astype(np.int64)
    return r0 & 0xFFFF, r0 >> 16, r1 & 0xFFFF, r1 >> 16


def tiles_per_record(proj16, shard=None):
    """tile-list entries of every record's rectangle (tile_rect, gs4d_internal.h); shard = (rank, world): the tile rows ty % world == rank"""
    x0, y0, x1, y1 = rects(proj16)
    ok = (x0 <= x1) & (y0 <= y1)
    wx = np.where(ok, x1 // TILE - x0 // TILE + 1, 0)
    ty0, ty1 = y0 // TILE, y1 // TILE
    if shard is None:
        rows = ty1 - ty0 + 1
    else:
        rank, world = shard
        first = ty0 + (rank + world - ty0 % world) % world
        rows = np.where(first > ty1, 0, (ty1 - first) // world + 1)
    return wx * np.where(ok, rows, 0)


def invisible(proj16):
    """records the cull drops: valid, alpha == 0 (float 6; -0.0 compares equal)"""
    return (proj16[:, 14] != 0) & (proj16[:, 6] == 0.0)
