"""Record statistics (gs4d_set_record_stats) restated in numpy, and the scenes of their tests.

Test infrastructure only (tests/test_record_stats_host.py, tests/test_gpu_record_stats.py).  Built like tests/id_cases.py: the compositor's
rules in float32 and in its order of operations (composite_common.h) over the device's own projected records (Context.debug_projected) and
the draw's blend order:
  - coverage: dx = (i + 0.5) - cx, dy = (j + 0.5) - cy, u = fma(a0x, dx, a0y * dy), v = fma(a1x, dx, a1y * dy), |u| <= 0.5 and |v| <= 0.5;
  - cg = exp(-32 (u^2 + v^2)); al = clamp(alpha * cg, 0, 1) if cg >= 1e-4 else 0;
  - front to back: w = T * al, T *= (1 - al);
  - a fragment with w > 0 (pixels inside the image only: the restatement has no others) adds to its record
        pixels += 1,  wmax = max(wmax, w),  wsum += (uint32) rint(w * 2^24)   (float32 product, round to nearest even).
The device evaluates exp with v_exp_f32 and may contract u * u + v * v into an FMA: its w agrees with numpy's to id_cases.TIE_REL.  Where a
covering fragment's cg lies within TIE_REL of the 1e-4 discard an ulp decides whether it counts at all: those pixels are `fragile`, and every
record is told how many of them it covers.
"""
import numpy as np

import id_cases
import scenes

F = np.float32
TIE_REL = id_cases.TIE_REL
Q_ONE = F(16777216.0)                      # 2^24
F32_MIN_NORMAL = F(1.17549435e-38)
STAT = np.dtype([("pixels", "<u4"), ("wmax", "<f4"), ("wsum", "<u8")])


def quantise(w):
    """q(w) of the contract: (uint32) rint(w * 2^24), the product in float32"""
    return np.rint(np.asarray(w, F) * Q_ONE).astype(np.uint32)


def restate(proj, order, W, H, nrecords=None):
    """One draw of the records `proj` (id_cases.from_device fields) in instance order `order` (None: record k at instance k).  nrecords: the
    length of the statistics table (default: the records); an entry whose record index is >= nrecords is drawn and not counted, one whose
    index is >= len(proj) is not drawn.  Returns a dict:
      stats          structured (pixels u32, wmax f32, wsum u64) per record
      fragile        (H, W) bool, id_cases.restate's mask
      fragile_cover  per record: fragile pixels it covers
      covered        pixels of the image some fragment covers
      layers         (H, W) fragments with w > 0 per pixel
      T              (H, W) final transmittance
      subnormal      a counted fragment's w is subnormal"""
    nproj = proj.shape[0]
    nstat = nproj if nrecords is None else int(nrecords)
    n = nproj if order is None else len(order)
    seq = np.arange(n, dtype=np.int64) if order is None else np.asarray(order, np.int64)
    T = np.ones((H, W), F)
    st = np.zeros(nstat, STAT)
    fragile = np.zeros((H, W), bool)
    anycov = np.zeros((H, W), bool)
    layers = np.zeros((H, W), np.int32)
    boxes = []
    subnormal = False
    for k in range(n - 1, -1, -1):                    # front to back: the last instance is blended first
        rec = int(seq[k])
        if rec >= nproj:
            continue
        p = proj[rec]
        if not p["valid"]:
            continue
        cx, cy, hx, hy = F(p["cx"]), F(p["cy"]), F(p["hx"]), F(p["hy"])
        i0, i1 = max(0, int(np.floor(cx - hx - F(1.5)))), min(W - 1, int(np.ceil(cx + hx + F(1.5))))
        j0, j1 = max(0, int(np.floor(cy - hy - F(1.5)))), min(H - 1, int(np.ceil(cy + hy + F(1.5))))
        if i0 > i1 or j0 > j1:
            continue
        fx = np.arange(i0, i1 + 1, dtype=F) + F(0.5)
        fy = np.arange(j0, j1 + 1, dtype=F) + F(0.5)
        dx, dy = np.broadcast_arrays((fx - cx)[None, :], (fy - cy)[:, None])
        u = id_cases._fma(np.full_like(dx, p["a0x"]), dx, F(p["a0y"]) * dy)
        v = id_cases._fma(np.full_like(dx, p["a1x"]), dx, F(p["a1y"]) * dy)
        cov = (np.abs(u) <= F(0.5)) & (np.abs(v) <= F(0.5))
        if not cov.any():
            continue
        cg = np.exp2((u * u + v * v) * F(-46.16624130844683)).astype(F)
        al = np.where(cov & (cg >= F(0.0001)), np.clip(F(p["alpha"]) * cg, F(0.0), F(1.0)), F(0.0)).astype(F)
        sl = (slice(j0, j1 + 1), slice(i0, i1 + 1))
        fragile[sl] |= cov & (np.abs(cg - F(0.0001)) <= F(TIE_REL * 0.0001))
        anycov[sl] |= cov
        t = T[sl]
        w = (t * al).astype(F)
        on = w > 0
        layers[sl] += on
        if rec < nstat and on.any():
            subnormal |= bool((w[on] < F32_MIN_NORMAL).any())
            st["pixels"][rec] += np.uint32(on.sum())
            st["wmax"][rec] = max(st["wmax"][rec], w[on].max())
            st["wsum"][rec] += np.uint64(quantise(w[on]).astype(np.uint64).sum())
        if rec < nstat:
            boxes.append((rec, sl, cov))
        T[sl] = (t * (F(1.0) - al)).astype(F)
    fragile_cover = np.zeros(nstat, np.int64)
    if fragile.any():
        for rec, sl, cov in boxes:
            fragile_cover[rec] += int((cov & fragile[sl]).sum())
    return {"stats": st, "fragile": fragile, "fragile_cover": fragile_cover, "covered": int(anycov.sum()), "layers": layers, "T": T, "subnormal": subnormal}


def check(got, ref):
    """The bar of the layered tests: `got` (read_record_stats) against restate()'s result.  pixels: equal for a record that covers no fragile
    pixel, else within the fragile pixels it covers; |d wsum| <= TIE_REL * wsum_ref + pixels (the device's w agrees with numpy's to TIE_REL
    and every fragment adds at most one unit of rounding); wmax within TIE_REL relative."""
    want, fc = ref["stats"], ref["fragile_cover"]
    dp = np.abs(got["pixels"].astype(np.int64) - want["pixels"].astype(np.int64))
    dw = np.abs(got["wsum"].astype(np.int64) - want["wsum"].astype(np.int64))
    dm = np.abs(got["wmax"].astype(np.float64) - want["wmax"].astype(np.float64))
    print(f"stats check: {int((want['pixels'] > 0).sum())} of {want.size} records count, max |d pixels| {int(dp.max(initial=0))}, max |d wsum| {int(dw.max(initial=0))} units "
          f"(largest allowance {float((TIE_REL * want['wsum'] + np.maximum(want['pixels'], got['pixels'])).max(initial=0)):.1f}), max rel d wmax "
          f"{float((dm / np.maximum(want['wmax'], 1e-30)).max(initial=0)):.2e}, fragile pixels {int(ref['fragile'].sum())}")
    bad = np.nonzero(dp > fc)[0]
    assert bad.size == 0, f"pixels differ beyond the fragile pixels covered: records {bad[:8]}, got {got['pixels'][bad[:8]]}, want {want['pixels'][bad[:8]]}, fragile {fc[bad[:8]]}"
    bad = np.nonzero(dw > TIE_REL * want["wsum"].astype(np.float64) + np.maximum(want["pixels"], got["pixels"]))[0]
    assert bad.size == 0, f"wsum differs: records {bad[:8]}, got {got['wsum'][bad[:8]]}, want {want['wsum'][bad[:8]]}"
    bad = np.nonzero(dm > TIE_REL * want["wmax"].astype(np.float64))[0]
    assert bad.size == 0, f"wmax differs: records {bad[:8]}, got {got['wmax'][bad[:8]]}, want {want['wmax'][bad[:8]]}"


# ---- scenes: splats facing a camera on the z axis, placed by pixel ------------------------------------------------------------------------
DIST = 200.0
CAM = ((0.0, 0.0, DIST), (0.0, 0.0, -1.0))
S_SMALL, S_LARGE = 1.0, 3.0               # splat scales: a box of <= 4 pixels (splat-parallel marking); one of > 4 (tested pixel-parallel)


def mats(gs4d, W, H):
    return gs4d.look_at(CAM[0], CAM[1]), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)


def world(gs4d, W, H, px, py, z, s):
    """positions, rotations and scales of splats whose centres project to pixel positions (px, py) (pixel p's centre: p + 0.5) at depth
    DIST - z; turned by 15 degrees and flattened (an isotropic splat's axes are ill-defined)"""
    _, proj = mats(gs4d, W, H)
    px, py, z, s = (np.asarray(a, np.float64) for a in (px, py, z, s))
    x = (px * 2.0 / W - 1.0) * (DIST - z) / proj[0]
    y = (py * 2.0 / H - 1.0) * (DIST - z) / proj[5]
    a = np.radians(15.0)
    q = np.tile(np.array([np.cos(a), 0.0, 0.0, np.sin(a)], np.float32), (px.size, 1))
    scale = (s[:, None] * (360.0 / H) * np.array([1.0, 0.8, 1.0])).astype(np.float32)      # (s: the footprint the scale has in a 360-row image)
    return np.stack([x, y, z], 1).astype(np.float32), q, scale


def records(gs4d, W, H, px, py, z, s, rgba):
    pos, q, scale = world(gs4d, W, H, px, py, z, s)
    return gs4d.build_records_3d(pos, q, scale, np.asarray(rgba, np.float32))


def quads(gs4d, W, H, px, py, z, s, rgba):
    pos, q, scale = world(gs4d, W, H, px, py, z, s)
    rgba = np.asarray(rgba, np.float32)
    return np.stack([gs4d.splat3d_mesh(pos[i], q[i], scale[i], rgba[i]) for i in range(pos.shape[0])])


def disjoint(kind, W=96, H=96):
    """a grid of records that do not overlap, some across 2 - 4 tiles: `small` (boxes of <= 4 pixels), `large` (> 4), `mixed` (both in every
    chunk).  Returns px, py, z, s, rgba."""
    rng = np.random.default_rng({"small": 11, "large": 12, "mixed": 13}[kind])
    step = {"small": 6.7, "large": 13.3, "mixed": 13.3}[kind]
    gx, gy = np.meshgrid(np.arange(4.0, W - 3.0, step), np.arange(4.0, H - 3.0, step))
    px, py = gx.ravel(), gy.ravel()
    n = px.size
    s = np.full(n, S_SMALL if kind == "small" else S_LARGE)
    if kind == "mixed":
        s[np.arange(n) % 2 == 1] = S_SMALL
    rgba = np.concatenate([rng.uniform(0.0, 1.0, (n, 3)), rng.uniform(0.05, 1.0, (n, 1))], 1)
    return px, py, rng.uniform(-5.0, 5.0, n), s, rgba


# the layered scenes: name -> (seed, W, H, background records, records on one tile)
LAYERED = {"overlap": (21, 96, 96, 2400, 0), "chunks": (22, 96, 96, 1500, 110), "per": (23, 96, 96, 1500, 300), "edges": (24, 61, 43, 700, 0)}
CLUSTER_TILE = (5, 6)


def layered(name):
    """overlapping records all over the image (alphas in [0.05, 1], a third of them large), plus `cluster` small ones on one tile: a list of more
    than 64 entries (several chunks), of more than 256 (a larger PER).  `edges`: an image that is no multiple of the tile, records over its right
    and top edge.  Returns W, H and px, py, z, s, rgba."""
    seed, W, H, nbg, cluster = LAYERED[name]
    rng = np.random.default_rng(seed)
    px, py = rng.uniform(-2.0, W + 2.0, nbg), rng.uniform(-2.0, H + 2.0, nbg)
    if cluster:                                          # (the cluster's tile keeps its list to itself: at most ~16 layers on a pixel)
        tx, ty = CLUSTER_TILE
        keep = (np.abs(px - (tx * 8 + 4)) > 12) | (np.abs(py - (ty * 8 + 4)) > 12)
        px, py = px[keep], py[keep]
    s = np.where(rng.uniform(size=px.size) < 0.33, S_LARGE, S_SMALL) * rng.uniform(0.7, 1.2, px.size)
    if name == "edges":                                  # a row of records on the right edge and one on the top edge, small and large
        k = 12
        px = np.concatenate([px, np.full(k, W - 0.7), np.linspace(2.0, W - 2.0, k)])
        py = np.concatenate([py, np.linspace(2.0, H - 2.0, k), np.full(k, H - 0.4)])
        s = np.concatenate([s, np.tile([S_SMALL, S_LARGE], k)])
    if cluster:
        tx, ty = CLUSTER_TILE
        px = np.concatenate([px, tx * 8 + rng.uniform(0.6, 7.4, cluster)])
        py = np.concatenate([py, ty * 8 + rng.uniform(0.6, 7.4, cluster)])
        s = np.concatenate([s, np.full(cluster, 0.7)])
    n = px.size
    rgba = np.concatenate([rng.uniform(0.0, 1.0, (n, 3)), rng.uniform(0.05, 1.0, (n, 1))], 1)
    if cluster:
        rgba[-cluster:, 3] = rng.uniform(0.05, 0.3, cluster)
    return W, H, (px, py, rng.uniform(-8.0, 8.0, n), s, rgba)
