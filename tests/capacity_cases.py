"""Scenes that fill a chosen list capacity of the unordered path's compositor (csrc/composite2.hip, k_composite_v2<PREMULT_C, PER, OUT, ZTEST>).

Test infrastructure only (tests/test_capacity_host.py, tests/test_gpu_capacity.py).  PER = list capacity / 64 is chosen by the host from the
longest tile list L of earlier draws: v2_list_capacity(L + L / 8) on the ladder 64 .. 1024 (csrc/gs4d_api.hip, resolve_lane).  Every case
below is one image whose longest list lands on one rung, built so that the list's ORDER is visible:

* the long tile (LONG) holds K entries and nothing else reaches it.  List position i (0 = farthest, blended first) is the entry's depth rank.
  Most entries are small (a box of 1 or 3 pixels, significant on one pixel) dealt over the tile's 64 pixels with alphas of 0.1 .. 0.2, so a
  pixel sees K / 64 <= 16 of them and the deepest still shows (0.85^16 = 0.07).  A share is large (a 6 x 6 pixel box): one in sixteen
  everywhere (mixed chunks: splat-parallel phase A/B plus the per-pixel test of the large ones) and most of the front-most 64 where K >= 128
  (popc(bigmask) * 2 > cnt: the pixel-parallel branch);
* at every probed position p (probed()) entries p and p + 1 lie on one pixel with alpha 0.5 and opposite colours: removing one, or swapping
  the two, moves that pixel by far more than the 1e-4 bar;
* equal depths (so equal view-z keys, GS4D_KEY_VIEW_Z): a pair every 16 positions, and positions 29 .. 98 (70 keys across the boundary at
  entry 64) where K >= 100.  Tied entries lie pairwise on one pixel with opposite colours; their record indices ascend with the position;
* other tiles hold 1, 2, 63, 64 and 65 entries (those shorter than K: the 64 rung's longest list has at most 57), one holds large footprints only, and single splats, small and large, lie on tiles all over the image.

The same entries are drawn as 4D records (MODE_4D_SORTED: order by key, record indices shuffled) and as 3D-Full quads (gs4d_draw_quads: order
by index, so quad k is entry k).  Entries beyond K (the PROBE frame of the rungs below 256: a list just over the rung) lie off screen
until the probe frame moves them in, so every frame of a case has the same number of records.
"""
import numpy as np

import scenes
import staged_cases as sc
import ztest_cases as zc

W, H = sc.W, sc.H
DIST = 200.0
CAM = ((0.0, 0.0, DIST), (0.0, 0.0, -1.0))
TILE = sc.TILE
LONG = (48, 15)                                        # the long tile (tile coordinates): ztest_cases.per_pixel_plane cuts it with its diagonal region and both stripes, so three thresholds meet on it
SHORT = {1: (10, 11), 2: (14, 11), 63: (18, 11), 64: (22, 11), 65: (26, 11)}
ALL_LARGE, N_ALL_LARGE = (30, 11), 12
ZLO, ZSPAN, ZSTEPS = -1.9, 3.8, 1200                   # depth of rank r: ZLO + ZSPAN * r / ZSTEPS
RUN = (29, 99)                                         # positions of the run of equal keys (lists of >= 100 entries)
CLUSTER_PIXELS = (9, 14, 49, 54, 17, 46)               # inner pixels away from the tile's centre, where the large footprints lie

# case -> (rung the host must choose, K = entries of the long tile, entries of the probe frame's long tile or None)
CASES = {"c64": (64, 50, 74), "c128": (128, 110, 138), "c192": (192, 165, 202), "c256": (256, 220, None), "c384": (384, 330, None),
         "c512": (512, 440, None), "c768": (768, 660, None), "c1024": (1024, 900, None), "full": (1024, 1024, None), "over": (None, 1060, None)}


def window(case):
    """the longest lists L for which the host's rule lands on the case's rung (inclusive bounds)"""
    rung = CASES[case][0]
    if case == "full":
        return 1024, 1024
    if case == "over":
        return 1025, 1100
    prev = ([0] + list(sc.LADDER))[sc.LADDER.index(rung)]
    ok = [L for L in range(1, sc.V2_MAX_LIST + 1) if prev < min(sc.V2_MAX_LIST, L + L // 8) <= rung]
    return ok[0], ok[-1]


def probed(L):
    """blend-order positions of the longest list whose removal, and whose swap with the successor, must show"""
    return sorted({p for p in (0, 1, 63, 64, 65, L // 2, L - 65, L - 64, L - 2, L - 1) if 0 <= p < L})


def mats(gs4d, w=W, h=H):
    return gs4d.look_at(CAM[0], CAM[1]), gs4d.perspective(scenes.FOV, w, h, scenes.ZNEAR, scenes.ZFAR)


def _tile_list(rng, n, k_design, long_tile):
    """n entries of one tile by list position: pixel (0..63), large?, alpha, rgb, tie groups (lists of positions); designed for a list of k_design"""
    pix = (np.arange(n) * 37 + 11) % 64
    large = (np.arange(n) % 16 == 9) if long_tile else np.zeros(n, bool)
    if long_tile and k_design >= 128:
        front = np.arange(n) >= k_design - 64
        large |= front & (np.arange(n) < k_design) & (np.arange(n) % 16 < 13)
    alpha = rng.uniform(0.1, 0.2, n)
    rgb = rng.uniform(0.0, 1.0, (n, 3))
    red, cyan = np.array([0.95, 0.05, 0.1]), np.array([0.05, 0.95, 0.9])
    groups = [[i, i + 1] for i in range(5, n - 1, 16)]
    if n >= 100 and long_tile:
        groups = [g for g in groups if g[1] < RUN[0] or g[0] >= RUN[1]] + [list(range(*RUN))]
    for g in groups:
        for a in range(0, len(g) - 1, 2):
            i, j = g[a], g[a + 1]
            pix[j] = pix[i]
            alpha[i], alpha[j] = rng.uniform(0.35, 0.45, 2)
            rgb[i], rgb[j] = red, cyan
            large[i] = large[j] = False
    if long_tile:
        cl, last = -1, -10
        for p in probed(k_design):
            if p > last + 1:
                cl += 1
                pix[p] = CLUSTER_PIXELS[cl]
            for i in (p, p + 1):
                if i < n:
                    pix[i] = CLUSTER_PIXELS[cl]
                    alpha[i] = rng.uniform(0.45, 0.55)
                    rgb[i] = red if i % 2 else cyan
                    large[i] = False
            last = p
    return pix, large, alpha, rgb, groups


class Scene:
    """the entries of one case (arrays over entries): pixel position, depth, scale, colour, tile, list position, which frames show them"""

    def __init__(self, case, w=W, h=H, long_tile=LONG):
        self.case, self.w, self.h, self.long_tile = case, w, h, long_tile
        self.rung, self.K, self.K_probe = CASES[case]
        rng = np.random.default_rng(sum(map(ord, case)))
        px, py, z, s, col, shown, groups = [], [], [], [], [], [], []
        n_long = max(self.K, self.K_probe or 0)
        tiles = [(long_tile, n_long, self.K, True)] + [(t, n, n, False) for n, t in SHORT.items() if n < self.K] + [(ALL_LARGE, N_ALL_LARGE, N_ALL_LARGE, False)]
        tiles += [((tx, ty), 1, 1, False) for ty in (5, 20, 31, 36, 41) for tx in range(2, 78, 2)]
        base = 0
        for k, ((tx, ty), n, design, is_long) in enumerate(tiles):
            pix, large, alpha, rgb, grp = _tile_list(rng, n, design, is_long)
            if (tx, ty) == ALL_LARGE or (n == 1 and (tx, ty) not in SHORT.values() and tx % 4 == 0):
                large[:] = True                                                    # (every other single splat is a large one: pixels for the ID caps)
            border = (pix % 8 == 0) | (pix % 8 == 7) | (pix // 8 == 0) | (pix // 8 == 7)
            if not is_long:                                                        # (footprints grow towards the image's edge: inner pixels only)
                pix = np.where(border, 27, pix)
                border[:] = False
            jit = rng.uniform(-0.1, 0.1, (n, 2)) * np.where(border, 0.3, 1.0)[:, None]
            cx = tx * TILE + np.where(large, 4.0, pix % 8 + 0.5) + np.where(large, 4.0, 1.0) * jit[:, 0]
            cy = ty * TILE + np.where(large, 4.0, pix // 8 + 0.5) + np.where(large, 4.0, 1.0) * jit[:, 1]
            rank = np.arange(n, dtype=np.float64) * ((ZSTEPS - 100) // n if is_long else 1)      # the long list spans the whole depth range: the thresholds cut it
            for g in grp:
                rank[g] = rank[g[0]]
            # (the other tiles' depths lie between the long tile's, all over its range: the depth test's thresholds find wide gaps at every quantile)
            zz = ZLO + ZSPAN * (rank + (0.0 if is_long else (k * 37) % 1000 + 0.05 + 0.9 * ((k * 0.6180339887) % 1.0))) / ZSTEPS
            px.append(cx); py.append(cy); z.append(zz)
            s.append(np.where(large, 3.0 if is_long else 2.7, np.where(border, 0.45, 1.0 if is_long else 0.85)))
            col.append(np.concatenate([rgb, np.where(large, 0.5, 1.0)[:, None] * alpha[:, None]], 1))
            shown.append(np.arange(n) < design)
            groups += [[base + i for i in g] for g in grp]
            base += n
        self.px, self.py, self.z, self.s = (np.concatenate(v) for v in (px, py, z, s))
        self.rgba = np.concatenate(col).astype(np.float32)
        self.shown = np.concatenate(shown)                                         # False: only the probe frame shows the entry
        self.groups = groups
        self.n = self.px.size
        # record index of every entry when drawn as 4D records: shuffled, ascending with the position inside every group of equal keys
        perm = rng.permutation(self.n)
        for g in groups:
            perm[g] = np.sort(perm[g])
        self.rec_of_entry = perm

    def _world(self, gs4d, probe):
        _, proj = mats(gs4d, self.w, self.h)
        on = np.ones(self.n, bool) if probe else self.shown
        px = np.where(on, self.px, -4000.0)                                        # far outside the image: no tile, culled
        x = (px * 2.0 / self.w - 1.0) * (DIST - self.z) / proj[0]
        y = (self.py * 2.0 / self.h - 1.0) * (DIST - self.z) / proj[5]
        a = np.radians(15.0)                                                       # (an isotropic splat's axes are ill-defined: turned and flattened)
        q = np.tile(np.array([np.cos(a), 0.0, 0.0, np.sin(a)], np.float32), (self.n, 1))
        scale = (self.s[:, None] * np.array([1.0, 0.8, 1.0])).astype(np.float32)
        return np.stack([x, y, self.z], 1).astype(np.float32), q, scale

    def records_4d(self, gs4d, probe=False):
        """(n, 24) records, entry e at record rec_of_entry[e]"""
        pos, q, scale = self._world(gs4d, probe)
        n = self.n
        rec = gs4d.build_records_4d(np.concatenate([pos, np.zeros((n, 1), np.float32)], 1), q, scale, np.full(n, 20.0, np.float32), np.full(n, 0.5, np.float32),
                                    np.zeros((n, 3), np.float32), self.rgba)
        out = np.empty_like(rec)
        out[self.rec_of_entry] = rec
        return out

    def quads(self, gs4d, probe=False):
        """(n, 4, 18) vertices, quad e is entry e; and the splat positions (n, 3)"""
        pos, q, scale = self._world(gs4d, probe)
        return np.stack([gs4d.splat3d_mesh(pos[i], q[i], scale[i], self.rgba[i]) for i in range(self.n)]), pos


def quad_depths(pos, view):
    """ztest_cases.depth_np on the splat positions of quads (a static record: time 0, no motion)"""
    r = np.zeros((pos.shape[0], 24), np.float32)
    r[:, 0:3] = pos
    r[:, 23] = 1.0
    return zc.depth_np(r, view, 0.0)


def hide(data, form, hidden):
    """the records / quads with alpha 0 where `hidden` (per record)"""
    out = data.copy()
    if form == "4d":
        out[hidden, 7] = 0.0
    else:
        out[hidden, :, 8] = 0.0
    return out


def load(eproj, w=W, h=H):
    return sc.Load(sc.rects_from_checker(eproj, w, h), w, h)


def long_list(eproj, order, tile, w=W, h=H):
    """indices into `order` (None: instance k draws record k) of the entries of `tile`, in blend order"""
    x0, y0, x1, y1 = sc.rects_from_checker(eproj, w, h)
    tx, ty = tile
    on = (x0 <= x1) & (y0 <= y1) & (x0 // TILE <= tx) & (tx <= x1 // TILE) & (y0 // TILE <= ty) & (ty <= y1 // TILE)
    seq = np.arange(eproj.shape[0]) if order is None else np.asarray(order, np.int64)
    return np.nonzero(on[seq])[0]


def expected_order(oracle, rec, view):
    """the library's own stable sort of the view-z keys (GS4D_KEY_VIEW_Z): keys and permutation"""
    idx, keys = oracle.keygen_viewz(rec, 0.0, view)
    _, perm = oracle.sort_pairs(keys.view(np.uint32), idx, "std")
    return keys, perm


class Prepared:
    """one frame of a case in one record form, as the CPU checker sees it: the data to upload, the checker's projected records, the blend
    order, the load (longest list, ...) and the record depths of the depth test"""


_PREPARED = {}


def prepared(gs4d, oracle, case, form, probe=False, w=W, h=H, long_tile=LONG):
    key = (case, form, probe, w, h, long_tile)
    if key in _PREPARED:
        return _PREPARED[key]
    p = Prepared()
    p.scene = s = Scene(case, w, h, long_tile)
    p.form, p.w, p.h = form, w, h
    p.view, p.proj = mats(gs4d, w, h)
    if form == "4d":
        p.data = s.records_4d(gs4d, probe)
        p.frag_mode = oracle.MODE_4D
        p.eproj = oracle.preprocess(oracle.MODE_4D, p.data, p.view, p.proj, w, h, 0.0, 0.0)
        p.keys, p.order = expected_order(oracle, p.data, p.view)
        p.depth = zc.depth_np(p.data, p.view, 0.0)
    else:
        p.data, pos = s.quads(gs4d, probe)
        p.frag_mode = oracle.MODE_3D
        p.eproj = oracle.preprocess(oracle.MODE_3D, p.data, p.view, p.proj, w, h)
        p.keys, p.order = None, None
        p.depth = quad_depths(pos, p.view)
    p.n = s.n
    p.load = load(p.eproj, w, h)
    p.L = p.load.longest
    p.list = long_list(p.eproj, p.order, long_tile, w, h)
    _PREPARED[key] = p
    return p


def order_array(p):
    return np.arange(p.n, dtype=np.uint32) if p.order is None else p.order.copy()


def reference_image(oracle, p, order="own", eproj=None):
    """the checker's image of the frame (order: "own", or an explicit array)"""
    o = p.order if isinstance(order, str) else order
    return oracle.composite(p.eproj if eproj is None else eproj, o, p.frag_mode, p.w, p.h, oracle.clear_image(p.w, p.h))
