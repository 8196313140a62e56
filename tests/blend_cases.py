"""Scenes for the general blend path: any glBlendFunc other than (SRC_ALPHA, ONE_MINUS_SRC_ALPHA).

Test infrastructure only (tests/test_blend_host.py checks every claim made here with the CPU checker alone, tests/test_gpu_blend.py runs
the library against the scenes).  Such a draw takes instance-ordered tile lists, k_composite<PREMULT_C, true, Colour, false> walking each list
in draw order, and blend_general / blend_factor (csrc/composite_common.h); the overlay lines use the same two functions (csrc/lines.hip).

* gl_blend: OpenGL 4.4 tables 17.1 / 17.2 restated in float64 from the specification (FUNC_ADD, the same factor on RGB and alpha), the
  statement the checker's own factor table is held against;
* Matrix: one 100 x 52 image (13 x 7 tiles, the last column and the last row 4 pixels wide) that every fragment source draws into — lines,
  a sorted 4D draw, 3D-Full quads (premultiplied colour), a 2D draw, a direct 4D draw — for all 196 factor pairs;
* Order: tile lists of 1 .. 200 entries whose LAST entry shows, bit for bit, under (ONE, ZERO);
* Rerun: draws of full-image splats whose tile-list entries outgrow the ordered path's capacity, under (ONE, ONE).

Everything is placed in pixel space: the camera looks down -z from DIST, so a world point (x, y, z) lands on pixel
((x * P00 / (DIST - z) + 1) * W / 2, ...) and splat sizes are calibrated against the checker's own projection.
"""
import numpy as np

import scenes

TOL = 1e-4
TILE = 8
DIST = 200.0
CAM = ((0.0, 0.0, DIST), (0.0, 0.0, -1.0))

# GL enum values of the blend factors the library accepts (include/gs4d.h GS4D_ZERO ..)
GL = {"ZERO": 0, "ONE": 1, "SRC_COLOR": 0x0300, "ONE_MINUS_SRC_COLOR": 0x0301, "SRC_ALPHA": 0x0302, "ONE_MINUS_SRC_ALPHA": 0x0303, "DST_ALPHA": 0x0304,
      "ONE_MINUS_DST_ALPHA": 0x0305, "DST_COLOR": 0x0306, "ONE_MINUS_DST_COLOR": 0x0307, "CONSTANT_COLOR": 0x8001, "ONE_MINUS_CONSTANT_COLOR": 0x8002,
      "CONSTANT_ALPHA": 0x8003, "ONE_MINUS_CONSTANT_ALPHA": 0x8004}
FACTORS = tuple(GL)
# The blend colour is never set: (0, 0, 0, 0).  CONSTANT_* are then ZERO and ONE_MINUS_CONSTANT_* are ONE: 10 distinct factors, 100 functions.
CLASS = {f: f for f in FACTORS}
CLASS.update({"CONSTANT_COLOR": "ZERO", "CONSTANT_ALPHA": "ZERO", "ONE_MINUS_CONSTANT_COLOR": "ONE", "ONE_MINUS_CONSTANT_ALPHA": "ONE"})
CLASSES = tuple(f for f in FACTORS if CLASS[f] == f)
OVER = ("SRC_ALPHA", "ONE_MINUS_SRC_ALPHA")


def enums(pair):
    return GL[pair[0]], GL[pair[1]]


# ---- OpenGL 4.4 core, 17.3.8: tables 17.1 (equations) and 17.2 (factors), written from the specification ---------------------------------
def gl_factor(name, src, dst, const=(0.0, 0.0, 0.0, 0.0)):
    """Table 17.2: the (n, 4) weighting factors (RGB factor, alpha factor) of `name` for (n, 4) float64 sources and destinations.
    (Rs, Gs, Bs, As) source, (Rd, Gd, Bd, Ad) destination, (Rc, Gc, Bc, Ac) the blend colour."""
    one = np.ones_like(src)
    a_s, a_d = src[:, 3:4] * one, dst[:, 3:4] * one                       # (As, As, As), As  /  (Ad, Ad, Ad), Ad
    c = np.asarray(const, np.float64)[None, :] * one
    a_c = c[:, 3:4] * one
    return {"ZERO": 0.0 * one, "ONE": one, "SRC_COLOR": src, "ONE_MINUS_SRC_COLOR": one - src, "DST_COLOR": dst, "ONE_MINUS_DST_COLOR": one - dst,
            "SRC_ALPHA": a_s, "ONE_MINUS_SRC_ALPHA": one - a_s, "DST_ALPHA": a_d, "ONE_MINUS_DST_ALPHA": one - a_d,
            "CONSTANT_COLOR": c, "ONE_MINUS_CONSTANT_COLOR": one - c, "CONSTANT_ALPHA": a_c, "ONE_MINUS_CONSTANT_ALPHA": one - a_c}[name]


def gl_blend(pair, src, dst):
    """Table 17.1, FUNC_ADD: C = Cs * S + Cd * D per component, clamped to [0, 1] (fixed-point framebuffer), in float64."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    return np.clip(src * gl_factor(pair[0], src, dst) + dst * gl_factor(pair[1], src, dst), 0.0, 1.0)


def same_function(pairs, seed=1):
    """Index of each pair's function among the distinct ones.  Some pairs of the table are ONE function of (src, dst) — (ZERO, SRC_COLOR) and
    (DST_COLOR, ZERO) both give src * dst; (DST_COLOR, ONE_MINUS_SRC_COLOR) gives dst like (ZERO, ONE) — and no picture can tell those apart:
    found here by evaluating the float64 statement on random interior points (a polynomial identity holds on all of them or on almost none)."""
    rng = np.random.default_rng(seed)
    src, dst = rng.uniform(0.05, 0.45, (64, 4)), rng.uniform(0.05, 0.45, (64, 4))          # no clamp is reached: the polynomials themselves
    seen, out = [], []
    for p in pairs:
        v = gl_blend(p, src, dst)
        for k, u in enumerate(seen):
            if np.abs(u - v).max() < 1e-12:
                out.append(k)
                break
        else:
            seen.append(v)
            out.append(len(seen) - 1)
    return np.array(out)


def pack8(img):
    """The documented RGBA8 rule: clamp, x 255, round to nearest even."""
    return np.rint(np.clip(img.astype(np.float32), 0.0, 1.0) * np.float32(255.0)).astype(np.int32)


def pack8_slack(img, tol=TOL):
    """True where the float value times 255 lies within 255 * tol of a rounding boundary (k + 0.5): only there may a byte differ by one."""
    x = np.clip(img.astype(np.float64), 0.0, 1.0) * 255.0
    return np.abs(x - np.floor(x) - 0.5) <= 255.0 * tol


# ---- placement -------------------------------------------------------------------------------------------------------------------------
def mats(gs4d, w, h):
    return gs4d.look_at(CAM[0], CAM[1]), gs4d.perspective(scenes.FOV, w, h, scenes.ZNEAR, scenes.ZFAR)


_CAL = {}


def _calibration(gs4d, oracle, w, h):
    """quad half-width in pixels, along its longer axis, of a splat of one world unit per pixel of scale at the image's centre (linear in the scale)"""
    if (w, h) not in _CAL:
        _CAL[(w, h)] = 1.0
        view, proj = mats(gs4d, w, h)
        pos, q, scale = world(gs4d, oracle, w, h, [w / 2.0], [h / 2.0], [0.0], [1.0])
        p = oracle.preprocess(oracle.MODE_4D, gs4d.build_records_3d(pos, q, scale, np.full((1, 4), 0.5, np.float32)), view, proj, w, h, 0.0, 0.0)
        _CAL[(w, h)] = 0.5 / float(np.hypot(p["a0x"][0], p["a0y"][0])) / 4.0
    return _CAL[(w, h)]


def world(gs4d, oracle, w, h, px, py, z, sigma_px):
    """positions (n, 3), rotations and scales of splats centred on pixel coordinates (px, py) at depth z whose quad reaches 4 sigma_px pixels along
    its longer axis (0.8 of that along the other)"""
    _, proj = mats(gs4d, w, h)
    px, py, z, sigma_px = (np.asarray(v, np.float64) for v in (px, py, z, sigma_px))
    x = (px * 2.0 / w - 1.0) * (DIST - z) / proj[0]
    y = (py * 2.0 / h - 1.0) * (DIST - z) / proj[5]
    unit = 2.0 * (DIST - z) / (proj[5] * h) / _calibration(gs4d, oracle, w, h)      # world units of scale per pixel of sigma at that depth
    n = x.size
    a = np.radians(15.0)                                                     # (an isotropic splat's axes are ill-defined: turned and flattened)
    q = np.tile(np.array([np.cos(a), 0.0, 0.0, np.sin(a)], np.float32), (n, 1))
    scale = ((sigma_px * unit)[:, None] * np.array([1.0, 0.8, 0.01])).astype(np.float32)
    return np.stack([x, y, z * np.ones(n)], 1).astype(np.float32), q, scale


def records_4d(gs4d, oracle, w, h, px, py, z, sigma_px, rgba):
    pos, q, scale = world(gs4d, oracle, w, h, px, py, z, sigma_px)
    return gs4d.build_records_3d(pos, q, scale, np.asarray(rgba, np.float32))


def quads(gs4d, oracle, w, h, px, py, z, sigma_px, rgba):
    pos, q, scale = world(gs4d, oracle, w, h, px, py, z, sigma_px)
    rgba = np.asarray(rgba, np.float32)
    return np.stack([gs4d.splat3d_mesh(pos[i], q[i], scale[i], rgba[i]) for i in range(pos.shape[0])])


def records_2d(gs4d, oracle, w, h, px, py, half_px, rgba, angle):
    """GS4D_MODE_2D records {pos4, col4, mat2} centred on pixels (px, py) with a quad of about half_px pixels half width: positions and sizes are
    calibrated against the checker's own projection (centre and half extent are linear in the record's position and standard deviation)."""
    view, proj = mats(gs4d, w, h)

    def build(x, y, s):
        rec = np.zeros((len(x), 12), np.float32)
        rec[:, 0], rec[:, 1] = x, y
        rec[:, 4:8] = np.asarray(rgba, np.float32)[:len(x)]
        for i in range(len(x)):
            c, sn = np.cos(angle[i]), np.sin(angle[i])
            R = np.array([[c, -sn], [sn, c]])
            S = R @ np.diag([s[i] ** 2, (0.8 * s[i]) ** 2]) @ R.T
            rec[i, 8:12] = [S[0, 0], S[1, 0], S[0, 1], S[1, 1]]
        return rec
    n = len(px)
    probe = oracle.preprocess(oracle.MODE_2D, build(np.array([0.0, 1.0]), np.array([0.0, 1.0]), np.array([1.0, 1.0])), view, proj, w, h)
    kx, ky = float(probe["cx"][1] - probe["cx"][0]), float(probe["cy"][1] - probe["cy"][0])
    x0, y0 = float(probe["cx"][0]), float(probe["cy"][0])
    hunit = float(max(probe["hx"][0], probe["hy"][0]))
    return build((np.asarray(px) - x0) / kx, (np.asarray(py) - y0) / ky, np.asarray(half_px) / hunit)[:n]


# ---- fragments of a scene as the checker's projected records give them, in float64 ---------------------------------------------------------
def fragment_weights(eproj, w, h, mode2d=False):
    """c of every (record, pixel) the coverage rule accepts (a superset by one part in 10^6), both as the kernel forms it —
    exp(-32 (u^2 + v^2)) — and as the checker does — exp(-x^T Q x / 2) with x = 8 R S (u, v); float64 from the float32 projected records."""
    out = []
    f = np.float32
    for p in eproj[eproj["valid"] != 0]:
        i0, i1 = int(max(0, np.floor(p["cx"] - p["hx"] - 2))), int(min(w - 1, np.ceil(p["cx"] + p["hx"] + 2)))
        j0, j1 = int(max(0, np.floor(p["cy"] - p["hy"] - 2))), int(min(h - 1, np.ceil(p["cy"] + p["hy"] + 2)))
        if i0 > i1 or j0 > j1:
            continue
        dx = (np.arange(i0, i1 + 1, dtype=f) + f(0.5) - p["cx"])[None, :].astype(np.float64)
        dy = (np.arange(j0, j1 + 1, dtype=f) + f(0.5) - p["cy"])[:, None].astype(np.float64)
        u = float(p["a0x"]) * dx + float(p["a0y"]) * dy
        v = float(p["a1x"]) * dx + float(p["a1y"]) * dy
        m = (np.abs(u) <= 0.5 + 1e-6) & (np.abs(v) <= 0.5 + 1e-6)
        u, v = u[m], v[m]
        out.append(np.exp(-32.0 * (u * u + v * v)))
        m00, m01, m10, m11 = (8.0 * float(p[k]) * float(p[s]) for k, s in (("e0x", "s0"), ("e0y", "s0"), ("e1x", "s1"), ("e1y", "s1")))
        x, y = m00 * u + m10 * v, m01 * u + m11 * v
        q00, q01, q10, q11 = (float(p[k]) for k in ("q00", "q01", "q10", "q11"))
        sx, sy = (q00 * x + q10 * y, q01 * x + q11 * y) if mode2d else (x * q00 + y * q01, x * q10 + y * q11)
        out.append(np.exp(-0.5 * (sx * x + sy * y)))
    return np.concatenate(out) if out else np.zeros(0)


def coverage(eproj, w, h):
    """fragments per pixel (coverage rule and c >= 1e-4 in float64) of a draw of these projected records"""
    cnt = np.zeros((h, w), int)
    f = np.float32
    for p in eproj[eproj["valid"] != 0]:
        i0, i1 = int(max(0, np.floor(p["cx"] - p["hx"] - 2))), int(min(w - 1, np.ceil(p["cx"] + p["hx"] + 2)))
        j0, j1 = int(max(0, np.floor(p["cy"] - p["hy"] - 2))), int(min(h - 1, np.ceil(p["cy"] + p["hy"] + 2)))
        if i0 > i1 or j0 > j1:
            continue
        dx = (np.arange(i0, i1 + 1, dtype=f) + f(0.5) - p["cx"])[None, :].astype(np.float64)
        dy = (np.arange(j0, j1 + 1, dtype=f) + f(0.5) - p["cy"])[:, None].astype(np.float64)
        u = float(p["a0x"]) * dx + float(p["a0y"]) * dy
        v = float(p["a1x"]) * dx + float(p["a1y"]) * dy
        cnt[j0:j1 + 1, i0:i1 + 1] += (np.abs(u) <= 0.5) & (np.abs(v) <= 0.5) & (np.exp(-32.0 * (u * u + v * v)) >= 1e-4)
    return cnt


DISCARD = 1e-4                                              # Splat4DFragShader.GLSL:30
DISCARD_MARGIN = DISCARD * 2.0 ** -16


def discard_margin(weights):
    """the smallest |c - 1e-4| of the fragments"""
    return float(np.min(np.abs(weights - DISCARD))) if weights.size else np.inf


def entries_of(eproj, w, h):
    """tile-list entries per tile of a draw of these projected records (staged_cases.Load in the image's own size)"""
    import staged_cases as sc
    return sc.Load(sc.rects_from_checker(eproj, w, h), w, h).tiles


def perturbed(eproj, rng, premult):
    """every record's alpha scaled by 1 +- 2^-18 (random sign) — and with it the premultiplied colour, which carries the same factor c"""
    out = eproj.copy()
    k = (1.0 + rng.choice([-1.0, 1.0], out.size) * 2.0 ** -18).astype(np.float32)
    out["alpha"] = out["alpha"] * k
    if premult:
        for ch in ("r", "g", "b"):
            out[ch] = out[ch] * k
    return out


# ---- 2. the matrix scene ------------------------------------------------------------------------------------------------------------------
class Matrix:
    """Lines, then a sorted 4D draw, then quads, then a 2D draw, then a direct 4D draw, on one small image.  Tiles (0..3, 4..6) — the upper
    left — stay untouched; fragments fall on the partial tiles of the last column and the last row."""
    W, H = 100, 52
    CLEAR = np.array([0.2, 0.5, 0.7, 0.4], np.float32)
    LINE_COLOUR = np.array([0.85, 0.35, 0.15, 0.55], np.float32)
    LINE_WIDTH = 2.0
    CROSS = (21, 16)                                        # the pixel the segments cross in
    NB, NC, ND, NE = 90, 50, 36, 60                         # records of steps b, c, d; step e draws the first NE records of b again
    UNTOUCHED = [(tx, ty) for tx in range(4) for ty in range(4, 7)]
    SEED = 5

    def __init__(self, gs4d, oracle, seed=None):
        w, h = self.W, self.H
        rng = np.random.default_rng(self.SEED if seed is None else seed)
        self.view, self.proj = mats(gs4d, w, h)
        # a. five NDC segments through the centre of pixel CROSS, short enough to stay below y = 32
        cx, cy = (self.CROSS[0] + 0.5) * 2.0 / w - 1.0, (self.CROSS[1] + 0.5) * 2.0 / h - 1.0
        ang = np.array([0.0, 0.5, 1.1, 1.9, 2.6])
        d = np.stack([np.cos(ang) * 12.0 * 2.0 / w, np.sin(ang) * 12.0 * 2.0 / h], 1)
        self.lines = np.stack([np.array([cx, cy]) - d, np.array([cx, cy]) + d], 1).reshape(-1, 2).astype(np.float32)

        def spots(n):
            """centres that leave the upper-left tiles alone (x >= 38 or y <= 26) and reach the right and the top edge"""
            px, py = rng.uniform(2.0, 99.0, n), rng.uniform(1.0, 51.5, n)
            bad = (px < 38.0) & (py > 26.0)
            py[bad] = rng.uniform(1.0, 26.0, bad.sum())
            return px, py

        def colours(n):
            c = np.stack([rng.uniform(0.6, 0.95, n), rng.uniform(0.36, 0.5, n), rng.uniform(0.03, 0.1, n), rng.uniform(0.15, 0.3, n)], 1)
            return np.take_along_axis(c, np.concatenate([rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1), np.full((n, 1), 3)], 1), 1).astype(np.float32)
        # b. 4D records, sorted by the reference's key: depths are random, so record indices are shuffled against depth
        px, py = spots(self.NB)
        self.rec_b = records_4d(gs4d, oracle, w, h, px, py, rng.uniform(-2.0, 2.0, self.NB), rng.uniform(0.35, 0.6, self.NB), colours(self.NB))
        self.eproj_b = oracle.preprocess(oracle.MODE_4D, self.rec_b, self.view, self.proj, w, h, 0.0, 0.0)
        idx, keys = oracle.keygen(self.rec_b, 0.0, CAM[0])
        _, self.order_b = oracle.sort_pairs(keys.view(np.uint32), idx, "std")
        # c. 3D-Full quads (the fragment colour is premultiplied by c)
        px, py = spots(self.NC)
        col = colours(self.NC)
        self.quads_c = quads(gs4d, oracle, w, h, px, py, rng.uniform(-2.0, 2.0, self.NC), rng.uniform(0.35, 0.6, self.NC), col)
        self.eproj_c = oracle.preprocess(oracle.MODE_3D, self.quads_c, self.view, self.proj, w, h)
        # d. 2D records
        px, py = spots(self.ND)
        self.rec_d = records_2d(gs4d, oracle, w, h, px, py, rng.uniform(2.0, 3.2, self.ND), colours(self.ND), rng.uniform(0.0, np.pi, self.ND))
        self.eproj_d = oracle.preprocess(oracle.MODE_2D, self.rec_d, self.view, self.proj, w, h)
        self.oracle = oracle
        self._cache = {}

    def steps(self, pair, eprojs=None):
        """the checker's image after each of the steps a .. e under the blend function `pair` (factor names)"""
        o, w, h = self.oracle, self.W, self.H
        blend = enums(pair)
        pb, pc, pd = eprojs or (self.eproj_b, self.eproj_c, self.eproj_d)
        e = o.clear_image(w, h, self.CLEAR)
        out = []
        o.draw_lines(e, self.lines, self.LINE_COLOUR, self.LINE_WIDTH, blend=blend)
        out.append(e.copy())
        o.composite(pb, self.order_b, o.MODE_4D, w, h, e, nthreads=1, blend=blend)
        out.append(e.copy())
        o.composite(pc, None, o.MODE_3D, w, h, e, nthreads=1, blend=blend)
        out.append(e.copy())
        o.composite(pd, None, o.MODE_2D, w, h, e, nthreads=1, blend=blend)
        out.append(e.copy())
        o.composite(pb, np.arange(self.NE, dtype=np.uint32), o.MODE_4D, w, h, e, nthreads=1, blend=blend)
        out.append(e.copy())
        return out

    def expected(self, pair):
        """steps() of the pair's class, computed once"""
        key = (CLASS[pair[0]], CLASS[pair[1]])
        if key not in self._cache:
            self._cache[key] = self.steps(key)
        return self._cache[key]

    def perturbed_steps(self, pair, seed=1):
        rng = np.random.default_rng(seed)
        return self.steps(pair, (perturbed(self.eproj_b, rng, False), perturbed(self.eproj_c, rng, True), perturbed(self.eproj_d, rng, False)))

    def weights(self):
        w, h = self.W, self.H
        return np.concatenate([fragment_weights(self.eproj_b, w, h), fragment_weights(self.eproj_c, w, h), fragment_weights(self.eproj_d, w, h, mode2d=True)])

    def depth(self):
        """fragments per pixel over all five steps, and of the lines alone"""
        o, w, h = self.oracle, self.W, self.H
        lines = np.zeros((h, w, 4), np.float32)
        o.draw_lines(lines, self.lines, np.array([1.0 / 64.0, 0, 0, 0], np.float32), self.LINE_WIDTH, blend=enums(("ONE", "ONE")))
        lines = np.rint(lines[..., 0] * 64.0).astype(int)
        first = self.eproj_b[:self.NE]
        return lines + coverage(self.eproj_b, w, h) + coverage(self.eproj_c, w, h) + coverage(self.eproj_d, w, h) + coverage(first, w, h), lines


_MATRIX = {}


def matrix(gs4d, oracle):
    if "m" not in _MATRIX:
        _MATRIX["m"] = Matrix(gs4d, oracle)
    return _MATRIX["m"]


# ---- 3. draw order, exactly ---------------------------------------------------------------------------------------------------------------
ONE_ZERO = ("ONE", "ZERO")


class Order:
    """Tile lists of K entries, one per tile, on tiles that are otherwise empty; the last sits on a partial edge tile (the 4 x 4 corner).  Every entry
    is centred on one pixel of its tile (probes) and covers it with c well above the discard, so under (ONE, ZERO) that pixel ends as the colour of the
    list's last entry.  One record set serves every way of drawing it:
      * sorted by the reference's key (the Euclidean distance: lateral jitter decides, record indices are shuffled against it);
      * sorted by GS4D_KEY_VIEW_Z: depth alone decides, and depths are equal in runs — positions 60 .. 68 of every list long enough, and the
        last three of every list — so the stable sort's tie rule (ascending record index) decides who is last and who straddles entry 64;
      * in index order (MODE_4D_DIRECT, quads): a list is its records in ascending index."""
    W, H = 100, 52
    CLEAR = np.array([0.2, 0.5, 0.7, 0.4], np.float32)
    KS = (1, 63, 64, 65, 127, 128, 129, 200, 70)
    CENTRES = ((12, 12), (28, 12), (44, 12), (60, 12), (76, 12), (12, 28), (36, 28), (60, 28), (99, 51))      # the probed pixel of each list (column, row)
    RUN = (60, 69)
    SEED = 3

    def __init__(self, gs4d, oracle, seed=None):
        w, h = self.W, self.H
        rng = np.random.default_rng(self.SEED if seed is None else seed)
        self.view, self.proj = mats(gs4d, w, h)
        n = sum(self.KS)
        lst = np.repeat(np.arange(len(self.KS)), self.KS)
        pos_in_list = np.concatenate([np.arange(k) for k in self.KS])
        rank = pos_in_list.astype(np.float64)
        for li, k in enumerate(self.KS):
            m = lst == li
            r = rank[m]
            if k > self.RUN[0] + 1:
                r[self.RUN[0]:min(self.RUN[1], k)] = self.RUN[0]
            if k >= 3:
                r[k - 3:] = k - 3
            rank[m] = r
        z = -2.0 + (rank + lst / 16.0) * 0.015                                 # rank 0 is farthest: drawn first under the view-z key
        cx = np.array([c[0] for c in self.CENTRES], float)[lst] + 0.5 + rng.uniform(-0.15, 0.15, n)
        cy = np.array([c[1] for c in self.CENTRES], float)[lst] + 0.5 + rng.uniform(-0.15, 0.15, n)
        # small footprints (a box of at most 4 x 4 pixels), large ones, or one in three large, by list
        large = np.where(lst % 3 == 0, False, np.where(lst % 3 == 2, True, pos_in_list % 3 == 1))
        sigma = np.where(large, rng.uniform(0.45, 0.5, n), rng.uniform(0.2, 0.27, n))
        rgba = np.concatenate([rng.uniform(0.05, 0.95, (n, 3)), rng.uniform(0.5, 0.9, (n, 1))], 1).astype(np.float32)
        perm = rng.permutation(n)                                              # entry e is record perm[e]
        self.n, self.lst = n, np.empty(n, np.int64)
        self.lst[perm] = lst
        args = [np.empty_like(v) for v in (cx, cy, z, sigma)]
        for a, v in zip(args, (cx, cy, z, sigma)):
            a[perm] = v
        self.rgba = np.empty_like(rgba)
        self.rgba[perm] = rgba
        self.rec = records_4d(gs4d, oracle, w, h, *args, self.rgba)
        self.quads = quads(gs4d, oracle, w, h, *args, self.rgba)
        self.eproj = oracle.preprocess(oracle.MODE_4D, self.rec, self.view, self.proj, w, h, 0.0, 0.0)
        self.eproj_q = oracle.preprocess(oracle.MODE_3D, self.quads, self.view, self.proj, w, h)
        idx, self.keys_ref = oracle.keygen(self.rec, 0.0, CAM[0])
        _, self.order_ref = oracle.sort_pairs(self.keys_ref.view(np.uint32), idx, "std")
        idx, self.keys_vz = oracle.keygen_viewz(self.rec, 0.0, self.view)
        _, self.order_vz = oracle.sort_pairs(self.keys_vz.view(np.uint32), idx, "std")
        self.oracle = oracle

    def order(self, way):
        return {"ref": self.order_ref, "viewz": self.order_vz, "direct": np.arange(self.n, dtype=np.uint32), "quads": np.arange(self.n, dtype=np.uint32)}[way]

    def list_order(self, way, li):
        """the records of list li in draw order"""
        o = self.order(way)
        return o[self.lst[o] == li]

    def probes(self, li):
        """(row, column) of the pixel every entry of the list is centred on"""
        cx, cy = self.CENTRES[li]
        return np.array([cy]), np.array([cx])

    def image(self, way, drop=0, swap=False):
        """the checker's image of every list drawn in `way` without its last `drop` entries (swap: the last two exchanged)"""
        o = self.oracle
        seq = []
        for li in range(len(self.KS)):
            s = self.list_order(way, li).copy()
            if swap and s.size >= 2:
                s[-1], s[-2] = s[-2], s[-1]
            seq.append(s[:s.size - drop] if drop else s)
        order = np.concatenate(seq).astype(np.uint32)
        quads_ = way == "quads"
        return o.composite(self.eproj_q if quads_ else self.eproj, order, o.MODE_3D if quads_ else o.MODE_4D, self.W, self.H, o.clear_image(self.W, self.H, self.CLEAR),
                           nthreads=1, blend=enums(ONE_ZERO))

    def weights(self):
        return np.concatenate([fragment_weights(self.eproj, self.W, self.H), fragment_weights(self.eproj_q, self.W, self.H)])


_ORDER = {}


def order_scene(gs4d, oracle):
    if "o" not in _ORDER:
        _ORDER["o"] = Order(gs4d, oracle)
    return _ORDER["o"]


# ---- 4. a re-run blends once --------------------------------------------------------------------------------------------------------------
ONE_ONE = ("ONE", "ONE")


def ordered_capacity(cap, known_entries, n):
    """what reserve_entries (csrc/gs4d_api.hip) leaves the lane: twice the draw's instances plus 65536, or one and a half times the entries of the
    last validated draw, never less than it has"""
    return max(cap, 2 * n + 65536, known_entries + known_entries // 2)


def expected_reruns(cap, known_entries, n, entries):
    """How often resolve_lane re-runs an ordered draw of n instances that produces `entries` tile-list entries, on a lane whose entry storage holds
    `cap` while the context's last validated draw had `known_entries` (gs4d_get_stats: capacity, entries): the draw overflows iff entries > capacity,
    and is then re-run with entries + entries / 8 + 1024 — which always fits.  Returns (reruns, capacity afterwards)."""
    cap = ordered_capacity(cap, known_entries, n)
    if entries <= cap:
        return 0, cap
    cap = max(cap, entries + entries // 8 + 1024)
    return 1, ordered_capacity(cap, entries, n)


class Rerun:
    """256 x 128 = 512 tiles.  A default-function draw of small splats brings some tiles into memory and leaves the rest lazily clear; N1 splats
    that each cover the whole image then make 512 N1 entries, more than the first draw's 2 N1 + 65536; N2 > 1.5 N1 of them overflow the grown
    capacity again.  Colours are tiny: under (ONE, ONE) the whole stack stays below 0.5, and blending a draw twice nearly doubles its part."""
    W, H = 256, 128
    CLEAR = np.array([0.05, 0.1, 0.15, 0.2], np.float32)
    N0, N1, N2 = 40, 200, 330
    LINE_COLOUR = np.array([0.04, 0.02, 0.03, 0.05], np.float32)

    def __init__(self, gs4d, oracle):
        w, h = self.W, self.H
        rng = np.random.default_rng(9)
        self.view, self.proj = mats(gs4d, w, h)
        col0 = np.concatenate([rng.uniform(0.1, 0.4, (self.N0, 3)), rng.uniform(0.3, 0.6, (self.N0, 1))], 1)
        self.rec0 = records_4d(gs4d, oracle, w, h, rng.uniform(20.0, 236.0, self.N0), rng.uniform(70.0, 120.0, self.N0), rng.uniform(-1.0, 1.0, self.N0), rng.uniform(0.6, 1.2, self.N0), col0)
        n = self.N2
        col = np.concatenate([rng.uniform(1e-4, 5e-4, (n, 3)), rng.uniform(2e-4, 8e-4, (n, 1))], 1)
        self.rec = records_4d(gs4d, oracle, w, h, rng.uniform(118.0, 138.0, n), rng.uniform(59.0, 69.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(45.0, 50.0, n), col)
        self.lines = np.array([[-0.9, -0.7], [0.8, 0.6], [-0.5, 0.9], [0.4, -0.95]], np.float32)
        self.oracle = oracle
        self._eproj = {}

    def eproj(self, which, t):
        o = self.oracle
        if (which, t) not in self._eproj:
            self._eproj[(which, t)] = o.preprocess(o.MODE_4D, self.rec0 if which == 0 else self.rec, self.view, self.proj, self.W, self.H, t, 0.0)
        return self._eproj[(which, t)]

    def entries(self, n, t=0.0):
        return int(entries_of(self.eproj(1, t)[:n], self.W, self.H).sum())

    def frame(self, t=0.0, twice=False):
        """the checker's images after the first and after the second general draw (twice: the second one blended two times — what a re-run
        on top of a first attempt that had blended would leave)"""
        o, w, h = self.oracle, self.W, self.H
        e = o.clear_image(w, h, self.CLEAR)
        o.composite(self.eproj(0, t), None, o.MODE_4D, w, h, e)
        o.composite(self.eproj(1, t), np.arange(self.N1, dtype=np.uint32), o.MODE_4D, w, h, e, blend=enums(ONE_ONE))
        first = e.copy()
        o.draw_lines(e, self.lines, self.LINE_COLOUR, 2.0, blend=enums(ONE_ONE))
        for _ in range(2 if twice else 1):
            o.composite(self.eproj(1, t), None, o.MODE_4D, w, h, e, blend=enums(ONE_ONE))
        return first, e


_RERUN = {}


def rerun_scene(gs4d, oracle):
    if "r" not in _RERUN:
        _RERUN["r"] = Rerun(gs4d, oracle)
    return _RERUN["r"]
